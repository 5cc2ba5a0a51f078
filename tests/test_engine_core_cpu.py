"""CPU: the arm and tree rollout engines share one host-side core (``envs/_engine.py``) - the shared members live on the
base class only, and a shard's start state is packed by the engine's layout.  Nothing here loads the library."""
import numpy as np

from mjmpc_amd.envs._engine import RolloutEngine
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine

SHARED = ("rollout", "rollout_device", "step_state", "close", "solver_failures", "diverged_substeps", "_stream", "_buffer",
          "_as_device", "_set_shard_states", "get_env_state")


def test_both_engines_derive_from_the_core():
    assert issubclass(ArmRolloutEngine, RolloutEngine) and issubclass(TreeRolloutEngine, RolloutEngine)


def test_shared_members_are_defined_once():
    """A guard against the copies growing back: neither subclass defines what the base holds."""
    for cls in (ArmRolloutEngine, TreeRolloutEngine):
        again = [name for name in SHARED if name in cls.__dict__]
        assert not again, (cls.__name__, again)
        for name in SHARED:
            assert getattr(cls, name) is getattr(RolloutEngine, name), (cls.__name__, name)


def _states(nq, nv, n=3):
    rng = np.random.RandomState(0)
    return [dict(qp=rng.uniform(1, 2, nq), qv=rng.uniform(3, 4, nv), target_pos=rng.uniform(5, 6, 3)) for _ in range(n)]


def _check_layout(engine, states, nq, nv, stride, ov, ot):
    arr = engine._pack_shard_states(states)
    assert arr.shape == (len(states), stride) and arr.dtype == np.float64
    used = np.zeros(stride, bool)
    used[:nq] = used[ov:ov + nv] = used[ot:ot + 3] = True
    for k, s in enumerate(states):
        assert np.array_equal(arr[k, :nq], s["qp"])
        assert np.array_equal(arr[k, ov:ov + nv], s["qv"])
        assert np.array_equal(arr[k, ot:ot + 3], s["target_pos"])
        assert np.all(arr[k, ~used] == 0.0)


def test_arm_shard_states_are_19_wide():
    """A 7-dof arm: qp | qv | target_pos at columns 0 | 8 | 16 of a 19-wide row (MJMPC_ARM_STATE_LEN)."""
    from mjmpc_amd.models.compile import compile_arm
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    eng = object.__new__(ArmRolloutEngine)
    eng.model = compile_arm(reacher7dof_raw())
    eng.closed = True                       # (no handle: __del__ has nothing to destroy)
    assert eng.model.nv == 7
    _check_layout(eng, _states(7, 7), 7, 7, 19, 8, 16)


def test_tree_shard_states_are_78_wide():
    """A tree with a free joint (nq != nv): qpos | qvel | target_pos at columns 0 | 40 | 72 of a 78-wide row."""
    from mjmpc_amd.models.compile_tree import compile_tree
    from mjmpc_amd.models.synthetic import synthetic_raw
    eng = object.__new__(TreeRolloutEngine)
    eng.model = compile_tree(synthetic_raw("tray"))
    eng.closed = True
    nq, nv = eng.model.nq, eng.model.nv
    assert nq != nv
    _check_layout(eng, _states(nq, nv), nq, nv, 78, 40, 72)
