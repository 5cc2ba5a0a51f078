"""GPU: an episode batch (``BatchedMPPI``) reproduces E separate single-episode runs to the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``MPPI(...,
noise_mode='device', seed=seed_e)``, ``make_device_rollout_fn(engine)``, ``enable_graph(post_step=engine.step_state)``
(tests/test_baseline_sizes_gpu.py's pattern), whose iteration runs ``mjmpc_tree_rollout_fused`` + the fused MPPI update
and steps the engine's device-resident real env.  Unless a test says otherwise every comparison is ``np.array_equal``:
the actions, real-env costs and next observations of every step, the final mean and the final state.
"""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, _cheetah_states, _torch

pytestmark = pytest.mark.gpu

# (the first of the batches' files: it has neither the guard against resets nor the one against a non-finite single run)
MPPI = bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype),
               guards=False)


def _check_against_singles(raw, states, seeds, P, H, T, lam, step_size, init_cov, dtype, **kw):
    return bc.check_against_singles(MPPI, raw, states, seeds, P, H, T, (lam, step_size, init_cov), dtype, **kw)["acts"]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_single_episodes(dtype):
    E = 4
    acts = _check_against_singles(bc.cheetah(), _cheetah_states(E), [123 + i * 12345 for i in range(E)], 256, 16, 20, 0.2, 1.0,
                                  0.3, dtype)
    assert not np.array_equal(acts[:, 0], acts[:, 1])          # (the episodes are different episodes)


def test_per_episode_hyperparameters():
    """Different lam, step_size and init_cov (and initial mean) per episode, base_action 'repeat'."""
    E, H = 4, 16
    init_mean = np.random.RandomState(5).uniform(-0.3, 0.3, (E, H, 6))
    _check_against_singles(bc.cheetah(), _cheetah_states(E), [7 + 3 * i for i in range(E)], 256, H, 20,
                           np.array([0.05, 0.2, 1.0, 0.5]), np.array([1.0, 0.8, 0.5, 0.9]), np.array([0.1, 0.3, 0.6, 1.0]),
                           "f64", base_action="repeat", init_mean=init_mean)


def test_free_joint_model_round_trips_quaternions():
    """A GEN model with a free joint (the tray's glass): the quaternion goes through the state shards and back."""
    raw, states = bc.synthetic_states("tray", 3)
    assert raw_has_free(raw)
    _check_against_singles(raw, states, [11, 12, 13], 256, 16, 10, 0.5, 1.0, 0.3, "f64")


def raw_has_free(raw):
    from mjmpc_amd.models.compile_tree import compile_tree
    m = compile_tree(raw)
    return m.nq > m.nv


def test_rk4_double_pendulum():
    raw, states = bc.synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    _check_against_singles(raw, states, [21, 22], 256, 16, 10, 0.2, 1.0, 0.3, "f64")


def test_permuting_the_episodes_permutes_the_results():
    lam, step, cov = np.array([0.1, 0.2, 0.3, 0.4]), np.array([1.0, 0.9, 0.8, 0.7]), np.array([0.2, 0.3, 0.4, 0.5])
    bc.check_permutation(MPPI, bc.cheetah(), _cheetah_states(4), [5, 6, 7, 8], 256, 16, 10, (lam, step, cov), "f64", [2, 0, 3, 1])


def test_one_episode_equals_the_single_path():
    _check_against_singles(bc.cheetah(), _cheetah_states(1), [123], 512, 16, 15, 0.2, 1.0, 0.3, "f64")


def test_reacher_on_the_tree_engine_with_per_episode_targets():
    """sawyer.xml (the reference's reacher) on the tree engine, eight episodes with their own targets, 512 x H32."""
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    raw, E = reacher7dof_raw(), 8
    env = Reacher7DOFEnv(engine=TreeRolloutEngine(raw))
    states = []
    for i in range(E):
        env.reset(seed=123 + i * 12345)
        st = env.get_env_state()
        states.append(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
    env.engine.close()
    assert len({tuple(s["target_pos"]) for s in states}) == E
    _check_against_singles(raw, states, [123 + i * 12345 for i in range(E)], 512, 32, 8, 0.01, 1.0, 1.0, "f64")


def test_batched_env_step_equals_single_steps_with_resets():
    """One launch steps E real envs as mjmpc_tree_step_state steps E single-state engines - bits and env-reset counts -
    including a start state already beyond MuJoCo's 1e10 bound (the kernel's emulation of mj_resetData)."""
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw, E = half_cheetah_raw(), 4
    states = _cheetah_states(E)
    states[2] = dict(qpos=states[2]["qpos"].copy(), qvel=states[2]["qvel"].copy())
    states[2]["qvel"][3] = 3e10
    rng = np.random.RandomState(0)
    actions = [rng.uniform(-1, 1, (E, 6)) for _ in range(3)]
    for dtype in ("f64", "f32"):
        # the batch: one engine, E state shards
        eng = TreeRolloutEngine(raw, dtype=dtype)
        eng.on_env_reset = "ignore"
        nq, nv, D = eng.model.nq, eng.model.nv, eng.d_obs
        arr = np.zeros((E, 78))
        for k, s in enumerate(states):
            arr[k, :nq], arr[k, 40:40 + nv], arr[k, 72:75] = s["qpos"], s["qvel"], eng.model.target_default
        lib, strm = eng._lib, eng._stream()
        _lib.check(lib.mjmpc_tree_set_shard_states(eng._h, arr.ctypes.data_as(_lib._dp), E, strm))
        tdt = torch.float32 if dtype == "f32" else torch.float64
        bc, bo = [], []
        for a in actions:
            ad = torch.from_numpy(a).cuda()
            cost, obs = torch.empty(E, dtype=tdt, device="cuda"), torch.empty((E, D), dtype=tdt, device="cuda")
            _lib.check(lib.mjmpc_tree_step_shard_states(eng._h, eng._code, ctypes.c_void_p(ad.data_ptr()),
                                                        ctypes.c_void_p(cost.data_ptr()), ctypes.c_void_p(obs.data_ptr()), strm))
            torch.cuda.synchronize()
            bc.append(cost.cpu().numpy())
            bo.append(obs.cpu().numpy())
        qp, qv = np.zeros((E, nq)), np.zeros((E, nv))
        _lib.check(lib.mjmpc_tree_get_shard_states(eng._h, qp.ctypes.data_as(_lib._dp), qv.ctypes.data_as(_lib._dp), strm))
        batch_resets = eng.env_resets()
        eng.close()
        # E single-state engines, mjmpc_tree_step_state
        single_resets = 0
        for e in range(E):
            s = TreeRolloutEngine(raw, dtype=dtype)
            s.on_env_reset = "ignore"
            s.set_env_state(dict(states[e]))
            for k, a in enumerate(actions):
                cost, obs = s.step_state(a[e])
                torch.cuda.synchronize()
                assert np.array_equal(cost.cpu().numpy()[0], bc[k][e]), (dtype, e, k)
                assert np.array_equal(obs.cpu().numpy(), bo[k][e]), (dtype, e, k)
            st = s.get_state_device()
            assert np.array_equal(st["qpos"], qp[e]) and np.array_equal(st["qvel"], qv[e]), (dtype, e)
            single_resets += s.env_resets()
            s.close()
        assert single_resets >= 1 and batch_resets == single_resets, (dtype, batch_resets, single_resets)
        assert np.all(np.isfinite(qp)) and np.all(np.abs(qv) < 1e10)


def test_env_reset_policy_is_checked_where_run_synchronises():
    """A real env that resets raises at the end of run() under the default policy (SimulationUnstableError)."""
    from mjmpc_amd.control import BatchedMPPI
    from mjmpc_amd.envs.tree_engine import SimulationUnstableError
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    states = _cheetah_states(2)
    bad = dict(qpos=states[1]["qpos"].copy(), qvel=states[1]["qvel"].copy())
    bad["qvel"][3] = 3e10
    b = BatchedMPPI(half_cheetah_raw(), 2, 8, 64, 0.2, 1.0, 0.3, 1.0, FILT, "null", [1, 2])
    b.set_states([states[0], bad])
    with pytest.raises(SimulationUnstableError):
        b.run(2)
    b.on_env_reset = "ignore"
    acts, _, _ = b.run(2)
    assert np.all(np.isfinite(acts))
    b.close()
