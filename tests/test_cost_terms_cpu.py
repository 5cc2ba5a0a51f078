"""CPU: user-defined cost terms (mjmpc_amd/envs/cost_terms.py) - the table's encoding, every refusal of the
builder and of ``set_cost_terms``, ``obs_layout()`` without a device, the C entry's argument checks, the config block and
the guards on the fused launches."""
import os

import numpy as np
import pytest
import yaml

from cost_terms_cases import ABS, COS, NORM, SQUARE, restate

from mjmpc_amd import _lib
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
from mjmpc_amd.models.half_cheetah import half_cheetah_raw
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
from mjmpc_amd.models.synthetic import synthetic_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reacher():
    return ArmRolloutEngine.host_only(reacher7dof_raw())


@pytest.fixture(scope="module")
def cartpole():
    return TreeRolloutEngine.host_only(synthetic_raw("cartpole"))


@pytest.fixture(scope="module")
def cheetah():
    return TreeRolloutEngine.host_only(half_cheetah_raw())


# ---- obs_layout ---------------------------------------------------------------------------------------------------------
def test_obs_layout_without_a_device(reacher, cheetah):
    assert reacher.obs_layout() == dict(qpos=slice(0, 7), qvel=slice(7, 14), site=slice(14, 17),
                                        site_minus_target=slice(17, 20))
    assert reacher.model.d_obs == 20
    m = cheetah.model                               # forward task: [qpos[obs_skip:], qvel]
    assert (m.obs_skip, m.nq, m.nv) == (1, 9, 9)
    assert cheetah.obs_layout() == dict(qpos=slice(0, 8), qvel=slice(8, 17)) and m.d_obs == 17
    tray = TreeRolloutEngine.host_only(synthetic_raw("tray"))
    m = tray.model                                  # a free joint: nq = nv + 1, qpos in MuJoCo's layout
    assert m.nq == m.nv + 1
    assert tray.obs_layout() == dict(qpos=slice(0, m.nq), qvel=slice(m.nq, m.nq + m.nv),
                                     site=slice(m.nq + m.nv, m.nq + m.nv + 3),
                                     site_minus_target=slice(m.nq + m.nv + 3, m.d_obs))


# ---- the table ----------------------------------------------------------------------------------------------------------
def test_every_kind_encodes_as_its_row(reacher):
    t = CostTerms(reacher)
    t.abs(obs="qvel", index=0, weight=2.0, target=0.5)
    t.square(action=3, weight=-0.25)
    t.cos(obs="qpos", index=[1, 2], weight=1.5, target=[0.1, -0.2])
    t.norm(obs=[14, 16], weight=3.0, target=[0.3, 0.4])
    want = np.array([[ABS, 0, 7, 2.0, 0.5, 0, 0, 0],
                     [SQUARE, 1, 3, -0.25, 0.0, 0, 0, 0],
                     [COS, 0, 1, 1.5, 0.1, 0, 0, 0],
                     [COS, 0, 2, 1.5, -0.2, 0, 0, 0],
                     [NORM, 0, 14, 3.0, 0.3, 1, 0, 0],
                     [NORM, 0, 16, 3.0, 0.4, 1, 0, 0]], float)
    tab = t.table()
    assert tab.dtype == np.float64 and np.array_equal(tab, want)
    assert len(t) == 6 and t.keep_builtin is False


def test_every_entry_expansion(reacher, cheetah):
    tab = CostTerms(reacher).square(obs="qvel", weight=0.01).table()
    assert np.array_equal(tab[:, 2], np.arange(7, 14)) and np.all(tab[:, 0] == SQUARE) and np.all(tab[:, 3] == 0.01)
    tab = CostTerms(reacher).abs(action=True).table()
    assert np.array_equal(tab[:, 2], np.arange(7)) and np.all(tab[:, 1] == 1)
    tab = CostTerms(cheetah, keep_builtin=True).square(obs="qpos").table()        # qpos[1:]: the block's entry 0 is qpos[1]
    assert np.array_equal(tab[:, 2], np.arange(8))
    assert np.array_equal(CostTerms(cheetah).abs(obs="qvel", index=0).table()[:, 2], [8])


def test_norm_groups_get_fresh_contiguous_ids_and_the_terminal_flag(reacher):
    t = CostTerms(reacher)
    t.norm(obs="site_minus_target", weight=5.0)
    t.norm(obs="site_minus_target", weight=2.0, terminal=True)     # a neighbour over the same entries must not merge
    t.abs(obs="qpos", index=0)
    t.norm(obs="qvel", index=[0, 1])
    tab = t.table()
    assert tab[:, 5].tolist() == [1, 1, 1, 2, 2, 2, 0, 3, 3]
    assert tab[:, 6].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0]
    for g in (1, 2, 3):                             # contiguous, all of kind NORM, one `when` per group
        rows = np.flatnonzero(tab[:, 5] == g)
        assert np.array_equal(rows, np.arange(rows[0], rows[-1] + 1)) and np.all(tab[rows, 0] == NORM)
        assert len(set(tab[rows, 6])) == 1


def test_builtin_reach_against_the_hand_written_table(reacher, cartpole):
    """Three ABS rows and one NORM group of weight 5 over ``site_minus_target``: four terms, and - a row reads one entry -
    six rows."""
    want = np.array([[0, 0, 17, 1, 0, 0, 0, 0], [0, 0, 18, 1, 0, 0, 0, 0], [0, 0, 19, 1, 0, 0, 0, 0],
                     [2, 0, 17, 5, 0, 1, 0, 0], [2, 0, 18, 5, 0, 1, 0, 0], [2, 0, 19, 5, 0, 1, 0, 0]], float)
    t = CostTerms.builtin_reach(reacher)
    assert np.array_equal(t.table(), want) and not t.keep_builtin
    assert CostTerms.builtin_reach(reacher, keep_builtin=True).keep_builtin
    want[:, 2] -= 10                                # the cart-pole: nq = nv = 2, d_obs 10
    assert np.array_equal(CostTerms.builtin_reach(cartpole).table(), want)
    # the restatement of those rows IS the built-in cost
    rng = np.random.default_rng(0)
    nobs = rng.uniform(-1, 1, (3, 2, 20))
    d = nobs[..., 17:]
    cost, _ = restate(t.table(), nobs, None, np.zeros((3, 2)), False, True)
    np.testing.assert_allclose(cost, np.abs(d).sum(-1) + 5 * np.sqrt((d * d).sum(-1)), rtol=1e-15)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(reacher, cheetah):
    with pytest.raises(ValueError, match="empty"):
        CostTerms(reacher).table()
    t = CostTerms(reacher)
    for _ in range(18):
        t.square(obs="qvel")                        # 126 rows
    t.abs(obs=[0, 1])                               # 128: the table is full
    assert len(t) == 128 and t.table().shape == (128, 8)
    with pytest.raises(ValueError, match="128"):
        t.abs(obs=0)                                # 129
    assert len(t) == 128
    late = CostTerms()                              # no engine yet: refused when the table is made
    for _ in range(129):
        late.abs(obs=0)
    with pytest.raises(ValueError, match="128"):
        late.table(reacher)
    with pytest.raises(ValueError, match="index 20"):
        CostTerms(reacher).abs(obs=20)              # == d_obs
    with pytest.raises(ValueError, match="index 7"):
        CostTerms(reacher).abs(action=7)            # == d_action
    with pytest.raises(ValueError, match="index 3"):
        CostTerms(reacher).abs(obs="site", index=3)
    with pytest.raises(ValueError, match="index 20"):
        CostTerms().abs(obs=20).table(reacher)
    with pytest.raises(ValueError, match="finite"):
        CostTerms(reacher).abs(obs=0, weight=float("nan"))
    with pytest.raises(ValueError, match="finite"):
        CostTerms(reacher).abs(obs=0, target=float("inf"))
    with pytest.raises(ValueError, match="unknown observation block"):
        CostTerms(reacher).abs(obs="qacc")
    with pytest.raises(ValueError, match="unknown observation block"):
        CostTerms(cheetah).abs(obs="site_minus_target")         # the forward task has no tracked site
    with pytest.raises(ValueError, match="reach"):
        CostTerms.builtin_reach(cheetah)
    with pytest.raises(ValueError):
        CostTerms(reacher).abs(obs=0, action=0)
    with pytest.raises(ValueError):
        CostTerms(reacher).abs()


def test_set_cost_terms_refuses_before_the_device(reacher):
    """``set_cost_terms`` resolves the table first: an engine without a device gets as far as the refusal."""
    with pytest.raises(ValueError, match="empty"):
        reacher.set_cost_terms(CostTerms())
    with pytest.raises(ValueError, match="index 20"):
        reacher.set_cost_terms(CostTerms().square(obs=[3, 20]))


# ---- the C entry --------------------------------------------------------------------------------------------------------
def test_mjmpc_cost_terms_bad_arguments_are_codes_and_messages():
    import ctypes
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = [
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 3, 1, None, p, p, 1, 0, 0, p, None),          # null observations
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 3, 1, p, p, None, 1, 0, 0, p, None),          # null table
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 3, 1, p, p, p, 1, 0, 0, None, None),          # null costs
        lambda: lib.mjmpc_cost_terms(_lib.F64, 0, 2, 3, 1, p, p, p, 1, 0, 0, p, None),             # P < 1
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 0, 3, 1, p, p, p, 1, 0, 0, p, None),             # H < 1
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 0, 1, p, p, p, 1, 0, 0, p, None),             # d_obs < 1
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 3, 1, p, p, p, 0, 0, 0, p, None),             # n_terms < 1
        lambda: lib.mjmpc_cost_terms(_lib.F64, 4, 2, 3, 1, p, p, p, 129, 0, 0, p, None),           # n_terms > 128
        lambda: lib.mjmpc_cost_terms(7, 4, 2, 3, 1, p, p, p, 1, 0, 0, p, None),                    # unknown dtype
    ]
    for call in bad:                                # (refused before anything is launched: these are host pointers)
        assert call() != 0
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms")


# ---- the config block ---------------------------------------------------------------------------------------------------
def test_the_config_block_parses_to_its_table(cartpole):
    block = yaml.safe_load("""
cost_terms:
  keep_builtin: false
  terms:
    - {kind: norm, obs: site_minus_target, weight: 5.0}
    - {kind: cos, obs: qpos, index: 1, weight: 1.0}
    - {kind: square, obs: qvel, weight: 0.01}
    - {kind: square, action: 0, weight: 0.001}
    - {kind: square, obs: qvel, weight: 1.0, terminal: true}
""")["cost_terms"]
    t = cost_terms_from_config(block, cartpole)
    want = np.array([[NORM, 0, 7, 5.0, 0, 1, 0, 0], [NORM, 0, 8, 5.0, 0, 1, 0, 0], [NORM, 0, 9, 5.0, 0, 1, 0, 0],
                     [COS, 0, 1, 1.0, 0, 0, 0, 0],
                     [SQUARE, 0, 2, 0.01, 0, 0, 0, 0], [SQUARE, 0, 3, 0.01, 0, 0, 0, 0],
                     [SQUARE, 1, 0, 0.001, 0, 0, 0, 0],
                     [SQUARE, 0, 2, 1.0, 0, 0, 1, 0], [SQUARE, 0, 3, 1.0, 0, 0, 1, 0]], float)
    assert np.array_equal(t.table(), want) and t.keep_builtin is False
    for broken in (dict(terms=[]), dict(terms=[dict(kind="huber", obs="qvel")]), dict(terms=[dict(kind="abs", obs="qvel", wieght=1)]),
                   dict(terms=[dict(kind="abs", obs="qvel")], keep=True)):
        with pytest.raises(ValueError):
            cost_terms_from_config(broken, cartpole)


def test_the_cartpole_terms_config_loads(cartpole):
    with open(os.path.join(ROOT, "examples", "configs", "cartpole_terms_gpu.yml")) as f:
        exp = yaml.safe_load(f)
    assert exp["env_name"] == "cartpole_friction-v0"
    tab = cost_terms_from_config(exp["cost_terms"], cartpole).table()
    kinds = tab[:, 0].tolist()
    assert COS in kinds and SQUARE in kinds                                 # angle; cart position, velocities, action
    assert np.any(tab[:, 1] == 1) and np.any(tab[:, 6] == 1)                # an action term, a terminal term
    assert tab[kinds.index(COS), 2] == 1                                    # the pole's angle is qpos[1]


# ---- the fused launches ---------------------------------------------------------------------------------------------------
def test_fused_launches_refuse_with_terms_set_before_touching_the_library():
    eng = ArmRolloutEngine.__new__(ArmRolloutEngine)        # no library, no handle: a call that got further would fail otherwise
    eng._cost_terms = CostTerms().abs(obs=0)
    for call in (lambda: eng.rollout_fused(8, 4, None, None, None, None),
                 lambda: eng.mppi_step(8, 4, *[None] * 12),
                 lambda: eng.rollout_sampled(8, 4, *[None] * 9),
                 lambda: eng.mppi_step_launcher(8, 4, *[None] * 12),
                 lambda: eng.mppi_combine_launcher(*[None] * 11)):
        with pytest.raises(RuntimeError, match="set_cost_terms"):
            call()
    tree = TreeRolloutEngine.__new__(TreeRolloutEngine)
    tree._cost_terms = eng._cost_terms
    with pytest.raises(RuntimeError, match="set_cost_terms"):
        tree.rollout_fused(8, 4, None, None, None, None)


def test_closures_carry_no_fused_launch_with_terms_and_the_engine_keeps_one_shape(reacher):
    def fresh(terms):
        eng = ArmRolloutEngine.__new__(ArmRolloutEngine)
        eng.num_shards, eng._cost_terms = 1, terms
        return eng
    eng = fresh(CostTerms().abs(obs=0))
    fn = make_device_rollout_fn(eng)
    assert fn.accepts_device and fn.engine is eng
    assert not any(hasattr(fn, a) for a in ("fused", "mono", "sampled", "mono_launcher", "combine_launcher"))
    with pytest.raises(RuntimeError, match="set the terms first"):
        eng.set_cost_terms(None)                    # the closure handed out offers no fused launch: it would stay that way
    eng = fresh(None)
    fn = make_device_rollout_fn(eng)
    assert all(hasattr(fn, a) for a in ("fused", "mono", "sampled", "mono_launcher", "combine_launcher"))
    with pytest.raises(RuntimeError, match="set the terms first"):
        eng.set_cost_terms(CostTerms().abs(obs=0))  # ... and this one would go on offering them
    eng.set_cost_terms(None)                        # the shape it already has: fine


def test_real_step_guard_marks_the_engine_in_every_mode():
    eng = ArmRolloutEngine.__new__(ArmRolloutEngine)
    eng.on_env_reset = "ignore"
    assert eng._in_real_step is False
    with eng.real_step_guard("test"):
        assert eng._in_real_step is True
    assert eng._in_real_step is False
    eng.on_env_reset = "raise"
    eng.diverged_substeps = lambda: 0
    with eng.real_step_guard("test"):
        assert eng._in_real_step is True
    assert eng._in_real_step is False
    with pytest.raises(KeyError):
        with eng.real_step_guard("test"):
            raise KeyError("inside")
    assert eng._in_real_step is False
