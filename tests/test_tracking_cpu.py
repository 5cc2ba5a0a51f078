"""CPU: cost terms that track a reference trajectory - the builder's ``reference=`` (shapes, the ``reserved`` and
``target`` columns, ``reference_table``, every refusal), the config block's ``reference`` / ``repeat`` / ``periodic`` keys, what the
episode batches accept and refuse per episode, the two entry points (declared, bound, exported; every argument refusal a code
and a message, nothing launched) and the restatement's own clamp and wrap on a hand-computed reference."""
import os

import numpy as np
import pytest

import batched_cases as bc
import tracking_cases as tc
from mjmpc_amd import _lib
from mjmpc_amd.control import BatchedMPPI
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
from mjmpc_amd.models.synthetic import synthetic_raw

ENTRY_POINTS = ["mjmpc_cost_terms_track", "mjmpc_cost_terms_track_batch"]


@pytest.fixture(scope="module")
def cartpole():
    return TreeRolloutEngine.host_only(synthetic_raw("cartpole"))


@pytest.fixture(scope="module")
def reacher():
    return ArmRolloutEngine.host_only(reacher7dof_raw())


# ---- the builder ----------------------------------------------------------------------------------------------------------
def test_reference_fills_the_reserved_and_target_columns(cartpole):
    lay = cartpole.obs_layout()
    s, q = lay["site_minus_target"].start, lay["qpos"].start
    one = np.array([0.5, 0.25, -1.0, 2.0])                              # [N]: one value for every index
    each = np.arange(12, dtype=np.float64).reshape(4, 3) / 8.0          # [N][n_idx]
    t = CostTerms(cartpole)
    assert not t.tracked and t.periodic is False and t.reference_table() is None
    t.abs(obs="qpos", index=0, weight=2.0)                              # a constant row before
    t.norm(obs="site_minus_target", weight=3.0, reference=each, periodic=True)
    t.square(obs="qvel", target=0.75)                                   # ... between (two rows)
    t.cos(action=0, weight=0.5, reference=one, periodic=True, terminal=True)
    t.square(obs="qpos", reference=one, periodic=True)                  # [N] over a block of two entries
    assert t.tracked and t.periodic is True
    want = np.array([[0, 0, q, 2.0, 0.0, 0, 0, 0],
                     [2, 0, s, 3.0, each[0, 0], 1, 0, 1], [2, 0, s + 1, 3.0, each[0, 1], 1, 0, 2],
                     [2, 0, s + 2, 3.0, each[0, 2], 1, 0, 3],
                     [1, 0, lay["qvel"].start, 1.0, 0.75, 0, 0, 0], [1, 0, lay["qvel"].start + 1, 1.0, 0.75, 0, 0, 0],
                     [3, 1, 0, 0.5, one[0], 0, 1, 4],
                     [1, 0, q, 1.0, one[0], 0, 0, 5], [1, 0, q + 1, 1.0, one[0], 0, 0, 6]], np.float64)
    assert np.array_equal(t.table(), want)
    ref = t.reference_table()
    assert ref.dtype == np.float64 and ref.shape == (4, 6) and ref.flags["C_CONTIGUOUS"]
    assert np.array_equal(ref, np.concatenate([each, one[:, None], one[:, None], one[:, None]], axis=1))
    # the builder keeps its own copy
    one[0] = 99.0
    assert t.reference_table()[0, 3] == 0.5
    # absolute indices without an engine resolve at table(engine)
    late = CostTerms().square(obs=[q, q + 1], reference=[[0.1, 0.2], [0.3, 0.4]]).abs(action=[0], reference=[1.0, 2.0])
    assert np.array_equal(late.table(cartpole)[:, 7], [1, 2, 3]) and np.array_equal(late.table(cartpole)[:, 4], [0.1, 0.2, 1.0])
    assert np.array_equal(late.reference_table(cartpole), [[0.1, 0.2, 1.0], [0.3, 0.4, 2.0]])
    assert late.periodic is False


def test_tables_without_a_reference_are_unchanged_bytes(cartpole, reacher):
    t = CostTerms(reacher)
    t.abs(obs="site_minus_target", index=0, weight=0.7)
    t.square(action=0, weight=0.05)
    t.norm(obs="site_minus_target", weight=4.0, target=[0.1, 0.2, 0.3])
    t.square(obs="qvel", index=0, weight=0.5, terminal=True)
    s = reacher.obs_layout()["site_minus_target"].start
    v = reacher.obs_layout()["qvel"].start
    want = np.array([[0, 0, s, 0.7, 0.0, 0, 0, 0], [1, 1, 0, 0.05, 0.0, 0, 0, 0],
                     [2, 0, s, 4.0, 0.1, 1, 0, 0], [2, 0, s + 1, 4.0, 0.2, 1, 0, 0], [2, 0, s + 2, 4.0, 0.3, 1, 0, 0],
                     [1, 0, v, 0.5, 0.0, 0, 1, 0]], np.float64)
    assert t.table().tobytes() == want.tobytes()
    assert not t.tracked and t.reference_table() is None and np.all(t.table()[:, 7] == 0)
    assert np.all(CostTerms.builtin_reach(cartpole).table()[:, 7] == 0)


def test_the_builder_refuses(cartpole):
    ok = [0.0, 0.1, 0.2]
    for make, match in [
        (lambda t: t.square(obs="qpos", index=0, reference=[0.0, np.nan]), "finite"),
        (lambda t: t.square(obs="qpos", index=0, reference=[0.0, np.inf]), "finite"),
        (lambda t: t.square(obs="qpos", index=0, reference=ok, target=0.5), "not both"),
        (lambda t: t.norm(obs="site_minus_target", reference=ok, target=[0.0, 0.1, 0.0]), "not both"),
        (lambda t: t.square(obs="qpos", index=0, reference=ok).abs(action=0, reference=[0.0, 0.1]), "share one N"),
        (lambda t: t.square(obs="qpos", index=0, reference=ok).abs(action=0, reference=ok, periodic=True), "periodic"),
        (lambda t: t.square(obs="qpos", index=0, reference=ok, periodic=True).abs(action=0, reference=ok), "periodic"),
        (lambda t: t.square(obs="qpos", index=0, periodic=True), "periodic"),                    # periodic without a reference
        (lambda t: t.square(obs="qpos", index=0, reference=[]), "rows"),                         # N = 0
        (lambda t: t.square(obs="qpos", index=0, reference=np.zeros((1 << 20) + 1)), "rows"),    # N > 2^20
        (lambda t: t.square(obs="qpos", index=0, reference=0.5), "reference must be"),           # no time axis
        (lambda t: t.square(obs="qpos", index=0, reference=np.zeros((2, 2, 2))), "reference must be"),
        (lambda t: t.norm(obs="site_minus_target", reference=np.zeros((4, 2))), "reference must be"),   # 2 columns, 3 indices
        (lambda t: t.square(obs="qpos", index=[0, 1], reference=np.zeros((4, 3))), "reference must be"),
    ]:
        t = CostTerms(cartpole)
        with pytest.raises(ValueError, match=match):
            make(t)
    # the limits themselves are fine; a refused term leaves the builder as it was
    t = CostTerms(cartpole).square(obs="qpos", index=0, reference=np.zeros(1 << 20)).abs(action=0, reference=np.zeros(1 << 20))
    assert t.reference_table().shape == (1 << 20, 2)
    t = CostTerms(cartpole).square(obs="qpos", index=0, reference=[1.5])
    with pytest.raises(ValueError):
        t.abs(action=0, reference=[0.0, 1.0])
    assert len(t) == 1 and t.reference_table().tolist() == [[1.5]] and t.periodic is False
    # without an engine the column count is checked when the engine is known
    late = CostTerms().norm(obs="site_minus_target", reference=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="reference must be"):
        late.table(cartpole)
    with pytest.raises(ValueError, match="reference must be"):
        late.reference_table(cartpole)


# ---- the config block -----------------------------------------------------------------------------------------------------
def test_config_reference_repeat_and_periodic(cartpole):
    block = dict(terms=[
        dict(kind="cos", obs="qpos", index=1, weight=4.0),
        dict(kind="square", obs="qpos", index=0, weight=0.5, reference=[0.0, 0.4, 0.0, -0.4], repeat=3, periodic=True),
        dict(kind="norm", obs="site_minus_target", index=[0, 2], reference=[[0.1, 0.2]] * 6 + [[0.3, 0.4]] * 6, periodic=True),
    ])
    t = cost_terms_from_config(block, cartpole)
    assert isinstance(t, CostTerms) and t.tracked and t.periodic
    ref = t.reference_table()
    assert ref.shape == (12, 3)
    assert ref[:, 0].tolist() == [0.0] * 3 + [0.4] * 3 + [0.0] * 3 + [-0.4] * 3
    assert np.array_equal(ref[:, 1:], [[0.1, 0.2]] * 6 + [[0.3, 0.4]] * 6)
    assert t.table()[:, 7].tolist() == [0, 1, 2, 3]
    # the same block for a batch whose episode count is no reference's length: one CostTerms
    assert isinstance(cost_terms_from_config(block, cartpole, num_episodes=5), CostTerms)
    for entry, match in [
        (dict(kind="square", obs="qpos", index=0, refrence=[0.0, 0.4]), "a term takes"),         # a misspelt key
        (dict(kind="square", obs="qpos", index=0, reference=[0.0, 0.4], repeats=2), "a term takes"),
        (dict(kind="square", obs="qpos", index=0, reference=[0.0, 0.4], repeat=0), "repeat"),
        (dict(kind="square", obs="qpos", index=0, reference=[0.0, 0.4], repeat=1.5), "repeat"),
        (dict(kind="square", obs="qpos", index=0, repeat=2), "go with a reference"),
        (dict(kind="square", obs="qpos", index=0, periodic=True), "go with a reference"),
        (dict(kind="square", obs="qpos", index=0, reference=0.5), "a reference is"),
        (dict(kind="square", obs="qpos", index=0, reference=[0.0, 0.4], target=1.0), "not both"),
        (dict(kind="square", obs="qpos", index=0, reference=[[[0.0], [0.4]]]), "per episode"),   # per episode without a batch
    ]:
        with pytest.raises(ValueError, match=match):
            cost_terms_from_config(dict(terms=[entry]), cartpole)


def test_config_reference_per_episode(cartpole):
    block = dict(terms=[
        dict(kind="square", obs="qpos", index=0, reference=[[0.0, 0.4], [0.1, 0.5], [0.2, 0.6]], repeat=2),
        dict(kind="norm", obs="site_minus_target", index=[0, 1],
             reference=[[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]] * 2 + [[[0.0, 0.0]] * 4]),
        dict(kind="square", action=0, weight=[0.1, 0.2, 0.3]),
    ])
    each = cost_terms_from_config(block, cartpole, num_episodes=3)
    assert isinstance(each, list) and len(each) == 3
    refs = [t.reference_table() for t in each]
    assert all(r.shape == (4, 3) for r in refs)
    assert [r[:, 0].tolist() for r in refs] == [[0.0, 0.0, 0.4, 0.4], [0.1, 0.1, 0.5, 0.5], [0.2, 0.2, 0.6, 0.6]]
    assert np.array_equal(refs[1][:, 1:], [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]) and np.all(refs[2][:, 1:] == 0)
    tables, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, 3)
    assert tables.shape == (3, 4, 8) and np.array_equal(tables[:, 0, 4], [0.0, 0.1, 0.2])
    stacked, periodic = BatchedMPPI._resolve_tracking(each, cartpole, 3)
    assert stacked.shape == (3, 4, 3) and stacked.dtype == np.float64 and periodic is False
    assert np.array_equal(stacked, np.stack(refs))
    with pytest.raises(ValueError, match="per episode"):                        # three levels: one per episode, of another count
        cost_terms_from_config(dict(terms=[dict(kind="square", obs="qpos", reference=[[[0.0, 0.1]], [[0.2, 0.3]]])]), cartpole,
                               num_episodes=3)


def test_both_example_configs_load(cartpole):
    import yaml
    for cfg, per_episode in (("cartpole_track_gpu.yml", False), ("cartpole_track_batch_gpu.yml", True)):
        with open(os.path.join(bc.ROOT, "examples", "configs", cfg)) as f:
            exp = yaml.safe_load(f)
        E = exp["n_episodes"]
        terms = cost_terms_from_config(exp["cost_terms"], cartpole, num_episodes=E if per_episode else None)
        each = terms if per_episode else [terms]
        assert len(each) == (4 if per_episode else 1)
        for t in each:
            ref = t.reference_table()
            assert t.tracked and t.periodic and ref.shape == (200, 1)
            assert all(len(set(ref[50 * i:50 * (i + 1), 0])) == 1 for i in range(4))
        assert each[0].reference_table()[::50, 0].tolist() == [0.0, 0.4, 0.0, -0.4]
        if per_episode:
            stacked, periodic = BatchedMPPI._resolve_tracking(each, cartpole, E)
            assert stacked.shape == (4, 200, 1) and periodic and len({r.tobytes() for r in stacked}) == 4


# ---- the batch resolver ---------------------------------------------------------------------------------------------------
def _tracked(engine, ref, periodic=False, which="qpos"):
    t = CostTerms(engine)
    t.abs(obs="site_minus_target", index=0, weight=1.0, **(dict(reference=ref, periodic=periodic) if which == "site" else {}))
    t.square(obs="qpos", index=0, weight=0.5, **(dict(reference=ref, periodic=periodic) if which == "qpos" else {}))
    return t


def test_batch_resolver_accepts_values_and_refuses_structure(cartpole):
    a, b, c = [0.0, 0.1, 0.2], [1.0, 1.1, 1.2], [2.0, 2.1, 2.2]
    each = [_tracked(cartpole, r) for r in (a, b, c)]
    BatchedMPPI._resolve_cost_terms(each, cartpole, 3)
    stacked, periodic = BatchedMPPI._resolve_tracking(each, cartpole, 3)
    assert np.array_equal(stacked[:, :, 0], [a, b, c]) and periodic is False
    one, _ = BatchedMPPI._resolve_tracking(each[1], cartpole, 3)            # one CostTerms for the batch
    assert one.shape == (1, 3, 1)
    assert BatchedMPPI._resolve_tracking(CostTerms(cartpole).abs(obs="qvel"), cartpole, 3) is None

    class _Device:
        def __getattr__(self, name):
            raise AssertionError("the device was reached: %s" % name)
    batch = BatchedMPPI.__new__(BatchedMPPI)
    batch.engine, batch.num_episodes = cartpole, 3
    batch.lib = batch.torch = _Device()
    for bad, match in [
        ([each[0], _tracked(cartpole, a + [0.3]), each[2]], "share N"),                     # another N
        ([each[0], each[1], _tracked(cartpole, c, periodic=True)], "periodic"),              # another periodic
        ([each[0], _tracked(cartpole, b, which="site"), each[2]], "rows differ"),            # another tracked-row set
        ([each[0], _tracked(cartpole, b, which=None), each[2]], "rows differ"),              # ... none tracked
    ]:
        with pytest.raises(ValueError, match=match):
            batch.set_cost_terms(bad)
    assert batch._terms is None and batch._track is None
    # env time: num_steps by default; set_track_step is host side
    batch.num_steps = 7
    assert batch._track_bias == 0
    batch.set_track_step(3)
    assert batch._track_bias == -4


# ---- the entry points -----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    bc.check_entry_points(ENTRY_POINTS, abi=4)
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_track"][1]) == 20
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_track_batch"][1]) == 24


def test_track_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)
    f = lib.mjmpc_cost_terms_track

    def call(dtype=_lib.F64, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             advance=0, costs=p):
        return f(dtype, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, ref, n_ref, n_cols, 0, step, 0, advance, costs, None)
    bad = [dict(nobs=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(P=0), dict(H=0), dict(d_obs=0), dict(A=-1, act=None), dict(A=0), dict(n_terms=0), dict(n_terms=129),
           dict(dtype=7), dict(n_ref=0), dict(n_ref=(1 << 20) + 1), dict(n_cols=0), dict(n_cols=129),
           dict(advance=1), dict(advance=1, P=1, H=2), dict(advance=1, P=2, H=1),
           dict(d_obs=8000), dict(dtype=_lib.F32, d_obs=16000)]
    for kw in bad:
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_track:"), (kw, lib.mjmpc_last_error())


def test_track_batch_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced)
    f = lib.mjmpc_cost_terms_track_batch

    def call(dtype=_lib.F64, E=2, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             costs=p, gseq=None, q0=None):
        return f(dtype, E, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, 0, ref, n_ref, n_cols, 0, 0, step, 0, costs, gseq,
                 q0, None)
    bad = [dict(nobs=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(E=0), dict(P=0), dict(H=0), dict(d_obs=0), dict(A=-1, act=None), dict(A=0), dict(n_terms=0), dict(n_terms=129),
           dict(dtype=7), dict(gseq=p), dict(q0=p), dict(n_ref=0), dict(n_ref=(1 << 20) + 1), dict(n_cols=0), dict(n_cols=129),
           dict(d_obs=8000), dict(dtype=_lib.F32, d_obs=15000)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_track_batch"), (kw, lib.mjmpc_last_error())


# ---- the restatement's own indices ----------------------------------------------------------------------------------------
def test_restatement_clamps_and_wraps_on_a_hand_computed_reference():
    N = 3
    assert [tc.ref_row(n, N, False) for n in (-5, -1, 0, 1, 2, 3, 31)] == [0, 0, 0, 1, 2, 2, 2]
    assert [tc.ref_row(n, N, True) for n in (-5, -1, 0, 1, 2, 3, 31)] == [1, 2, 0, 1, 2, 0, 1]
    ref = np.array([[10.0, 1.0], [20.0, 2.0], [30.0, 3.0]])
    # an ABS row on observation entry 0 (column 0 of the reference) and a SQUARE row on action 0 (column 1), weight 1
    table = np.array([[0, 0, 0, 1.0, 10.0, 0, 0, 1], [1, 1, 0, 1.0, 1.0, 0, 0, 2]], np.float64)
    H = 4
    nobs, act, zero = np.zeros((1, H, 1)), np.zeros((1, H, 1)), np.zeros((1, H))
    # base 0: the observation reads rows 1, 2, 3, 4 and the action rows 0, 1, 2, 3
    cost, _ = tc.restate(table, ref, False, 0, nobs, act, zero, False, True)
    assert cost[0].tolist() == [20.0 + 1.0, 30.0 + 4.0, 30.0 + 9.0, 30.0 + 9.0]
    cost, _ = tc.restate(table, ref, True, 0, nobs, act, zero, False, True)
    assert cost[0].tolist() == [20.0 + 1.0, 30.0 + 4.0, 10.0 + 9.0, 20.0 + 1.0]
    # base -2: the observation reads rows -1, 0, 1, 2 and the action rows -2, -1, 0, 1
    cost, _ = tc.restate(table, ref, False, -2, nobs, act, zero, False, True)
    assert cost[0].tolist() == [10.0 + 1.0, 10.0 + 1.0, 20.0 + 1.0, 30.0 + 4.0]
    cost, _ = tc.restate(table, ref, True, -2, nobs, act, zero, False, True)
    assert cost[0].tolist() == [30.0 + 4.0, 10.0 + 9.0, 20.0 + 1.0, 30.0 + 4.0]
    # the table it was given is left alone; an untracked row keeps its target at every step
    assert table[0, 4] == 10.0 and tc.table_at(np.array([[0, 0, 0, 1.0, 7.0, 0, 0, 0]]), ref, True, 5, 2)[0, 4] == 7.0
