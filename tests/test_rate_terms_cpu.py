"""CPU: action-rate rows and one-sided kinds - the builder's ``action_rate=``, ``above`` / ``below`` /
``above_square`` / ``below_square`` and ``outside`` (rows and refusals), the config block, per-episode lists, tables without
either unchanged byte for byte, the restatement on hand-computed values, and the two entry points: declared, bound, exported,
every argument refusal a code and a message with nothing launched."""
import os

import numpy as np
import pytest
import yaml

import batched_cases as bc
import rate_cases as rc
from cost_terms_cases import bound
from mjmpc_amd import _lib
from mjmpc_amd.control import BatchedMPPI
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.envs.cost_terms import KINDS, CostTerms, cost_terms_from_config
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
from mjmpc_amd.models.synthetic import synthetic_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mjmpc_cost_terms_rate", "mjmpc_cost_terms_rate_batch"]


@pytest.fixture(scope="module")
def cartpole():
    return TreeRolloutEngine.host_only(synthetic_raw("cartpole"))


@pytest.fixture(scope="module")
def reacher():
    return ArmRolloutEngine.host_only(reacher7dof_raw())


# ---- the builder ----------------------------------------------------------------------------------------------------------
def test_action_rate_rows_new_kinds_and_outside(reacher):
    lay = reacher.obs_layout()
    q, v = lay["qpos"].start, lay["qvel"].start
    t = CostTerms(reacher)
    assert not t.needs_rate_entry and not t.reads_action_rate
    t.square(action_rate=2, weight=0.5)
    t.norm(action_rate=[0, 3], weight=2.0, target=[0.1, -0.1])
    t.abs(action_rate="all", index=6, weight=0.25, terminal=True)
    t.above(obs="qvel", index=1, target=3.0, weight=1.5)
    t.below(obs=[q + 2], target=-1.0)
    t.above_square(action=1, target=0.5, weight=4.0)
    t.below_square(action_rate=True, index=[0, 1], target=-0.2)
    t.outside(obs="qpos", index=0, low=-2.0, high=2.0, weight=10.0)
    t.outside(obs="qvel", index=[0, 1], high=[3.0, 4.0], squared=False)
    t.outside(action_rate=5, low=-0.3, weight=2.0, terminal=True)
    want = np.array([[1, 2, 2, 0.5, 0.0, 0, 0, 0],
                     [2, 2, 0, 2.0, 0.1, 1, 0, 0], [2, 2, 3, 2.0, -0.1, 1, 0, 0],
                     [0, 2, 6, 0.25, 0.0, 0, 1, 0],
                     [4, 0, v + 1, 1.5, 3.0, 0, 0, 0],
                     [5, 0, q + 2, 1.0, -1.0, 0, 0, 0],
                     [6, 1, 1, 4.0, 0.5, 0, 0, 0],
                     [7, 2, 0, 1.0, -0.2, 0, 0, 0], [7, 2, 1, 1.0, -0.2, 0, 0, 0],
                     [7, 0, q, 10.0, -2.0, 0, 0, 0], [6, 0, q, 10.0, 2.0, 0, 0, 0],
                     [4, 0, v, 1.0, 3.0, 0, 0, 0], [4, 0, v + 1, 1.0, 4.0, 0, 0, 0],
                     [7, 2, 5, 2.0, -0.3, 0, 1, 0]], np.float64)
    assert np.array_equal(t.table(), want)
    assert t.needs_rate_entry and t.reads_action_rate and len(t) == len(want)
    # a one-sided kind alone needs the entry but no previous action; a tracked rate row fills `reserved` like any tracked row
    b = CostTerms(reacher).above(obs="qvel", index=0, target=1.0)
    assert b.needs_rate_entry and not b.reads_action_rate
    r = CostTerms(reacher).square(action_rate=0, reference=[0.0, 0.1, 0.2]).above(action_rate=1, reference=[1.0, 2.0, 3.0])
    assert np.array_equal(r.table()[:, [0, 1, 2, 4, 7]], [[1, 2, 0, 0.0, 1], [4, 2, 1, 1.0, 2]])
    assert r.reference_table().shape == (3, 2) and r.tracked
    # the names of the kinds
    assert [KINDS[k] for k in ("abs", "square", "norm", "cos", "above", "below", "above_square", "below_square")] == list(range(8))


def test_refusals(reacher, cartpole):
    t = CostTerms(reacher)
    for kw in (dict(obs="qvel", action=0), dict(obs="qvel", action_rate=0), dict(action=0, action_rate=0),
               dict(obs="qvel", action=0, action_rate=0), dict()):
        for add in (t.square, t.above, t.below_square):
            with pytest.raises(ValueError, match="exactly one"):
                add(**kw)
        with pytest.raises(ValueError, match="exactly one"):
            t.outside(low=0.0, **kw)
    with pytest.raises(ValueError, match="index 7"):
        t.square(action_rate=7)
    with pytest.raises(ValueError, match="index 1"):
        CostTerms(cartpole).abs(action_rate=1)                      # (the cart-pole has one motor)
    with pytest.raises(ValueError, match="index 7"):
        t.outside(action_rate="all", index=7, low=0.0, high=1.0)
    with pytest.raises(ValueError, match="index 7"):
        CostTerms().square(action_rate=[7]).table(reacher)          # (resolved late)
    with pytest.raises(ValueError, match="drop index"):
        t.square(action_rate=0, index=1)
    with pytest.raises(ValueError, match="unknown action_rate block"):
        t.square(action_rate="every")
    with pytest.raises(ValueError, match="low <= high"):
        t.outside(obs="qpos", index=0, low=1.0, high=0.5)
    with pytest.raises(ValueError, match="low <= high"):
        t.outside(obs="qpos", index=[0, 1], low=[0.0, 1.0], high=[1.0, 0.5])
    with pytest.raises(ValueError, match="low=, high= or both"):
        t.outside(obs="qpos", index=0)
    with pytest.raises(ValueError, match="finite"):
        t.outside(obs="qpos", index=0, low=-np.inf, high=1.0)
    with pytest.raises(ValueError, match="one number per index"):
        t.outside(obs="qpos", index=[0, 1], low=[0.0, 0.0, 0.0], high=5.0)     # (the low rows were taken back too)
    with pytest.raises(TypeError):
        t.above(obs="qvel", low=0.0)
    assert t._terms == []


def test_tables_without_rate_rows_or_new_kinds_are_unchanged_bytes(reacher, cartpole):
    t = CostTerms(reacher)
    t.abs(obs="site_minus_target", index=0, weight=0.7)
    t.square(action=0, weight=0.05)
    t.norm(obs="site_minus_target", weight=4.0, target=[0.1, 0.2, 0.3])
    t.cos(action="all", index=[1, 2], weight=0.3, target=0.2)
    t.square(obs="qvel", index=0, weight=0.5, terminal=True)
    s = reacher.obs_layout()["site_minus_target"].start
    v = reacher.obs_layout()["qvel"].start
    want = np.array([[0, 0, s, 0.7, 0.0, 0, 0, 0], [1, 1, 0, 0.05, 0.0, 0, 0, 0],
                     [2, 0, s, 4.0, 0.1, 1, 0, 0], [2, 0, s + 1, 4.0, 0.2, 1, 0, 0], [2, 0, s + 2, 4.0, 0.3, 1, 0, 0],
                     [3, 1, 1, 0.3, 0.2, 0, 0, 0], [3, 1, 2, 0.3, 0.2, 0, 0, 0],
                     [1, 0, v, 0.5, 0.0, 0, 1, 0]], np.float64)
    assert t.table().tobytes() == want.tobytes()
    assert not t.needs_rate_entry and not t.reads_action_rate
    assert not CostTerms.builtin_reach(cartpole).needs_rate_entry
    tracked = CostTerms(cartpole).square(obs="qpos", index=0, reference=[0.0, 0.4])
    assert not tracked.needs_rate_entry


# ---- the config block -----------------------------------------------------------------------------------------------------
BLOCK = dict(keep_builtin=False, terms=[
    dict(kind="norm", obs="site_minus_target", weight=5.0),
    dict(kind="square", action_rate=0, weight=0.1),
    dict(kind="outside", obs="qpos", index=0, low=-2.0, high=2.0, weight=10.0),
    dict(kind="above", obs="qvel", index=1, target=3.0, weight=0.5, terminal=True),
    dict(kind="outside", action_rate="all", high=0.5, squared=False),
])


def test_config_block_parses_to_its_table(cartpole):
    lay = cartpole.obs_layout()
    s, q, v = lay["site_minus_target"].start, lay["qpos"].start, lay["qvel"].start
    t = cost_terms_from_config(BLOCK, cartpole)
    want = np.array([[2, 0, s, 5.0, 0, 1, 0, 0], [2, 0, s + 1, 5.0, 0, 1, 0, 0], [2, 0, s + 2, 5.0, 0, 1, 0, 0],
                     [1, 2, 0, 0.1, 0, 0, 0, 0],
                     [7, 0, q, 10.0, -2.0, 0, 0, 0], [6, 0, q, 10.0, 2.0, 0, 0, 0],
                     [4, 0, v + 1, 0.5, 3.0, 0, 1, 0],
                     [4, 2, 0, 1.0, 0.5, 0, 0, 0]], np.float64)
    assert isinstance(t, CostTerms) and np.array_equal(t.table(), want) and t.needs_rate_entry and t.reads_action_rate
    for broken in (dict(kind="huber", obs="qvel"), dict(kind="square", action_rate=0, wieght=1),
                   dict(kind="outside", obs="qpos", index=0, low=0.0, target=1.0),
                   dict(kind="above", obs="qvel", low=0.0), dict(kind="square", action=0, action_rate=0),
                   dict(kind="outside", obs="qpos", index=0, low=1.0, high=0.0), dict(kind="outside", obs="qpos", index=0),
                   dict(kind="square", action_rate=1)):
        with pytest.raises(ValueError):
            cost_terms_from_config(dict(terms=[broken]), cartpole)


def test_per_episode_lists_give_one_table_per_episode(cartpole):
    E = 3
    block = dict(terms=[
        dict(kind="square", action_rate=0, weight=[0.0, 0.1, 1.0]),
        dict(kind="outside", obs="qpos", index=0, low=[-1.0, -2.0, -3.0], high=2.0, weight=[1.0, 2.0, 3.0]),
        dict(kind="below", obs="qvel", index=0, target=[0.1, 0.2, 0.3]),
    ])
    each = cost_terms_from_config(block, cartpole, num_episodes=E)
    assert isinstance(each, list) and len(each) == E
    tables = np.stack([t.table() for t in each])
    assert np.array_equal(tables[:, 0, 3], [0.0, 0.1, 1.0])
    assert np.array_equal(tables[:, 1, 4], [-1.0, -2.0, -3.0]) and np.array_equal(tables[:, 2, 4], [2.0, 2.0, 2.0])
    assert np.array_equal(tables[:, 1, 3], [1.0, 2.0, 3.0]) and np.array_equal(tables[:, 2, 3], [1.0, 2.0, 3.0])
    assert np.array_equal(tables[:, 3, 4], [0.1, 0.2, 0.3])
    assert np.array_equal(tables[0][:, [0, 1]], [[1, 2], [7, 0], [6, 0], [5, 0]])
    stacked, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, E)
    assert stacked.shape == (E, 4, 8) and not keep and reads
    # the episodes share the rows: a rate row against an action row, a bound against its mirror image
    other = CostTerms(cartpole).square(action=0, weight=0.1)
    other.outside(obs="qpos", index=0, low=-1.0, high=2.0).below(obs="qvel", index=0, target=0.1)
    with pytest.raises(ValueError, match="rows differ"):
        BatchedMPPI._resolve_cost_terms([each[0], other, each[2]], cartpole, E)
    # one CostTerms without a list as ever; a weight list of another length is refused
    assert isinstance(cost_terms_from_config(BLOCK, cartpole, num_episodes=E), CostTerms)
    with pytest.raises(ValueError, match="one weight per episode"):
        cost_terms_from_config(dict(terms=[dict(kind="square", action_rate=0, weight=[1.0, 2.0])]), cartpole, num_episodes=E)


@pytest.mark.parametrize("name,E", [("cartpole_smooth_gpu.yml", None), ("cartpole_smooth_batch_gpu.yml", 4)])
def test_example_configs_parse(cartpole, name, E):
    with open(os.path.join(ROOT, "examples", "configs", name)) as f:
        cfg = yaml.safe_load(f)
    terms = cost_terms_from_config(cfg["cost_terms"], cartpole, num_episodes=E)
    each = terms if E else [terms]
    assert len(each) == (E or 1)
    for t in each:
        table = t.table()
        assert t.needs_rate_entry and t.reads_action_rate
        assert np.any((table[:, 0] == 1) & (table[:, 1] == 2) & (table[:, 2] == 0))         # a square on action rate 0
        q = cartpole.obs_layout()["qpos"].start
        assert np.any((table[:, 0] >= 6) & (table[:, 2] == q) & (table[:, 1] == 0))          # a band on the cart position
    if E:
        assert len({t.table()[:, 3].tobytes() for t in each}) == E                          # a rate weight per episode


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_on_hand_computed_values():
    """2 particles x 3 steps x 1 action.  Particle 0: actions 1, 4, 2 -> rates (1 - prev), 3, -2; particle 1: 0, -1, -1."""
    act = np.array([[[1.0], [4.0], [2.0]], [[0.0], [-1.0], [-1.0]]])
    nobs = np.array([[[0.5], [2.5], [-1.0]], [[3.0], [0.0], [1.0]]])
    zero = np.zeros((2, 3))
    assert np.array_equal(rc.rates(act, np.array([0.25]))[:, :, 0], [[0.75, 3.0, -2.0], [-0.25, -1.0, 0.0]])
    assert np.array_equal(rc.rates(act, np.array([np.nan]))[:, :, 0], [[0.0, 3.0, -2.0], [0.0, -1.0, 0.0]])
    assert np.array_equal(rc.rates(act, None)[:, :, 0], [[0.0, 3.0, -2.0], [0.0, -1.0, 0.0]])
    assert np.array_equal(rc.rates(act, np.array([[0.25], [np.nan]]))[:, :, 0], [[0.75, 3.0, -2.0], [0.0, -1.0, 0.0]])
    # one SQUARE rate row of weight 2: 2 rate^2
    sq = np.array([[1, 2, 0, 2.0, 0.0, 0, 0, 0]], np.float64)
    cost, mag = rc.restate(sq, nobs, act, np.array([0.25]), zero, False, True)
    assert np.array_equal(cost, [[2 * 0.5625, 18.0, 8.0], [2 * 0.0625, 2.0, 0.0]]) and np.array_equal(mag, cost)
    cost, _ = rc.restate(sq, nobs, act, np.array([np.nan]), zero, False, True)
    assert np.array_equal(cost, [[0.0, 18.0, 8.0], [0.0, 2.0, 0.0]])
    # the four one-sided kinds on the observation with the bound 1: r = -0.5, 1.5, -2 and 2, -1, 0
    for kind, want in ((rc.ABOVE, [[0, 1.5, 0], [2, 0, 0]]), (rc.BELOW, [[0.5, 0, 2], [0, 1, 0]]),
                       (rc.ABOVE_SQUARE, [[0, 2.25, 0], [4, 0, 0]]), (rc.BELOW_SQUARE, [[0.25, 0, 4], [0, 1, 0]])):
        cost, _ = rc.restate(np.array([[kind, 0, 0, 1.0, 1.0, 0, 0, 0]], np.float64), nobs, act, None, zero, False, True)
        assert np.array_equal(cost, np.array(want, np.float64)), kind
    # a rate row with a goal (the rate should be 1), an ABOVE on the rate, the incoming cost kept, a terminal row at t = 2 only,
    # and a NORM group over the action and its rate: sqrt(u^2 + du^2)
    table = np.array([[0, 2, 0, 1.0, 1.0, 0, 0, 0], [4, 2, 0, 10.0, 2.0, 0, 0, 0], [1, 0, 0, 1.0, 0.0, 0, 1, 0],
                      [2, 1, 0, 1.0, 0.0, 7, 0, 0], [2, 2, 0, 1.0, 0.0, 7, 0, 0]], np.float64)
    inc = np.array([[1.0, np.inf, 0.0], [0.0, 0.0, np.nan]])
    cost, mag = rc.restate(table, nobs, act, np.array([1.0]), inc, True, True)
    assert cost[0, 0] == 1.0 + 1.0 + 0.0 + 1.0 and np.isposinf(cost[0, 1]) and np.isposinf(cost[1, 2])
    assert cost[0, 2] == 3.0 + 0.0 + 1.0 + np.sqrt(8.0)
    assert cost[1, 0] == 2.0 + 0.0 + np.sqrt(1.0) and cost[1, 1] == 2.0 + 0.0 + np.sqrt(2.0)
    assert mag[0, 1] == 2.0 + 10.0 + np.sqrt(25.0) and np.all(bound(table, cost, mag, True)[np.isfinite(cost)] > 0)
    # a tracked rate row reads the action-time row b + t; a tracked observation row b + t + 1
    ref = np.array([[0.0, 10.0], [1.0, 20.0], [2.0, 30.0]])
    tracked = np.array([[0, 2, 0, 1.0, 0.0, 0, 0, 1], [0, 0, 0, 1.0, 10.0, 0, 0, 2]], np.float64)
    cost, _ = rc.restate(tracked, np.zeros((1, 3, 1)), np.zeros((1, 3, 1)), None, np.zeros((1, 3)), False, True, ref, False, 0)
    assert cost[0].tolist() == [0.0 + 20.0, 1.0 + 30.0, 2.0 + 30.0]
    # without rate rows or new kinds it is cost_terms_cases.restate
    from cost_terms_cases import random_table, restate
    rng = np.random.default_rng(5)
    old = random_table(rng, 12, 4, 2)
    o, a, c = rng.uniform(-2, 2, (3, 4, 4)), rng.uniform(-2, 2, (3, 4, 2)), rng.uniform(-1, 1, (3, 4))
    for x, y in zip(rc.restate(old, o, a, np.array([0.1, 0.2]), c, True, True), restate(old, o, a, c, True, True)):
        assert np.array_equal(x, y)


def test_random_extended_tables_hold_every_kind_and_source():
    rng = np.random.default_rng(9)
    for K, d_obs, A in ((5, 10, 1), (37, 43, 7), (128, 43, 7), (20, 130, 3)):
        table = rc.random_extended_table(rng, K, d_obs, A)
        assert table.shape == (K, 8) and np.any(table[:, 1] == 2)
        assert set(table[:, 0]) <= set(map(float, range(8))) and np.any(table[:, 0] >= 4)
        if K >= 20:                 # (K = 5 closes with a norm group of three rows: two rows are left for the new kinds)
            assert set(table[:, 0]) >= {4.0, 5.0, 6.0, 7.0}
        act = table[:, 1] != 0
        assert np.all(table[act, 2] < A) and np.all(table[~act, 2] < d_obs) and np.all(table[:, 2] >= 0)
        if K >= 37:
            assert set(table[:, 1]) == {0.0, 1.0, 2.0}
            norm = table[table[:, 0] == 2]
            assert any(len(set(norm[norm[:, 5] == g][:, 1])) > 1 for g in set(norm[:, 5]))     # a group that mixes sources


# ---- the entry points -----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    bc.check_entry_points(ENTRY_POINTS, abi=4)
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_rate"][1]) == 21
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_rate_batch"][1]) == 26
    # the four existing entries keep their signatures
    assert [len(_lib.SIGNATURES[n][1]) for n in ("mjmpc_cost_terms", "mjmpc_cost_terms_batch", "mjmpc_cost_terms_track",
                                                 "mjmpc_cost_terms_track_batch")] == [13, 17, 20, 24]


def test_rate_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)
    f = lib.mjmpc_cost_terms_rate

    def call(dtype=_lib.F64, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             advance=0, prev=p, costs=p):
        return f(dtype, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, ref, n_ref, n_cols, 0, step, 0, advance, prev, costs, None)
    bad = [dict(nobs=None), dict(act=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(P=0), dict(H=0), dict(d_obs=0), dict(A=0), dict(A=-1), dict(n_terms=0), dict(n_terms=129),
           dict(dtype=7), dict(n_ref=0), dict(n_ref=(1 << 20) + 1), dict(n_cols=0), dict(n_cols=129),
           dict(advance=1), dict(advance=1, P=1, H=2), dict(advance=1, P=2, H=1), dict(advance=1, ref=None, step=None),
           dict(d_obs=8000), dict(dtype=_lib.F32, d_obs=16000), dict(d_obs=3, A=3900), dict(ref=None, step=None, A=3900)]
    for kw in bad:
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_rate:"), (kw, lib.mjmpc_last_error())


def test_rate_batch_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced)
    f = lib.mjmpc_cost_terms_rate_batch

    def call(dtype=_lib.F64, E=2, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             prev=p, advance_prev=0, costs=p, gseq=None, q0=None):
        return f(dtype, E, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, 0, ref, n_ref, n_cols, 0, 0, step, 0, prev,
                 advance_prev, costs, gseq, q0, None)
    bad = [dict(nobs=None), dict(act=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(E=0), dict(P=0), dict(H=0), dict(d_obs=0), dict(A=0), dict(A=-1), dict(n_terms=0), dict(n_terms=129),
           dict(dtype=7), dict(gseq=p), dict(q0=p), dict(n_ref=0), dict(n_ref=(1 << 20) + 1), dict(n_cols=0), dict(n_cols=129),
           dict(advance_prev=1), dict(advance_prev=1, P=1, H=2), dict(advance_prev=1, P=2, H=1),
           dict(advance_prev=1, ref=None, step=None), dict(d_obs=8000), dict(dtype=_lib.F32, d_obs=15000), dict(A=3600)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_rate_batch:"), (kw, lib.mjmpc_last_error())
