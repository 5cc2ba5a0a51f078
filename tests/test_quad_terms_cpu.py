"""CPU: quadratic forms and signed linear rows - the builder's ``quadratic`` (block, index-list and ``parts=``
forms, the symmetrised pool, every refusal) and ``linear``, which entry a table needs, the restatement against three
anchors it does not share code with, the config block and the two example configs, per-episode tables with one pool, and the
two entry points: declared, bound, exported, every argument refusal a code and a message with nothing launched."""
import os

import numpy as np
import pytest
import yaml

import batched_cases as bc
import quad_cases as qc
import rate_cases as rc
from cost_terms_cases import bound, restate
from mjmpc_amd import _lib
from mjmpc_amd.control import BatchedMPPI
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.envs.cost_terms import KIND_LINEAR, KIND_QUAD, KINDS, CostTerms, cost_terms_from_config
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
from mjmpc_amd.models.synthetic import synthetic_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mjmpc_cost_terms_quad", "mjmpc_cost_terms_quad_batch"]


@pytest.fixture(scope="module")
def cartpole():
    return TreeRolloutEngine.host_only(synthetic_raw("cartpole"))


@pytest.fixture(scope="module")
def reacher():
    return ArmRolloutEngine.host_only(reacher7dof_raw())


# ---- the builder ----------------------------------------------------------------------------------------------------------
def test_quadratic_rows_and_pool(reacher):
    lay = reacher.obs_layout()
    q, v = lay["qpos"].start, lay["qvel"].start
    rng = np.random.default_rng(1)
    M7, M2, M4 = rng.uniform(-1, 1, (7, 7)), np.array([[1.0, 4.0], [0.0, 3.0]]), rng.uniform(-1, 1, (4, 4))
    t = CostTerms(reacher)
    assert not t.needs_quad_entry and t.quad_table() is None
    t.quadratic(obs="qvel", matrix=M7, weight=0.5, terminal=True)                                   # a block
    t.quadratic(obs=[q + 2, q], matrix=M2, target=[0.1, -0.1])                                      # an index list
    t.quadratic(action_rate="all", index=[1, 3, 5], matrix=[1.0, 2.0, 3.0], weight=2.0)              # [n]: a diagonal
    t.quadratic(parts=[dict(obs="qpos", index=[0, 1], target=0.25), dict(action=6), dict(action_rate=[0])], matrix=M4,
                weight=-1.5)
    t.linear(obs="qvel", index=1, weight=-2.0, target=0.5)
    t.linear(action=[0, 1], weight=0.25, terminal=True)
    want = np.array([[8, 0, v + i, 0.5, 0.0, 1, 1, 0] for i in range(7)]
                    + [[8, 0, q + 2, 1.0, 0.1, 2, 0, 0], [8, 0, q, 1.0, -0.1, 2, 0, 0]]
                    + [[8, 2, i, 2.0, 0.0, 3, 0, 0] for i in (1, 3, 5)]
                    + [[8, 0, q, -1.5, 0.25, 4, 0, 0], [8, 0, q + 1, -1.5, 0.25, 4, 0, 0], [8, 1, 6, -1.5, 0.0, 4, 0, 0],
                       [8, 2, 0, -1.5, 0.0, 4, 0, 0]]
                    + [[9, 0, v + 1, -2.0, 0.5, 0, 0, 0], [9, 1, 0, 0.25, 0.0, 0, 1, 0], [9, 1, 1, 0.25, 0.0, 0, 1, 0]], np.float64)
    assert np.array_equal(t.table(), want) and len(t) == len(want)
    pool = t.quad_table()
    assert pool.dtype == np.float64 and pool.shape == (49 + 4 + 9 + 16,)
    assert np.array_equal(pool[:49].reshape(7, 7), 0.5 * (M7 + M7.T))                               # symmetrised
    assert np.array_equal(pool[49:53], [1.0, 2.0, 2.0, 3.0])
    assert np.array_equal(pool[53:62].reshape(3, 3), np.diag([1.0, 2.0, 3.0]))
    assert np.array_equal(pool[62:].reshape(4, 4), 0.5 * (M4 + M4.T))
    assert [(k, n, off) for k, n, off in qc.groups(t.table())] == [(0, 7, 0), (7, 2, 49), (9, 3, 53), (12, 4, 62)]
    assert t.needs_quad_entry and t.reads_action_rate
    assert KINDS["quadratic"] == KIND_QUAD == 8 and KINDS["linear"] == KIND_LINEAR == 9
    # fresh group ids: two neighbouring groups over the same rows, and a norm between quadratics, never merge
    n = CostTerms(reacher).quadratic(action=[0, 1], matrix=np.eye(2)).quadratic(action=[0, 1], matrix=np.eye(2))
    n.norm(action=[0, 1]).quadratic(action=[2], matrix=[[2.0]])
    assert n.table()[:, 5].tolist() == [1, 1, 2, 2, 3, 3, 4] and [g[1] for g in qc.groups(n.table())] == [2, 2, 1]
    # a tracked part fills `reserved` like any tracked row; the other parts keep their constant targets
    r = CostTerms(reacher).quadratic(parts=[dict(obs="qpos", index=[0, 1], reference=[[0.0, 1.0], [0.5, 1.5]]),
                                            dict(action=0, target=0.3)], matrix=np.eye(3), periodic=True)
    assert np.array_equal(r.table()[:, [0, 1, 2, 4, 7]], [[8, 0, q, 0.0, 1], [8, 0, q + 1, 1.0, 2], [8, 1, 0, 0.3, 0]])
    assert r.reference_table().shape == (2, 2) and r.tracked and r.periodic
    # resolved late, without an engine
    late = CostTerms().quadratic(obs=[3, 4], matrix=[[1.0, 0.5], [0.5, 1.0]])
    assert np.array_equal(late.table(reacher)[:, [0, 2, 5]], [[8, 3, 1], [8, 4, 1]]) and late.quad_table(reacher).shape == (4,)


def test_which_entry_a_table_needs(reacher, cartpole):
    old = CostTerms(reacher).abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0)
    assert not old.needs_quad_entry and not old.needs_rate_entry
    rate = CostTerms(reacher).square(action_rate=0).above(obs="qvel", index=0)
    assert not rate.needs_quad_entry and rate.needs_rate_entry
    assert not CostTerms.builtin_reach(cartpole).needs_quad_entry
    quad = CostTerms(reacher).quadratic(action=[0, 1], matrix=np.eye(2))
    assert quad.needs_quad_entry and not quad.needs_rate_entry and not quad.reads_action_rate
    lin = CostTerms(reacher).linear(obs="qvel", index=0, weight=-1.0)
    assert lin.needs_quad_entry and not lin.needs_rate_entry and lin.quad_table() is None
    both = CostTerms(reacher).quadratic(action_rate=[0, 1], matrix=np.eye(2)).below(obs="qvel", index=0)
    assert both.needs_quad_entry and both.needs_rate_entry and both.reads_action_rate


def test_refusals(reacher):
    t = CostTerms(reacher)
    eye = np.eye(2)
    with pytest.raises(ValueError, match="square"):
        t.quadratic(action=[0, 1], matrix=np.ones((2, 3)))                      # non-square
    with pytest.raises(ValueError, match="square"):
        t.quadratic(action=[0, 1], matrix=np.ones((2, 2, 2)))
    with pytest.raises(ValueError, match="2 x 2, the group has 3 rows"):
        t.quadratic(action=[0, 1, 2], matrix=eye)                               # wrong size
    with pytest.raises(ValueError, match="7 x 7, the group has 14 rows"):
        t.quadratic(parts=[dict(obs="qpos"), dict(obs="qvel")], matrix=np.eye(7))
    with pytest.raises(ValueError, match="finite"):
        t.quadratic(action=[0, 1], matrix=[[1.0, np.nan], [0.0, 1.0]])          # non-finite
    with pytest.raises(ValueError, match="finite"):
        t.quadratic(action=[0, 1], matrix=[np.inf, 1.0])
    with pytest.raises(ValueError, match="at most 32"):
        t.quadratic(obs=list(range(20)) + list(range(13)), matrix=np.eye(33))   # n = 33
    with pytest.raises(ValueError, match="not both"):
        t.quadratic(action=[0, 1], matrix=eye, target=0.5, reference=[0.0, 1.0])        # target and reference
    with pytest.raises(ValueError, match="not both"):
        t.quadratic(parts=[dict(action=0), dict(action=1, target=0.5, reference=[0.0, 1.0])], matrix=eye)
    with pytest.raises(ValueError, match="needs matrix"):
        t.quadratic(action=[0, 1])
    with pytest.raises(ValueError, match="exactly one"):
        t.quadratic(obs="qvel", action=0, matrix=eye)
    with pytest.raises(ValueError, match="go into the parts"):
        t.quadratic(obs="qvel", parts=[dict(action=0)], matrix=[1.0])
    with pytest.raises(ValueError, match="a part takes"):
        t.quadratic(parts=[dict(action=0, weight=2.0)], matrix=[1.0])
    with pytest.raises(ValueError, match="index 7"):
        t.quadratic(parts=[dict(action=0), dict(action_rate=7)], matrix=eye)
    with pytest.raises(ValueError, match="periodic"):
        t.quadratic(action=[0, 1], matrix=eye, periodic=True)
    with pytest.raises(ValueError, match="exactly one"):
        t.linear(obs="qvel", action=0)
    assert t._terms == [] and t._periodic is None                               # (a refused group leaves no part behind)
    # row 129: four groups of 32 rows fill the table; one more row is refused and the table stays
    for _ in range(4):
        t.quadratic(obs=list(range(20)) + list(range(12)), matrix=np.eye(32))
    assert len(t) == 128 and t.quad_table().shape == (4096,)
    with pytest.raises(ValueError, match="at most 128"):
        t.linear(action=0)
    with pytest.raises(ValueError, match="at most 128"):
        t.quadratic(parts=[dict(action=0)], matrix=[1.0])
    assert len(t) == 128 and t.table().shape == (128, 8)
    # resolved late: the matrix meets its rows in table() at the latest
    with pytest.raises(ValueError, match="7 x 7, the group has 14 rows"):
        CostTerms().quadratic(parts=[dict(obs="qpos"), dict(obs="qvel")], matrix=np.eye(7)).table(reacher)


def test_tables_without_the_new_kinds_are_unchanged_bytes(reacher):
    t = CostTerms(reacher)
    t.abs(obs="site_minus_target", index=0, weight=0.7)
    t.norm(obs="site_minus_target", weight=4.0, target=[0.1, 0.2, 0.3])
    t.below_square(action_rate=0, target=-0.2)
    s = reacher.obs_layout()["site_minus_target"].start
    want = np.array([[0, 0, s, 0.7, 0.0, 0, 0, 0], [2, 0, s, 4.0, 0.1, 1, 0, 0], [2, 0, s + 1, 4.0, 0.2, 1, 0, 0],
                     [2, 0, s + 2, 4.0, 0.3, 1, 0, 0], [7, 2, 0, 1.0, -0.2, 0, 0, 0]], np.float64)
    assert t.table().tobytes() == want.tobytes() and t.needs_rate_entry and not t.needs_quad_entry


# ---- the restatement: three anchors ---------------------------------------------------------------------------------------
def _data(rng, Pn, Hn, d_obs, A):
    return rng.uniform(-3, 3, (Pn, Hn, d_obs)), rng.uniform(-3, 3, (Pn, Hn, A)), rng.uniform(-1, 1, (Pn, Hn))


def test_a_diagonal_matrix_is_the_square_rows(reacher):
    """w sum_i Q_ii r_i^2 against SQUARE rows of weight w Q_ii (``rate_cases.restate``), within the two bounds added."""
    rng = np.random.default_rng(2)
    d_obs, A = reacher.model.d_obs, 7
    nobs, act, cin = _data(rng, 5, 4, d_obs, A)
    prev = rng.uniform(-1, 1, A)
    diag, w, target = rng.uniform(-2, 2, 6), -0.7, rng.uniform(-1, 1, 6)
    parts = [dict(obs="qvel", index=[0, 3], target=target[:2]), dict(action=[1, 2], target=target[2:4]),
             dict(action_rate=[0, 6], target=target[4:])]
    quad = CostTerms(reacher).quadratic(parts=parts, matrix=diag, weight=w, terminal=True)
    rows = CostTerms(reacher)
    singles = [dict(obs="qvel", index=0), dict(obs="qvel", index=3), dict(action=1), dict(action=2), dict(action_rate=0),
               dict(action_rate=6)]
    for i, one in enumerate(singles):
        rows.square(weight=w * diag[i], target=target[i], terminal=True, **one)
    assert len(rows) == 6 and np.array_equal(rows.table()[:, [1, 2, 4]], quad.table()[:, [1, 2, 4]])
    for terminal in (False, True):
        got, gmag = qc.restate(quad.table(), quad.quad_table(), nobs, act, prev, cin, True, terminal)
        want, wmag = rc.restate(rows.table(), nobs, act, prev, cin, True, terminal)
        tol = qc.bound(quad.table(), got, gmag, False) + bound(rows.table(), want, wmag, False)
        assert np.all(np.abs(got - want) <= tol) and np.all(tol < 1e-10)
        assert np.array_equal(got[:, :-1], cin[:, :-1]) and (np.array_equal(got[:, -1], cin[:, -1]) != terminal)


def test_the_identity_is_the_norm_squared(reacher):
    """I over ``site_minus_target`` with weight 1 against the NORM group's value, squared."""
    rng = np.random.default_rng(3)
    nobs, act, cin = _data(rng, 6, 3, reacher.model.d_obs, 7)
    quad = CostTerms(reacher).quadratic(obs="site_minus_target", matrix=np.eye(3), target=[0.1, 0.2, 0.3])
    norm = CostTerms(reacher).norm(obs="site_minus_target", target=[0.1, 0.2, 0.3])
    got, gmag = qc.restate(quad.table(), quad.quad_table(), nobs, act, None, cin, False, True)
    root, rmag = restate(norm.table(), nobs, act, cin, False, True)
    # (d(x^2) = 2 x dx: the norm's bound, through the square, and one more rounding for the product)
    tol = qc.bound(quad.table(), got, gmag, False) + 2.0 * root * bound(norm.table(), root, rmag, False) + 2.0 ** -52 * root * root
    assert np.all(np.abs(got - root * root) <= tol) and np.all(got > 0) and np.all(tol < 1e-12)


def test_linear_minus_its_mirror_image_is_zero(reacher):
    """``linear`` with weight w on v - g and ``linear`` with weight -w on the negated entry and goal: w r + (-w)(-r)...
    the second is w r again, so the first MINUS it is exactly zero - and each alone is w r with its sign."""
    rng = np.random.default_rng(4)
    nobs, act, cin = _data(rng, 4, 3, reacher.model.d_obs, 7)
    zero = np.zeros_like(cin)
    w, g = 1.75, 0.4
    a = CostTerms(reacher).linear(action=2, weight=w, target=g)
    b = CostTerms(reacher).linear(action=2, weight=-w, target=-g)
    one, _ = qc.restate(a.table(), np.zeros(1), nobs, act, None, zero, False, True)
    other, _ = qc.restate(b.table(), np.zeros(1), nobs, -act, None, zero, False, True)
    assert np.array_equal(one - other, zero) and np.array_equal(one, w * (act[:, :, 2] - g))
    assert np.any(one < 0) and np.any(one > 0)                                  # signed
    both = CostTerms(reacher).linear(action=2, weight=w, target=g).linear(action=2, weight=-w, target=g)
    total, mag = qc.restate(both.table(), np.zeros(1), nobs, act, None, zero, False, True)
    assert np.array_equal(total, zero) and np.array_equal(mag, 2 * np.abs(one))


def test_restatement_on_hand_computed_values():
    """Two groups and the pool's offsets: r = (1, 2) with Q = [[1, 2], [2, -1]] is 1 + 8 - 4 = 5 (indefinite matrices count
    with their sign); r = (3) with Q = [[0.5]] is 4.5, found behind the first group's four entries."""
    table = np.array([[8, 0, 0, 2.0, 0.0, 1, 0, 0], [8, 1, 0, 99.0, 1.0, 1, 0, 0], [9, 0, 1, -1.0, 0.0, 0, 0, 0],
                      [8, 2, 0, 1.0, 0.0, 2, 1, 0]], np.float64)
    pool = np.array([1.0, 2.0, 2.0, -1.0, 0.5])
    nobs = np.array([[[1.0, 10.0], [1.0, 20.0]]])
    act = np.array([[[3.0], [6.0]]])
    cost, mag = qc.restate(table, pool, nobs, act, np.array([1.0]), np.zeros((1, 2)), False, True)
    assert cost.tolist() == [[2.0 * 5.0 - 10.0, 2.0 * (1 + 4 * 5 - 25) - 20.0 + 4.5]]
    assert mag.tolist() == [[2.0 * 13.0 + 10.0, 2.0 * (1 + 20 + 25) + 20.0 + 4.5]]
    cost, _ = qc.restate(table, pool, nobs, act, np.array([1.0]), np.array([[np.inf, 1.0]]), True, False)
    assert np.isposinf(cost[0, 0]) and cost[0, 1] == 1.0 + 2.0 * (1 + 20 - 25) - 20.0
    assert qc.n_max(table) == 2 and qc.bound(table, cost, mag, False)[0, 1] == 4.0 * (4 + 4 + 4) * 2.0 ** -52 * mag[0, 1]
    # without new rows it is rate_cases.restate
    rng = np.random.default_rng(5)
    old = rc.random_extended_table(rng, 12, 4, 2)
    o, a, c = _data(rng, 3, 4, 4, 2)
    for x, y in zip(qc.restate(old, np.zeros(1), o, a, np.array([0.1, 0.2]), c, True, True),
                    rc.restate(old, o, a, np.array([0.1, 0.2]), c, True, True)):
        assert np.array_equal(x, y)


def test_random_quad_tables_hold_every_kind_and_source():
    rng = np.random.default_rng(9)
    for K, d_obs, A, sizes in ((5, 10, 1, [2, 1]), (37, 43, 7, None), (128, 43, 7, [32] * 4), (40, 85, 3, None)):
        table = qc.random_quad_table(rng, K, d_obs, A, sizes)
        gs = qc.groups(table)
        assert table.shape == (K, 8) and gs[-1][0] + gs[-1][1] == K            # a group closes the table
        assert all(1 <= n <= 32 for _, n, _ in gs) and len(set(table[[k for k, _, _ in gs], 5])) == len(gs)
        assert qc.random_pool(rng, table).shape == (sum(n * n for _, n, _ in gs),)
        act = table[:, 1] != 0
        assert np.all(table[act, 2] < A) and np.all(table[~act, 2] < d_obs) and np.all(table[:, 2] >= 0)
        if sizes == [32] * 4:
            assert np.all(table[:, 0] == 8) and gs[-1][2] + 32 * 32 == 4096
        elif sizes is None:
            assert set(table[:, 0]) == set(map(float, range(10)))               # all ten kinds
            quad = table[table[:, 0] == 8]
            assert set(quad[:, 1]) == {0.0, 1.0, 2.0}
            # taking the new rows out merges no NORM groups: the ids of neighbours differ
            old = table[table[:, 0] < 8]
            norm_runs = [g for k, g in enumerate(old[:, 5]) if old[k, 0] == 2 and (k == 0 or old[k - 1, 5] != g or old[k - 1, 0] != 2)]
            assert len(norm_runs) == len(set(norm_runs))


# ---- the config block -----------------------------------------------------------------------------------------------------
def test_config_block_parses_to_its_table(cartpole):
    lay = cartpole.obs_layout()
    q, v = lay["qpos"].start, lay["qvel"].start
    block = dict(terms=[
        dict(kind="quadratic", parts=[dict(obs="qpos"), dict(obs="qvel", index=1, target=0.5), dict(action=0)],
             matrix=[[1.0, 0.0, 0.5, 0.0], [0.0, 2.0, 0.0, 0.0], [0.5, 0.0, 3.0, 0.25], [0.0, 0.0, 0.25, 4.0]], weight=0.5),
        dict(kind="linear", obs="qvel", index=0, weight=-1.0),
        dict(kind="quadratic", obs="qvel", matrix=[1.0, 2.0], terminal=True),
    ])
    t = cost_terms_from_config(block, cartpole)
    want = np.array([[8, 0, q, 0.5, 0, 1, 0, 0], [8, 0, q + 1, 0.5, 0, 1, 0, 0], [8, 0, v + 1, 0.5, 0.5, 1, 0, 0],
                     [8, 1, 0, 0.5, 0, 1, 0, 0], [9, 0, v, -1.0, 0, 0, 0, 0],
                     [8, 0, v, 1.0, 0, 2, 1, 0], [8, 0, v + 1, 1.0, 0, 2, 1, 0]], np.float64)
    assert isinstance(t, CostTerms) and np.array_equal(t.table(), want) and t.needs_quad_entry
    assert np.array_equal(t.quad_table()[:16].reshape(4, 4), block["terms"][0]["matrix"])
    assert np.array_equal(t.quad_table()[16:], [1.0, 0.0, 0.0, 2.0])
    for broken in (dict(kind="quadratic", obs="qvel"), dict(kind="quadratic", obs="qvel", matrix=[1.0, 2.0, 3.0]),
                   dict(kind="square", obs="qvel", matrix=[1.0, 2.0]), dict(kind="linear", obs="qvel", parts=[dict(obs="qpos")]),
                   dict(kind="quadratic", parts=[dict(obs="qpos", kind="square")], matrix=[1.0, 1.0]),
                   dict(kind="quadratic", obs="qvel", matrix=[[1.0, 2.0]])):
        with pytest.raises(ValueError):
            cost_terms_from_config(dict(terms=[broken]), cartpole)


@pytest.mark.parametrize("name,E", [("cartpole_lqr_gpu.yml", None), ("cartpole_lqr_batch_gpu.yml", 4)])
def test_example_configs_parse(cartpole, name, E):
    with open(os.path.join(ROOT, "examples", "configs", name)) as f:
        cfg = yaml.safe_load(f)
    assert (cfg["n_episodes"] if E else 1) == (E or 1)
    terms = cost_terms_from_config(cfg["cost_terms"], cartpole, num_episodes=E)
    each = terms if E else [terms]
    assert len(each) == (E or 1)
    for t in each:
        table, pool = t.table(), t.quad_table()
        assert t.needs_quad_entry and [n for _, n, _ in qc.groups(table)] == [4, 1, 4] and pool.shape == (33,)
        Q, P = pool[:16].reshape(4, 4), pool[17:].reshape(4, 4)
        assert np.array_equal(Q, Q.T) and np.array_equal(P, P.T) and np.count_nonzero(Q - np.diag(np.diag(Q))) == 4
        assert np.linalg.eigvalsh(Q).min() > 0 and np.linalg.eigvalsh(P).min() > 0
        assert np.all(table[-4:, 6] == 1) and np.all(table[:4, 6] == 0)                     # the Riccati form is terminal
        assert np.array_equal(table[[0, 1, 2, 3], 2], table[[-4, -3, -2, -1], 2])           # over the same state
    if E:
        assert [t.table()[-1, 3] for t in each] == cfg["cost_terms"]["terms"][-1]["weight"]    # a terminal weight per episode
        assert len({t.quad_table().tobytes() for t in each}) == 1                          # one pool


def test_per_episode_weights_share_one_pool_and_different_matrices_are_refused(cartpole):
    E = 3
    block = dict(terms=[
        dict(kind="quadratic", parts=[dict(obs="qpos"), dict(obs="qvel")], matrix=np.eye(4).tolist(), weight=[0.5, 1.0, 2.0]),
        dict(kind="linear", obs="qvel", index=0, weight=-1.0, target=[0.0, 0.1, 0.2]),
    ])
    each = cost_terms_from_config(block, cartpole, num_episodes=E)
    assert isinstance(each, list) and len(each) == E
    stacked, keep, reads = BatchedMPPI._resolve_cost_terms(each, cartpole, E)
    assert stacked.shape == (E, 5, 8) and not keep and not reads
    assert np.array_equal(stacked[:, 0, 3], [0.5, 1.0, 2.0]) and np.array_equal(stacked[:, 4, 4], [0.0, 0.1, 0.2])
    assert len({t.quad_table().tobytes() for t in each}) == 1
    other = CostTerms(cartpole).quadratic(parts=[dict(obs="qpos"), dict(obs="qvel")], matrix=2.0 * np.eye(4), weight=1.0)
    other.linear(obs="qvel", index=0, weight=-1.0, target=0.1)
    with pytest.raises(ValueError, match="episode 1's quadratic matrices differ"):
        BatchedMPPI._resolve_cost_terms([each[0], other, each[2]], cartpole, E)
    # one CostTerms for all, and tables without a group, resolve as ever
    assert BatchedMPPI._resolve_cost_terms(each[0], cartpole, E)[0].shape == (1, 5, 8)
    assert BatchedMPPI._resolve_cost_terms(CostTerms.builtin_reach(cartpole), cartpole, E)[0].shape == (1, 6, 8)


# ---- the entry points -----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    bc.check_entry_points(ENTRY_POINTS, abi=4)
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_quad"][1]) == 23
    assert len(_lib.SIGNATURES["mjmpc_cost_terms_quad_batch"][1]) == 28
    # the rate entries' arguments in their order, the pool in front of the costs
    for quad, rate, at in (("mjmpc_cost_terms_quad", "mjmpc_cost_terms_rate", 19), ("mjmpc_cost_terms_quad_batch",
                                                                                  "mjmpc_cost_terms_rate_batch", 22)):
        q, r = _lib.SIGNATURES[quad][1], _lib.SIGNATURES[rate][1]
        assert q[:at] == r[:at] and q[at + 2:] == r[at:] and q[at:at + 2] == [_lib._vp, _lib._int]
    # the six existing entries keep their signatures
    assert [len(_lib.SIGNATURES[n][1]) for n in ("mjmpc_cost_terms", "mjmpc_cost_terms_batch", "mjmpc_cost_terms_track",
                                                 "mjmpc_cost_terms_track_batch", "mjmpc_cost_terms_rate",
                                                 "mjmpc_cost_terms_rate_batch")] == [13, 17, 20, 24, 21, 26]


def test_quad_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced: every call below is refused before anything is launched)
    f = lib.mjmpc_cost_terms_quad

    def call(dtype=_lib.F64, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             advance=0, prev=p, quad=p, quad_len=16, costs=p):
        return f(dtype, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, ref, n_ref, n_cols, 0, step, 0, advance, prev, quad,
                 quad_len, costs, None)
    bad = [dict(quad=None), dict(quad_len=0), dict(quad_len=4097), dict(quad_len=-1),
           dict(nobs=None), dict(act=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(P=0), dict(H=0), dict(d_obs=0), dict(A=0), dict(n_terms=0), dict(n_terms=129), dict(dtype=7), dict(n_ref=0),
           dict(n_ref=(1 << 20) + 1), dict(n_cols=0), dict(n_cols=129), dict(advance=1), dict(advance=1, ref=None, step=None),
           # a row beyond the tile: the rate entry's 60 KiB less 1 KiB and the scratch - 43 KiB with a full pool, 58.5 KiB with one entry
           dict(d_obs=8000), dict(d_obs=5600, quad_len=4096), dict(dtype=_lib.F32, d_obs=11200, quad_len=4096)]
    for kw in bad:
        assert call(**kw) == -1, kw                 # MJMPC_E_BADARG
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_quad:"), (kw, lib.mjmpc_last_error())
    call(d_obs=5600, quad_len=4096)
    assert b"44032 bytes" in lib.mjmpc_last_error() and b"32 rows" in lib.mjmpc_last_error()       # the actual limit
    call(d_obs=8000, quad_len=1)
    assert b"59904 bytes" in lib.mjmpc_last_error()


def test_quad_batch_bad_arguments_are_codes_and_messages():
    lib = _lib.load()
    p = 64          # (never dereferenced)
    f = lib.mjmpc_cost_terms_quad_batch

    def call(dtype=_lib.F64, E=2, P=4, H=2, d_obs=3, A=1, nobs=p, act=p, terms=p, n_terms=1, ref=p, n_ref=3, n_cols=1, step=p,
             prev=p, advance_prev=0, quad=p, quad_len=16, costs=p, gseq=None, q0=None):
        return f(dtype, E, P, H, d_obs, A, nobs, act, terms, n_terms, 0, 0, 0, ref, n_ref, n_cols, 0, 0, step, 0, prev,
                 advance_prev, quad, quad_len, costs, gseq, q0, None)
    bad = [dict(quad=None), dict(quad_len=0), dict(quad_len=4097),
           dict(nobs=None), dict(act=None), dict(terms=None), dict(costs=None), dict(ref=None), dict(step=None),
           dict(E=0), dict(P=0), dict(H=0), dict(d_obs=0), dict(A=0), dict(n_terms=0), dict(n_terms=129), dict(dtype=7),
           dict(gseq=p), dict(q0=p), dict(n_ref=0), dict(n_cols=129), dict(advance_prev=1),
           dict(advance_prev=1, ref=None, step=None), dict(d_obs=8000), dict(d_obs=5100, quad_len=4096)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.mjmpc_last_error().startswith(b"mjmpc_cost_terms_quad_batch:"), (kw, lib.mjmpc_last_error())
    call(d_obs=5100, quad_len=4096)
    assert b"39936 bytes" in lib.mjmpc_last_error()         # 56 KiB less 1 KiB less the scratch of 32 x 64 doubles
