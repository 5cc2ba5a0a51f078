"""CPU: the references of tests/diverged_cases.py are the oracle's operations on the finite particles.

Every long-double reference, given a spoiled population, must equal ``oracle/controllers_ref.py`` (pinned on golden vectors of
the reference implementation) run on the particles that stayed finite, to 1e-13 absolute, at the shapes the GPU tests use.
The pattern generator's own assertions are exercised for both block sizes of the update kernels.
"""
import numpy as np
import pytest

import diverged_cases as dc
from oracle import controllers_ref as cr

TOL = 1e-13
SHAPES = [(197, 3, 2, dc.FCH), (4165, 2, 2, dc.FCH), (37, 3, 2, dc.CHUNK), (111, 3, 2, dc.CHUNK)]


def _close(got, want):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=TOL)


@pytest.mark.parametrize("B", [16, 64])
@pytest.mark.parametrize("P", [37, 70 + 64, 197, 4165])
def test_patterns_keep_their_promise(P, B):
    if (P + B - 1) // B < 3:
        with pytest.raises(AssertionError):
            dc.pattern("block", P, B)
        return
    for name in dc.PATTERNS:
        idx = dc.pattern(name, P, B)
        assert idx.size < P and np.array_equal(idx, np.unique(idx))
        assert bool(dc.whole_blocks(idx, P, B)) == (name in dc.WHOLE_BLOCK)
    nb = (P + B - 1) // B
    per = (nb + 3) // 4
    assert dc.whole_blocks(dc.pattern("slice", P, B), P, B) == list(range(per, 2 * per))
    assert dc.pattern("all_but_one", P, B).size == P - 1
    assert dc.whole_blocks(dc.pattern("ragged_last", P, B), P, B) == [nb - 1]


def test_a_pattern_that_lost_its_block_is_refused():
    with pytest.raises(AssertionError):
        dc.pattern("block", 128, 64)            # no ragged last block
    assert dc.whole_blocks(np.arange(32, 96), 197, 64) == [] and dc.whole_blocks(np.arange(64, 128), 197, 64) == [1]
    assert dc.whole_blocks(np.arange(192, 197), 197, 64) == [3]


def test_spoilers_write_every_kind():
    costs = np.ones((24, 4))
    bad = dc.spoil_costs(costs, np.arange(12))
    assert np.array_equal(bad[12:], costs[12:])
    fin = dc.finite_columns(bad, cr.gamma_seq(0.97, 4).reshape(-1))
    assert not fin[:12, 0].any() and fin[12:].all()
    assert np.isfinite(bad[3]).all()                                    # two 1e308: finite costs, overflowing cost-to-go
    assert fin[5, 1:].all() and not fin[4].any()                        # +inf at step 0 only / at the last step only
    q = dc.spoil_q0(np.ones(12), np.arange(8))
    assert not np.isfinite(q[:8]).any() and np.isfinite(q[8:]).all()
    assert np.isnan(q[2]) and np.isnan(q[3]) and np.signbit(q[3]) and not np.signbit(q[2]) and q[0] > 0 and q[1] < 0


@pytest.mark.parametrize("P,H,A,B", SHAPES)
@pytest.mark.parametrize("lam", [0.05, 1.0])
def test_references_equal_the_oracle_on_the_finite_particles(P, H, A, B, lam):
    pr = dc.problem(P, H, A, seed=P + H)
    step, gs = 0.9, pr["gseq"].reshape(1, -1)
    covinv = np.linalg.inv(pr["cov"])
    for name in ("block", "ragged_last", "scattered", "all_but_one"):
        idx = dc.pattern(name, P, B)
        keep = np.setdiff1d(np.arange(P), idx)
        # "+inf at step 0 only" stays finite in the later columns: kept out of the time-based comparison below
        costs = dc.spoil_costs(pr["costs"], idx)
        c, a = pr["costs"][keep], pr["actions"][keep]
        assert not dc.finite_columns(costs, pr["gseq"])[idx, 0].any()
        for alpha, ci in ((1, None), (0, covinv)):
            _close(dc.ref_softmax_mean(costs, pr["actions"], pr["mean"], pr["gseq"], lam, step, False, ci),
                   cr.mppi_update(c, a, pr["mean"], pr["cov"], gs, lam, alpha, step))
            _close(dc.ref_softmax_value(costs, pr["actions"], pr["mean"], pr["gseq"], lam, keep.size, ci),
                   cr.mppi_value(c, a, pr["mean"], pr["cov"], gs, lam, alpha))
        for mode, kind in ((1, "diagonal"), (2, "full")):
            m_ref, c_ref = cr.dmd_update(c, a, pr["mean"], pr["cov"], gs, lam, step, True, kind)
            _close(dc.ref_softmax_mean(costs, pr["actions"], pr["mean"], pr["gseq"], lam, step), m_ref)
            _close(dc.ref_softmax_cov(costs, pr["actions"], pr["mean"], pr["cov"], pr["gseq"], lam, step, mode), c_ref)
        w = dc.ref_softmax_weights(costs, pr["actions"], pr["mean"], pr["gseq"], lam)
        assert np.all(w[idx] == 0)
        _close(w[keep], cr.pf_weights(c, gs, lam))
        # time-based weights: every column of the spoiled particles dead (+inf at the last step)
        tb = pr["costs"].copy()
        tb[idx, -1] = np.inf
        for alpha, ci in ((1, None), (0, covinv)):
            _close(dc.ref_softmax_mean(tb, pr["actions"], pr["mean"], pr["gseq"], lam, step, True, ci),
                   cr.mppi_update(c, a, pr["mean"], pr["cov"], gs, lam, alpha, step, True))
        # from q0
        q0 = cr.cost_to_go(pr["costs"].copy(), gs)[:, 0]
        bad = dc.spoil_q0(q0, idx)
        _close(dc.ref_q0_mean(bad, pr["actions"], pr["mean"], lam, step), cr.mppi_update(c, a, pr["mean"], pr["cov"], gs, lam, 1, step))
        _close(dc.ref_q0_value(bad, lam, keep.size), cr.mppi_value(c, a, pr["mean"], pr["cov"], gs, lam, 1))
        wq = dc.ref_pf_weights(bad, lam)
        assert np.all(wq[idx] == 0)
        _close(wq[keep], cr.pf_weights(c, gs, lam))
        rec = np.asarray(dc.ref_q0_record(bad, pr["actions"], lam), np.float64)
        want = cr.softmax_record(c, a, pr["mean"], gs, lam)[:2 + H * A]
        np.testing.assert_allclose(rec, want, rtol=1e-13, atol=TOL)


def test_a_dead_first_column_only_drops_that_column():
    """Time-based weights, +inf at step 0 only: column 0 is the update without those particles, the others keep them."""
    P, H, A = 37, 3, 2
    pr = dc.problem(P, H, A, seed=5)
    gs, idx = pr["gseq"].reshape(1, -1), dc.pattern("block", P, dc.CHUNK)
    costs = pr["costs"].copy()
    costs[idx, 0] = np.inf
    keep = np.setdiff1d(np.arange(P), idx)
    got = np.asarray(dc.ref_softmax_mean(costs, pr["actions"], pr["mean"], pr["gseq"], 0.3, 0.9, True), np.float64)
    all_in = cr.mppi_update(pr["costs"], pr["actions"], pr["mean"], pr["cov"], gs, 0.3, 1, 0.9, True)
    without = cr.mppi_update(pr["costs"][keep], pr["actions"][keep], pr["mean"], pr["cov"], gs, 0.3, 1, 0.9, True)
    np.testing.assert_allclose(got[0], without[0], rtol=0, atol=TOL)
    np.testing.assert_allclose(got[1:], all_in[1:], rtol=0, atol=TOL)


@pytest.mark.parametrize("tbw", [False, True])
@pytest.mark.parametrize("alpha", [1, 0])
@pytest.mark.parametrize("td_lam", [0.85, 0.0])
def test_mppiq_reference_equals_the_oracle(td_lam, alpha, tbw):
    P, H, A = 37, 3, 2
    pr = dc.problem(P, H, A, seed=11)
    idx = dc.pattern("block", P, dc.CHUNK)
    keep = np.setdiff1d(np.arange(P), idx)
    costs = pr["costs"].copy()
    costs[idx] = np.inf
    cov = np.diag([0.9, 0.5])
    for beta in (0.05, 1.0):
        got = dc.ref_mppiq_mean(costs, pr["actions"], pr["mean"], beta, 0.97, td_lam, 0.9, tbw, None if alpha else np.linalg.inv(cov))
        want = cr.mppiq_update(pr["costs"][keep], pr["actions"][keep], None, pr["mean"], cov, beta, alpha, 0.97, td_lam, 0.9, tbw)
        _close(got, want)


@pytest.mark.parametrize("P,H,A,B", SHAPES[:1] + SHAPES[2:3])
def test_selection_references_equal_the_oracle(P, H, A, B):
    pr = dc.problem(P, H, A, seed=3 + P)
    gs = pr["gseq"].reshape(1, -1)
    q0 = cr.cost_to_go(pr["costs"].copy(), gs)[:, 0]
    idx = dc.pattern("block", P, B)
    keep = np.setdiff1d(np.arange(P), idx)
    bad = dc.spoil_q0(q0, idx)
    k = 20 if P > 100 else 7
    ids = dc.elite_ids(bad, k)
    assert not set(ids) & set(idx)
    assert np.array_equal(ids, keep[np.argsort(q0[keep], kind="stable")[:k]])
    for full, kind in ((1, "full"), (0, "diagonal")):
        _, m, c = dc.ref_cem(bad, pr["actions"], pr["mean"], pr["cov"], k, 0.8, full)
        m_ref, c_ref = cr.cem_update(pr["costs"][keep], pr["actions"][keep], pr["mean"], pr["cov"], gs, (k + 0.5) / keep.size, 0.8, kind)
        _close(m, m_ref)
        _close(c, c_ref)
    assert dc.rs_best(bad) == keep[np.argmin(q0[keep])]
    _close(dc.ref_rs(bad, pr["actions"], pr["mean"], 0.7), cr.rs_update(pr["costs"][keep], pr["actions"][keep], pr["mean"], gs, 0.7))
    # ties rank by index, non-finite entries after every finite one and among themselves by index
    assert list(dc.elite_ids(np.array([np.nan, 1.0, -np.inf, 1.0, np.inf, 0.5]), 5)) == [5, 1, 3, 0, 2]
    assert dc.rs_best(dc.q0_kinds()) == 0 and dc.rs_best(np.array([np.nan, -np.inf, 2.0, 2.0])) == 2
