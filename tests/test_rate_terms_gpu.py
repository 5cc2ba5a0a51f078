"""GPU: action-rate rows and one-sided kinds.

1. ``mjmpc_cost_terms_rate`` against the numpy restatement of the contract (tests/rate_cases.py) within the derived bound of
   tests/cost_terms_cases.py - tile boundaries in mid-particle and at t = 0, a tile of fewer than 64 rows, every ``prev``
   (finite, NaN, one NaN entry, NULL), with and without a reference, ``advance``; a pointed case whose cost IS the rate;
   ``mjmpc_cost_terms_rate_batch`` against the single entry per episode, bit for bit; old tables through the new entries
   against the old entries, bit for bit; all six entries at the widths that put a tile exactly on its LDS budget.  2. the
   engines: ``rollout_device`` against the restatement, ``step_state`` and the env classes' ``step`` record the applied
   action, eager / hipGraph / launch-tape loops agree.  3. the six episode-batch classes:
   real-env costs from consecutive published actions, ``_prev_actions``, ``reset()``; ``BatchedMPPI`` against sequential
   single-episode captured loops.  4. tables that need no new entry, and ``None``, cost what they did and never reach it."""

import numpy as np
import pytest

import batched_cases as bc
import batched_terms_cases as btc
import rate_cases as rc
import tracking_cases as tc
from batched_cases import FILT, _torch
from cost_terms_cases import H, P, _engine, _mppi, _noise, bound, mixed_terms, random_table, restate

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]


def _seen(x, f32):
    """What the device holds of float64 values in the storage type, as float64."""
    return np.asarray(x, np.float64).astype(np.float32 if f32 else np.float64).astype(np.float64)


# ---- 1. the entry points ------------------------------------------------------------------------------------------------
# (P, H): a workgroup boundary in mid-particle (64 = 12 particles and 4 steps: the previous row lies in another tile); a
# boundary that is a particle's t = 0; H above a tile; every element a t = 0; the controlled env's step
SHAPES = [(24, 5), (2, 64), (3, 70), (8, 1), (1, 1)]
# (reference: None or (N, periodic), prev: 'finite', 'nan', 'one' NaN entry or None): every value of either at least once
COMBOS = [(None, "finite"), (None, "nan"), (None, "one"), (None, None), ((3, 0), "finite"), ((3, 1), "one"), ((40, 0), None),
          ((40, 1), "nan")]


def _prev_vector(rng, A, how):
    if how is None:
        return None
    prev = rng.uniform(-5.0, 5.0, A)
    if how == "nan":
        prev[:] = np.nan
    elif how == "one":
        prev[int(rng.integers(0, A))] = np.nan
    return prev


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
@pytest.mark.parametrize("d_obs,A,K", [(10, 1, 5), (43, 7, 37), (43, 7, 128), (130, 3, 20)])
def test_rate_kernel_matches_the_restatement(d_obs, A, K, f32):
    """(130, 3, 20) in f64: 64 rows of 131 + 3 words and one more action row exceed the tile's 60 KiB - 32 rows."""
    torch = _torch()
    rng = np.random.default_rng(4000 * d_obs + 40 * A + K)
    tdt = btc.tdtype(f32)
    settings = [(0, 1), (1, 0), (1, 1), (0, 0)]                 # (keep_builtin, terminal), taken in turn
    turn = 0
    for Pn, Hn in SHAPES:
        nobs_h = rng.uniform(-5.0, 5.0, (Pn, Hn, d_obs))
        act_h = rng.uniform(-5.0, 5.0, (Pn, Hn, A))
        nobs, act = torch.from_numpy(nobs_h).to(tdt).cuda(), torch.from_numpy(act_h).to(tdt).cuda()
        nobs_seen, act_seen = nobs.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        for reference, how in COMBOS:
            for advance in ((0, 1) if (Pn, Hn) == (1, 1) else (0,)):
                table = rc.random_extended_table(rng, K, d_obs, A)
                ref = d_ref = counter = None
                now = bias = periodic = 0
                if reference is not None:
                    N, periodic = reference
                    table, ref = tc.track_rows(rng, table, N)
                    now, bias = (0, N - 2, 10 * N + 1)[turn % 3], -(turn % 2)
                    d_ref = torch.from_numpy(ref).cuda()
                    counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
                d_tab = torch.from_numpy(table).cuda()
                prev_h = _prev_vector(rng, A, how)
                prev = None if prev_h is None else torch.from_numpy(prev_h).cuda()
                keep, terminal = settings[turn % 4]
                turn += 1
                cin = rng.uniform(-3.0, 3.0, (Pn, Hn))
                if Pn * Hn >= 15:               # an incoming +inf and an incoming NaN: both leave as +inf
                    cin.reshape(-1)[4], cin.reshape(-1)[Pn * Hn - 2] = np.inf, np.nan
                costs = torch.from_numpy(cin).to(tdt).cuda()
                cin_seen = costs.cpu().numpy().astype(np.float64)
                btc.cost_terms_rate(d_tab, d_ref, periodic, counter, bias, advance, prev, nobs, act, costs, keep, terminal, f32)
                torch.cuda.synchronize()
                where = (Pn, Hn, reference, how, now, bias, keep, terminal, advance)
                if counter is not None:
                    assert int(counter.item()) == now + advance, where
                if prev is not None:            # the applied action, exactly, or what it was
                    after = prev.cpu().numpy()
                    assert np.array_equal(after, act_seen[0, 0] if advance else prev_h, equal_nan=True), where
                got = costs.cpu().numpy().astype(np.float64)
                want, mag = rc.restate(table, nobs_seen, act_seen, prev_h, cin_seen, keep, terminal, ref, periodic, now + bias)
                bad = ~np.isfinite(cin_seen)
                assert np.all(np.isposinf(got[bad])) and np.all(np.isposinf(want[bad])), where
                err = np.abs(got[~bad] - want[~bad])
                tol = bound(table, want, mag, f32)[~bad]
                assert np.all(err <= tol), "%s: error %.3g over the bound by %.3g" % (where, err.max(), (err - tol).max())


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_rate_kernel_reads_the_step_before(f32):
    """One ABS rate row of weight 1 on the actions 1000 p + (0, 1, 3, 6, ...): the cost IS the difference - t for t >= 1,
    whichever tile the step before lies in, and 1000 p - prev at t = 0."""
    torch = _torch()
    tdt = btc.tdtype(f32)
    table = torch.tensor([[0, 2, 1, 1.0, 0.0, 0, 0, 0]], dtype=torch.float64, device="cuda")
    for Pn, Hn in [(3, 70), (24, 5), (2, 64), (130, 1)]:
        t = np.arange(Hn, dtype=np.float64)
        act_h = np.zeros((Pn, Hn, 2))
        act_h[:, :, 1] = 1000.0 * np.arange(Pn)[:, None] + (t * (t + 1) / 2)[None, :]
        act_h[:, :, 0] = 77.0                                           # (the column no row reads)
        act = torch.from_numpy(act_h).to(tdt).cuda()
        nobs = torch.zeros((Pn, Hn, 3), dtype=tdt, device="cuda")
        for prev_h in (np.array([5.0, -2.0]), np.array([0.0, np.nan]), None):
            costs = torch.zeros((Pn, Hn), dtype=tdt, device="cuda")
            prev = None if prev_h is None else torch.from_numpy(prev_h).cuda()
            btc.cost_terms_rate(table, None, 0, None, 0, 0, prev, nobs, act, costs, 0, 1, f32)
            want = np.tile(t, (Pn, 1))
            want[:, 0] = 0.0 if prev_h is None or np.isnan(prev_h[1]) else np.abs(1000.0 * np.arange(Pn) - prev_h[1])
            assert np.array_equal(costs.cpu().numpy().astype(np.float64), want), (Pn, Hn, prev_h)


# (E, P, H): workgroups that straddle episodes; H above the 64-element chunk; several particles per workgroup and episodes of
# fewer particles than a workgroup holds; one particle per episode; the E real envs' step, which records the actions
BATCH_KERNEL_SHAPES = [(3, 8, 5), (2, 8, 70), (4, 3, 7), (3, 1, 64), (5, 1, 1)]


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_rate_batch_kernel_equals_the_single_kernel_per_episode(f32):
    torch = _torch()
    rng = np.random.default_rng(78)
    tdt = btc.tdtype(f32)
    d_obs, A, K, N = 11, 2, 9, 6
    for E, Pn, Hn in BATCH_KERNEL_SHAPES:
        n = E * Pn
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, A))).to(tdt).cuda()
        gseq_h = np.cumprod([1.0] + [0.93] * (Hn - 1))
        gseq = torch.from_numpy(gseq_h).cuda()
        plain = rc.random_extended_table(rng, K, d_obs, A)
        first, ref0 = tc.track_rows(rng, plain, N)
        # (tables per episode, references: None / shared / per episode, periodic, counter, bias, prev rows?)
        for tab_pe, ref_pe, periodic, now, bias, with_prev in [(0, None, 0, 0, 0, 1), (1, None, 0, 0, 0, 1), (1, 1, 1, 4, -1, 1),
                                                               (0, 1, 0, 3, 0, 0), (1, 0, 1, 61, 0, 1), (0, None, 0, 0, 0, 0)]:
            base = plain if ref_pe is None else first
            tables = np.stack([base] * (E if tab_pe else 1))
            if tab_pe:
                tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
                tables[1:, :, 4] = rng.uniform(-5.0, 5.0, (E - 1, K))
            d_tabs = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
            d_refs = counter = None
            if ref_pe is not None:
                refs = np.stack([ref0] * (E if ref_pe else 1))
                if ref_pe:
                    refs[1:] = rng.uniform(-5.0, 5.0, (E - 1,) + ref0.shape)
                d_refs = torch.from_numpy(np.ascontiguousarray(refs)).cuda()
                counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
            prev_h = rng.uniform(-5.0, 5.0, (E, A))
            prev_h[E - 1, 0] = np.nan                               # one episode with an entry not applied yet
            advance = int((Pn, Hn) == (1, 1))
            cin = rng.uniform(-3.0, 3.0, (n, Hn))
            if n * Hn >= 15:
                cin.reshape(-1)[4], cin.reshape(-1)[n * Hn - 2] = np.inf, np.nan
            d_cin = torch.from_numpy(cin).to(tdt).cuda()
            want = d_cin.clone()
            want_prev = torch.from_numpy(prev_h).cuda() if with_prev else None
            for e in range(E):
                rows = slice(e * Pn, (e + 1) * Pn)
                one_counter = None if counter is None else counter.clone()
                btc.cost_terms_rate(d_tabs[e if tab_pe else 0], None if d_refs is None else d_refs[e if ref_pe else 0], periodic,
                                    one_counter, bias, advance, None if want_prev is None else want_prev[e], nobs[rows], act[rows],
                                    want[rows], 1, 1, f32)
            got, q0 = d_cin.clone(), torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            got_prev = torch.from_numpy(prev_h).cuda() if with_prev else None
            btc.cost_terms_rate_batch(d_tabs, d_refs, periodic, counter, bias, E, got_prev, advance, nobs, act, got, 1, 1, f32, gseq,
                                      q0)
            torch.cuda.synchronize()
            where = (E, Pn, Hn, tab_pe, ref_pe, periodic, now, bias, with_prev)
            got_h = got.cpu().numpy()
            assert counter is None or int(counter.item()) == now, where             # (the batch entry never advances it)
            assert np.array_equal(got_h, want.cpu().numpy()), where
            assert np.array_equal(q0.cpu().numpy(), btc.numpy_q0(got_h, gseq_h)), where
            assert np.sum(~np.isfinite(got_h)) == (2 if n * Hn >= 15 else 0), where
            if with_prev:
                assert np.array_equal(got_prev.cpu().numpy(), want_prev.cpu().numpy(), equal_nan=True), where
                after = act.cpu().numpy().astype(np.float64)[:, 0] if advance else prev_h
                assert np.array_equal(got_prev.cpu().numpy(), after, equal_nan=True), where


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_old_tables_through_the_new_entries_equal_the_old_entries(f32):
    """Kinds 0 .. 3 and sources 0 / 1, NULL ``prev``: the four new kernels against the four old ones, bit for bit."""
    torch = _torch()
    rng = np.random.default_rng(79)
    tdt = btc.tdtype(f32)
    d_obs, A, K, N = 43, 7, 37, 5
    for E, Pn, Hn in [(3, 8, 5), (2, 3, 70)]:
        n = E * Pn
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, A))).to(tdt).cuda()
        gseq = torch.from_numpy(np.cumprod([1.0] + [0.93] * (Hn - 1))).cuda()
        table = random_table(rng, K, d_obs, A)
        tracked, ref = tc.track_rows(rng, table, N)
        tables = np.stack([table] * E)
        tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
        d_tab, d_tracked, d_ref = torch.from_numpy(table).cuda(), torch.from_numpy(tracked).cuda(), torch.from_numpy(ref).cuda()
        d_tabs = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
        counter = torch.full((1,), 2, dtype=torch.int64, device="cuda")
        cin = rng.uniform(-3.0, 3.0, (n, Hn))
        cin.reshape(-1)[4] = np.inf
        d_cin = torch.from_numpy(cin).to(tdt).cuda()
        pairs = []
        old, new = d_cin.clone(), d_cin.clone()
        btc.cost_terms(d_tab, nobs, act, old, 1, 1, f32)
        btc.cost_terms_rate(d_tab, None, 0, None, 0, 0, None, nobs, act, new, 1, 1, f32)
        pairs.append(("single", old, new))
        old, new = d_cin.clone(), d_cin.clone()
        btc.cost_terms_track(d_tracked, d_ref, 1, counter, -1, 0, nobs, act, old, 0, 1, f32)
        btc.cost_terms_rate(d_tracked, d_ref, 1, counter, -1, 0, None, nobs, act, new, 0, 1, f32)
        pairs.append(("tracked", old, new))
        old, new = d_cin.clone(), d_cin.clone()
        q_old, q_new = (torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        btc.cost_terms_batch(d_tabs, E, nobs, act, old, 1, 1, f32, gseq, q_old)
        btc.cost_terms_rate_batch(d_tabs, None, 0, None, 0, E, None, 0, nobs, act, new, 1, 1, f32, gseq, q_new)
        pairs += [("batch", old, new), ("batch q0", q_old, q_new)]
        old, new = d_cin.clone(), d_cin.clone()
        q_old, q_new = (torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        d_trs = torch.from_numpy(np.ascontiguousarray(np.stack([tracked] * E))).cuda()
        btc.cost_terms_track_batch(d_trs, d_ref[None], 0, counter, 0, E, nobs, act, old, 1, 1, f32, gseq, q_old)
        btc.cost_terms_rate_batch(d_trs, d_ref[None], 0, counter, 0, E, None, 0, nobs, act, new, 1, 1, f32, gseq, q_new)
        pairs += [("tracked batch", old, new), ("tracked batch q0", q_old, q_new)]
        torch.cuda.synchronize()
        for what, a, b in pairs:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.all(np.isfinite(a.reshape(-1)[5:])) and np.array_equal(a, b), (what, E, Pn, Hn)


def test_tile_rows_at_the_lds_budget():
    """f64 rows that put a 64-row tile exactly on a budget, through all six entries (one tile-sizing function serves them).
    (109, 3): pitches 109 + 3 = 112 words, 64 x 112 x 8 = 57344 bytes = the batch budget - the plain and tracked batch entries
    keep 64 rows, the rate batch entry's one more action row takes it to 32, every flat entry keeps 64.  (117, 3): pitches
    117 + 3 = 120 words, 64 x 120 x 8 = 61440 bytes = the flat budget - flat plain and tracked keep 64 rows, flat rate drops to
    32, every batch entry runs at 32.  Each flat entry against its numpy restatement per episode, each batch entry against its
    flat entry bit for bit, q0 against the forward loop."""
    torch = _torch()
    rng = np.random.default_rng(80)
    f32, K, N, periodic, now, bias = False, 9, 6, 1, 4, -1
    for d_obs, A in [(109, 3), (117, 3)]:
        for E, Pn, Hn in [(2, 3, 70), (3, 1, 1)]:
            n = E * Pn
            nobs_h, act_h = rng.uniform(-5.0, 5.0, (n, Hn, d_obs)), rng.uniform(-5.0, 5.0, (n, Hn, A))
            nobs, act = torch.from_numpy(nobs_h).cuda(), torch.from_numpy(act_h).cuda()
            gseq_h = np.cumprod([1.0] + [0.93] * (Hn - 1))
            gseq = torch.from_numpy(gseq_h).cuda()
            plain = random_table(rng, K, d_obs, A)
            tracked, ref0 = tc.track_rows(rng, plain, N)
            extended, ref1 = tc.track_rows(rng, rc.random_extended_table(rng, K, d_obs, A), N)
            advance = int((Pn, Hn) == (1, 1))
            for entry, base, ref in [("plain", plain, None), ("track", tracked, ref0), ("rate", extended, ref1)]:
                tables = np.stack([base] * E)                       # a table, a reference and a previous action per episode
                tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
                tables[1:, :, 4] = rng.uniform(-5.0, 5.0, (E - 1, K))
                d_tabs = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
                refs = d_refs = counter = None
                if ref is not None:
                    refs = np.stack([ref] * E)
                    refs[1:] = rng.uniform(-5.0, 5.0, (E - 1,) + ref.shape)
                    d_refs = torch.from_numpy(np.ascontiguousarray(refs)).cuda()
                    counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
                prev_h = rng.uniform(-5.0, 5.0, (E, A))
                prev_h[E - 1, 0] = np.nan
                cin = rng.uniform(-3.0, 3.0, (n, Hn))
                if n * Hn >= 15:
                    cin.reshape(-1)[4], cin.reshape(-1)[n * Hn - 2] = np.inf, np.nan
                d_cin = torch.from_numpy(cin).cuda()
                want = d_cin.clone()
                want_prev, got_prev = (torch.from_numpy(prev_h).cuda() for _ in range(2))
                got, q0 = d_cin.clone(), torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
                where = (d_obs, A, E, Pn, Hn, entry)
                for e in range(E):
                    rows = slice(e * Pn, (e + 1) * Pn)
                    if entry == "plain":
                        btc.cost_terms(d_tabs[e], nobs[rows], act[rows], want[rows], 1, 1, f32)
                        ref_cost, mag = restate(tables[e], nobs_h[rows], act_h[rows], cin[rows], 1, 1)
                    elif entry == "track":
                        btc.cost_terms_track(d_tabs[e], d_refs[e], periodic, counter, bias, 0, nobs[rows], act[rows], want[rows],
                                             1, 1, f32)
                        ref_cost, mag = tc.restate(tables[e], refs[e], periodic, now + bias, nobs_h[rows], act_h[rows], cin[rows],
                                                   1, 1)
                    else:
                        btc.cost_terms_rate(d_tabs[e], d_refs[e], periodic, counter.clone(), bias, advance, want_prev[e],
                                            nobs[rows], act[rows], want[rows], 1, 1, f32)
                        ref_cost, mag = rc.restate(tables[e], nobs_h[rows], act_h[rows], prev_h[e], cin[rows], 1, 1, refs[e],
                                                   periodic, now + bias)
                    flat = want[rows].cpu().numpy()
                    bad = ~np.isfinite(cin[rows])
                    assert np.all(np.isposinf(flat[bad])) and np.all(np.isposinf(ref_cost[bad])), where + (e,)
                    err = np.abs(flat[~bad] - ref_cost[~bad])
                    tol = bound(tables[e], ref_cost, mag, f32)[~bad]
                    assert np.all(err <= tol), "%s: error %.3g over the bound by %.3g" % (where + (e,), err.max(),
                                                                                        (err - tol).max())
                if entry == "plain":
                    btc.cost_terms_batch(d_tabs, E, nobs, act, got, 1, 1, f32, gseq, q0)
                elif entry == "track":
                    btc.cost_terms_track_batch(d_tabs, d_refs, periodic, counter, bias, E, nobs, act, got, 1, 1, f32, gseq, q0)
                else:
                    btc.cost_terms_rate_batch(d_tabs, d_refs, periodic, counter, bias, E, got_prev, advance, nobs, act, got, 1, 1,
                                              f32, gseq, q0)
                torch.cuda.synchronize()
                got_h = got.cpu().numpy()
                assert counter is None or int(counter.item()) == now, where
                assert np.array_equal(got_h, want.cpu().numpy()), where
                assert np.array_equal(q0.cpu().numpy(), btc.numpy_q0(got_h, gseq_h)), where
                assert np.sum(~np.isfinite(got_h)) == (2 if n * Hn >= 15 else 0), where
                if entry == "rate":
                    assert np.array_equal(got_prev.cpu().numpy(), want_prev.cpu().numpy(), equal_nan=True), where
                    assert np.array_equal(got_prev.cpu().numpy(), act_h[:, 0] if advance else prev_h, equal_nan=True), where


# ---- 2. the engines -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_rollout_device_costs_equal_the_restatement(model, dtype):
    torch = _torch()
    f32 = dtype == "f32"
    eng = _engine(model, dtype)
    terms = rc.smooth_terms(eng)
    table = terms.table()
    eng.set_cost_terms(terms)
    assert np.all(np.isnan(eng.prev_action()))
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    last = 0.3 * np.cos(np.arange(eng.d_action))
    for prev in (None, last):
        if prev is not None:
            eng.set_prev_action(prev)
            assert np.array_equal(eng.prev_action(), prev)
        costs, act, _, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        got = costs.cpu().numpy().astype(np.float64)
        want, mag = rc.restate(table, nobs.cpu().numpy(), act.cpu().numpy(), prev, np.zeros((P, H)), False, True)
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound(table, want, mag, f32))
        # the rate rows and the band count: other numbers than the same rows as plain action rows and without the bounds
        assert np.all(mag > 0) and eng.prev_action() is not None
        if prev is not None:
            assert np.array_equal(eng.prev_action(), prev)          # (a plan reads it and leaves it alone)
            none, _ = rc.restate(table, nobs.cpu().numpy(), act.cpu().numpy(), None, np.zeros((P, H)), False, True)
            assert np.all(np.abs(none[:, 0] - want[:, 0]) > bound(table, want, mag, f32)[:, 0])
    eng.set_prev_action(None)
    assert np.all(np.isnan(eng.prev_action()))
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_step_state_and_env_steps_record_the_applied_action(model, dtype):
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.synthetic_env import CartPoleEnv
    torch = _torch()
    f32 = dtype == "f32"
    eng = _engine(model, dtype)
    A, w = eng.d_action, 0.75
    terms = CostTerms(eng).square(action_rate="all", weight=w)
    table = terms.table()
    eng.set_cost_terms(terms)
    a1, a2 = 0.3 * np.cos(np.arange(A)), 0.2 * np.sin(1.0 + np.arange(A))

    def rate_cost(a, before):
        want, mag = rc.restate(table, np.zeros((1, 1, eng.d_obs)), _seen(a, f32).reshape(1, 1, A), before, np.zeros((1, 1)),
                               False, False)
        return want[0, 0], bound(table, want, mag, f32)[0, 0]
    # two steps of the device-resident env: the first costs 0, the second w |a2 - a1|^2
    c1 = float(eng.step_state(a1)[0].cpu()[0])
    assert c1 == 0.0 and np.array_equal(eng.prev_action(), _seen(a1, f32))
    c2 = float(eng.step_state(a2)[0].cpu()[0])
    want, tol = rate_cost(a2, _seen(a1, f32))
    assert abs(c2 - want) <= tol and abs(want - w * np.sum((_seen(a2, f32) - _seen(a1, f32)) ** 2)) <= 1e-12 * want and want > 0
    assert np.array_equal(eng.prev_action(), _seen(a2, f32))
    # a plan in between reads the vector and leaves it alone; set_env_state leaves it alone; a guarded rollout of another shape
    # cannot be one env step; set_cost_terms starts over
    eng.rollout_device(P, H, np.zeros((H, A)), _noise(eng))
    eng.set_env_state(eng.get_env_state()[0])
    assert np.array_equal(eng.prev_action(), _seen(a2, f32))
    with pytest.raises(ValueError, match="one particle and one step"):
        with eng.real_step_guard("test"):
            eng.rollout_device(2, 1, np.zeros((1, A)), None)
    eng.set_cost_terms(terms)
    assert np.all(np.isnan(eng.prev_action()))
    # the env classes' step
    env = (Reacher7DOFEnv if model == "reacher" else CartPoleEnv)(engine=eng)
    env.reset(seed=1)
    assert np.all(np.isnan(eng.prev_action()))                      # (making and resetting an env plans, it does not step)
    _, rew1, _, _ = env.step(a1)
    _, rew2, _, _ = env.step(a2)
    assert rew1 == 0.0 and abs(-rew2 - want) <= tol
    assert np.array_equal(eng.prev_action(), _seen(a2, f32))
    # without rate rows there is no vector
    eng.set_cost_terms(CostTerms(eng).above(obs="qvel", index=0, target=0.0))
    assert eng._terms_rate and eng._prev_action is None
    assert np.isfinite(float(eng.step_state(a1)[0].cpu()[0]))
    with pytest.raises(RuntimeError, match="action-rate"):
        eng.prev_action()
    with pytest.raises(RuntimeError, match="action-rate"):
        eng.set_prev_action(a1)
    eng.set_cost_terms(None)
    assert not eng._terms_rate and eng._prev_action is None
    eng.close()


def _loop(model, dtype, mode, T=4):
    """``T`` control steps of MPPI on an engine that is its own real env: ``mode`` 'eager', 'graph' (hipGraph replay) or 'tape'."""
    torch = _torch()
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    eng = _engine(model, dtype)
    terms = rc.smooth_terms(eng)
    eng.set_cost_terms(terms)
    c = _mppi(eng)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    if mode != "eager":
        c.enable_graph(post_step=eng.step_state, tape=mode == "tape")
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize({})
        if mode == "eager":
            eng.step_state(np.array(a, np.float64))
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    if mode != "eager":
        assert c._graph is not None and not getattr(c, "graph_fallback", False) and not c._mono
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), prev=eng.prev_action(), table=terms.table())
    assert eng.env_resets() == 0
    eng.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_eager_graph_and_tape_loops_agree_and_cost_the_change_of_their_action(model, dtype):
    T, f32 = 4, dtype == "f32"
    eager, graph, tape = (_loop(model, dtype, mode, T) for mode in ("eager", "graph", "tape"))
    assert np.all(np.isfinite(eager["acts"])) and np.abs(eager["acts"]).max() > 0
    for other in (graph, tape):
        for k in ("acts", "costs", "nobs", "prev"):
            assert np.array_equal(other[k], eager[k]), (k, np.abs(other[k].astype(float) - eager[k].astype(float)).max())
    assert np.array_equal(eager["prev"], _seen(eager["acts"][-1], f32))
    # the real cost of step s: the rate from the action of step s - 1 (none at s = 0), no terminal rows
    table = eager["table"]
    for s in range(T):
        o = eager["nobs"][s].astype(np.float64).reshape(1, 1, -1)
        a = _seen(eager["acts"][s], f32).reshape(1, 1, -1)
        before = None if s == 0 else _seen(eager["acts"][s - 1], f32)
        want, mag = rc.restate(table, o, a, before, np.zeros((1, 1)), False, False)
        assert abs(float(eager["costs"][s]) - want[0, 0]) <= bound(table, want, mag, f32)[0, 0], s
    # ... and it is not the cost of a loop that forgot the applied action
    forgot, _ = rc.restate(table, eager["nobs"][2].astype(np.float64).reshape(1, 1, -1), _seen(eager["acts"][2], f32).reshape(1, 1, -1),
                           None, np.zeros((1, 1)), False, False)
    assert abs(float(eager["costs"][2]) - forgot[0, 0]) > 1e-6 * abs(forgot[0, 0])


# ---- 3. the episode batches -----------------------------------------------------------------------------------------------
SEEDS = [123 + i * 12345 for i in range(3)]
DMD = bc.case("BatchedDMDMPC", "DMDMPC", ("lam", "step_size", "init_cov", "beta"),
              lambda dtype: dict(update_cov=True, noise_dtype=dtype), extra=("cov_action", "cov"))
MPPIQ = bc.case("BatchedMPPIQ", "MPPIQ", ("beta", "step_size", "init_cov", "td_lam"),
                lambda dtype: dict(alpha=1, time_based_weights=True, noise_dtype=dtype))
# every class with per-episode settings (tests/test_batched_terms_gpu.py's values)
CASES = dict(
    BatchedMPPI=(bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype)),
                 (np.array([0.01, 0.05, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedCEM=(bc.case("BatchedCEM", "CEM", ("init_cov", "elite_frac", "step_size", "beta"), None, extra=("cov_action", "cov")),
                (np.array([1.0, 0.5, 0.3]), np.array([0.25, 0.125, 0.5]), np.array([1.0, 0.9, 0.8]), np.array([0.1, 0.2, 0.0]))),
    BatchedPFMPC=(bc.case("BatchedPFMPC", "PFMPC", ("cov_shift", "cov_resample", "lam"), None, gamma=0.99,
                          extra=("action_samples", "action_samples")),
                  (np.array([0.3, 0.2, 0.5]), np.array([0.1, 0.3, 0.2]), np.array([0.05, 0.2, 0.1]))),
    BatchedDMDMPC=(DMD, (np.array([0.05, 0.1, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]), np.array([0.1, 0.0, 0.2]))),
    BatchedRandomShooting=(bc.case("BatchedRandomShooting", "RandomShooting", ("step_size", "init_cov"), None),
                           (np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedMPPIQ=(MPPIQ, (np.array([0.2, 0.1, 0.5]), np.array([1.0, 0.8, 0.5]), np.array([0.3, 0.2, 0.5]), np.array([0.9, 0.0, 1.0]))),
)


def _episode_terms(eng, e):
    """Episode e's terms: the rows of every episode, a rate weight of its own."""
    return rc.smooth_terms(eng, rate_weight=0.5 * (1 + e))


def _make(cls, name, E, Pn, Hn, dtype, per_episode=True):
    case, hyper = CASES[cls]
    raw, states, kind = btc.model(name, E)
    b = bc.make_batch(case, raw, states, SEEDS[:E], Pn, Hn, [v[:E] for v in hyper], dtype, engine=kind)
    b.set_cost_terms([_episode_terms(b.engine, e) for e in range(E)] if per_episode else _episode_terms(b.engine, 0))
    return case, b


@pytest.mark.parametrize("cls,name,dtype", [(c, "cartpole", d) for c in sorted(CASES) for d in DTYPES]
                         + [(c, "reacher", "f64") for c in sorted(CASES)])
def test_every_batch_class_costs_the_change_of_its_published_actions(cls, name, dtype):
    E, Pn, Hn, T, f32 = 3, 64, 6, 3, dtype == "f32"
    case, b = _make(cls, name, E, Pn, Hn, dtype)
    assert b._rate and b._prev_actions.shape == (E, b.d_action) and np.all(np.isnan(b._prev_actions.cpu().numpy()))
    tables = [_episode_terms(b.engine, e).table() for e in range(E)]
    acts, costs, nobs = b.run(T)
    assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs)) and np.abs(acts).max() > 0
    assert b.engine.env_resets() == 0
    for s in range(T):
        for e in range(E):
            before = None if s == 0 else _seen(acts[s - 1, e], f32)
            want, mag = rc.restate(tables[e], nobs[s, e].astype(np.float64).reshape(1, 1, -1), _seen(acts[s, e], f32).reshape(1, 1, -1),
                                   before, np.zeros((1, 1)), False, False)
            assert abs(float(costs[s, e]) - want[0, 0]) <= bound(tables[e], want, mag, f32)[0, 0], (s, e)
    # the rate row counts in the real costs: step 1 is not the cost of a batch that forgot its actions
    forgot, _ = rc.restate(tables[0], nobs[1, 0].astype(np.float64).reshape(1, 1, -1), _seen(acts[1, 0], f32).reshape(1, 1, -1), None,
                           np.zeros((1, 1)), False, False)
    assert abs(float(costs[1, 0]) - forgot[0, 0]) > 1e-9 * abs(forgot[0, 0])
    assert np.array_equal(b._prev_actions.cpu().numpy(), _seen(acts[-1], f32))
    b.reset()
    assert np.all(np.isnan(b._prev_actions.cpu().numpy()))
    b.set_cost_terms(None)
    assert b._prev_actions is None and not b._rate
    b.close()


def _single(case, kind, raw, state, seed, Pn, Hn, T, hyper, dtype, make_terms):
    """The sequential single-episode loop: an engine of its own with the same terms, ``make_device_rollout_fn`` and
    ``enable_graph(post_step=engine.step_state)``."""
    torch = _torch()
    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    eng = btc.engine(raw, kind, dtype)
    eng.set_env_state(dict(state))
    eng.set_cost_terms(make_terms(eng))
    kw = dict(zip(case.hyper, hyper), **case.single_kw(dtype))
    c = getattr(control, case.single)(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=Hn,
                                      base_action="null", num_particles=Pn, gamma=case.gamma, n_iters=1,
                                      action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed,
                                      noise_mode="device", **kw)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    c.enable_graph(post_step=eng.step_state)
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize(None)
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), mean=bc._host(c.mean_action),
               state=eng.get_state_device(), prev=eng.prev_action())
    assert eng.env_resets() == 0, "the single path's real env reset"
    eng.close()
    return out


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batched_mppi_equals_the_sequential_captured_loops(name):
    """With rate rows or one-sided kinds the batch takes the general update, like the single-episode MPPI behind a cost launch
    (``BatchedMPPI.set_cost_terms``): episode e is the sequential loop bit for bit, on both engines."""
    E, Pn, Hn, T, dtype = 3, 64, 6, 3, "f64"
    case, b = _make("BatchedMPPI", name, E, Pn, Hn, dtype)
    hyper = CASES["BatchedMPPI"][1]
    prev = None
    acts, costs, nobs = b.run(T)
    prev = b._prev_actions.cpu().numpy()
    mean, state = b.mean_action, b.get_states()
    assert b.engine.env_resets() == 0
    b.close()
    raw, states, kind = btc.model(name, E)
    for e in range(E):
        one = _single(case, kind, raw, states[e], SEEDS[e], Pn, Hn, T, [v[e] for v in hyper], dtype,
                      lambda eng, e=e: _episode_terms(eng, e))
        assert np.array_equal(acts[:, e], one["acts"]), (e, np.abs(acts[:, e] - one["acts"]).max())
        assert np.array_equal(costs[:, e], one["costs"]) and np.array_equal(nobs[:, e], one["nobs"]), e
        assert np.array_equal(mean[e], one["mean"]) and np.array_equal(prev[e], one["prev"]), e
        for x, y in zip(bc._qpos_qvel(state[e]), bc._qpos_qvel(one["state"])):
            assert np.array_equal(x, y), e


# ---- 4. no behaviour change -----------------------------------------------------------------------------------------------
def _never(*a, **k):
    raise AssertionError("a table that needs no rate entry reached one")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_tables_without_rate_rows_or_bounds_cost_what_they_did(model, dtype, monkeypatch):
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.cost_terms import CostTerms
    lib = _lib.require_gpu()
    eng = _engine(model, dtype)
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    builtin = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    eng.set_cost_terms(rc.smooth_terms(eng))
    smooth = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    assert eng._terms_rate and eng._prev_action is not None
    monkeypatch.setattr(lib, "mjmpc_cost_terms_rate", _never)
    monkeypatch.setattr(lib, "mjmpc_cost_terms_rate_batch", _never)
    # plain terms behind smooth ones: the existing entry's costs on the same observations and actions
    plain = mixed_terms(eng, CostTerms)
    eng.set_cost_terms(plain)
    assert not eng._terms_rate and eng._prev_action is None
    costs, act, _, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
    got = costs.cpu().numpy().copy()
    want = torch.zeros_like(costs)
    btc.cost_terms(torch.from_numpy(plain.table()).cuda(), nobs, act, want, False, True, dtype == "f32")
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy()) and not np.array_equal(got, smooth)
    assert np.isfinite(float(eng.step_state(np.zeros(eng.d_action))[0].cpu()[0]))
    # tracked terms without rate rows: the tracking entry, as before
    eng.set_cost_terms(tc.tracked_reach_terms(eng))
    assert not eng._terms_rate and eng._track_step is not None
    assert np.all(np.isfinite(eng.rollout_device(P, H, mean, noise)[0].cpu().numpy()))
    eng.step_state(np.zeros(eng.d_action))
    assert eng.track_step() == 1
    # None: the built-in cost, exactly
    eng.set_cost_terms(None)
    assert eng._terms_dev is None and eng._prev_action is None
    assert np.array_equal(eng.rollout_device(P, H, mean, noise)[0].cpu().numpy(), builtin)
    eng.close()


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batches_without_rate_rows_or_bounds_cost_what_they_did(name, monkeypatch):
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    monkeypatch.setattr(lib, "mjmpc_cost_terms_rate", _never)
    monkeypatch.setattr(lib, "mjmpc_cost_terms_rate_batch", _never)
    E, Pn, Hn, T = 3, 8, 5, 3
    case, hyper = CASES["BatchedMPPI"]
    raw, states, kind = btc.model(name, E)
    runs = []
    for separate in (False, True):
        b = bc.make_batch(case, raw, states, SEEDS[:E], Pn, Hn, [v[:E] for v in hyper], "f64", engine=kind)
        b.set_cost_terms(btc.terms_for(name, b.engine, E, True))
        assert not b._rate and b._prev_actions is None and b._generic is None
        runs.append(bc.run_batch(case, btc.as_separate_launches(b) if separate else b, T))
    btc.assert_same_runs(runs[0], runs[1], name)
