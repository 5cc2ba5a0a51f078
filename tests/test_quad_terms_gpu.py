"""GPU: quadratic forms and signed linear rows.

1. ``mjmpc_cost_terms_quad`` against the numpy restatement of the contract (tests/quad_cases.py) within its derived bound -
   the shapes and the reference / previous-action combinations of tests/test_rate_terms_gpu.py, groups of 1 to 32 rows over all
   three sources, some rows tracked, a pool and a scratch filled to their limits, a tile the scratch halves;
   ``mjmpc_cost_terms_quad_batch`` against the flat entry per episode, bit for bit; tables without the new kinds through the
   new entries against the rate entries, bit for bit.  2. the engines: ``rollout_device`` against the restatement, the
   controlled env's steps never count terminal groups and advance counter and previous action, eager / hipGraph / launch-tape
   loops agree.  3. the six episode-batch classes with a weight per episode; ``BatchedMPPI`` against sequential single-episode
   captured loops.  4. tables that need no new entry never reach one."""

import numpy as np
import pytest

import batched_cases as bc
import batched_terms_cases as btc
import quad_cases as qc
import rate_cases as rc
import tracking_cases as tc
from batched_cases import _torch
from cost_terms_cases import H, P, _engine, _mppi, _noise, mixed_terms
from test_rate_terms_gpu import BATCH_KERNEL_SHAPES, CASES, COMBOS, SEEDS, SHAPES, _prev_vector, _seen, _single

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]


def _within(got, want, mag, table, cin_seen, f32, where):
    """Every element: the two planted non-finite incoming costs leave as +inf on both sides, all others meet the bound."""
    bad = ~np.isfinite(cin_seen)
    assert np.all(np.isposinf(got[bad])) and np.all(np.isposinf(want[bad])), where
    err = np.abs(got[~bad] - want[~bad])
    tol = qc.bound(table, want, mag, f32)[~bad]
    assert np.all(err <= tol), "%s: error %.3g over the bound by %.3g" % (where, err.max(), (err - tol).max())


# ---- 1. the entry points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
@pytest.mark.parametrize("d_obs,A,K,sizes", [(10, 1, 5, [2, 1]), (43, 7, 37, None), (43, 7, 128, [32] * 4), (85, 3, 20, None)],
                         ids=["small", "mixed", "full", "halved"])
def test_quad_kernel_matches_the_restatement(d_obs, A, K, sizes, f32):
    """small: groups of 2 and 1 rows.  mixed: all ten kinds, groups of 1 - 7 rows, one the table's last rows.  full: four
    groups of 32 rows - the pool's 4096 doubles and the scratch's 32 entries.  halved, in f64: 64 rows of 85 + 3 words are
    45056 bytes and the leading action row 24 more - inside the rate kernel's 60 KiB, but the pool handed over here holds 4096
    doubles, so the quad entry sizes its scratch for groups of 32 rows (16 KiB), its tile budget is 59 KiB - 16 KiB = 44032
    bytes and the tile halves to 32 rows."""
    torch = _torch()
    rng = np.random.default_rng(5000 * d_obs + 50 * A + K)
    tdt = btc.tdtype(f32)
    settings = [(0, 1), (1, 0), (1, 1), (0, 0)]                 # (keep_builtin, terminal), taken in turn
    turn = 0
    for Pn, Hn in SHAPES:
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (Pn, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (Pn, Hn, A))).to(tdt).cuda()
        nobs_seen, act_seen = nobs.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        for reference, how in COMBOS:
            for advance in ((0, 1) if (Pn, Hn) == (1, 1) else (0,)):
                table = qc.random_quad_table(rng, K, d_obs, A, sizes)
                pool = qc.random_pool(rng, table)
                if d_obs == 85:                                 # (the pool of a table that could hold groups of 32 rows)
                    pool = np.concatenate([pool, np.zeros(4096 - len(pool))])
                ref = d_ref = counter = None
                now = bias = periodic = 0
                if reference is not None:
                    N, periodic = reference
                    table, ref = tc.track_rows(rng, table, N)
                    now, bias = (0, N - 2, 10 * N + 1)[turn % 3], -(turn % 2)
                    d_ref = torch.from_numpy(ref).cuda()
                    counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
                d_tab, d_pool = torch.from_numpy(table).cuda(), torch.from_numpy(pool).cuda()
                prev_h = _prev_vector(rng, A, how)
                prev = None if prev_h is None else torch.from_numpy(prev_h).cuda()
                keep, terminal = settings[turn % 4]
                turn += 1
                cin = rng.uniform(-3.0, 3.0, (Pn, Hn))
                if Pn * Hn >= 15:               # an incoming +inf and an incoming NaN: both leave as +inf
                    cin.reshape(-1)[4], cin.reshape(-1)[Pn * Hn - 2] = np.inf, np.nan
                costs = torch.from_numpy(cin).to(tdt).cuda()
                cin_seen = costs.cpu().numpy().astype(np.float64)
                qc.cost_terms_quad(d_tab, d_pool, d_ref, periodic, counter, bias, advance, prev, nobs, act, costs, keep, terminal,
                                   f32)
                torch.cuda.synchronize()
                where = (Pn, Hn, reference, how, now, bias, keep, terminal, advance)
                if counter is not None:
                    assert int(counter.item()) == now + advance, where
                if prev is not None:            # the applied action, exactly, or what it was
                    assert np.array_equal(prev.cpu().numpy(), act_seen[0, 0] if advance else prev_h, equal_nan=True), where
                got = costs.cpu().numpy().astype(np.float64)
                want, mag = qc.restate(table, pool, nobs_seen, act_seen, prev_h, cin_seen, keep, terminal, ref, periodic,
                                       now + bias)
                _within(got, want, mag, table, cin_seen, f32, where)
                assert np.sum(~np.isfinite(got)) == (2 if Pn * Hn >= 15 else 0), where


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_quad_kernel_on_a_hand_computed_form(f32):
    """One group over an observation, an action and its rate with the indefinite Q = [[1, 2, 0], [2, -1, 0.5], [0, 0.5, 3]] on
    small integers: every product and sum is exact, so the cost IS r' Q r - whichever tile the step before lies in."""
    torch = _torch()
    tdt = btc.tdtype(f32)
    Q = np.array([[1.0, 2.0, 0.0], [2.0, -1.0, 0.5], [0.0, 0.5, 3.0]])
    table = torch.tensor([[8, 0, 1, 2.0, 1.0, 1, 0, 0], [8, 1, 0, 7.0, 0.0, 1, 0, 0], [8, 2, 0, 7.0, 0.0, 1, 0, 0],
                          [9, 0, 0, -1.0, 0.0, 0, 0, 0]], dtype=torch.float64, device="cuda")
    pool = torch.from_numpy(Q.reshape(-1)).cuda()
    for Pn, Hn in [(3, 70), (24, 5), (130, 1)]:
        t = np.arange(Hn, dtype=np.float64)
        nobs_h = np.zeros((Pn, Hn, 2))
        nobs_h[:, :, 0], nobs_h[:, :, 1] = np.arange(Pn)[:, None], (t % 5)[None, :]
        act_h = (np.arange(Pn)[:, None] + (t * (t + 1) / 2)[None, :])[:, :, None] % 64
        nobs, act = torch.from_numpy(nobs_h).to(tdt).cuda(), torch.from_numpy(act_h).to(tdt).cuda()
        costs = torch.zeros((Pn, Hn), dtype=tdt, device="cuda")
        qc.cost_terms_quad(table, pool, None, 0, None, 0, 0, torch.tensor([2.0], dtype=torch.float64, device="cuda"), nobs, act,
                           costs, 0, 1, f32)
        rate = np.diff(act_h[:, :, 0], axis=1, prepend=2.0)
        r = np.stack([nobs_h[:, :, 1] - 1.0, act_h[:, :, 0], rate], axis=2)
        want = 2.0 * np.einsum("pti,ij,ptj->pt", r, Q, r) - nobs_h[:, :, 0]
        assert np.array_equal(costs.cpu().numpy().astype(np.float64), want), (Pn, Hn)


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_quad_batch_kernel_equals_the_flat_kernel_per_episode(f32):
    """Tables, references and previous actions per episode with workgroups that straddle two episodes; one pool."""
    torch = _torch()
    rng = np.random.default_rng(81)
    tdt = btc.tdtype(f32)
    d_obs, A, K, N = 11, 2, 14, 6
    for E, Pn, Hn in BATCH_KERNEL_SHAPES:
        n = E * Pn
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, A))).to(tdt).cuda()
        gseq_h = np.cumprod([1.0] + [0.93] * (Hn - 1))
        gseq = torch.from_numpy(gseq_h).cuda()
        plain = qc.random_quad_table(rng, K, d_obs, A)
        pool = qc.random_pool(rng, plain)
        d_pool = torch.from_numpy(pool).cuda()
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
                qc.cost_terms_quad(d_tabs[e if tab_pe else 0], d_pool, None if d_refs is None else d_refs[e if ref_pe else 0],
                                   periodic, None if counter is None else counter.clone(), bias, advance,
                                   None if want_prev is None else want_prev[e], nobs[rows], act[rows], want[rows], 1, 1, f32)
            got, q0 = d_cin.clone(), torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            got_prev = torch.from_numpy(prev_h).cuda() if with_prev else None
            qc.cost_terms_quad_batch(d_tabs, d_pool, d_refs, periodic, counter, bias, E, got_prev, advance, nobs, act, got, 1, 1,
                                     f32, gseq, q0)
            torch.cuda.synchronize()
            where = (E, Pn, Hn, tab_pe, ref_pe, periodic, now, bias, with_prev)
            got_h = got.cpu().numpy()
            assert counter is None or int(counter.item()) == now, where             # (the batch entry never advances it)
            want_h = want.cpu().numpy()
            differ = np.flatnonzero((got_h != want_h).reshape(-1) & np.isfinite(want_h).reshape(-1))
            assert np.array_equal(got_h, want_h), where + (differ[:8].tolist(), got_h.reshape(-1)[differ[:8]].tolist(),
                                                           want_h.reshape(-1)[differ[:8]].tolist())
            assert np.array_equal(q0.cpu().numpy(), btc.numpy_q0(got_h, gseq_h)), where
            assert np.sum(~np.isfinite(got_h)) == (2 if n * Hn >= 15 else 0), where
            if with_prev:
                after = act.cpu().numpy().astype(np.float64)[:, 0] if advance else prev_h
                assert np.array_equal(got_prev.cpu().numpy(), after, equal_nan=True), where
        # the flat entry itself against the restatement at this shape: episode 0 of the last setting
        rows = slice(0, Pn)
        ref_cost, mag = qc.restate(tables[0], pool, nobs[rows].cpu().numpy().astype(np.float64),
                                   act[rows].cpu().numpy().astype(np.float64), None, d_cin[rows].cpu().numpy().astype(np.float64),
                                   1, 1)
        _within(want[rows].cpu().numpy().astype(np.float64), ref_cost, mag, tables[0],
                d_cin[rows].cpu().numpy().astype(np.float64), f32, (E, Pn, Hn, "flat"))


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_tables_without_the_new_kinds_through_the_new_entries_equal_the_rate_entries(f32):
    """Kinds 0 .. 7 and all three sources, tracked and not: the quad kernels against the rate kernels, bit for bit."""
    torch = _torch()
    rng = np.random.default_rng(82)
    tdt = btc.tdtype(f32)
    d_obs, A, K, N = 43, 7, 37, 5
    d_pool = torch.zeros(1, dtype=torch.float64, device="cuda")
    for E, Pn, Hn in [(3, 8, 5), (2, 3, 70)]:
        n = E * Pn
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, A))).to(tdt).cuda()
        gseq = torch.from_numpy(np.cumprod([1.0] + [0.93] * (Hn - 1))).cuda()
        table = rc.random_extended_table(rng, K, d_obs, A)
        tracked, ref = tc.track_rows(rng, table, N)
        tables = np.stack([table] * E)
        tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
        d_tab, d_tracked, d_ref = torch.from_numpy(table).cuda(), torch.from_numpy(tracked).cuda(), torch.from_numpy(ref).cuda()
        d_tabs = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
        d_trs = torch.from_numpy(np.ascontiguousarray(np.stack([tracked] * E))).cuda()
        counter = torch.full((1,), 2, dtype=torch.int64, device="cuda")
        prev, prevs = torch.from_numpy(rng.uniform(-5.0, 5.0, A)).cuda(), torch.from_numpy(rng.uniform(-5.0, 5.0, (E, A))).cuda()
        cin = rng.uniform(-3.0, 3.0, (n, Hn))
        cin.reshape(-1)[4] = np.inf
        d_cin = torch.from_numpy(cin).to(tdt).cuda()
        pairs = []
        old, new = d_cin.clone(), d_cin.clone()
        btc.cost_terms_rate(d_tab, None, 0, None, 0, 0, prev, nobs, act, old, 1, 1, f32)
        qc.cost_terms_quad(d_tab, d_pool, None, 0, None, 0, 0, prev, nobs, act, new, 1, 1, f32)
        pairs.append(("flat", old, new))
        old, new = d_cin.clone(), d_cin.clone()
        btc.cost_terms_rate(d_tracked, d_ref, 1, counter, -1, 0, None, nobs, act, old, 0, 1, f32)
        qc.cost_terms_quad(d_tracked, d_pool, d_ref, 1, counter, -1, 0, None, nobs, act, new, 0, 1, f32)
        pairs.append(("flat tracked", old, new))
        for what, tabs, refs in (("batch", d_tabs, None), ("batch tracked", d_trs, d_ref[None])):
            old, new = d_cin.clone(), d_cin.clone()
            q_old, q_new = (torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
            btc.cost_terms_rate_batch(tabs, refs, 0, None if refs is None else counter, 0, E, prevs, 0, nobs, act, old, 1, 1, f32,
                                      gseq, q_old)
            qc.cost_terms_quad_batch(tabs, d_pool, refs, 0, None if refs is None else counter, 0, E, prevs, 0, nobs, act, new, 1,
                                     1, f32, gseq, q_new)
            pairs += [(what, old, new), (what + " q0", q_old, q_new)]
        torch.cuda.synchronize()
        for what, a, b in pairs:
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.all(np.isfinite(a.reshape(-1)[5:])) and np.array_equal(a, b), (what, E, Pn, Hn)


# ---- 2. the engines -------------------------------------------------------------------------------------------------------
def _restated(terms, nobs, act, prev, terminal, base, f32):
    """The cost of ``terms`` (an engine's ``CostTerms``) over device or host observations and actions, and its bound."""
    table, pool, ref = terms.table(), terms.quad_table(), terms.reference_table()
    nobs = np.asarray(nobs.cpu() if hasattr(nobs, "cpu") else nobs, np.float64)
    act = np.asarray(act.cpu() if hasattr(act, "cpu") else act, np.float64)
    want, mag = qc.restate(table, pool, nobs, act, prev, np.zeros(nobs.shape[:2]), False, terminal, ref, terms.periodic, base)
    return want, qc.bound(table, want, mag, f32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_rollout_device_costs_equal_the_restatement(model, dtype):
    f32 = dtype == "f32"
    eng = _engine(model, dtype)
    terms = qc.lqr_terms(eng)
    eng.set_cost_terms(terms)
    assert eng._terms_quad is not None and eng._terms_quad.shape[0] == len(terms.quad_table())
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    last = 0.3 * np.cos(np.arange(eng.d_action))
    for prev, now in ((None, 0), (last, 3)):
        if prev is not None:
            eng.set_prev_action(prev)
            eng.set_track_step(now)
        costs, act, _, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        got = costs.cpu().numpy().astype(np.float64)
        want, tol = _restated(terms, nobs, act, prev, True, now, f32)
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= tol)
        assert eng.track_step() == now                                  # (a plan reads the counter and leaves it alone)
        # the terminal form counts, at the last step only; so does the coupling: the diagonal alone is another number
        none, _ = _restated(terms, nobs, act, prev, False, now, f32)
        assert np.array_equal(none[:, :-1], want[:, :-1]) and np.all(np.abs(none[:, -1] - want[:, -1]) > tol[:, -1])
        diag = qc.restate(terms.table(), _diagonal(terms.table(), terms.quad_table()), nobs.cpu().numpy().astype(np.float64),
                          act.cpu().numpy().astype(np.float64), prev, np.zeros((P, H)), False, True, terms.reference_table(),
                          False, now)[0]
        assert np.all(np.abs(diag - want) > tol)
    eng.close()


def _diagonal(table, pool):
    out = np.array(pool)
    for _, n, off in qc.groups(table):
        out[off:off + n * n] = np.diag(np.diag(pool[off:off + n * n].reshape(n, n))).reshape(-1)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_step_state_and_env_steps_leave_terminal_groups_out_and_advance(model, dtype):
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.synthetic_env import CartPoleEnv
    f32 = dtype == "f32"
    eng = _engine(model, dtype)
    A = eng.d_action
    terms = qc.lqr_terms(eng)
    eng.set_cost_terms(terms)
    a1, a2 = 0.3 * np.cos(np.arange(A)), 0.2 * np.sin(1.0 + np.arange(A))

    def check(cost, nobs, a, before, now):
        want, tol = _restated(terms, np.asarray(nobs, np.float64).reshape(1, 1, -1), _seen(a, f32).reshape(1, 1, A), before, False,
                              now, f32)
        assert abs(float(cost) - want[0, 0]) <= tol[0, 0], (float(cost), want[0, 0])
        with_terminal, _ = _restated(terms, np.asarray(nobs, np.float64).reshape(1, 1, -1), _seen(a, f32).reshape(1, 1, A), before,
                                     True, now, f32)
        assert abs(float(cost) - with_terminal[0, 0]) > tol[0, 0]
    assert eng.track_step() == 0 and np.all(np.isnan(eng.prev_action()))
    cost, nobs = eng.step_state(a1)
    check(cost.cpu()[0], nobs.cpu().numpy(), a1, None, 0)
    assert eng.track_step() == 1 and np.array_equal(eng.prev_action(), _seen(a1, f32))
    cost, nobs = eng.step_state(a2)
    check(cost.cpu()[0], nobs.cpu().numpy(), a2, _seen(a1, f32), 1)
    assert eng.track_step() == 2 and np.array_equal(eng.prev_action(), _seen(a2, f32))
    with pytest.raises(ValueError, match="one particle and one step"):
        with eng.real_step_guard("test"):
            eng.rollout_device(2, 1, np.zeros((1, A)), None)
    # the env classes' step: a (1, 1) rollout under the guard
    eng.set_cost_terms(terms)
    env = (Reacher7DOFEnv if model == "reacher" else CartPoleEnv)(engine=eng)
    env.reset(seed=1)
    now = eng.track_step()
    assert np.all(np.isnan(eng.prev_action()))
    stepped, rollout = [], eng.rollout

    def recording(*a, **k):             # (the next observation of the env's step, as the engine returned it)
        out = rollout(*a, **k)
        stepped.append(np.asarray(out[5], np.float64)[0, 0])
        return out
    eng.rollout = recording
    _, rew1, _, _ = env.step(a1)
    assert eng.track_step() == now + 1 and np.array_equal(eng.prev_action(), _seen(a1, f32))
    check(-rew1, stepped[-1], a1, None, now)
    _, rew2, _, _ = env.step(a2)
    assert eng.track_step() == now + 2 and np.array_equal(eng.prev_action(), _seen(a2, f32))
    check(-rew2, stepped[-1], a2, _seen(a1, f32), now + 1)
    del eng.rollout
    eng.set_cost_terms(None)
    assert eng._terms_quad is None and eng._terms_dev is None
    eng.close()


def _loop(model, dtype, mode, T=4):
    """``T`` control steps of MPPI on an engine that is its own real env: ``mode`` 'eager', 'graph' (hipGraph replay) or 'tape'."""
    torch = _torch()
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    eng = _engine(model, dtype)
    terms = qc.lqr_terms(eng)
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
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), prev=eng.prev_action(),
               now=np.array(eng.track_step()), terms=terms)
    assert eng.env_resets() == 0
    eng.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_eager_graph_and_tape_loops_agree(model, dtype):
    T, f32 = 4, dtype == "f32"
    eager, graph, tape = (_loop(model, dtype, mode, T) for mode in ("eager", "graph", "tape"))
    assert np.all(np.isfinite(eager["acts"])) and np.abs(eager["acts"]).max() > 0 and eager["now"] == T
    for other in (graph, tape):
        for k in ("acts", "costs", "nobs", "prev", "now"):
            assert np.array_equal(other[k], eager[k]), (k, np.abs(other[k].astype(float) - eager[k].astype(float)).max())
    assert np.array_equal(eager["prev"], _seen(eager["acts"][-1], f32))
    for s in range(T):                  # the real cost of step s: env time s, the action of step s - 1, no terminal group
        before = None if s == 0 else _seen(eager["acts"][s - 1], f32)
        want, tol = _restated(eager["terms"], eager["nobs"][s].astype(np.float64).reshape(1, 1, -1),
                              _seen(eager["acts"][s], f32).reshape(1, 1, -1), before, False, s, f32)
        assert abs(float(eager["costs"][s]) - want[0, 0]) <= tol[0, 0], s


# ---- 3. the episode batches -----------------------------------------------------------------------------------------------
def _episode_terms(eng, e):
    """Episode e's terms: the rows and matrices of every episode, weights of its own."""
    return qc.lqr_terms(eng, weight=0.5 * (1 + e), terminal_weight=1.0 + e)


def _make(cls, name, E, Pn, Hn, dtype):
    case, hyper = CASES[cls]
    raw, states, kind = btc.model(name, E)
    b = bc.make_batch(case, raw, states, SEEDS[:E], Pn, Hn, [v[:E] for v in hyper], dtype, engine=kind)
    b.set_cost_terms([_episode_terms(b.engine, e) for e in range(E)])
    return case, b


@pytest.mark.parametrize("cls,name,dtype", [(c, "cartpole", d) for c in sorted(CASES) for d in DTYPES]
                         + [(c, "reacher", "f64") for c in sorted(CASES)])
def test_every_batch_class_costs_what_the_restatement_says(cls, name, dtype):
    E, Pn, Hn, T, f32 = 3, 64, 6, 3, dtype == "f32"
    case, b = _make(cls, name, E, Pn, Hn, dtype)
    each = [_episode_terms(b.engine, e) for e in range(E)]
    assert b._quad is not None and b._quad.shape[0] == len(each[0].quad_table()) and b._terms[2] == 1
    acts, costs, nobs = b.run(T)
    assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs)) and np.abs(acts).max() > 0
    assert b.engine.env_resets() == 0
    for s in range(T):
        for e in range(E):
            before = None if s == 0 else _seen(acts[s - 1, e], f32)
            want, tol = _restated(each[e], nobs[s, e].astype(np.float64).reshape(1, 1, -1), _seen(acts[s, e], f32).reshape(1, 1, -1),
                                  before, False, s, f32)
            assert abs(float(costs[s, e]) - want[0, 0]) <= tol[0, 0], (s, e)
    # the weights are the episode's own: episode 1's step is not costed with episode 0's table
    other, tol = _restated(each[0], nobs[1, 1].astype(np.float64).reshape(1, 1, -1), _seen(acts[1, 1], f32).reshape(1, 1, -1),
                           _seen(acts[0, 1], f32), False, 1, f32)
    assert abs(float(costs[1, 1]) - other[0, 0]) > tol[0, 0]
    with pytest.raises(ValueError, match="episode 2's quadratic matrices differ"):
        b.set_cost_terms([each[0], each[1], qc.lqr_terms(b.engine, seed=6)])
    b.set_cost_terms(None)
    assert b._quad is None and b._terms is None
    b.close()


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batched_mppi_equals_the_sequential_captured_loops(name):
    """With a quadratic group or a linear row the batch takes the general update, like the single-episode MPPI behind a cost
    launch: episode e is the sequential loop bit for bit, on both engines."""
    E, Pn, Hn, T, dtype = 3, 64, 6, 3, "f64"
    case, b = _make("BatchedMPPI", name, E, Pn, Hn, dtype)
    hyper = CASES["BatchedMPPI"][1]
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
    raise AssertionError("a table that needs no quad entry reached one")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_tables_without_the_new_kinds_never_reach_the_new_entries(model, dtype, monkeypatch):
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.cost_terms import CostTerms
    lib = _lib.require_gpu()
    eng = _engine(model, dtype)
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    builtin = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    eng.set_cost_terms(qc.lqr_terms(eng))
    quad = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    monkeypatch.setattr(lib, "mjmpc_cost_terms_quad", _never)
    monkeypatch.setattr(lib, "mjmpc_cost_terms_quad_batch", _never)
    with pytest.raises(AssertionError, match="reached one"):           # (the patch is in the engine's way)
        eng.rollout_device(P, H, mean, noise)
    for terms, rate, tracked in ((rc.smooth_terms(eng), True, False), (mixed_terms(eng, CostTerms), False, False),
                                 (tc.tracked_reach_terms(eng), False, True)):
        eng.set_cost_terms(terms)
        assert eng._terms_quad is None and eng._terms_rate == rate and (eng._track_step is not None) == tracked
        costs, act, _, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        got = costs.cpu().numpy().copy()
        assert np.all(np.isfinite(got)) and not np.array_equal(got, quad)
        if not rate and not tracked:            # the plain entry's costs on the same observations and actions
            want = torch.zeros_like(costs)
            btc.cost_terms(torch.from_numpy(terms.table()).cuda(), nobs, act, want, False, True, dtype == "f32")
            torch.cuda.synchronize()
            assert np.array_equal(got, want.cpu().numpy())
        assert np.isfinite(float(eng.step_state(np.zeros(eng.d_action))[0].cpu()[0]))
    eng.set_cost_terms(None)
    assert np.array_equal(eng.rollout_device(P, H, mean, noise)[0].cpu().numpy(), builtin)
    eng.close()


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batches_without_the_new_kinds_never_reach_the_new_entries(name, monkeypatch):
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    monkeypatch.setattr(lib, "mjmpc_cost_terms_quad", _never)
    monkeypatch.setattr(lib, "mjmpc_cost_terms_quad_batch", _never)
    E, Pn, Hn, T = 3, 8, 5, 3
    case, hyper = CASES["BatchedMPPI"]
    raw, states, kind = btc.model(name, E)
    for make in (lambda eng: btc.terms_for(name, eng, E, True), lambda eng: [rc.smooth_terms(eng, 0.5 * (1 + e)) for e in range(E)]):
        b = bc.make_batch(case, raw, states, SEEDS[:E], Pn, Hn, [v[:E] for v in hyper], "f64", engine=kind)
        b.set_cost_terms(make(b.engine))
        assert b._quad is None
        acts, costs, _ = b.run(T)
        assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs))
        b.close()
