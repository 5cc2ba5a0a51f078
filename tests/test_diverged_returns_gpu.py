"""GPU: diverged returns weigh nothing on EVERY update path, also where a whole block, record or merge slice diverged.

DESIGN 7: a rollout that diverged numerically carries a non-finite return and gets zero weight - never elite, never the best -,
and the updated distribution equals the update over the finite particles alone.  Dynamics-randomized shards diverge together:
a contiguous run of particles, i.e. whole workgroup blocks (64 particles in the fused MPPI update, 16 in the softmax partial
moments), a whole per-GPU record, or a whole slice of the fused update's four-slice merge.  Every entry point of the update
family is run through the C ABI on populations spoiled that way (tests/diverged_cases.py: patterns, the mix of non-finite
kinds, the long-double references over the finite particles) and compared with rtol = atol = 1e-12, the controller-update
tolerance of tests/test_controllers_gpu.py; with f32 storage the reference is computed on the inputs rounded to f32
(accumulation is float64 either way).  ``scattered`` and ``straddle`` hold no whole block: the controls.

A row or run WITHOUT any finite return is outside the promise (the softmax paths give a NaN mean, the selections particle 0 /
the first k by index); of such rows only their isolation from the other rows is asserted.
"""
import ctypes

import numpy as np
import pytest

import diverged_cases as dc
from batched_cases import _torch, _vp

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)
LAMS = [0.05, 1.0]
STEP = 0.9
FUSED_CASES = ([((197, 3, 2), name) for name in dc.PATTERNS] +
               [((4165, 2, 2), name) for name in ("block", "ragged_last", "slice", "all_but_one")])


def _lib():
    from mjmpc_amd import _lib
    return _lib, _lib.require_gpu()


def _stream():
    return ctypes.c_void_p(_torch().cuda.current_stream().cuda_stream)


_ALIVE = []         # every device tensor of the running test: a pointer handed to a launch stays valid until the test ends


@pytest.fixture(autouse=True)
def _keep_device_tensors_alive():
    yield
    _ALIVE.clear()


def _hold(t):
    _ALIVE.append(t)
    return t


def _dev(a, dt=None):
    t = _torch().from_numpy(np.ascontiguousarray(a)).to("cuda")
    return _hold(t if dt is None else t.to(dt))


def _f64(*shape, fill=0.0):
    torch = _torch()
    return _hold(torch.full(shape, fill, dtype=torch.float64, device="cuda"))


def _counter(v):
    torch = _torch()
    return _hold(torch.full((1,), v, dtype=torch.int64, device="cuda"))


def _types(dtype):
    torch = _torch()
    from mjmpc_amd import _lib
    return (_lib.F32, torch.float32) if dtype == "f32" else (_lib.F64, torch.float64)


def _stored(a, dtype):
    """What the kernels read back from storage of ``dtype``."""
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else np.asarray(a, np.float64)


def _workspace(lib, P, H, A):
    torch = _torch()
    ws = _hold(torch.zeros((lib.mjmpc_update_workspace_bytes(P, H, A) + 7) // 8, dtype=torch.float64, device="cuda"))
    addr = lib.mjmpc_workspace_q0(_vp(ws), P, H, A)
    return ws, ws[(addr - ws.data_ptr()) // 8:][:P]


def _close(got, want, what=""):
    got = np.asarray(got)
    assert np.isfinite(got).all(), "%s: not finite" % what
    np.testing.assert_allclose(got, np.asarray(want, np.float64), err_msg=what, **TOL)


_PROBLEMS = {}


def _problem(P, H, A):
    """One population per shape with its clean cost-to-go, made once and shared read-only."""
    if (P, H, A) not in _PROBLEMS:
        pr = dc.problem(P, H, A, seed=P + 7 * H)
        pr["q0"] = dc.cost_to_go64(pr["costs"], pr["gseq"])[:, 0]
        _PROBLEMS[(P, H, A)] = pr
    return _PROBLEMS[(P, H, A)]


# ---------------------------------------------------------------------------------------------------------- a. fused MPPI
def _fused(q0, actions, mean0, lam, step, shift_mode, dtype, record=False, value=False, draw=None):
    """mjmpc_mppi_fused_update (``draw``: _draw_next with dict(seed, chol)) -> dict of host arrays."""
    torch = _torch()
    _l, lib = _lib()
    code, tdt = _types(dtype)
    P, H, A = actions.shape
    d_q0, d_act, d_mean = _dev(q0), _dev(actions, tdt), _dev(mean0)
    out, counter = _f64(A), _counter(5)
    rec = _f64(2 + H * A, fill=float("nan")) if record else None
    val = _f64(1, fill=float("nan")) if value else None
    ws, _ = _workspace(lib, P, H, A)
    args = [code, P, H, A, _vp(d_q0), _vp(d_act), float(lam), float(step), int(shift_mode), _vp(d_mean), _vp(out), _vp(rec),
            _vp(val), None, _vp(counter), _vp(ws)]
    got = {}
    if draw is None:
        _l.check(lib.mjmpc_mppi_fused_update(*args, _stream()))
    else:
        noise = torch.zeros((P, H, A), dtype=tdt, device="cuda")
        _l.check(lib.mjmpc_mppi_fused_update_draw_next(*args, _vp(noise), _vp(_dev(draw["chol"])), draw["seed"], 1, 0, _vp(counter),
                                                       1, _stream()))
        got["noise"] = noise
    torch.cuda.synchronize()
    got.update(mean=d_mean, action=out, counter=counter)
    if record:
        got["record"] = rec
    if value:
        got["value"] = val
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("kinds", ["mixed", "inf"])
@pytest.mark.parametrize("shape,name", FUSED_CASES, ids=["%d-%s" % (s[0], n) for s, n in FUSED_CASES])
def test_fused_mppi_update(shape, name, kinds, lam, dtype):
    """``mjmpc_mppi_fused_update``, plain and with the record and value outputs: 197 particles = 4 partials and the 256-thread
    merge; 4165 = 66 partials, more than 64, and the 1024-thread four-slice merge.  ``inf``: the spoiled q0 are all +inf, what
    the rollouts hand on - there only a whole diverged block can go wrong, and ``scattered`` / ``straddle`` are controls in the
    strict sense; ``mixed``: -inf and NaN of both signs too, which must weigh nothing wherever they sit."""
    P, H, A = shape
    pr = _problem(P, H, A)
    idx = dc.pattern(name, P, dc.FCH)
    q0, actions = dc.spoil_q0(pr["q0"], idx, only_inf=kinds == "inf"), _stored(pr["actions"], dtype)
    new = dc.ref_q0_mean(q0, actions, pr["mean"], lam, STEP)
    plain = _fused(q0, pr["actions"], pr["mean"], lam, STEP, 1, dtype)
    _close(plain["mean"], dc.shift(new, 1), "shifted mean")
    _close(plain["action"], new[0], "action")
    assert int(plain["counter"][0]) == 6
    full = _fused(q0, pr["actions"], pr["mean"], lam, STEP, 1, dtype, record=True, value=True)
    assert np.array_equal(full["mean"], plain["mean"]) and np.array_equal(full["action"], plain["action"])
    _close(full["record"], dc.ref_q0_record(q0, actions, lam), "record")
    _close(full["value"], dc.ref_q0_value(q0, lam, P), "value")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_mppi_update_draw_next(dtype):
    """``mjmpc_mppi_fused_update_draw_next``: the update as above, and the next step's samples are those drawn beside a
    population without a non-finite particle."""
    P, H, A = 197, 3, 2
    pr = _problem(P, H, A)
    q0 = dc.spoil_q0(pr["q0"], dc.pattern("block", P, dc.FCH))
    draw = dict(seed=2 ** 40 + 11, chol=np.diag([0.7, 1.3]))
    got = _fused(q0, pr["actions"], pr["mean"], 0.05, STEP, 1, dtype, draw=draw)
    clean = _fused(pr["q0"], pr["actions"], pr["mean"], 0.05, STEP, 1, dtype, draw=draw)
    new = dc.ref_q0_mean(q0, _stored(pr["actions"], dtype), pr["mean"], 0.05, STEP)
    _close(got["mean"], dc.shift(new, 1), "shifted mean")
    _close(got["action"], new[0], "action")
    assert np.isfinite(got["noise"]).all() and np.any(got["noise"] != 0)
    assert np.array_equal(got["noise"], clean["noise"])
    assert int(got["counter"][0]) == 6


# ---------------------------------------------------------------------------------------------------------- b. its batch
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fused_mppi_update_batch_rows_are_isolated(dtype):
    """``mjmpc_mppi_fused_update_batch``: row 0 with a diverged block, row 1 without any finite return, row 2 clean.  Rows 0
    and 2 are the reference and, bit for bit, their single calls; nothing is asserted about row 1's values."""
    torch = _torch()
    _l, lib = _lib()
    code, tdt = _types(dtype)
    E, P, H, A = 3, 197, 3, 2
    pr = _problem(P, H, A)
    rs = np.random.RandomState(2)
    actions = np.stack([pr["actions"], pr["actions"][::-1], pr["actions"] + 0.1 * rs.randn(P, H, A)])
    q0 = np.stack([dc.spoil_q0(pr["q0"], dc.pattern("block", P, dc.FCH)), np.full(P, np.inf), pr["q0"][::-1].copy()])
    means0 = np.stack([pr["mean"], pr["mean"] + 0.1, pr["mean"] - 0.1])
    lams, steps = np.array([0.05, 0.5, 1.0]), np.array([STEP, 0.5, STEP])
    d_means, out, counter = _dev(means0), _f64(E, A), _counter(8)
    ws = torch.zeros(lib.mjmpc_update_batch_workspace_bytes(E, P, H, A) // 8 + 1, dtype=torch.float64, device="cuda")
    _l.check(lib.mjmpc_mppi_fused_update_batch(code, E, P, H, A, _vp(_dev(q0)), _vp(_dev(actions, tdt)), _vp(_dev(lams)),
                                              _vp(_dev(steps)), 1, _vp(d_means), _vp(out), _vp(counter), _vp(ws), _stream()))
    torch.cuda.synchronize()
    got_means, got_out = d_means.cpu().numpy(), out.cpu().numpy()
    assert int(counter.item()) == 9                     # advanced once
    for e in (0, 2):
        new = dc.ref_q0_mean(q0[e], _stored(actions[e], dtype), means0[e], lams[e], steps[e])
        _close(got_means[e], dc.shift(new, 1), "row %d: shifted mean" % e)
        _close(got_out[e], new[0], "row %d: action" % e)
        one = _fused(q0[e], actions[e], means0[e], lams[e], steps[e], 1, dtype)
        assert np.array_equal(got_means[e], one["mean"]) and np.array_equal(got_out[e], one["action"]), e


# ---------------------------------------------------------------------------------------------------------- c. its combine
@pytest.mark.parametrize("lam", LAMS)
def test_fused_mppi_combine_with_a_diverged_shard(lam):
    """``mjmpc_mppi_fused_combine``: G = 3 shards of 70 particles (one block and a ragged 6), shard 1 without a finite return.
    Its record - from ``mjmpc_mppi_fused_update`` in record mode, which leaves the shard's mean alone - is {-inf, 0, 0...},
    what the arm engine's own record code writes for such a workgroup; the merge is the update over shards 0 and 2."""
    torch = _torch()
    _l, lib = _lib()
    G, n, H, A = 3, 70, 3, 2
    P = G * n
    pr = _problem(P, H, A)
    q0 = dc.spoil_q0(pr["q0"], np.arange(n, 2 * n))
    assert dc.whole_blocks(np.arange(n), n, dc.FCH) == [0, 1]
    recs = _f64(G, 2 + H * A, fill=float("nan"))
    for g in range(G):
        sl = slice(g * n, (g + 1) * n)
        mean, ws = _dev(pr["mean"]), _workspace(lib, n, H, A)[0]
        _l.check(lib.mjmpc_mppi_fused_update(_l.F64, n, H, A, _vp(_dev(q0[sl])), _vp(_dev(pr["actions"][sl])), lam, 0.0, -1,
                                             _vp(mean), None, _vp(recs[g]), None, None, None, _vp(ws), _stream()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(mean.cpu().numpy(), pr["mean"])           # record mode leaves the mean alone
    r = recs.cpu().numpy()
    assert r[1, 0] == -np.inf and np.array_equal(r[1, 1:], np.zeros(1 + H * A))
    for g in (0, 2):
        sl = slice(g * n, (g + 1) * n)
        _close(r[g], dc.ref_q0_record(q0[sl], pr["actions"][sl], lam), "record %d" % g)
    mean, act, counter = _dev(pr["mean"]), _f64(A), _counter(41)
    pinned = torch.zeros(A + 1, dtype=torch.float64).pin_memory()
    value = _f64(1, fill=float("nan"))
    _l.check(lib.mjmpc_mppi_fused_combine(_vp(recs), G, float(P), H, A, lam, STEP, 1, _vp(mean), _vp(act), _vp(value),
                                          _vp(pinned), _vp(counter), _stream()))
    torch.cuda.synchronize()
    new = dc.ref_q0_mean(q0, pr["actions"], pr["mean"], lam, STEP)
    _close(act.cpu().numpy(), new[0], "action")
    _close(pinned.numpy()[:A], new[0], "pinned action")
    assert pinned.numpy()[A] == 42.0 and int(counter.item()) == 42
    _close(mean.cpu().numpy(), dc.shift(new, 1), "shifted mean")
    _close(value.cpu().numpy(), dc.ref_q0_value(q0, lam, P), "value")


# ---------------------------------------------------------------------------------------------------------- d. the arm engine's
def test_arm_mppi_combine_ignores_a_record_without_a_finite_return(raw_arm):
    """``mjmpc_arm_mppi_combine`` on three synthetic records, the middle one {-inf, 0, zeros}: the merge of the other two,
    computed from the numbers (the guards this launch already has)."""
    torch = _torch()
    _l, lib = _lib()
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    eng = ArmRolloutEngine(raw_arm, dtype="f64")
    H, A = 4, 7
    rs = np.random.RandomState(12)
    recs = np.zeros((3, 2 + H * A))
    for g, m in ((0, -3.25), (2, -1.5)):
        recs[g] = np.concatenate([[m, rs.uniform(1.0, 40.0)], rs.randn(H * A) * 5.0])
    recs[1, 0] = -np.inf
    mean0 = 0.2 * rs.randn(H, A)
    M = max(recs[0, 0], recs[2, 0])
    sc = np.exp(np.array([recs[0, 0], recs[2, 0]], dc.LD) - dc.LD(M))
    S = sc[0] * dc.LD(recs[0, 1]) + sc[1] * dc.LD(recs[2, 1])
    W = (sc[0] * recs[0, 2:].astype(dc.LD) + sc[1] * recs[2, 2:].astype(dc.LD)).reshape(H, A)
    new = (dc.LD(1) - dc.LD(STEP)) * mean0.astype(dc.LD) + dc.LD(STEP) * (W / S)
    for rows in ((0, 1, 2), (0, 2)):
        d_recs, mean, mean_out, act, counter = _dev(recs[list(rows)]), _dev(mean0), _f64(H, A, fill=float("nan")), _f64(A), _counter(3)
        _l.check(lib.mjmpc_arm_mppi_combine(eng._h, eng._code, _vp(d_recs), len(rows), H, _vp(mean), _vp(mean_out), _vp(counter),
                                            STEP, 1, _vp(act), None, 0, None, None, _stream()))
        torch.cuda.synchronize()
        _close(mean_out.cpu().numpy(), dc.shift(new, 1), "shifted mean, records %s" % (rows,))
        _close(act.cpu().numpy(), new[0], "action")
        assert int(counter.item()) == 4 and np.array_equal(mean.cpu().numpy(), mean0)
    eng.close()


# ---------------------------------------------------------------------------------------------------------- e. sharded softmax
def _sharded_costs(case, pr, n):
    costs = pr["costs"].copy()
    if case == "dead_shard":                    # every particle of shard 1, every kind
        return dc.spoil_costs(costs, np.arange(n, 2 * n))
    if case == "step0_shard":                   # with time-based weights column 0 alone is dead in record 1
        costs[n:2 * n, 0] = np.inf
        return costs
    return dc.spoil_costs(costs, dc.pattern("block", n, dc.CHUNK))       # the control: a block inside shard 0


@pytest.mark.parametrize("case", ["dead_shard", "step0_shard", "block_in_shard0"])
@pytest.mark.parametrize("cov_mode", [0, 1, 2])
@pytest.mark.parametrize("alpha", [1, 0])
@pytest.mark.parametrize("tbw", [0, 1])
def test_sharded_softmax_records(tbw, alpha, cov_mode, case):
    """``mjmpc_softmax_stats`` per shard + ``mjmpc_softmax_combine`` over G = 3 records of 37 particles (two chunks of 16 and a
    ragged 5): mean, covariance, value and ``mjmpc_softmax_weights``.  Time-based weights together with a covariance are
    refused by ``mjmpc_softmax_stats`` before any launch (the scatter has one weight per particle): those cases assert that."""
    torch = _torch()
    _l, lib = _lib()
    G, n, H, A = 3, 37, 3, 2
    P = G * n
    pr = _problem(P, H, A)
    costs = _sharded_costs(case, pr, n)
    covinv = np.linalg.inv(pr["cov"])
    ci = covinv if alpha == 0 else None
    rlen = lib.mjmpc_softmax_record_len(H, A, tbw)
    d_gseq, d_cinv = _dev(pr["gseq"]), _dev(covinv)
    if tbw and cov_mode:
        rec, ws = _f64(rlen), _workspace(lib, n, H, A)[0]
        rc = lib.mjmpc_softmax_stats(_l.F64, n, H, A, _vp(_dev(costs[:n])), _vp(_dev(pr["actions"][:n])), _vp(_dev(pr["mean"])),
                                     _vp(d_cinv), _vp(d_gseq), 0, 1.0, alpha, tbw, 1, _vp(rec), _vp(ws), _stream())
        assert rc == -1 and b"exclusive" in lib.mjmpc_last_error()
        return
    for lam in LAMS:
        recs, wss = _f64(G, rlen, fill=float("nan")), []
        for g in range(G):
            sl = slice(g * n, (g + 1) * n)
            ws = _workspace(lib, n, H, A)[0]
            _l.check(lib.mjmpc_softmax_stats(_l.F64, n, H, A, _vp(_dev(costs[sl])), _vp(_dev(pr["actions"][sl])), _vp(_dev(pr["mean"])),
                                             _vp(d_cinv), _vp(d_gseq), 0, lam, alpha, tbw, int(cov_mode != 0), _vp(recs[g]), _vp(ws),
                                             _stream()))
            wss.append(ws)
        mean, cov, value, wnorm = _dev(pr["mean"]), _dev(pr["cov"]), _f64(1, fill=float("nan")), _f64(2, fill=float("nan"))
        _l.check(lib.mjmpc_softmax_combine(_vp(recs), G, H, A, tbw, lam, STEP, cov_mode, float(P), _vp(mean),
                                           _vp(cov) if cov_mode else None, _vp(value), _vp(wnorm), _stream()))
        torch.cuda.synchronize()
        what = "lam %g" % lam
        assert np.isfinite(recs.cpu().numpy()[[0, 2]]).all(), what
        _close(mean.cpu().numpy(), dc.ref_softmax_mean(costs, pr["actions"], pr["mean"], pr["gseq"], lam, STEP, bool(tbw), ci), what + ": mean")
        if cov_mode:
            _close(cov.cpu().numpy(), dc.ref_softmax_cov(costs, pr["actions"], pr["mean"], pr["cov"], pr["gseq"], lam, STEP, cov_mode,
                                                         bool(tbw), ci), what + ": covariance")
        _close(value.cpu().numpy(), dc.ref_softmax_value(costs, pr["actions"], pr["mean"], pr["gseq"], lam, P, ci), what + ": value")
        if not tbw:                             # (the weights entry reads one weight per particle)
            w = _f64(P)
            for g in range(G):
                _l.check(lib.mjmpc_softmax_weights(n, H, A, _vp(wnorm), _vp(wss[g]), _vp(w[g * n:(g + 1) * n]), _stream()))
            torch.cuda.synchronize()
            w = w.cpu().numpy()
            dead = ~dc.finite_columns(costs, pr["gseq"])[:, 0]
            assert dead.any() and np.all(w[dead] == 0)
            _close(w, dc.ref_softmax_weights(costs, pr["actions"], pr["mean"], pr["gseq"], lam, ci), what + ": weights")
            np.testing.assert_allclose(w.sum(), 1.0, **TOL)


# ---------------------------------------------------------------------------------------------------------- f. softmax batches
@pytest.mark.parametrize("cov_mode", [1, 2])
@pytest.mark.parametrize("lams", [(0.05, 1.0), (1.0, 0.05)])
def test_dmd_update_batch(lams, cov_mode):
    """``mjmpc_dmd_update_batch``: E = 2 rows of 37 particles, row 0 with a diverged chunk of 16."""
    torch = _torch()
    _l, lib = _lib()
    E, P, H, A = 2, 37, 3, 2
    pr = _problem(P, H, A)
    idx = dc.pattern("block", P, dc.CHUNK)
    costs = np.stack([dc.spoil_costs(pr["costs"], idx), pr["costs"][::-1]])
    actions = np.stack([pr["actions"], pr["actions"][::-1]])
    means0, covs0 = np.stack([pr["mean"], pr["mean"] + 0.1]), np.stack([pr["cov"], 0.5 * pr["cov"]])
    steps, beta = np.array([STEP, 0.7]), np.array([0.05, 0.3])
    means, covs, out, counter = _dev(means0), _dev(covs0), _f64(E, A), _counter(0)
    ws = torch.zeros(lib.mjmpc_dmd_batch_workspace_bytes(E, P, H, A) // 8, dtype=torch.float64, device="cuda")
    _l.check(lib.mjmpc_dmd_update_batch(_l.F64, E, P, H, A, _vp(_dev(costs)), _vp(_dev(actions)), _vp(_dev(pr["gseq"])),
                                        _vp(_dev(np.array(lams))), _vp(_dev(steps)), cov_mode, _vp(_dev(beta)), 1, _vp(means),
                                        _vp(covs), _vp(out), _vp(counter), _vp(ws), _stream()))
    torch.cuda.synchronize()
    assert int(counter.item()) == 1
    for e in range(E):
        new = dc.ref_softmax_mean(costs[e], actions[e], means0[e], pr["gseq"], lams[e], steps[e])
        _close(means.cpu().numpy()[e], dc.shift(new, 1), "row %d: shifted mean" % e)
        _close(out.cpu().numpy()[e], new[0], "row %d: action" % e)
        cov = dc.ref_softmax_cov(costs[e], actions[e], means0[e], covs0[e], pr["gseq"], lams[e], steps[e], cov_mode)
        _close(covs.cpu().numpy()[e], cov + dc.LD(beta[e]) * np.eye(A), "row %d: covariance" % e)


@pytest.mark.parametrize("tbw", [0, 1])
@pytest.mark.parametrize("alpha", [1, 0])
@pytest.mark.parametrize("betas", [(0.05, 1.0), (1.0, 0.05)])
def test_mppiq_update_batch(betas, alpha, tbw):
    """``mjmpc_mppiq_update_batch``: E = 2 rows of 37 particles, row 0 with a chunk of 16 whose costs are +inf at every step
    (tests/test_batched_mppiq_gpu.py: a single +inf step is not a clean case for the TD(lambda) returns)."""
    torch = _torch()
    _l, lib = _lib()
    E, P, H, A = 2, 37, 3, 2
    pr = _problem(P, H, A)
    costs = np.stack([pr["costs"], pr["costs"][::-1]])
    costs[0, dc.pattern("block", P, dc.CHUNK)] = np.inf
    actions = np.stack([pr["actions"], pr["actions"][::-1]])
    means0 = np.stack([pr["mean"], pr["mean"] + 0.1])
    td_lam, gamma, steps = np.array([0.85, 0.0]), 0.97, np.array([STEP, 0.7])
    wseq = np.stack([np.cumprod([1.0] + [gamma * l] * (H - 2)) for l in td_lam])
    wzero = np.array([int(bool(np.any(w == 0))) for w in wseq], np.int32)
    cov_diag = [(0.9, 0.5), (0.6, 1.1)]
    covinv = np.stack([np.linalg.inv(np.diag(c)) for c in cov_diag])
    means, out, counter = _dev(means0), _f64(E, A), _counter(0)
    assert lib.mjmpc_mppiq_batch_supported(E, P, H, A, tbw)
    ws = torch.zeros(lib.mjmpc_mppiq_batch_workspace_bytes(E, P, H, A, tbw) // 8, dtype=torch.float64, device="cuda")
    _l.check(lib.mjmpc_mppiq_update_batch(_l.F64, E, P, H, A, _vp(_dev(costs)), _vp(_dev(actions)), _vp(_dev(np.array(betas))),
                                          _vp(_dev(steps)), _vp(_dev(td_lam)), _vp(_dev(wseq)), _vp(_dev(wzero)), gamma, alpha,
                                          _vp(_dev(covinv)) if alpha == 0 else None, tbw, 1, _vp(means), _vp(out), _vp(counter),
                                          _vp(ws), _stream()))
    torch.cuda.synchronize()
    assert int(counter.item()) == 1
    for e in range(E):
        new = dc.ref_mppiq_mean(costs[e], actions[e], means0[e], betas[e], gamma, td_lam[e], steps[e], bool(tbw),
                                covinv[e] if alpha == 0 else None)
        _close(means.cpu().numpy()[e], dc.shift(new, 1), "row %d: shifted mean" % e)
        _close(out.cpu().numpy()[e], new[0], "row %d: action" % e)


# ---------------------------------------------------------------------------------------------------------- g. PFMPC weights
@pytest.mark.parametrize("lam", LAMS)
def test_pf_weights_with_every_threads_first_stride_diverged(lam):
    """``mjmpc_pf_weights`` and ``_batch``: M = 1100, particles [0, 1024) not finite - the first stride of every thread of the
    1024-thread workgroup.  Zero weight there, the reference elsewhere, sum 1."""
    torch = _torch()
    _l, lib = _lib()
    M = 1100
    rs = np.random.RandomState(6)
    clean = rs.uniform(0.5, 4.0, M)
    q0 = dc.spoil_q0(clean, np.arange(1024))
    want = dc.ref_pf_weights(q0, lam)
    w, first = _f64(M, fill=float("nan")), _f64(1)
    _l.check(lib.mjmpc_pf_weights(M, _vp(_dev(q0)), lam, 17, 0, _vp(_counter(2)), _vp(w), _vp(first), _stream()))
    rows = np.stack([q0, clean[::-1]])
    lams = np.array([lam, 0.3])
    wb, firstb = _f64(2, M, fill=float("nan")), _f64(2)
    _l.check(lib.mjmpc_pf_weights_batch(2, M, _vp(_dev(rows)), _vp(_dev(lams)), _vp(_dev(np.array([17, 18], np.int64))), 0,
                                        _vp(_counter(2)), _vp(wb), _vp(firstb), _stream()))
    torch.cuda.synchronize()
    w, wb = w.cpu().numpy(), wb.cpu().numpy()
    for got in (w, wb[0]):
        assert np.all(got[:1024] == 0)
        _close(got, want, "weights")
        np.testing.assert_allclose(got.sum(), 1.0, **TOL)
    assert np.array_equal(w, wb[0])
    _close(wb[1], dc.ref_pf_weights(rows[1], 0.3), "clean row")


# ---------------------------------------------------------------------------------------------------------- h. CEM selection
def _cem_case():
    P, H, A, k = 197, 3, 2, 20
    pr = _problem(P, H, A)
    idx = dc.pattern("block", P, dc.FCH)
    q0 = dc.spoil_q0(pr["q0"], idx)
    # (all four kinds inside the block: by its bits alone a -inf or a NaN with the sign bit set would rank first)
    assert set(np.unique(idx % 4)) == {0, 1, 2, 3} and not set(dc.elite_ids(q0, k)) & set(idx)
    return P, H, A, k, pr, idx, q0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cem_elite_sums_rank_non_finite_last(dtype):
    """``mjmpc_cem_elite_sums`` (q0 from the workspace, and as the gathered q_all): k elites, the reference's set - a NaN with
    the sign bit set and a -inf are never elite."""
    torch = _torch()
    _l, lib = _lib()
    code, tdt = _types(dtype)
    P, H, A, k, pr, idx, q0 = _cem_case()
    actions = _stored(pr["actions"], dtype)
    want = actions[dc.elite_ids(q0, k)].astype(dc.LD).sum(axis=0).reshape(-1)
    d_act, d_q0 = _dev(pr["actions"], tdt), _dev(q0)
    for gathered in (False, True):
        ws, q0_view = _workspace(lib, P, H, A)
        q0_view.copy_(d_q0)
        rec = _f64(1 + H * A, fill=float("nan"))
        _l.check(lib.mjmpc_cem_elite_sums(code, P, H, A, _vp(d_act), _vp(d_q0) if gathered else None, P, 0, k, _vp(rec), _vp(ws),
                                          _stream()))
        torch.cuda.synchronize()
        rec = rec.cpu().numpy()
        assert rec[0] == k
        _close(rec[1:], want, "sum of the elite rows")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("full", [1, 0])
def test_cem_select_moments_rank_non_finite_last(full, dtype):
    """``mjmpc_cem_select_moments`` and ``_batch`` (each with its finish launch): mean and covariance of the reference's elites."""
    torch = _torch()
    _l, lib = _lib()
    code, tdt = _types(dtype)
    P, H, A, k, pr, idx, q0 = _cem_case()
    step = 0.8
    assert lib.mjmpc_cem_fused_supported(P, P, k, H, A)
    _, new_mean, new_cov = dc.ref_cem(q0, _stored(pr["actions"], dtype), pr["mean"], pr["cov"], k, step, full)
    # -- single
    ws, q0_view = _workspace(lib, P, H, A)
    q0_view.copy_(_dev(q0))
    d_act, mean, cov, counter, status = _dev(pr["actions"], tdt), _dev(pr["mean"]), _dev(pr["cov"]), _counter(3), torch.zeros(
        1, dtype=torch.int32, device="cuda")
    chol, out = _f64(A, A), _f64(A)
    _l.check(lib.mjmpc_cem_select_moments(code, P, H, A, _vp(d_act), None, P, 0, k, _vp(mean), _vp(cov), _vp(counter), _vp(ws), _stream()))
    _l.check(lib.mjmpc_cem_finish(code, P, H, A, k, None, 1, float(k), full, step, 0, _vp(mean), _vp(cov), _vp(chol), _vp(status),
                                  None, 0.0, _vp(out), None, _vp(counter), None, 0, 0, 0, _vp(ws), _stream()))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and int(counter.item()) == 4
    _close(mean.cpu().numpy(), dc.shift(new_mean, 0), "shifted mean")
    _close(cov.cpu().numpy(), new_cov, "covariance")
    _close(out.cpu().numpy(), new_mean[0], "action")
    # -- batch: row 0 as above, row 1 clean
    E = 2
    qb, ab = np.stack([q0, pr["q0"][::-1]]), np.stack([pr["actions"], pr["actions"][::-1]])
    means0, covs0 = np.stack([pr["mean"], pr["mean"] + 0.1]), np.stack([pr["cov"], 0.5 * pr["cov"]])
    ks, steps = np.array([k, k], np.int64), np.array([step, 0.6])
    assert lib.mjmpc_cem_batch_supported(E, P, k, H, A)
    wsb = torch.zeros(lib.mjmpc_cem_batch_workspace_bytes(E, P, k, H, A) // 8, dtype=torch.float64, device="cuda")
    means, covs, counter, statusb = _dev(means0), _dev(covs0), _counter(3), torch.zeros(E, dtype=torch.int32, device="cuda")
    d_k, d_ab, outb = _dev(ks), _dev(ab, tdt), _f64(E, A)
    _l.check(lib.mjmpc_cem_select_moments_batch(code, E, P, H, A, _vp(d_ab), _vp(_dev(qb)), _vp(d_k), _vp(means), _vp(covs),
                                                _vp(counter), _vp(wsb), _stream()))
    _l.check(lib.mjmpc_cem_finish_batch(code, E, P, H, A, _vp(d_k), full, _vp(_dev(steps)), 0, _vp(means), _vp(covs), None,
                                        _vp(statusb), None, None, _vp(outb), _vp(counter), None, None, 0, _vp(wsb), _stream()))
    torch.cuda.synchronize()
    assert not statusb.cpu().numpy().any() and int(counter.item()) == 4
    assert np.array_equal(means.cpu().numpy()[0], mean.cpu().numpy()) and np.array_equal(covs.cpu().numpy()[0], cov.cpu().numpy())
    for e in range(E):
        _, m, c = dc.ref_cem(qb[e], _stored(ab[e], dtype), means0[e], covs0[e], k, steps[e], full)
        _close(means.cpu().numpy()[e], dc.shift(m, 0), "row %d: shifted mean" % e)
        _close(covs.cpu().numpy()[e], c, "row %d: covariance" % e)


# ---------------------------------------------------------------------------------------------------------- i. random shooting
def _rs_single(q0, actions_padded, P, mean0, step):
    """mjmpc_rs_best + mjmpc_rs_combine on q0 [P] -> (record, mean)."""
    torch = _torch()
    _l, lib = _lib()
    H, A = mean0.shape
    ws, q0_view = _workspace(lib, P, H, A)
    q0_view.copy_(_dev(q0))
    rec, mean = _f64(2 + H * A, fill=float("nan")), _dev(mean0)
    _l.check(lib.mjmpc_rs_best(_l.F64, P, H, A, _vp(actions_padded), 0, _vp(rec), _vp(ws), _stream()))
    _l.check(lib.mjmpc_rs_combine(_vp(rec), 1, H, A, step, _vp(mean), _stream()))
    torch.cuda.synchronize()
    return rec.cpu().numpy(), mean.cpu().numpy()


def _rs_actions(pr):
    """The actions with one more row of NaN behind the population: a pick of index P shows as NaN, inside this allocation."""
    P, H, A = pr["actions"].shape
    return _dev(np.concatenate([pr["actions"], np.full((1, H, A), np.nan)]))


def test_rs_single_path_picks_particle_0_without_a_finite_return():
    """``mjmpc_rs_best`` + ``mjmpc_rs_combine`` on a row without a finite entry: particle 0, as ``mjmpc_rs_update_batch``."""
    P, H, A = 197, 3, 2
    pr = _problem(P, H, A)
    q0 = dc.spoil_q0(pr["q0"], np.arange(P))
    rec, mean = _rs_single(q0, _rs_actions(pr), P, pr["mean"], 0.7)
    assert rec[1] == 0.0 and rec[0] == np.inf
    assert np.array_equal(rec[2:], pr["actions"][0].reshape(-1))
    _close(mean, dc.ref_rs(q0, pr["actions"], pr["mean"], 0.7), "mean")


def test_rs_ranks_non_finite_last_on_both_paths():
    """A row with a diverged block (NaN of both signs and -inf included) on the single path and in ``mjmpc_rs_update_batch``,
    beside a row without a finite entry."""
    torch = _torch()
    _l, lib = _lib()
    P, H, A = 197, 3, 2
    pr = _problem(P, H, A)
    q0 = dc.spoil_q0(pr["q0"], dc.pattern("block", P, dc.FCH))
    best = dc.rs_best(q0)
    assert np.isfinite(q0[best])
    rec, mean = _rs_single(q0, _rs_actions(pr), P, pr["mean"], 0.7)
    assert rec[1] == best and rec[0] == q0[best]
    _close(mean, dc.ref_rs(q0, pr["actions"], pr["mean"], 0.7), "mean")
    E = 2
    rows = np.stack([q0, dc.spoil_q0(pr["q0"], np.arange(P))])
    actions, means0, steps = np.stack([pr["actions"], pr["actions"][::-1]]), np.stack([pr["mean"], pr["mean"] + 0.1]), np.array([0.7, 0.4])
    means, out, counter = _dev(means0), _f64(E, A), _counter(3)
    picked = torch.full((E,), -1, dtype=torch.int64, device="cuda")
    _l.check(lib.mjmpc_rs_update_batch(_l.F64, E, P, H, A, _vp(_dev(rows)), _vp(_dev(actions)), _vp(_dev(steps)), 1, _vp(means),
                                       _vp(out), _vp(counter), _vp(picked), _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(picked.cpu().numpy(), [best, 0]) and int(counter.item()) == 4
    for e in range(E):
        new = dc.ref_rs(rows[e], actions[e], means0[e], steps[e])
        _close(means.cpu().numpy()[e], dc.shift(new, 1), "row %d: shifted mean" % e)
        _close(out.cpu().numpy()[e], new[0], "row %d: action" % e)
    assert np.array_equal(np.asarray(dc.shift(mean, 1)), means.cpu().numpy()[0])          # the batch row = the single path


# ---------------------------------------------------------------------------------------------------------- j. real kernel output
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("scale,mid_horizon", [(1e9, False), (300.0, True)])
def test_a_diverged_model_shard_of_the_arm_engine(raw_arm, scale, mid_horizon, lam):
    """The rollout kernels' way of marking a particle meets the update kernels' way of ignoring it: four shards with their own
    start states, one of them beyond what the simulation survives, ``set_reset_returns("inf")``.  The diverged shard is exactly
    one aligned block of the fused update; the engine's own costs and actions go through ``mjmpc_traj_cost`` +
    ``mjmpc_mppi_fused_update`` and through ``softmax_update`` with time-based weights.  Start velocities scaled by 1e9 (the
    scale of test_reset_returns_inf_option_arm) reset every particle of the shard within the first env step - measured: all 64
    carry +inf from step 0 -; scaled by 300 the shard survives two env steps and all 64 turn +inf at step 2, mid-horizon
    (by 1000: at step 1; by 100: none diverges)."""
    torch = _torch()
    _l, lib = _lib()
    from mjmpc_amd.control._device import DeviceUpdater
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    P, H, A, S = 256, 6, 7, 4
    eng = ArmRolloutEngine(raw_arm, dtype="f64", num_shards=S)
    rs = np.random.RandomState(9)
    mean0, noise = 0.3 * rs.standard_normal((H, A)), 0.5 * rs.standard_normal((P, H, A))
    vels = [1.0, scale, 3.0, 1.0]
    tgt = np.array([0.15, -0.1, 0.2])
    eng.set_env_state([dict(qp=rs.uniform(-0.5, 0.5, 7), qv=rs.uniform(-1, 1, 7) * vl, target_pos=tgt) for vl in vels])
    eng.set_reset_returns("inf")
    _, rew, actions, _, _, _ = eng.rollout(P, H, mean0, noise)
    eng.close()
    costs = -rew
    bad = np.flatnonzero(~np.isfinite(costs).all(axis=1))
    first = np.argmax(np.isinf(costs[bad]), axis=1)
    print("diverged particles %d..%d, first +inf step per particle: %s" % (bad.min(), bad.max(), np.bincount(first, minlength=H)))
    assert np.array_equal(bad, np.arange(64, 128)) and dc.whole_blocks(bad, P, dc.FCH) == [1]
    assert np.all(costs[bad, -1] == np.inf) and not np.isnan(costs).any()
    assert bool((first > 0).any()) == mid_horizon, "the diverged shard's particles turn +inf %s" % ("at step 0" if mid_horizon else "later")
    for p, t in zip(bad[:8], first[:8]):
        assert np.isinf(costs[p, t:]).all() and np.isfinite(costs[p, :t]).all()         # +inf from the reset's env step on
    gseq = np.cumprod([1.0] + [0.97] * (H - 1))
    # -- mjmpc_traj_cost + mjmpc_mppi_fused_update on the workspace's q0
    ws, q0_view = _workspace(lib, P, H, A)
    d_costs, d_act, mean, out = _dev(costs), _dev(actions), _dev(mean0), _f64(A)
    _l.check(lib.mjmpc_traj_cost(_l.F64, P, H, A, _vp(d_costs), _vp(_dev(gseq)), 0, _vp(ws), _stream()))
    _l.check(lib.mjmpc_mppi_fused_update(_l.F64, P, H, A, None, _vp(d_act), lam, STEP, 1, _vp(mean), _vp(out), None, None, None,
                                         None, _vp(ws), _stream()))
    torch.cuda.synchronize()
    q0 = q0_view.cpu().numpy()
    assert np.all(q0[bad] == np.inf) and np.isfinite(np.delete(q0, bad)).all()
    new = dc.ref_softmax_mean(costs, actions, mean0, gseq, lam, STEP)
    _close(mean.cpu().numpy(), dc.shift(new, 1), "fused update: shifted mean")
    _close(out.cpu().numpy(), new[0], "fused update: action")
    # -- the softmax path with time-based weights
    dev = DeviceUpdater(H, A, gseq)
    dev.set_mean(mean0)
    dev.softmax_update(costs, actions, lam, STEP, time_based_weights=True)
    _close(dev.get_mean(), dc.ref_softmax_mean(costs, actions, mean0, gseq, lam, STEP, True), "softmax update, time-based weights")
