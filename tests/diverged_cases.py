"""What the tests of diverged returns share (tests/test_diverged_cases_cpu.py, tests/test_diverged_returns_gpu.py).

DESIGN 7's promise: a rollout that diverged numerically carries a non-finite return and gets zero weight - it is never elite
and never the best -, so the updated distribution equals the update over the finite particles alone.  The kernels reduce the
particles in aligned blocks (``FCH`` per workgroup in the fused MPPI update, ``CHUNK`` in the softmax partial moments) and merge
the blocks max-rescaled; a block, a record or a merge slice WITHOUT a finite return is where that arithmetic can turn
``exp(-inf + inf)`` or ``0 * NaN`` into a NaN mean.  This module makes such populations and the plain references:

``pattern(name, P, B)``     which particles to spoil, by their position relative to the blocks of ``B`` particles;
``spoil_costs`` / ``spoil_q0``  write a fixed mix of non-finite kinds into a copy;
the ``ref_*`` functions     the same operation in plain form over the particles whose return is finite, in ``np.longdouble``.

The rule for every entry point is the one ``traj_cost_body`` and ``pf_weights_body`` state: not finite means zero weight /
ranked last.  Whether a return is finite is decided in float64, in the kernels' summation order (``1e308 + 1e308`` overflows
there and not in long double); the arithmetic on the kept particles is long double.  With time-based weights a particle is
dropped from a column only where that column's cost-to-go is not finite.
"""
import numpy as np

FCH = 64        # particles per workgroup of the fused MPPI update (csrc/update.hip)
CHUNK = 16      # particles per workgroup of the softmax partial moments (csrc/update.hip)
LD = np.longdouble

PATTERNS = ("scattered", "block", "first_block", "ragged_last", "straddle", "all_but_one", "slice")
WHOLE_BLOCK = ("block", "first_block", "ragged_last", "slice", "all_but_one")     # contain a whole aligned block
CONTROLS = ("scattered", "straddle")                                               # contain none


def whole_blocks(idx, P, B):
    """The aligned blocks [b B, min((b + 1) B, P)) every particle of which is in ``idx``."""
    bad = np.zeros(P, bool)
    bad[np.asarray(idx, int)] = True
    return [b for b in range((P + B - 1) // B) if bad[b * B:min((b + 1) * B, P)].all()]


def pattern(name, P, B):
    """Sorted indices of the particles to spoil.  ``slice``: every block of slice 1 of the fused update's four-slice merge
    (blocks [per, 2 per), per = ceil(nb / 4)).  Asserts what the name promises, so that a change of the block size cannot
    quietly turn a whole-block case into a scattered one."""
    nb = (P + B - 1) // B
    assert P % B != 0 and nb >= 3, "the shapes keep a ragged last block and a middle block"
    if name == "scattered":
        idx = np.array([3, P // 3, (2 * P) // 3 + 1, P - 1])
    elif name == "block":
        idx = np.arange(B, 2 * B)
    elif name == "first_block":
        idx = np.arange(0, B)
    elif name == "ragged_last":
        idx = np.arange(P - P % B, P)
    elif name == "straddle":
        idx = np.arange(B // 2, B + B // 2)
    elif name == "all_but_one":
        idx = np.setdiff1d(np.arange(P), [(nb // 2) * B + B // 3])
    elif name == "slice":
        per = (nb + 3) // 4
        idx = np.arange(per * B, min(2 * per * B, P))
    else:
        raise ValueError(name)
    idx = np.unique(idx)
    assert idx.size and idx.min() >= 0 and idx.max() < P
    assert idx.size < P, "every pattern leaves a finite particle"
    whole = whole_blocks(idx, P, B)
    if name in WHOLE_BLOCK:
        assert whole, "%s at P = %d, B = %d holds no whole aligned block" % (name, P, B)
    else:
        assert not whole, "%s at P = %d, B = %d holds a whole aligned block" % (name, P, B)
    if name == "slice":
        per = (nb + 3) // 4
        assert per >= 1 and 2 * per <= nb and whole == list(range(per, 2 * per))
    return idx


# ---------------------------------------------------------------------------------------------------------- the spoilers
N_COST_KINDS = 6


def spoil_costs(costs, idx):
    """A copy of ``costs`` [P][H] with the particles ``idx`` made non-finite, the kind cycling with the particle index (so
    every block holds several): 0 a NaN, 1 a +inf, 2 a -inf (each at the middle step), 3 two 1e308 at steps 0 and 1 (finite
    costs whose cost-to-go overflows), 4 +inf at the last step only, 5 +inf at step 0 only."""
    out = np.array(costs, dtype=np.float64, copy=True)
    H = out.shape[1]
    assert H >= 2
    for p in np.asarray(idx, int):
        kind = p % N_COST_KINDS
        if kind == 0:
            out[p, H // 2] = np.nan
        elif kind == 1:
            out[p, H // 2] = np.inf
        elif kind == 2:
            out[p, H // 2] = -np.inf
        elif kind == 3:
            out[p, 0] = out[p, 1] = 1e308
        elif kind == 4:
            out[p, H - 1] = np.inf
        else:
            out[p, 0] = np.inf
    return out


def q0_kinds():
    """+inf, -inf, and a NaN of either sign bit."""
    nans = np.array([0x7FF8000000000000, 0xFFF8000000000000], dtype=np.uint64).view(np.float64)
    assert np.isnan(nans).all() and not np.signbit(nans[0]) and np.signbit(nans[1])
    return np.array([np.inf, -np.inf, nans[0], nans[1]])


def spoil_q0(q0, idx, only_inf=False):
    """A copy of ``q0`` [P] with the particles ``idx`` set to +inf, -inf, NaN, NaN with the sign bit, cycling with the index;
    ``only_inf``: to +inf alone, what the rollout kernels and ``traj_cost_body`` hand on (a NaN or -inf q0 reaches an entry
    only from a caller's own array)."""
    out = np.array(q0, dtype=np.float64, copy=True)
    kinds = np.full(4, np.inf) if only_inf else q0_kinds()
    idx = np.asarray(idx, int)
    out[idx] = kinds[idx % 4]
    return out


# ---------------------------------------------------------------------------------------------------------- the references
def cost_to_go64(costs, gseq):
    """control_utils.cost_to_go in float64 and the kernels' order (reverse running sum, then / gseq): decides finiteness."""
    costs, gseq = np.asarray(costs, np.float64), np.asarray(gseq, np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        if np.any(gseq == 0):
            return costs.copy()
        return np.cumsum((gseq * costs)[:, ::-1], axis=-1)[:, ::-1] / gseq


def cost_to_go_ld(costs, gseq):
    costs, gseq = np.asarray(costs, LD), np.asarray(gseq, LD).reshape(1, -1)
    if np.any(gseq == 0):
        return costs.copy()
    return np.cumsum((gseq * costs)[:, ::-1], axis=-1)[:, ::-1] / gseq


def finite_columns(costs, gseq):
    """[P][H] bool: the cost-to-go of particle p from step t on is finite."""
    return np.isfinite(cost_to_go64(costs, gseq))


def _control_cost_ld(actions, mean, covinv):
    """MPPI._control_costs' per-step term: sum_a 0.5 u_n (mean + 2 delta), u_n = mean cov^-1."""
    mean = np.asarray(mean, LD)
    un = mean @ np.asarray(covinv, LD)
    return np.sum(LD(0.5) * un[None] * (mean[None] + LD(2) * (np.asarray(actions, LD) - mean[None])), axis=-1)


def _weights_ld(x, keep):
    """Column-wise softmax of x [P][Hw] over the rows where ``keep``; 0 elsewhere.  -> (w, xmax [Hw], sum of exp(x - xmax))."""
    x = np.where(keep, x, -np.inf).astype(LD)
    xmax = x.max(axis=0)
    with np.errstate(all="ignore"):
        e = np.where(keep, np.exp(x - xmax[None]), LD(0))
    s = e.sum(axis=0)
    return e / s[None], xmax, s


def ref_softmax_x(costs, actions, mean, gseq, lam, tbw=False, covinv=None):
    """x [P][Hw] = (-1 / lam) (cost_to_go(costs) + lam cost_to_go(control cost)) in long double and the mask of the finite
    columns (Hw = H with time-based weights, else the first column)."""
    keep = finite_columns(costs, gseq)
    clean = np.where(np.isfinite(np.asarray(costs, np.float64)), costs, 0.0)
    q = cost_to_go_ld(clean, gseq)
    if covinv is not None:
        q = q + LD(lam) * cost_to_go_ld(_control_cost_ld(actions, mean, covinv), gseq)
    x = (LD(-1) / LD(lam)) * q
    return (x, keep) if tbw else (x[:, :1], keep[:, :1])


def ref_softmax_mean(costs, actions, mean, gseq, lam, step, tbw=False, covinv=None):
    """MPPI / DMD-MPC mean update over the finite particles (per column with time-based weights)."""
    x, keep = ref_softmax_x(costs, actions, mean, gseq, lam, tbw, covinv)
    w, _, _ = _weights_ld(x, keep)
    H = np.shape(actions)[1]
    w = np.broadcast_to(w, (w.shape[0], H))
    weighted = np.einsum("pt,pta->ta", w, np.asarray(actions, LD))
    return (LD(1) - LD(step)) * np.asarray(mean, LD) + LD(step) * weighted


def ref_softmax_cov(costs, actions, mean, cov, gseq, lam, step, cov_mode, tbw=False, covinv=None):
    """DMD-MPC covariance update (1 diagonal, 2 full) with the weights of column 0, scatter about the mean before the update."""
    x, keep = ref_softmax_x(costs, actions, mean, gseq, lam, tbw, covinv)
    w = _weights_ld(x, keep)[0][:, 0]
    d = np.asarray(actions, LD) - np.asarray(mean, LD)[None]
    upd = np.einsum("p,pti,ptj->ij", w, d, d) / LD(np.shape(actions)[1])
    if cov_mode == 1:
        upd = np.diag(np.diag(upd))
    return (LD(1) - LD(step)) * np.asarray(cov, LD) + LD(step) * upd


def ref_softmax_value(costs, actions, mean, gseq, lam, P_total, covinv=None):
    """-lam logsumexp(x, b = 1 / P_total) over the finite particles (the kernels' P_total counts every particle)."""
    x, keep = ref_softmax_x(costs, actions, mean, gseq, lam, False, covinv)
    _, xmax, s = _weights_ld(x, keep)
    return -LD(lam) * (np.log(s[0] / LD(P_total)) + xmax[0])


def ref_softmax_weights(costs, actions, mean, gseq, lam, covinv=None):
    """The normalised per-particle weights (column 0); 0 for a particle without a finite return."""
    x, keep = ref_softmax_x(costs, actions, mean, gseq, lam, False, covinv)
    return _weights_ld(x, keep)[0][:, 0]


def ref_q0_mean(q0, actions, mean, lam, step):
    """The fused MPPI update from q0 [P]: weights softmax(-q0 / lam) over the finite q0."""
    q0 = np.asarray(q0, np.float64)
    keep = np.isfinite(q0)[:, None]
    x = (LD(-1) / LD(lam)) * np.where(keep[:, 0], q0, 0.0).astype(LD)
    w = _weights_ld(x[:, None], keep)[0][:, 0]
    return (LD(1) - LD(step)) * np.asarray(mean, LD) + LD(step) * np.einsum("p,pta->ta", w, np.asarray(actions, LD))


def ref_q0_value(q0, lam, P_total):
    q0 = np.asarray(q0, np.float64)
    keep = np.isfinite(q0)[:, None]
    x = (LD(-1) / LD(lam)) * np.where(keep[:, 0], q0, 0.0).astype(LD)
    _, xmax, s = _weights_ld(x[:, None], keep)
    return -LD(lam) * (np.log(s[0] / LD(P_total)) + xmax[0])


def ref_q0_record(q0, actions, lam):
    """[xmax | S | W[H*A]] of the fused update over the finite q0."""
    q0 = np.asarray(q0, np.float64)
    keep = np.isfinite(q0)[:, None]
    x = (LD(-1) / LD(lam)) * np.where(keep[:, 0], q0, 0.0).astype(LD)
    w, xmax, s = _weights_ld(x[:, None], keep)
    W = np.einsum("p,pta->ta", w[:, 0] * s[0], np.asarray(actions, LD)).reshape(-1)
    return np.concatenate([[xmax[0], s[0]], W])


def ref_pf_weights(q0, lam):
    """PFMPC weights from q0 [M]: softmax(-q0 / lam) over the finite q0, 0 elsewhere."""
    q0 = np.asarray(q0, np.float64)
    keep = np.isfinite(q0)[:, None]
    x = (LD(-1) / LD(lam)) * np.where(keep[:, 0], q0, 0.0).astype(LD)
    return _weights_ld(x[:, None], keep)[0][:, 0]


def shift(mean, mode):
    """OLGaussianMPC._shift: 0 'null', 1 'repeat'; < 0 none."""
    mean = np.array(mean, copy=True)
    if mode < 0:
        return mean
    last = mean[-1].copy()
    mean[:-1] = mean[1:]
    mean[-1] = 0.0 if mode == 0 else last
    return mean


def ref_mppiq_mean(costs, actions, mean, beta, gamma, td_lam, step, tbw=False, covinv=None):
    """MPPIQ update without Q estimates over the particles whose costs are finite at every step: TD(lambda) returns of
    total = cost + beta * per-step control cost (``covinv`` given: alpha = 0), weights softmax(-returns / beta)."""
    costs = np.asarray(costs, np.float64)
    keep_p = np.isfinite(costs).all(axis=1)
    P, H = costs.shape
    total = np.where(keep_p[:, None], costs, 0.0).astype(LD)
    if covinv is not None:
        total = total + LD(beta) * _control_cost_ld(actions, mean, covinv)
    q = np.zeros((P, H), LD)
    q[:, -1] = total[:, -1]
    out = q.copy()
    if H > 1:
        td = total[:, :-1] + LD(gamma) * q[:, 1:] - q[:, :-1]
        wseq = np.cumprod(np.array([1.0] + [gamma * td_lam] * (H - 2), LD)).reshape(1, H - 1)
        out[:, :-1] = q[:, :-1] + LD(td_lam) * cost_to_go_ld(td, wseq)
    x = (LD(-1) / LD(beta)) * out
    keep = np.broadcast_to(keep_p[:, None], (P, H))
    if not tbw:
        x, keep = x[:, :1], keep[:, :1]
    w = np.broadcast_to(_weights_ld(x, keep)[0], (P, H))
    return (LD(1) - LD(step)) * np.asarray(mean, LD) + LD(step) * np.einsum("pt,pta->ta", w, np.asarray(actions, LD))


def elite_ids(q0, k):
    """The k smallest returns in (q0, index) order, a non-finite q0 ranking as +inf."""
    q = np.asarray(q0, np.float64).copy()
    q[~np.isfinite(q)] = np.inf
    return np.argsort(q, kind="stable")[:k]


def ref_cem(q0, actions, mean, cov, k, step, full):
    """CEM._update_distribution from q0: mean of the elite actions, np.var (ddof 0, diagonal) / np.cov (ddof 1) of their
    deltas over the H k rows."""
    ids = elite_ids(q0, k)
    a = np.asarray(actions, LD)[ids]
    H, A = a.shape[1], a.shape[2]
    d = (a - np.asarray(mean, LD)[None]).reshape(H * k, A)
    dc = d - d.mean(axis=0, keepdims=True)
    if full:
        upd = dc.T @ dc / LD(H * k - 1)
    else:
        upd = np.diag((dc ** 2).sum(axis=0) / LD(H * k))
    new_mean = (LD(1) - LD(step)) * np.asarray(mean, LD) + LD(step) * a.mean(axis=0)
    return ids, new_mean, (LD(1) - LD(step)) * np.asarray(cov, LD) + LD(step) * upd


def rs_best(q0):
    """First index of the minimum, a non-finite q0 as +inf; 0 for a row without a finite entry."""
    q = np.asarray(q0, np.float64).copy()
    q[~np.isfinite(q)] = np.inf
    return int(np.argmin(q))


def ref_rs(q0, actions, mean, step):
    return (LD(1) - LD(step)) * np.asarray(mean, LD) + LD(step) * np.asarray(actions, LD)[rs_best(q0)]


def problem(P, H, A, seed):
    """One seeded population: costs [P][H] > 0, actions about a mean, a full covariance, the discount sequence."""
    rs = np.random.RandomState(seed)
    mean = 0.3 * rs.randn(H, A)
    B = rs.randn(A, A)
    cov = B @ B.T / A + 0.5 * np.eye(A)
    actions = mean[None] + rs.randn(P, H, A)
    costs = rs.rand(P, H) * 2 + 0.1 * np.abs(actions).sum(-1)
    gseq = np.cumprod([1.0] + [0.97] * (H - 1))
    return dict(P=P, H=H, A=A, mean=mean, cov=cov, actions=actions, costs=costs, gseq=gseq)
