"""Shared by tests/test_quad_terms_cpu.py and tests/test_quad_terms_gpu.py: the numpy restatement of a cost-term table with
quadratic groups and signed linear rows, written from the contract and not from the kernel:

* kind 8 QUAD: consecutive rows of kind 8 with one group id form ``r_i = v_i - goal_i``; the group is worth
  ``w_first sum_i sum_j r_i Q_ij r_j`` - the full double sum over the stored matrix, no use of its symmetry -, ``Q`` being the
  group's ``n x n`` block of the pool, found at the sum of ``n^2`` over the groups before it;
* kind 9 LINEAR: ``w r``.

Everything old is ``rate_cases.restate`` on the table without the new rows (the groups' ids are fresh, so taking rows out
merges no NORM groups); the values and goals of the new rows come the same way as there - the rates appended to the actions,
``tracking_cases.table_at`` for the goals of step t.  ``mag`` counts a group as ``|w| sum_ij |r_i Q_ij r_j|`` and a linear row
as ``|w r|``.

The bound is ``cost_terms_cases.bound`` with the additions counted: a group of n rows is n^2 products of three factors (two
roundings each, the factor 2 of the kernel's symmetric form is exact) and n^2 additions, its weight one more - every one at most
an ulp of a partial sum no larger than ``mag`` - so ``|c - c_ref| <= 4 (K + n_max^2 + 4) 2^-52 mag`` with n_max the table's
largest group, plus half an ulp of f32 for f32 storage."""
import ctypes

import numpy as np

import rate_cases as rc
import tracking_cases as tc
from cost_terms_cases import NORM

QUAD, LINEAR = 8, 9
MAX_QUAD = 32


def groups(table):
    """[(first row, rows, pool offset)] of the QUAD groups of ``table`` in order."""
    out, k, off, K = [], 0, 0, len(table)
    while k < K:
        if table[k, 0] != QUAD:
            k += 1
            continue
        n = 1
        while k + n < K and table[k + n, 0] == QUAD and table[k + n, 5] == table[k, 5]:
            n += 1
        out.append((k, n, off))
        off += n * n
        k += n
    return out


def n_max(table):
    return max([n for _, n, _ in groups(table)] or [0])


def restate(table, quad, next_obs, actions, prev, incoming, keep_builtin, terminal, ref=None, periodic=False, base=0):
    """-> (cost [P][H] float64, sum of |values| [P][H]) of ``table`` with the pool ``quad``; the other arguments are
    ``rate_cases.restate``'s."""
    table = np.array(table, np.float64)
    next_obs, actions = np.asarray(next_obs, np.float64), np.asarray(actions, np.float64)
    incoming = np.asarray(incoming, np.float64)
    P, H = incoming.shape
    A = actions.shape[2]
    new = (table[:, 0] == QUAD) | (table[:, 0] == LINEAR)
    old = table[~new]
    if len(old):
        cost, mag = rc.restate(old, next_obs, actions, prev, incoming, keep_builtin, terminal, ref, periodic, base)
    else:
        first = incoming if keep_builtin else np.zeros((P, H))
        cost = np.where(np.isfinite(incoming), first, np.inf)
        mag = np.where(np.isfinite(first), np.abs(first), 0.0)
    if not np.any(new):
        return cost, mag
    both = np.concatenate([actions, rc.rates(actions, prev)], axis=2)
    plain = table.copy()
    for k in range(len(plain)):
        if plain[k, 1] == rc.RATE:
            plain[k, 1], plain[k, 2] = 1.0, plain[k, 2] + A
    add, add_mag = np.zeros((P, H)), np.zeros((P, H))
    for t in range(H):
        at = plain if ref is None else tc.table_at(plain, ref, periodic, base, t)
        last = bool(terminal) and t == H - 1

        def residual(k):
            v = both[:, t, int(at[k, 2])] if at[k, 1] == 1 else next_obs[:, t, int(at[k, 2])]
            return v - at[k, 4]

        for k in np.flatnonzero(at[:, 0] == LINEAR):
            if at[k, 6] == 1 and not last:
                continue
            val = at[k, 3] * residual(k)
            add[:, t] += val
            add_mag[:, t] += np.abs(val)
        for k0, n, off in groups(at):
            if at[k0, 6] == 1 and not last:
                continue
            Q = np.asarray(quad, np.float64)[off:off + n * n].reshape(n, n)
            R = np.stack([residual(k0 + i) for i in range(n)], axis=1)              # [P][n]
            terms = R[:, :, None] * Q[None, :, :] * R[:, None, :]                   # r_i Q_ij r_j
            add[:, t] += at[k0, 3] * terms.sum(axis=(1, 2))
            add_mag[:, t] += abs(at[k0, 3]) * np.abs(terms).sum(axis=(1, 2))
    return np.where(np.isfinite(incoming), cost + add, np.inf), mag + add_mag


def bound(table, cost_ref, mag, f32):
    """``|c - c_ref| <= 4 (K + n_max^2 + 4) 2^-52 mag``, plus ``2^-24 |c_ref|`` for f32 storage (the module docstring)."""
    b = 4.0 * (len(table) + n_max(table) ** 2 + 4) * 2.0 ** -52 * mag
    if f32:
        b = b + 2.0 ** -24 * np.abs(np.where(np.isfinite(cost_ref), cost_ref, 0.0))
    return b


def random_pool(rng, table):
    """A symmetric matrix with entries in [-1, 1] for every group of ``table`` (indefinite as a rule), back to back."""
    out = []
    for _, n, _ in groups(table):
        M = rng.uniform(-1.0, 1.0, (n, n))
        out.append((0.5 * (M + M.T)).reshape(-1))
    return np.concatenate(out) if out else np.zeros(1)


def _quad_rows(rng, n, d_obs, A, group, when):
    rows = []
    for _ in range(n):
        source = int(rng.integers(0, 3))
        index = int(rng.integers(0, A if source else d_obs))
        rows.append([QUAD, source, index, float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-5.0, 5.0)), group, when, 0.0])
    return rows


def random_quad_table(rng, K, d_obs, A, sizes=None):
    """K rows: ``rate_cases.random_extended_table`` (all of 0 .. 7, rate rows, NORM groups, terminal rows) with QUAD groups of
    ``sizes`` rows (default: 1 - 7 rows each, about a third of the table) put between its rows - never inside a NORM group -,
    the last of them the table's last rows, rows of all three sources, a later row's weight unlike the first's (it must not
    count), a few groups terminal; and about a fifth of the other rows outside NORM groups made LINEAR (one at least where
    there is one).  ``sizes`` that fill K: nothing but QUAD groups."""
    if sizes is None:
        sizes, left = [], max(1, K // 3)
        while left > 0:
            sizes.append(min(int(rng.integers(1, 8)), left))
            left -= sizes[-1]
    n_old = K - sum(sizes)
    assert n_old >= 0 and max(sizes) <= MAX_QUAD
    old = rc.random_extended_table(rng, n_old, d_obs, A) if n_old else np.zeros((0, 8))
    free = np.flatnonzero(old[:, 0] != NORM) if n_old else []
    free = free[4:] if len(free) > 4 else free[-1:]         # (the first four hold the one-sided kinds, once each)
    for i, k in enumerate(free):
        if i == 0 or rng.random() < 0.2:
            old[k, 0] = LINEAR
    group = int(old[:, 5].max()) if n_old else 0
    # where a group may stand: in front of row k of the old rows (k = n_old: behind them) unless k - 1 and k share a NORM group
    open_at = [k for k in range(n_old + 1)
               if not (0 < k < n_old and old[k, 0] == NORM and old[k - 1, 0] == NORM and old[k, 5] == old[k - 1, 5])]
    places = sorted(int(open_at[int(rng.integers(0, len(open_at)))]) for _ in sizes[:-1]) + [n_old]
    rows, at = [], 0
    for n, place in zip(sizes, places):
        rows += old[at:place].tolist()
        at = place
        group += 1
        rows += _quad_rows(rng, n, d_obs, A, group, float(place < n_old and rng.random() < 0.25))
    assert at == n_old and len(rows) == K
    return np.asarray(rows, np.float64)


def lqr_terms(eng, weight=1.0, terminal_weight=2.0, seed=5, CostTerms=None):
    """Terms over any reach-task engine: a full matrix over (qpos, qvel) with a target, a full ``R`` on the actions, a form
    over mixed sources - a tracked qpos entry, a qvel entry, an action and an action rate -, a signed linear reward, a terminal
    form, beside a NORM group and a one-sided row."""
    if CostTerms is None:
        from mjmpc_amd.envs.cost_terms import CostTerms
    rng = np.random.default_rng(seed)
    lay = eng.obs_layout()
    n = lay["qvel"].stop - lay["qpos"].start
    A = eng.d_action

    def spd(m):
        M = rng.uniform(-1.0, 1.0, (m, m))
        return M @ M.T / m + 0.1 * np.eye(m)
    t = CostTerms(eng)
    t.quadratic(parts=[dict(obs="qpos", target=0.05), dict(obs="qvel")], matrix=spd(n), weight=weight)
    t.norm(obs="site_minus_target", weight=4.0)
    t.quadratic(action="all", matrix=spd(A), weight=0.05)
    N = 6
    t.quadratic(parts=[dict(obs="qpos", index=0, reference=0.1 * np.sin(0.8 * np.arange(N))), dict(obs="qvel", index=0),
                       dict(action=0), dict(action_rate=0)], matrix=rng.uniform(-1.0, 1.0, (4, 4)), weight=0.3)
    t.linear(obs="qvel", index=0, weight=-0.2)
    t.above(obs="qvel", index=0, target=0.1, weight=0.7)
    t.quadratic(obs="qvel", matrix=spd(lay["qvel"].stop - lay["qvel"].start), weight=terminal_weight, terminal=True)
    return t


# ---------------------------------------------------------------------------------------------------------- the entry points
def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cost_terms_quad(d_tab, d_quad, d_ref, periodic, counter, bias, advance, prev, nobs, act, costs, keep, terminal, f32):
    """``mjmpc_cost_terms_quad`` on device tensors ([P][H][..]), in place in ``costs``; ``d_ref`` / ``counter`` / ``prev`` may be
    ``None``."""
    from batched_terms_cases import stream
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    Pn, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_quad(
        _lib.F32 if f32 else _lib.F64, Pn, Hn, d_obs, act.shape[2], _vp(nobs), _vp(act), _vp(d_tab), d_tab.shape[0], int(keep),
        int(terminal), _vp(d_ref), 0 if d_ref is None else d_ref.shape[0], 0 if d_ref is None else d_ref.shape[1], int(periodic),
        _vp(counter), int(bias), int(advance), _vp(prev), _vp(d_quad), d_quad.shape[0], _vp(costs), stream()))


def cost_terms_quad_batch(d_tabs, d_quad, d_refs, periodic, counter, bias, E, prevs, advance_prev, nobs, act, costs, keep,
                          terminal, f32, gseq=None, q0=None):
    """``mjmpc_cost_terms_quad_batch`` on device tensors ([E P][H][..]); ``d_tabs``: [1 or E][K][8], ``d_refs``: [1 or E][N][R] or
    ``None``, ``prevs``: [E][A] or ``None``, ``d_quad``: the one pool."""
    from batched_terms_cases import stream
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    N, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_quad_batch(
        _lib.F32 if f32 else _lib.F64, E, N // E, Hn, d_obs, act.shape[2], _vp(nobs), _vp(act), _vp(d_tabs), d_tabs.shape[1],
        int(d_tabs.shape[0] > 1), int(keep), int(terminal), _vp(d_refs), 0 if d_refs is None else d_refs.shape[1],
        0 if d_refs is None else d_refs.shape[2], int(d_refs is not None and d_refs.shape[0] > 1), int(periodic), _vp(counter),
        int(bias), _vp(prevs), int(advance_prev), _vp(d_quad), d_quad.shape[0], _vp(costs), _vp(gseq), _vp(q0), stream()))
