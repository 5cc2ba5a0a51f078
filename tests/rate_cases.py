"""Shared by tests/test_rate_terms_cpu.py and tests/test_rate_terms_gpu.py: the numpy restatement of a cost-term table with
action-rate rows and one-sided kinds, written from the contract and not from the kernel, in plain loops:

* a row of ``source`` 2 reads ``u[p][t][i] - u[p][t-1][i]`` for ``t >= 1`` and ``u[p][0][i] - prev[i]`` for ``t = 0``, 0 where
  ``prev[i]`` is NaN or there is no ``prev``;  ``r = v - goal`` as for every row, a tracked rate row with the ACTION-time
  reference row;
* kinds 4 .. 7: ``w max(0, r)``, ``w max(0, -r)``, ``w max(0, r)^2``, ``w max(0, -r)^2``; kinds 0 .. 3 as ever.

The rates are formed first and appended to the actions, a rate row becomes a ``source`` 1 row of index ``index + A``, so that
``tracking_cases.table_at`` picks the action-time row, and the rows are then evaluated in row order.  The difference of two
stored actions is one correctly rounded float64 operation on exactly converted values, and ``max`` rounds nothing: the
bound is ``cost_terms_cases.bound``, unchanged."""
import numpy as np

import tracking_cases as tc
from cost_terms_cases import ABS, COS, NORM, SQUARE, random_table

ABOVE, BELOW, ABOVE_SQUARE, BELOW_SQUARE = 4, 5, 6, 7
RATE = 2


def rates(actions, prev):
    """``[P][H][A]`` float64: the change of the action from the step before; ``prev``: ``[A]``, ``[P][A]`` (a row per
    particle: its episode's) or ``None``."""
    actions = np.asarray(actions, np.float64)
    P, H, A = actions.shape
    out = np.zeros((P, H, A))
    for p in range(P):
        for t in range(H):
            for i in range(A):
                if t >= 1:
                    out[p, t, i] = actions[p, t, i] - actions[p, t - 1, i]
                elif prev is not None:
                    before = float(np.asarray(prev, np.float64).reshape(-1, A)[p if np.ndim(prev) == 2 else 0, i])
                    out[p, t, i] = 0.0 if np.isnan(before) else actions[p, t, i] - before
    return out


def _row_values(table, next_obs, actions, incoming, keep_builtin, terminal):
    """``cost_terms_cases.restate`` with the kinds 4 .. 7 (sources 0 and 1 only: the rates were appended to the actions)."""
    P, H = incoming.shape
    K = len(table)
    cost, mag = np.zeros((P, H)), np.zeros((P, H))
    for p in range(P):
        for t in range(H):
            acc = float(incoming[p, t]) if keep_builtin else 0.0
            m = abs(acc) if np.isfinite(acc) else 0.0
            sq, w_first = 0.0, 0.0
            for k in range(K):
                kind, source, index, w, target, group, when = table[k, :7]
                if when == 1 and not (terminal and t == H - 1):
                    continue
                v = float(actions[p, t, int(index)]) if source == 1 else float(next_obs[p, t, int(index)])
                r = v - target
                if kind == ABS:
                    val = w * abs(r)
                elif kind == SQUARE:
                    val = w * (r * r)
                elif kind == COS:
                    val = w * (2.0 * np.sin(0.5 * r) ** 2)
                elif kind == ABOVE:
                    val = w * max(0.0, r)
                elif kind == BELOW:
                    val = w * max(0.0, -r)
                elif kind == ABOVE_SQUARE:
                    val = w * (max(0.0, r) * max(0.0, r))
                elif kind == BELOW_SQUARE:
                    val = w * (max(0.0, -r) * max(0.0, -r))
                else:
                    assert kind == NORM
                    first = k == 0 or table[k - 1, 0] != NORM or table[k - 1, 5] != group
                    last = k == K - 1 or table[k + 1, 0] != NORM or table[k + 1, 5] != group
                    if first:
                        sq, w_first = 0.0, w
                    sq += r * r
                    if not last:
                        continue
                    val = w_first * np.sqrt(sq)
                acc += val
                m += abs(val)
            cost[p, t] = acc if np.isfinite(incoming[p, t]) else np.inf
            mag[p, t] = m
    return cost, mag


def restate(table, next_obs, actions, prev, incoming, keep_builtin, terminal, ref=None, periodic=False, base=0):
    """-> (cost [P][H] float64, sum of |row values| [P][H]) of an extended ``table`` over ``next_obs`` [P][H][d_obs] and
    ``actions`` [P][H][A] with the previous action ``prev``; ``ref`` ([N][R]) / ``periodic`` / ``base``: the tracked rows'
    reference at base time ``base`` (tests/tracking_cases.py)."""
    next_obs, actions = np.asarray(next_obs, np.float64), np.asarray(actions, np.float64)
    incoming = np.asarray(incoming, np.float64)
    P, H = incoming.shape
    A = actions.shape[2]
    both = np.concatenate([actions, rates(actions, prev)], axis=2)
    plain = np.array(table, np.float64)
    for k in range(len(plain)):
        if plain[k, 1] == RATE:
            plain[k, 1], plain[k, 2] = 1.0, plain[k, 2] + A
    cost, mag = np.zeros((P, H)), np.zeros((P, H))
    for t in range(H):
        at = plain if ref is None else tc.table_at(plain, ref, periodic, base, t)
        c, m = _row_values(at, next_obs[:, t:t + 1], both[:, t:t + 1], incoming[:, t:t + 1], keep_builtin,
                           bool(terminal) and t == H - 1)
        cost[:, t], mag[:, t] = c[:, 0], m[:, 0]
    return cost, mag


def random_extended_table(rng, K, d_obs, A, terminal_rows=True):
    """``cost_terms_cases.random_table`` (every kind 0 .. 3, norm groups, terminal rows) with about a third of the rows that
    read an action turned into rate rows - rows inside norm groups too, so that groups mix rates, actions and observations -
    and about a third of the rows outside norm groups given a one-sided kind.  At least one rate row and one row of each new
    kind where K allows."""
    table = random_table(rng, K, d_obs, A, terminal_rows)
    acts = np.flatnonzero(table[:, 1] == 1)
    for k in acts:
        if rng.random() < 0.35:
            table[k, 1] = RATE
    free = np.flatnonzero(table[:, 0] != NORM)
    for k in free:
        if rng.random() < 0.35:
            table[k, 0] = float(rng.integers(ABOVE, BELOW_SQUARE + 1))
    # the guarantees: a rate row (on an action index), and each new kind once
    if not np.any(table[:, 1] == RATE):
        k = int(acts[0]) if len(acts) else int(rng.integers(0, K))
        table[k, 1], table[k, 2] = RATE, min(int(table[k, 2]), A - 1)
    for kind, k in zip((ABOVE, BELOW, ABOVE_SQUARE, BELOW_SQUARE), free):
        table[k, 0] = kind
    return table


def smooth_terms(eng, rate_weight=0.5, CostTerms=None):
    """Terms over any reach-task engine with a squared action rate, a rate norm, a soft band on qpos[0] and a one-sided
    limit on qvel[0], beside ordinary rows and a terminal one."""
    if CostTerms is None:
        from mjmpc_amd.envs.cost_terms import CostTerms
    t = CostTerms(eng)
    t.norm(obs="site_minus_target", weight=4.0)
    t.square(action_rate=0, weight=rate_weight)
    t.norm(action_rate="all", weight=0.2)
    t.outside(obs="qpos", index=0, low=-0.05, high=0.05, weight=3.0)
    t.above(obs="qvel", index=0, target=0.1, weight=0.7)
    t.square(action=0, weight=0.01)
    t.below_square(obs="qvel", index=0, target=0.0, weight=0.5, terminal=True)
    return t
