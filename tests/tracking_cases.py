"""Shared by tests/test_tracking_cpu.py and tests/test_tracking_gpu.py: the numpy restatement of cost terms that track a
reference trajectory, written from the contract - reference row n is the goal for env time n; with the base
time b an observation row of step t reads row b + t + 1, an action row reads row b + t; a row outside [0, N - 1] is clamped
(the last goal is held) or, periodic, taken mod N - and not from the kernel: for every step the table is copied, the goals
of that step are written into the target column and ``cost_terms_cases.restate`` costs the step.  Tracking adds no rounding
step (r = v - goal stays one subtraction), so the bound is ``cost_terms_cases.bound``."""
import numpy as np

from cost_terms_cases import restate as restate_constant


def ref_row(n, N, periodic):
    """The reference row for env time ``n`` (any integer)."""
    n, N = int(n), int(N)
    if periodic:
        return n - N * (n // N)             # (floor division: non-negative for negative n too)
    return 0 if n < 0 else N - 1 if n > N - 1 else n


def table_at(table, ref, periodic, base, t):
    """``table`` with the goals of plan step ``t`` of a launch with base time ``base`` in the target column of its tracked rows
    (reserved = 1 + the row's column of ``ref``)."""
    out = np.array(table, np.float64)
    for k in range(len(out)):
        c = int(out[k, 7]) - 1
        if c >= 0:
            n = base + t if out[k, 1] == 1 else base + t + 1
            out[k, 4] = ref[ref_row(n, len(ref), periodic), c]
    return out


def restate(table, ref, periodic, base, next_obs, actions, incoming, keep_builtin, terminal):
    """-> (cost [P][H] float64, sum of |row values| [P][H]): ``cost_terms_cases.restate`` step by step on the H = 1 slices,
    `terminal` only at t = H - 1."""
    next_obs, incoming = np.asarray(next_obs, np.float64), np.asarray(incoming, np.float64)
    P, H = incoming.shape
    cost, mag = np.zeros((P, H)), np.zeros((P, H))
    for t in range(H):
        c, m = restate_constant(table_at(table, ref, periodic, base, t), next_obs[:, t:t + 1],
                                None if actions is None else np.asarray(actions, np.float64)[:, t:t + 1], incoming[:, t:t + 1],
                                keep_builtin, bool(terminal) and t == H - 1)
        cost[:, t], mag[:, t] = c[:, 0], m[:, 0]
    return cost, mag


def track_rows(rng, table, N, fraction=0.5):
    """A random subset of ``table``'s rows (at least one) becomes tracked -> (table with `reserved` = 1 + column and `target` =
    the first goal, reference float64 [N][R] with goals in [-5, 5])."""
    table = np.array(table, np.float64)
    pick = rng.random(len(table)) < fraction
    pick[int(rng.integers(0, len(table)))] = True
    rows = np.flatnonzero(pick)
    ref = rng.uniform(-5.0, 5.0, (N, len(rows)))
    for c, k in enumerate(rows):
        table[k, 7] = 1.0 + c
        table[k, 4] = ref[0, c]
    return table, ref


def cartpole_schedule(N=8, scale=0.4):
    """A cart-position schedule of N rows: a square wave through [0, scale, 0, -scale]."""
    return np.array([[0.0, scale, 0.0, -scale][(n * 4) // N % 4] for n in range(N)])


def tracked_reach_terms(eng, ref_scale=1.0, periodic=False, N=5, actions=True):
    """Mixed terms over a reach-task engine, three of them tracked: a scalar reference for one observation entry, a
    [N][3] reference for a NORM group, and (``actions``) a reference for an action row; one constant row; one terminal row."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    n = np.arange(N, dtype=np.float64)
    t = CostTerms(eng)
    t.square(obs="qpos", index=0, weight=2.0, reference=ref_scale * 0.3 * np.sin(0.9 * n), periodic=periodic)
    t.norm(obs="site_minus_target", weight=4.0,
           reference=ref_scale * 0.05 * np.stack([np.cos(n), np.sin(n), 0.5 * np.cos(2.0 * n)], axis=1), periodic=periodic)
    if actions:
        t.square(action=0, weight=0.05, reference=ref_scale * 0.1 * np.cos(0.7 * n), periodic=periodic)
    t.cos(obs="qpos", index=0, weight=0.3, target=0.2)
    t.square(obs="qvel", index=0, weight=0.5, terminal=True)
    return t
