"""Shared by tests/test_cost_terms_cpu.py and the cost-term GPU tests: the numpy restatement of a cost-term table's
row semantics (plain loops in row order, float64 accumulation - written from the row format, not from ``CostTerms`` or the
kernel), the derived error bound, random valid tables, and the engines, noise and MPPI of the GPU tests' closed loops."""
import numpy as np

from batched_cases import FILT

ABS, SQUARE, NORM, COS = 0, 1, 2, 3
REACHER_START = dict(qp=np.array([0.1, 0.2, 0.0, -0.5, 0.0, -0.3, 0.0]), qv=np.zeros(7), target_pos=np.array([0.2, -0.1, 0.2]))
P, H = 64, 8


def restate(table, next_obs, actions, incoming, keep_builtin, terminal):
    """-> (cost [P][H] float64, sum of |row values| [P][H]) of ``table`` ([K][8]: kind, source, index, weight, target,
    group, when, reserved) over ``next_obs`` [P][H][d_obs] and ``actions`` [P][H][A].

    COS rows are ``w (1 - cos r)``, evaluated as ``2 w sin^2(r / 2)`` - the same number, but ``1 - cos r`` computed
    literally loses everything to cancellation near r = 0 and the restatement's own error would then exceed the bound
    below, which is relative to the row's value."""
    next_obs = np.asarray(next_obs, np.float64)
    actions = None if actions is None else np.asarray(actions, np.float64)
    incoming = np.asarray(incoming, np.float64)
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
                else:
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


def bound(table, cost_ref, mag, f32):
    """Every row's value carries a few ulp and the K additions one each: |c - c_ref| <= 4 (K + 4) 2^-52 sum_k |row value|;
    an f32 result adds half an ulp of f32 (at most 2^-24 |c_ref|)."""
    b = 4.0 * (len(table) + 4) * 2.0 ** -52 * mag
    if f32:
        b = b + 2.0 ** -24 * np.abs(np.where(np.isfinite(cost_ref), cost_ref, 0.0))
    return b


def random_table(rng, K, d_obs, A, terminal_rows=True):
    """K valid rows: every kind, both sources, weights of both signs, targets in [-5, 5], norm groups of 1 - 3 rows with
    fresh ids - one of them the table's last rows when K >= 3 -, and a few terminal rows (a group shares one flag)."""
    rows, group = [], 0

    def row(kind, g, when):
        source = int(rng.integers(0, 2)) if A > 0 else 0
        index = int(rng.integers(0, A if source else d_obs))
        return [kind, source, index, float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-5.0, 5.0)), g, when, 0.0]

    tail = min(3, K - 1) if K >= 3 else 0           # the closing norm group
    while len(rows) < K - tail:
        when = float(terminal_rows and rng.random() < 0.25)
        kind = int(rng.integers(0, 4))
        if kind == NORM:
            group += 1
            for _ in range(min(int(rng.integers(1, 4)), K - tail - len(rows))):
                rows.append(row(NORM, group, when))
        else:
            rows.append(row(kind, 0, when))
    if tail:
        group += 1
        rows += [row(NORM, group, 0.0) for _ in range(tail)]
    return np.asarray(rows, np.float64)


def mixed_terms(engine, CostTerms):
    """ABS, SQUARE on an action, NORM, COS and one terminal row, over any reach-task engine."""
    t = CostTerms(engine)
    t.abs(obs="site_minus_target", index=0, weight=0.7)
    t.square(action=0, weight=0.05)
    t.norm(obs="site_minus_target", weight=4.0)
    t.cos(obs="qpos", index=0, weight=0.3, target=0.2)
    t.square(obs="qvel", index=0, weight=0.5, terminal=True)
    return t


def _engine(model, dtype="f64"):
    """The arm engine on the reacher or the tree engine on a synthetic model ('cartpole', 'tray'), at the model's start
    state (inside every model's stable range in the existing tests)."""
    if model == "reacher":
        from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
        from mjmpc_amd.models.reacher7dof import reacher7dof_raw
        eng = ArmRolloutEngine(reacher7dof_raw(), dtype=dtype)
        eng.set_env_state(REACHER_START)
        return eng
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw
    raw = synthetic_raw(model)
    eng = TreeRolloutEngine(raw, dtype=dtype)
    st = start_state(model, raw)
    eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
    return eng


def _noise(eng, seed=3, cov=0.1):
    return np.sqrt(cov) * np.random.default_rng(seed).standard_normal((P, H, eng.d_action))


def _mppi(eng, **over):
    from mjmpc_amd import control
    kw = dict(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1, gamma=0.98,
              action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=11, base_action="null",
              noise_mode="device", init_cov=0.1, lam=0.05, step_size=0.8, alpha=1)
    return control.MPPI(**dict(kw, **over))
