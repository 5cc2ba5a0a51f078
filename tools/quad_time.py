#!/usr/bin/env python
"""What quadratic groups cost on the device, f64, device events, the variants alternating in one process.

    python tools/quad_time.py [--windows 7] [--launches 200] [--steps 100] [--part all|launches|reacher|cartpole]

1. ``mjmpc_cost_terms_quad`` alone at the reacher's shape, 4096 x 32 with d_obs 20 and A 7, against ``mjmpc_cost_terms_rate`` on
   the same table with every group replaced by its diagonal as SQUARE rows: a 14 x 14 group over ``qpos``, ``qvel``, a 7 x 7
   group on the action and ``builtin_reach()``'s six rows; and one 32 x 32 group (the 20 observation entries, the 7 actions
   and 5 action rates) beside those six rows.  Beside them the diagonal table through the quad entry: the QUAD instantiation's
   decode, scratch and tile with no group to evaluate.
2. ``mjmpc_cost_terms_quad_batch`` against ``mjmpc_cost_terms_rate_batch`` at 16 x 256 x 32, both with the cost-to-go, likewise.
3. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on the reacher (arm engine, 4096 x 32) with
   the first table and on the cart-pole (tree engine, 1024 x 48) with examples/configs/cartpole_lqr_gpu.yml's terms, each
   against the same step with the diagonal table, ms per step.

Every line gives the median, minimum and maximum over the windows."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tracking_time import _alternate, _show        # noqa: E402


def _spd(rng, n):
    M = rng.uniform(-1.0, 1.0, (n, n))
    return M @ M.T / n + 0.1 * np.eye(n)


def reach_lqr_terms(engine, full=True):
    """A 14 x 14 group over qpos, qvel, a 7 x 7 group on the action and ``builtin_reach()``'s six rows; ``full=False``: every
    group as its diagonal in SQUARE rows."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    rng = np.random.default_rng(0)
    Q, R = _spd(rng, 14), 0.01 * _spd(rng, 7)
    t = CostTerms(engine)
    if full:
        t.quadratic(parts=[dict(obs="qpos"), dict(obs="qvel")], matrix=Q, weight=0.1)
        t.quadratic(action="all", matrix=R)
    else:
        for i, name in enumerate(("qpos", "qvel")):
            for k in range(7):
                t.square(obs=name, index=k, weight=0.1 * Q[7 * i + k, 7 * i + k])
        for k in range(7):
            t.square(action=k, weight=R[k, k])
    return t.abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0)


def big_group_terms(engine, full=True):
    """One 32 x 32 group over the reacher's 20 observation entries, its 7 actions and 5 action rates, and ``builtin_reach()``'s
    six rows."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    rng = np.random.default_rng(1)
    d, A = int(engine.model.d_obs), int(engine.model.nu)
    n_rates = 32 - d - A
    assert 0 < n_rates <= A
    Q = _spd(rng, 32)
    t = CostTerms(engine)
    if full:
        t.quadratic(parts=[dict(obs=list(range(d))), dict(action="all"), dict(action_rate=list(range(n_rates)))], matrix=Q,
                    weight=0.1)
    else:
        for k in range(d):
            t.square(obs=[k], weight=0.1 * Q[k, k])
        for k in range(A):
            t.square(action=k, weight=0.1 * Q[d + k, d + k])
        for k in range(n_rates):
            t.square(action_rate=k, weight=0.1 * Q[d + A + k, d + A + k])
    return t.abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0)


def time_launches(windows, launches):
    import torch
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    lib = _lib.require_gpu()
    host = ArmRolloutEngine.host_only(reacher7dof_raw())
    E, P, H, D, A = 16, 256, 32, int(host.model.d_obs), 7
    N = E * P
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
    nobs, act, costs = dev(rng.uniform(-1, 1, (N, H, D))), dev(rng.uniform(-1, 1, (N, H, A))), dev(rng.uniform(0, 1, (N, H)))
    gseq, q0 = dev(np.cumprod([1.0] + [0.99] * (H - 1))), torch.empty(N, dtype=torch.float64, device="cuda")
    one = dev(np.zeros(1))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    chk = _lib.check
    for label, make in (("14 x 14 + 7 x 7 + builtin_reach", reach_lqr_terms), ("32 x 32 + builtin_reach", big_group_terms)):
        full, diag = make(host, True), make(host, False)
        tab, pool, K = dev(full.table()), dev(full.quad_table()), len(full)
        dtab, dK = dev(diag.table()), len(diag)
        assert K == dK and not diag.needs_quad_entry
        single = {
            "mjmpc_cost_terms_rate, diagonals as SQUARE rows": lambda: chk(lib.mjmpc_cost_terms_rate(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(dtab), dK, 0, 1, None, 0, 0, 0, None, 0, 0, None, vp(costs), stream)),
            "mjmpc_cost_terms_quad, diagonals as SQUARE rows": lambda: chk(lib.mjmpc_cost_terms_quad(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(dtab), dK, 0, 1, None, 0, 0, 0, None, 0, 0, None, vp(one), 1, vp(costs),
                stream)),
            "mjmpc_cost_terms_quad, full matrices": lambda: chk(lib.mjmpc_cost_terms_quad(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 1, None, 0, 0, 0, None, 0, 0, None, vp(pool), pool.shape[0],
                vp(costs), stream)),
        }
        _show("%d x %d  %s, %d rows [us]" % (N, H, label, K), _alternate(single, windows, launches, 1e3))
        batch = {
            "mjmpc_cost_terms_rate_batch + q0, diagonals as SQUARE rows": lambda: chk(lib.mjmpc_cost_terms_rate_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(act), vp(dtab), dK, 0, 0, 1, None, 0, 0, 0, 0, None, 0, None, 0, vp(costs),
                vp(gseq), vp(q0), stream)),
            "mjmpc_cost_terms_quad_batch + q0, full matrices": lambda: chk(lib.mjmpc_cost_terms_quad_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 0, 1, None, 0, 0, 0, 0, None, 0, None, 0, vp(pool),
                pool.shape[0], vp(costs), vp(gseq), vp(q0), stream)),
        }
        _show("%d x %d x %d  %s, %d rows [us]" % (E, P, H, label, K), _alternate(batch, windows, launches, 1e3))


def time_control_steps(windows, steps, only=None):
    import gc

    import yaml
    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    def cartpole_terms(engine, full):
        """examples/configs/cartpole_lqr_gpu.yml's terms, or the same groups as their diagonals in SQUARE rows."""
        with open(os.path.join(ROOT, "examples", "configs", "cartpole_lqr_gpu.yml")) as f:
            block = yaml.safe_load(f)["cost_terms"]
        if full:
            return cost_terms_from_config(block, engine)
        t = CostTerms(engine)
        for entry in block["terms"]:
            if entry["kind"] != "quadratic":
                t.outside(**{k: v for k, v in entry.items() if k != "kind"})
                continue
            M = np.asarray(entry["matrix"], np.float64)
            d = M if M.ndim == 1 else np.diag(M)
            names = [("obs", "qpos", 0), ("obs", "qpos", 1), ("obs", "qvel", 0), ("obs", "qvel", 1)] if "parts" in entry else \
                [("action", 0, None)]
            for w, (key, what, index) in zip(d, names):
                kw = {key: what, "weight": float(w) * entry.get("weight", 1.0), "terminal": entry.get("terminal", False)}
                if index is not None:
                    kw["index"] = index
                t.square(**kw)
        return t

    for label, make_engine, make_terms, P, H in (
            ("reacher, arm engine, MPPI 4096 x 32", lambda: ArmRolloutEngine(reacher7dof_raw()), reach_lqr_terms, 4096, 32),
            ("cart-pole, tree engine, MPPI 1024 x 48", lambda: TreeRolloutEngine(synthetic_raw("cartpole")), cartpole_terms, 1024, 48)):
        if only is not None and not label.replace("-", "").startswith(only):
            continue
        loops = {}
        for variant, full in (("diagonals as SQUARE rows", False), ("full matrices", True)):
            eng = make_engine()
            if "cart" in label:
                st = start_state("cartpole", eng.raw)
                eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
            eng.on_env_reset = "ignore"
            eng.set_cost_terms(make_terms(eng, full))
            c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                             gamma=0.98, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                             seed=11, base_action="null", noise_mode="device", init_cov=0.1, lam=0.05, step_size=0.8, alpha=1)
            c.rollout_fn = make_device_rollout_fn(eng)
            c.set_sim_state_fn = lambda s: None
            c.enable_graph(post_step=eng.step_state)
            loops[variant] = (lambda c=c: c.optimize({}))
            # (the first call captures the iteration: no collection of an earlier controller's graphs and streams meanwhile)
            gc.collect()
            gc.disable()
            try:
                loops[variant]()
            finally:
                gc.enable()
            print("%-34s %-28s %s" % (label, variant, c.launch_mode), flush=True)
        _show(label + " [ms per step]", _alternate(loops, windows, steps, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--part", choices=["all", "launches", "reacher", "cartpole"], default="all")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    if args.part in ("all", "launches"):
        time_launches(args.windows, args.launches)
    if args.part != "launches":
        time_control_steps(args.windows, args.steps, None if args.part == "all" else args.part)


if __name__ == "__main__":
    main()
