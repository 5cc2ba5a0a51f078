#!/usr/bin/env python
"""What action-rate rows and one-sided kinds cost on the device, f64, device events, the variants alternating in
one process.

    python tools/rate_time.py [--windows 7] [--launches 200] [--steps 100] [--part all|launches|reacher|cartpole]

1. ``mjmpc_cost_terms_rate`` alone at the reacher's shape, 4096 x 32 with d_obs 20 and A 7, against ``mjmpc_cost_terms`` on
   the same table with the rate rows rewritten as plain action rows (and, in the second table, the bound rows as SQUARE
   rows): ``builtin_reach()``'s six rows plus 7 rate rows, and a 32-row table with 7 rate rows and 4 bound rows.  Beside them
   the same entry with a one-row reference that no row reads - the tracked instantiation on an untracked table, which is
   what a run-time test for a reference in place of the template flag would run.
2. ``mjmpc_cost_terms_rate_batch`` against ``mjmpc_cost_terms_batch`` at 16 x 256 x 32, both with the cost-to-go, likewise.
3. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on the reacher (arm engine, 4096 x 32) and
   the cart-pole (tree engine, 1024 x 48) with the smooth config's terms against the same step with those rows as plain
   action rows and two-sided squares, ms per step.

Every line gives the median, minimum and maximum over the windows."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tracking_time import _alternate, _show        # noqa: E402


def as_plain(table):
    """The table with its rate rows as action rows and its one-sided rows as SQUARE rows: what the old entries can run."""
    out = np.array(table, np.float64)
    out[out[:, 1] == 2, 1] = 1.0
    out[out[:, 0] >= 4, 0] = 1.0
    return out


def reach_rate_terms(engine):
    """``builtin_reach()``'s six rows and a squared rate on every action."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    return CostTerms.builtin_reach(engine).square(action_rate="all", weight=0.1)


def mixed_rate_terms(engine):
    """32 rows over the reacher's observation and action: 7 rate rows (a norm group) and 4 bound rows among them."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = CostTerms(engine).square(obs="qvel", weight=0.01).square(action=True, weight=0.001)
    t.norm(action_rate="all", weight=0.2)
    t.outside(obs="qpos", index=[1, 3], low=-1.0, high=1.0, weight=10.0)
    t.abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0)
    t.square(obs="qvel", index=0, weight=1.0, terminal=True)
    assert len(t) == 32
    return t


def time_launches(windows, launches):
    import torch
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    lib = _lib.require_gpu()
    host = ArmRolloutEngine.host_only(reacher7dof_raw())
    E, P, H, D, A = 16, 256, 32, 20, 7
    N = E * P
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
    nobs, act, costs = dev(rng.uniform(-1, 1, (N, H, D))), dev(rng.uniform(-1, 1, (N, H, A))), dev(rng.uniform(0, 1, (N, H)))
    gseq, q0 = dev(np.cumprod([1.0] + [0.99] * (H - 1))), torch.empty(N, dtype=torch.float64, device="cuda")
    prev, prevs = dev(rng.uniform(-1, 1, A)), dev(rng.uniform(-1, 1, (E, A)))
    ref, step = dev(np.zeros((1, 1))), torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    chk = _lib.check
    for label, terms in (("builtin_reach + 7 rate rows", reach_rate_terms(host)), ("mixed, 7 rate and 4 bound rows of 32", mixed_rate_terms(host))):
        table = terms.table()
        tab, plain, K = dev(table), dev(as_plain(table)), len(table)
        single = {
            "mjmpc_cost_terms, rate rows as action rows": lambda: chk(lib.mjmpc_cost_terms(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(plain), K, 0, 1, vp(costs), stream)),
            "mjmpc_cost_terms_rate": lambda: chk(lib.mjmpc_cost_terms_rate(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 1, None, 0, 0, 0, None, 0, 0, vp(prev), vp(costs), stream)),
            "mjmpc_cost_terms_rate, no prev": lambda: chk(lib.mjmpc_cost_terms_rate(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 1, None, 0, 0, 0, None, 0, 0, None, vp(costs), stream)),
            "mjmpc_cost_terms_rate, tracked instantiation (unread reference)": lambda: chk(lib.mjmpc_cost_terms_rate(
                _lib.F64, N, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 1, vp(ref), 1, 1, 0, vp(step), 0, 0, vp(prev), vp(costs),
                stream)),
        }
        _show("%d x %d  %s [us]" % (N, H, label), _alternate(single, windows, launches, 1e3))
        batch = {
            "mjmpc_cost_terms_batch + q0, rate rows as action rows": lambda: chk(lib.mjmpc_cost_terms_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(act), vp(plain), K, 0, 0, 1, vp(costs), vp(gseq), vp(q0), stream)),
            "mjmpc_cost_terms_rate_batch + q0": lambda: chk(lib.mjmpc_cost_terms_rate_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 0, 1, None, 0, 0, 0, 0, None, 0, vp(prevs), 0, vp(costs),
                vp(gseq), vp(q0), stream)),
            "mjmpc_cost_terms_rate_batch + q0, tracked instantiation (unread reference)": lambda: chk(lib.mjmpc_cost_terms_rate_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(act), vp(tab), K, 0, 0, 1, vp(ref), 1, 1, 0, 0, vp(step), 0, vp(prevs), 0,
                vp(costs), vp(gseq), vp(q0), stream)),
        }
        _show("%d x %d x %d  %s [us]" % (E, P, H, label), _alternate(batch, windows, launches, 1e3))


def time_control_steps(windows, steps, only=None):
    import gc
    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    def cartpole_terms(engine, smooth):
        """examples/configs/cartpole_smooth_gpu.yml's terms, or the same rows as a plain action row and two-sided squares of
        weight 0 at the band's edges (the same row count; a weighted square there would drive the cart elsewhere, and the
        tree rollout's time depends on the states it visits)."""
        t = CostTerms(engine).cos(obs="qpos", index=1, weight=4.0).square(obs="qpos", index=0, weight=0.5)
        t.square(obs="qvel", weight=0.01).square(action=0, weight=0.001)
        if smooth:
            t.square(action_rate=0, weight=0.05).outside(obs="qpos", index=0, low=-1.5, high=1.5, weight=20.0)
        else:
            t.square(action=0, weight=0.05).square(obs="qpos", index=0, weight=0.0, target=-1.5)
            t.square(obs="qpos", index=0, weight=0.0, target=1.5)
        return t.square(obs="qvel", weight=0.5, terminal=True)

    def reacher_terms(engine, smooth):
        t = CostTerms.builtin_reach(engine)
        return t.square(action_rate="all", weight=0.1) if smooth else t.square(action="all", weight=0.1)

    for label, make_engine, make_terms, P, H in (
            ("reacher, arm engine, MPPI 4096 x 32", lambda: ArmRolloutEngine(reacher7dof_raw()), reacher_terms, 4096, 32),
            ("cart-pole, tree engine, MPPI 1024 x 48", lambda: TreeRolloutEngine(synthetic_raw("cartpole")), cartpole_terms, 1024, 48)):
        if only is not None and not label.replace("-", "").startswith(only):
            continue
        loops = {}
        for variant, smooth in (("rate rows as action rows, bounds as squares", False), ("rate rows and bounds", True)):
            eng = make_engine()
            if "cart" in label:
                st = start_state("cartpole", eng.raw)
                eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
            eng.on_env_reset = "ignore"
            eng.set_cost_terms(make_terms(eng, smooth))
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
            print("%-34s %-58s %s" % (label, variant, c.launch_mode), flush=True)
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
