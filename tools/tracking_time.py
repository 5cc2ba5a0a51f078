#!/usr/bin/env python
"""What tracked cost terms cost on the device, f64, device events, the variants alternating in one process.

    python tools/tracking_time.py [--windows 7] [--launches 200] [--steps 100]

1. ``mjmpc_cost_terms_track`` alone against ``mjmpc_cost_terms`` alone on the same table and buffers (the untracked entry reads
   a tracked table as "hold the first goal") at the reacher's shape, 4096 x 32 with d_obs 20 and A 7: the six rows of
   ``builtin_reach()`` with the three ABS rows tracked, and a 32-row table with 15 rows tracked.  The reference has 200 rows.
2. ``mjmpc_cost_terms_track_batch`` against ``mjmpc_cost_terms_batch`` at 16 x 256 x 32, both with the cost-to-go, with one
   reference for the batch and with one per episode.
3. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on the reacher (arm engine, 4096 x 32) and
   the cart-pole (tree engine, 1024 x 48) with tracked terms against the same terms with constant targets, ms per step.

Every line gives the median, minimum and maximum over the windows."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_REF = 200


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _show(label, res):
    for v, xs in res.items():
        print("%-34s %-58s median %9.3f  (min %9.3f, max %9.3f)" % (label, v, _median(xs), min(xs), max(xs)), flush=True)


def _alternate(variants, windows, launches, scale):
    import torch
    for fn in variants.values():
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    res = {v: [] for v in variants}
    for _ in range(windows):
        for v, fn in variants.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(launches):
                fn()
            e.record()
            torch.cuda.synchronize()
            res[v].append(scale * s.elapsed_time(e) / launches)
    return res


def reach_terms(engine, tracked):
    """``builtin_reach()`` with its three ABS rows following a reference (or holding its first row)."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    n = np.arange(N_REF, dtype=np.float64)
    ref = 0.05 * np.stack([np.cos(0.1 * n), np.sin(0.1 * n), 0.5 * np.cos(0.2 * n)], axis=1)
    t = CostTerms(engine)
    t.abs(obs="site_minus_target", **(dict(reference=ref) if tracked else dict(target=ref[0])))
    t.norm(obs="site_minus_target", weight=5.0)
    return t


def mixed_terms(engine, tracked):
    """32 rows over the reacher's observation and action, 15 of them tracked."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    n = np.arange(N_REF, dtype=np.float64)
    wave = 0.2 * np.sin(0.05 * n)
    goal = (lambda k: dict(reference=np.repeat(wave[:, None], k, axis=1))) if tracked else (lambda k: dict(target=wave[0]))
    t = CostTerms(engine).square(obs="qvel", weight=0.01).square(action=True, weight=0.001, **goal(7))
    t.cos(obs="qpos", weight=0.1).abs(obs="site_minus_target", **goal(3)).norm(obs="site_minus_target", weight=5.0)
    t.square(obs="qvel", index=[0, 1, 2, 3, 4], weight=1.0, terminal=True, **goal(5))
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
    step = torch.full((1,), 17, dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for label, terms in (("builtin_reach, 3 of 6 rows tracked", reach_terms(host, True)), ("mixed, 15 of 32 rows tracked", mixed_terms(host, True))):
        table, ref = terms.table(), terms.reference_table()
        tab, K, R = dev(table), len(table), ref.shape[1]
        d_ref, refs = dev(ref), dev(np.stack([ref] * E))
        a = act if np.any(table[:, 1] != 0) else None
        chk = _lib.check
        single = {
            "mjmpc_cost_terms": lambda: chk(lib.mjmpc_cost_terms(_lib.F64, N, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 1, vp(costs), stream)),
            "mjmpc_cost_terms_track": lambda: chk(lib.mjmpc_cost_terms_track(
                _lib.F64, N, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 1, vp(d_ref), N_REF, R, 0, vp(step), 0, 0, vp(costs), stream)),
            "mjmpc_cost_terms_track, periodic": lambda: chk(lib.mjmpc_cost_terms_track(
                _lib.F64, N, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 1, vp(d_ref), N_REF, R, 1, vp(step), 0, 0, vp(costs), stream)),
        }
        _show("%d x %d  %s [us]" % (N, H, label), _alternate(single, windows, launches, 1e3))
        batch = {
            "mjmpc_cost_terms_batch + q0": lambda: chk(lib.mjmpc_cost_terms_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 0, 1, vp(costs), vp(gseq), vp(q0), stream)),
            "mjmpc_cost_terms_track_batch + q0": lambda: chk(lib.mjmpc_cost_terms_track_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 0, 1, vp(d_ref), N_REF, R, 0, 0, vp(step), 0, vp(costs),
                vp(gseq), vp(q0), stream)),
            "mjmpc_cost_terms_track_batch + q0, a reference per episode": lambda: chk(lib.mjmpc_cost_terms_track_batch(
                _lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 0, 1, vp(refs), N_REF, R, 1, 1, vp(step), 0, vp(costs),
                vp(gseq), vp(q0), stream)),
        }
        _show("%d x %d x %d  %s [us]" % (E, P, H, label), _alternate(batch, windows, launches, 1e3))


def time_control_steps(windows, steps):
    import torch
    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    def cartpole_terms(engine, tracked):
        sched = np.repeat([0.0, 0.4, 0.0, -0.4], 50)
        t = CostTerms(engine).cos(obs="qpos", index=1, weight=4.0)
        t.square(obs="qpos", index=0, weight=0.5, **(dict(reference=sched, periodic=True) if tracked else dict(target=sched[0])))
        return t.square(obs="qvel", weight=0.01).square(obs="qvel", weight=0.5, terminal=True)

    for label, make_engine, make_terms, P, H in (
            ("reacher, arm engine, MPPI 4096 x 32", lambda: ArmRolloutEngine(reacher7dof_raw()), reach_terms, 4096, 32),
            ("cart-pole, tree engine, MPPI 1024 x 48", lambda: TreeRolloutEngine(synthetic_raw("cartpole")), cartpole_terms, 1024, 48)):
        loops = {}
        for variant, tracked in (("constant targets", False), ("tracked", True)):
            eng = make_engine()
            if "cart" in label:
                st = start_state("cartpole", eng.raw)
                eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
            eng.on_env_reset = "ignore"
            eng.set_cost_terms(make_terms(eng, tracked))
            c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                             gamma=0.98, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                             seed=11, base_action="null", noise_mode="device", init_cov=0.1, lam=0.05, step_size=0.8, alpha=1)
            c.rollout_fn = make_device_rollout_fn(eng)
            c.set_sim_state_fn = lambda s: None
            c.enable_graph(post_step=eng.step_state)
            loops[variant] = (lambda c=c: c.optimize({}))
            loops[variant]()
            print("%-34s %-58s %s" % (label, variant, c.launch_mode), flush=True)
        _show(label + " [ms per step]", _alternate(loops, windows, steps, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    time_launches(args.windows, args.launches)
    time_control_steps(args.windows, args.steps)


if __name__ == "__main__":
    main()
