#!/usr/bin/env python
"""What the world positions of points cost on the device, f64, device events, the variants alternating in one
process.

    python tools/points_time.py [--windows 7] [--launches 200] [--steps 100] [--part all|launches|reacher|tray|batch]

1. ``mjmpc_points`` alone over 4096 x 32 rows: the reacher with one point on its last link; the tray with two points and a
   difference (examples/configs/tray_points_gpu.yml); a worst case of 16 points on paths of 32 hinges each over a 70-entry
   observation.  Beside each a device ``copy_`` of as many bytes as the launch moves (the rows in, the augmented rows out):
   the yardstick DESIGN 12 uses for the cost launch.
2. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) with terms on points against the same
   number of rows of the same kinds on plain observation entries: the reacher on the arm engine at 4096 x 32, the tray on the
   tree engine at 1024 x 48, and one BatchedMPPI step of 16 x 256 x 32 on the arm engine, ms per step.

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


def reacher_terms(engine, points):
    """Three ABS rows and a NORM group on the last link's origin minus a constant goal (points) or on ``site_minus_target``."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = CostTerms(engine)
    if points:
        t.point("tip", body=engine.raw.bodies[-1].name)
        return t.abs(obs="tip", target=[0.5, 0.1, 0.3]).norm(obs="tip", weight=5.0, target=[0.5, 0.1, 0.3])
    return t.abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0)


def tray_terms(engine, points):
    """examples/configs/tray_points_gpu.yml's terms, or as many rows of the same kinds on plain observation entries."""
    import yaml
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    if points:
        with open(os.path.join(ROOT, "examples", "configs", "tray_points_gpu.yml")) as f:
            return cost_terms_from_config(yaml.safe_load(f)["cost_terms"], engine)
    t = CostTerms(engine, keep_builtin=True)
    t.norm(obs="site_minus_target", index=[0, 1], weight=3.0)
    return t.below_square(obs="site", index=2, target=0.40, weight=10.0)


def worst_case_program(rng, n_points=16, n_nodes=32):
    """16 points on paths of 32 hinges each, with anchors, refs and rotated frames: the largest program but one node a path."""
    rows = []
    for _ in range(n_points):
        for k in range(n_nodes):
            row = np.zeros(16)
            axis, quat = rng.standard_normal(3), rng.standard_normal(4)
            row[0], row[1], row[2] = 1, k, rng.uniform(-0.1, 0.1)
            row[3:6], row[6:10] = rng.uniform(-0.1, 0.1, 3), quat / np.linalg.norm(quat)
            row[10:13], row[13:16] = axis / np.linalg.norm(axis), rng.uniform(-0.05, 0.05, 3)
            rows.append(row)
        row = np.zeros(16)
        row[3:6] = rng.uniform(-0.1, 0.1, 3)
        rows.append(row)
    return np.stack(rows), len(rows), n_points, 0


def time_launches(windows, launches):
    import torch
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    lib = _lib.require_gpu()
    N = 4096 * 32
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    reacher, tray = ArmRolloutEngine.host_only(reacher7dof_raw()), TreeRolloutEngine.host_only(synthetic_raw("tray"))
    cases = [("reacher, 1 point", reacher_terms(reacher, True).points_table(), int(reacher.model.d_obs), reacher._nq),
             ("tray, 2 points and 1 difference", tray_terms(tray, True).points_table(), int(tray.model.d_obs), tray._nq),
             ("16 points on 32-hinge paths", worst_case_program(rng), 70, 32)]
    for label, (program, n_rows, n_points, n_diff), d_obs, nq in cases:
        d_aug = d_obs + 3 * (n_points + n_diff)
        obs = rng.uniform(-1.0, 1.0, (N, d_obs))
        obs[:, :nq] /= np.maximum(1.0, np.linalg.norm(obs[:, :nq], axis=1, keepdims=True)) * 0.5       # (no zero quaternion)
        obs, out, prog = dev(obs), torch.empty((N, d_aug), dtype=torch.float64, device="cuda"), dev(program)
        half = N * (d_obs + d_aug) // 2
        src, dst = torch.empty(half, dtype=torch.float64, device="cuda").normal_(), torch.empty(half, dtype=torch.float64, device="cuda")
        variants = {
            "mjmpc_points": lambda: _lib.check(lib.mjmpc_points(_lib.F64, N, d_obs, nq, vp(obs), vp(prog), n_rows, n_points,
                                                                n_diff, vp(out), stream)),
            "copy_ of %.1f MB in and out" % (8e-6 * N * (d_obs + d_aug)): lambda: dst.copy_(src),
        }
        _show("4096 x 32  %s, d_obs %d -> %d, %d program rows [us]" % (label, d_obs, d_aug, len(program)),
              _alternate(variants, windows, launches, 1e3))


def time_control_steps(windows, steps, only=None):
    import gc

    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    for label, make_engine, make_terms, P, H, cov in (
            ("reacher, arm engine, MPPI 4096 x 32", lambda: ArmRolloutEngine(reacher7dof_raw()), reacher_terms, 4096, 32, 0.1),
            ("tray, tree engine, MPPI 1024 x 48", lambda: TreeRolloutEngine(synthetic_raw("tray")), tray_terms, 1024, 48, 0.01)):
        if only is not None and not label.startswith(only):
            continue
        loops = {}
        for variant, points in (("rows on plain observation entries", False), ("rows on points", True)):
            eng = make_engine()
            if "tray" in label:
                st = start_state("tray", eng.raw)
                eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
            eng.on_env_reset = "ignore"
            terms = make_terms(eng, points)
            eng.set_cost_terms(terms)
            c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                             gamma=0.98, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                             seed=11, base_action="null", noise_mode="device", init_cov=cov, lam=0.05, step_size=0.8, alpha=1)
            c.rollout_fn = make_device_rollout_fn(eng)
            c.set_sim_state_fn = lambda s: None
            c.enable_graph(post_step=eng.step_state)
            loops[variant] = (lambda c=c: c.optimize({}))
            gc.collect()
            gc.disable()
            try:
                loops[variant]()
            finally:
                gc.enable()
            print("%-36s %-34s %d rows  %s" % (label, variant, len(terms), c.launch_mode), flush=True)
        _show(label + " [ms per step]", _alternate(loops, windows, steps, 1.0))

    if only in (None, "batch"):
        from mjmpc_amd.control import BatchedMPPI
        from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
        E, P, H = 16, 256, 32
        env = Reacher7DOFEnv()
        states = []
        for e in range(E):
            env.reset(seed=123 + e)
            st = env.get_env_state()
            states.append(dict(qp=st["qp"].copy(), qv=st["qv"].copy(), target_pos=st["target_pos"].copy()))
        env.engine.close()
        loops = {}
        for variant, points in (("rows on plain observation entries", False), ("rows on points", True)):
            b = BatchedMPPI(reacher7dof_raw(), E, H, P, 0.05, 0.8, 0.1, 0.98, [0.25, 0.8, 0.0], "null", list(range(E)), dtype="f64",
                            engine="arm")
            b.set_states([dict(s) for s in states])
            b.set_cost_terms(reacher_terms(b.engine, points))
            loops[variant] = b.step
        _show("reacher, arm engine, BatchedMPPI 16 x 256 x 32 [ms per step]", _alternate(loops, windows, steps, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--part", choices=["all", "launches", "reacher", "tray", "batch"], default="all")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    if args.part in ("all", "launches"):
        time_launches(args.windows, args.launches)
    if args.part != "launches":
        time_control_steps(args.windows, args.steps, None if args.part == "all" else args.part)


if __name__ == "__main__":
    main()
