#!/usr/bin/env python
"""What body axes and velocities in the cost terms cost on the device, f64 (``--dtype f32``: the launches of part 1
on f32 rows), device events, the variants alternating in one process.

    python tools/motion_time.py [--windows 7] [--launches 200] [--steps 100] [--part all|launches|tray] [--dtype f64|f32]

1. The launch alone over 4096 x 32 rows: ``mjmpc_points_motion`` for the reacher with a point, its velocity and an axis on the
   last link against ``mjmpc_points`` with that point alone; the tray with examples/configs/tray_upright_gpu.yml's outputs
   against tray_points_gpu.yml's; and an axes-only table (one axis on the reacher's last link) through the motion entry against
   the same path through ``mjmpc_points`` as a point - what the six extra doubles and the cross products cost a walk that
   needs neither.
2. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on the tray, tree engine, 1024 x 48, with
   the upright config's terms against the same number of rows of the same kinds on plain observation entries, ms per step.

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


def reacher_terms(engine, which):
    """The last link's origin ('point'), with its velocity and the link's z axis ('motion'), or the axis alone ('axis')."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t, last = CostTerms(engine), engine.raw.bodies[-1].name
    if which in ("point", "motion"):
        t.point("tip", body=last)
    if which == "motion":
        t.velocity("tip_vel", "tip")
    if which in ("axis", "motion"):
        t.axis("tip_z", body=last, axis=(0.0, 0.0, 1.0))
    return t


def tray_terms(engine, which):
    """examples/configs/tray_upright_gpu.yml's terms ('motion'), tray_points_gpu.yml's ('points'), or as many rows as the
    upright config's of the same kinds on plain observation entries ('plain')."""
    import yaml
    from mjmpc_amd.envs.cost_terms import CostTerms, cost_terms_from_config
    if which != "plain":
        with open(os.path.join(ROOT, "examples", "configs", "tray_%s_gpu.yml" % ("upright" if which == "motion" else "points"))) as f:
            return cost_terms_from_config(yaml.safe_load(f)["cost_terms"], engine)
    t = CostTerms(engine, keep_builtin=True)
    t.norm(obs="site_minus_target", index=[0, 1], weight=3.0)
    t.below_square(obs="site", index=2, target=0.40, weight=10.0)
    t.linear(obs="site", index=2, weight=-2.0)
    return t.norm(obs="qvel", index=[0, 1, 2], weight=0.5)


def time_launches(windows, launches, dtype="f64"):
    import torch
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    lib = _lib.require_gpu()
    N = 4096 * 32
    code, tdt = (_lib.F32, torch.float32) if dtype == "f32" else (_lib.F64, torch.float64)
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    reacher, tray = ArmRolloutEngine.host_only(reacher7dof_raw()), TreeRolloutEngine.host_only(synthetic_raw("tray"))

    def launcher(engine, obs, table):
        d_obs, nq, nv = int(engine.model.d_obs), engine._nq, int(engine.model.nv)
        program, n_rows, n_out, n_diff = table[:4]
        out, prog = torch.empty((N, d_obs + 3 * (n_out + n_diff)), dtype=tdt, device="cuda"), dev(program)
        if len(table) == 4:
            return lambda: _lib.check(lib.mjmpc_points(code, N, d_obs, nq, vp(obs), vp(prog), n_rows, n_out, n_diff, vp(out),
                                                       stream))
        dof = dev(table[4])
        return lambda: _lib.check(lib.mjmpc_points_motion(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                          n_diff, vp(out), stream))

    for label, engine, variants in (
            ("reacher, last link", reacher, (("mjmpc_points: the point", reacher_terms(reacher, "point")),
                                             ("mjmpc_points_motion: point, velocity, axis", reacher_terms(reacher, "motion")))),
            ("tray", tray, (("mjmpc_points: tray_points_gpu.yml", tray_terms(tray, "points")),
                            ("mjmpc_points_motion: tray_upright_gpu.yml", tray_terms(tray, "motion")))),
            ("reacher, one walk of the last link's path", reacher,
             (("mjmpc_points: the walk closed by a point", reacher_terms(reacher, "point")),
              ("mjmpc_points_motion: the walk closed by an axis", reacher_terms(reacher, "axis"))))):
        d_obs = int(engine.model.d_obs)
        obs = rng.uniform(-1.0, 1.0, (N, d_obs))
        obs[:, :engine._nq] /= np.maximum(1.0, np.linalg.norm(obs[:, :engine._nq], axis=1, keepdims=True)) * 0.5
        obs = dev(obs).to(tdt)
        runs = {}
        for name, terms in variants:
            table = terms.points_table()
            runs["%s (%d program rows, %d entries)" % (name, len(table[0]), terms.n_extra)] = launcher(engine, obs, table)
        _show("4096 x 32 %s  %s, d_obs %d [us]" % (dtype, label, d_obs), _alternate(runs, windows, launches, 1e3))


def time_control_steps(windows, steps):
    import gc

    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    label, P, H = "tray, tree engine, MPPI 1024 x 48", 1024, 48
    loops = {}
    for variant, which in (("rows on plain observation entries", "plain"), ("the upright config's terms", "motion")):
        eng = TreeRolloutEngine(synthetic_raw("tray"))
        st = start_state("tray", eng.raw)
        eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
        eng.on_env_reset = "ignore"
        terms = tray_terms(eng, which)
        eng.set_cost_terms(terms)
        c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                         gamma=0.98, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                         seed=11, base_action="null", noise_mode="device", init_cov=0.01, lam=0.05, step_size=0.8, alpha=1)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--part", choices=["all", "launches", "tray"], default="all")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64", help="storage type of the launches of part 1")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    if args.part in ("all", "launches"):
        time_launches(args.windows, args.launches, args.dtype)
    if args.part in ("all", "tray"):
        time_control_steps(args.windows, args.steps)


if __name__ == "__main__":
    main()
