#!/usr/bin/env python
"""What orientation errors in the cost terms cost on the device, device events, the variants alternating in one
process.

    python tools/orient_time.py [--windows 7] [--launches 200] [--steps 50] [--part all|launches|forced|tray] [--dtype f64|f32]

1. ``mjmpc_points_orient`` alone over 4096 x 32 rows, on the reacher's last link and on the tray's glass: one absolute orientation,
   one relative orientation (to the first link / to the tray), and what a user could launch without it - ``mjmpc_points_motion``
   with three ``axis`` outputs on the same body, which pins the orientation with three slots and no angle.
2. A table with no orientation (examples/configs/tray_upright_gpu.yml) forced through the new entry against its own entry.
   For the record: the engines never do this.
3. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on the tray, 4096 x 32, with
   examples/configs/tray_level_gpu.yml's terms against as many rows of the same kinds on plain observation entries.

Every line gives the median, minimum and maximum over the windows."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from com_time import _config_terms, _tile          # noqa: E402
from tracking_time import _alternate, _show        # noqa: E402

N = 4096 * 32


def _launchers(dtype):
    import torch
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    code, tdt = (_lib.F32, torch.float32) if dtype == "f32" else (_lib.F64, torch.float64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                            # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def observations(engine, rng):
        d_obs = int(engine.model.d_obs)
        obs = rng.uniform(-1.0, 1.0, (N, d_obs))
        obs[:, :engine._nq] /= np.maximum(1.0, np.linalg.norm(obs[:, :engine._nq], axis=1, keepdims=True)) * 0.5
        return dev(obs).to(tdt)

    def launcher(engine, obs, table, force_orient=False):
        """The table's own entry, or - ``force_orient`` - ``mjmpc_points_orient`` whatever the table holds."""
        d_obs, nq, nv = int(engine.model.d_obs), engine._nq, int(engine.model.nv)
        program, n_rows, n_out, n_diff = table[:4]
        out, prog = torch.empty((N, d_obs + 3 * (n_out + n_diff)), dtype=tdt, device="cuda"), dev(program)
        dof = dev(table[4])
        levels = table[5] if len(table) > 5 else 0
        if len(table) > 6 or force_orient:
            return lambda: _lib.check(lib.mjmpc_points_orient(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                              n_diff, levels, vp(out), stream))
        if len(table) > 5:
            return lambda: _lib.check(lib.mjmpc_points_tree(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                            n_diff, levels, vp(out), stream))
        return lambda: _lib.check(lib.mjmpc_points_motion(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                          n_diff, vp(out), stream))
    return observations, launcher


def time_launches(windows, launches, dtype):
    from mjmpc_amd.envs import cost_terms as ct
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    observations, launcher = _launchers(dtype)
    rng = np.random.default_rng(0)
    word = 4 if dtype == "f32" else 8
    reacher, tray = reacher7dof_raw(), synthetic_raw("tray")
    last = max(i for i, b in enumerate(reacher.bodies) if b.joint is not None)
    first = min(i for i, b in enumerate(reacher.bodies) if b.joint is not None)
    for label, engine, body, other in (("reacher, last link", ArmRolloutEngine.host_only(reacher), reacher.bodies[last].name,
                                        reacher.bodies[first].name),
                                       ("tray, the glass", TreeRolloutEngine.host_only(tray), "glass", "wrist")):
        obs, d_obs = observations(engine, rng), int(engine.model.d_obs)
        tables = {"mjmpc_points_orient: one absolute orientation": ct.CostTerms(engine).orientation(
                      "r", body=body, target=(0.6, 0.0, 0.8, 0.0)).points_table(),
                  "mjmpc_points_orient: one orientation relative to %s" % other: ct.CostTerms(engine).orientation(
                      "r", body=body, relative_to=other).points_table(),
                  "mjmpc_points_motion: three axes of the body": ct.CostTerms(engine).axis("x", body=body, axis=(1, 0, 0)).axis(
                      "y", body=body, axis=(0, 1, 0)).axis("z", body=body, axis=(0, 0, 1)).points_table()}
        runs = {}
        for what, table in tables.items():
            rows, lds = _tile(word, d_obs, table[2], 0)
            runs["%s (%d program rows, tile %d rows, %d B LDS)" % (what, table[1], rows, lds)] = launcher(engine, obs, table)
        _show("4096 x 32 %s  %s, d_obs %d [us]" % (dtype, label, d_obs), _alternate(runs, windows, launches, 1e3))


def time_forced(windows, launches, dtype):
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.synthetic import synthetic_raw
    observations, launcher = _launchers(dtype)
    engine = TreeRolloutEngine.host_only(synthetic_raw("tray"))
    obs = observations(engine, np.random.default_rng(1))
    table = _config_terms(engine, "tray_upright_gpu.yml").points_table()
    runs = {"mjmpc_points_motion: tray_upright_gpu.yml (%d program rows)" % table[1]: launcher(engine, obs, table),
            "mjmpc_points_orient: the same table, n_levels 0": launcher(engine, obs, table, force_orient=True)}
    _show("4096 x 32 %s  tray, a table without an orientation, d_obs %d [us]" % (dtype, int(engine.model.d_obs)),
          _alternate(runs, windows, launches, 1e3))


def time_control_steps(windows, steps):
    import gc

    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.synthetic import start_state, synthetic_raw

    label, P, H = "tray, tree engine, MPPI 4096 x 32", 4096, 32
    loops = {}
    for variant in ("rows on plain observation entries", "tray_level_gpu.yml's terms"):
        raw = synthetic_raw("tray")
        eng = TreeRolloutEngine(raw)
        eng.on_env_reset = "ignore"
        st = start_state("tray", raw)
        eng.set_env_state(dict(qp=st["qp"], qv=np.zeros(raw.nv), target_pos=st["target_pos"]))
        if variant.startswith("rows"):
            # (a norm over two entries, a one-sided square, a norm over three: the kinds and row counts of the example's terms)
            terms = CostTerms(eng, keep_builtin=True).norm(obs="qpos", index=[0, 1], weight=3.0)
            terms.below_square(obs="qpos", index=2, target=0.40, weight=10.0).norm(obs="qvel", index=[0, 1, 2], weight=2.0)
        else:
            terms = _config_terms(eng, "tray_level_gpu.yml")
        eng.set_cost_terms(terms)
        c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                         gamma=1.0, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                         seed=11, base_action="null", noise_mode="device", init_cov=0.01, lam=0.02, step_size=1.0, alpha=1)
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
        print("%-40s %-34s %d rows  %s" % (label, variant, len(terms), c.launch_mode), flush=True)
    _show(label + " [ms per step]", _alternate(loops, windows, steps, 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--part", choices=["all", "launches", "forced", "tray"], default="all")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64", help="storage type of the launches of parts 1 and 2")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    if args.part in ("all", "launches"):
        time_launches(args.windows, args.launches, args.dtype)
    if args.part in ("all", "forced"):
        time_forced(args.windows, args.launches, args.dtype)
    if args.part in ("all", "tray"):
        time_control_steps(args.windows, args.steps)


if __name__ == "__main__":
    main()
