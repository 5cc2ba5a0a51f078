#!/usr/bin/env python
"""What centres of mass in the cost terms cost on the device, device events, the variants alternating in one
process.

    python tools/com_time.py [--windows 7] [--launches 200] [--steps 50] [--part all|launches|forced|cheetah] [--dtype f64|f32]

1. ``mjmpc_points_tree`` alone over 4096 x 32 rows: HalfCheetah's and hand24's whole-model centre of mass with its velocity
   against what a user can launch without it - ``mjmpc_points_motion`` with a point and its velocity at every heavy body's
   inertial position, in as many launches as 16 outputs a table make necessary (the weighted sum would still be ``linear`` rows).
2. A table with no centre of mass (examples/configs/tray_upright_gpu.yml) forced through the new entry against its own entry.
   For the record: the engines never do this.
3. The captured control step (MPPI, ``enable_graph(post_step=engine.step_state)``) on HalfCheetah, 4096 x 32, with
   examples/configs/half_cheetah_com_gpu.yml's terms against as many rows of the same kinds on plain observation entries.

Every line gives the median, minimum and maximum over the windows."""
import argparse
import ctypes
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tracking_time import _alternate, _show        # noqa: E402

N = 4096 * 32


def _tile(word, d_obs, n_out, n_levels):
    """The launcher's sizing rule (include/mjmpc_amd.h): rows of a workgroup's tile and its LDS bytes."""
    rows = 256
    lds = lambda r: (r * word * (d_obs | 1) + 7) // 8 * 8 + r * (24 * n_out + 104 * n_levels)      # noqa: E731
    while lds(rows) > 60 * 1024:
        rows >>= 1
    return rows, lds(rows)


def _cheetah_raw():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    return dataclasses.replace(half_cheetah_raw(), obs_skip=0)


def _config_terms(engine, name):
    import yaml
    from mjmpc_amd.envs.cost_terms import cost_terms_from_config
    with open(os.path.join(ROOT, "examples", "configs", name)) as f:
        return cost_terms_from_config(yaml.safe_load(f)["cost_terms"], engine)


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

    def launcher(engine, obs, table, force_tree=False):
        d_obs, nq, nv = int(engine.model.d_obs), engine._nq, int(engine.model.nv)
        program, n_rows, n_out, n_diff = table[:4]
        out, prog = torch.empty((N, d_obs + 3 * (n_out + n_diff)), dtype=tdt, device="cuda"), dev(program)
        dof = dev(table[4])
        if len(table) > 5 or force_tree:
            levels = table[5] if len(table) > 5 else 0
            return lambda: _lib.check(lib.mjmpc_points_tree(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                            n_diff, levels, vp(out), stream))
        return lambda: _lib.check(lib.mjmpc_points_motion(code, N, d_obs, nq, nv, vp(obs), vp(prog), vp(dof), n_rows, n_out,
                                                          n_diff, vp(out), stream))
    return observations, launcher


def time_launches(windows, launches, dtype):
    from mjmpc_amd.envs import cost_terms as ct
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.hand24 import hand24_raw
    observations, launcher = _launchers(dtype)
    rng = np.random.default_rng(0)
    word = 4 if dtype == "f32" else 8
    for label, raw in (("HalfCheetah", _cheetah_raw()), ("hand24", hand24_raw())):
        engine = TreeRolloutEngine.host_only(raw)
        obs, d_obs = observations(engine, rng), int(engine.model.d_obs)
        terms = ct.CostTerms(engine).com("com").com_velocity("vel", "com")
        table = terms.points_table()
        rows, lds = _tile(word, d_obs, table[2], table[5])
        runs = {"mjmpc_points_tree: the centre of mass and its velocity (%d program rows, n_levels %d, tile %d rows, %d B LDS)"
                % (table[1], table[5], rows, lds): launcher(engine, obs, table)}
        mass, ipos = ct.inertials(engine)
        heavy = [b for b in range(len(raw.bodies)) if mass[b] > 0]
        parts, n_prog = [], 0
        for at in range(0, len(heavy), 8):
            t = ct.CostTerms(engine)
            for b in heavy[at:at + 8]:
                t.point("p%d" % b, body=raw.bodies[b].name, pos=ipos[b]).velocity("v%d" % b, "p%d" % b)
            parts.append(launcher(engine, obs, t.points_table()))
            n_prog += t.points_table()[1]
        rows_m, lds_m = _tile(word, d_obs, 2 * min(8, len(heavy)), 0)
        runs["mjmpc_points_motion: a point and its velocity at %d bodies' ipos (%d launches, %d program rows, tile %d rows, %d B LDS)"
             % (len(heavy), len(parts), n_prog, rows_m, lds_m)] = (lambda parts=parts: [p() for p in parts])
        _show("4096 x 32 %s  %s, d_obs %d [us]" % (dtype, label, d_obs), _alternate(runs, windows, launches, 1e3))


def time_forced(windows, launches, dtype):
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.synthetic import synthetic_raw
    observations, launcher = _launchers(dtype)
    engine = TreeRolloutEngine.host_only(synthetic_raw("tray"))
    obs = observations(engine, np.random.default_rng(1))
    table = _config_terms(engine, "tray_upright_gpu.yml").points_table()
    runs = {"mjmpc_points_motion: tray_upright_gpu.yml (%d program rows)" % table[1]: launcher(engine, obs, table),
            "mjmpc_points_tree: the same table, n_levels 0": launcher(engine, obs, table, force_tree=True)}
    _show("4096 x 32 %s  tray, a table without a centre of mass, d_obs %d [us]" % (dtype, int(engine.model.d_obs)),
          _alternate(runs, windows, launches, 1e3))


def time_control_steps(windows, steps):
    import gc

    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine

    label, P, H = "HalfCheetah, tree engine, MPPI 4096 x 32", 4096, 32
    loops = {}
    for variant in ("rows on plain observation entries", "half_cheetah_com_gpu.yml's terms"):
        eng = TreeRolloutEngine(_cheetah_raw())
        eng.on_env_reset = "ignore"
        if variant.startswith("rows"):
            terms = CostTerms(eng, keep_builtin=True).linear(obs="qvel", index=0, weight=-1.0)
            terms.outside(obs="qpos", index=1, low=-0.15, high=0.25, weight=5.0)
        else:
            terms = _config_terms(eng, "half_cheetah_com_gpu.yml")
        eng.set_cost_terms(terms)
        c = control.MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1,
                         gamma=1.0, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
                         seed=11, base_action="null", noise_mode="device", init_cov=0.3, lam=0.2, step_size=1.0, alpha=1)
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
    ap.add_argument("--part", choices=["all", "launches", "forced", "cheetah"], default="all")
    ap.add_argument("--dtype", choices=["f64", "f32"], default="f64", help="storage type of the launches of parts 1 and 2")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    if args.part in ("all", "launches"):
        time_launches(args.windows, args.launches, args.dtype)
    if args.part in ("all", "forced"):
        time_forced(args.windows, args.launches, args.dtype)
    if args.part in ("all", "cheetah"):
        time_control_steps(args.windows, args.steps)


if __name__ == "__main__":
    main()
