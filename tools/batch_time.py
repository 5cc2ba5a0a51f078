#!/usr/bin/env python
"""Episode batches (BatchedMPPI): ms per batched control step and episode-steps/s, against the sequential loop.

For every model x E x P x H: one ``BatchedMPPI`` of E episodes of P particles (f64), timed with device events over
--steps control steps after --warmup; in the same process the single-episode device path on its own engine (MPPI,
noise_mode='device', graph replay, the env step on the device: what each episode of the reference's loop would run), timed
the same way.  The sequential loop of E episodes costs E times that per control step (the episodes are independent runs of
the same shape).  One JSON line per configuration, then a table.

    python tools/batch_time.py [--models half_cheetah,swimmer,sawyer] [--E 1,4,16,64] [--P 256,1024] [--H 16,32]
        [--model-shards K]

--model-shards K: the batch rolls out K randomized model shards per episode (a set per episode, body masses
+- 20 %) and the single-episode path is the sequential dynamics-randomized loop - a K-shard engine with randomized blocks
and a nominal real env.  K = 1 without the option is the un-randomized batch.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FILT = [0.25, 0.8, 0.0]


def models():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.swimmer import swimmer_raw
    return {"half_cheetah": (half_cheetah_raw, 0.2, 0.3), "swimmer": (swimmer_raw, 0.2, 0.3), "sawyer": (reacher7dof_raw, 0.01, 1.0)}


def dyn_cfg(raw):
    """Body masses +- 20 %: the first three bodies with a joint."""
    return {"body_mass": {b.name: [0.2, 0.0] for b in [b for b in raw.bodies if b.joint is not None][:3]}}


def time_batch(raw, E, P, H, lam, cov, steps, warmup, K=0):
    import torch
    from mjmpc_amd.control import BatchedMPPI
    b = BatchedMPPI(raw, E, H, P, lam, 1.0, cov, 1.0, FILT, "null", [123 + i * 12345 for i in range(E)])
    b.on_env_reset = "ignore"
    if K:
        b.randomize_dynamics(dyn_cfg(raw), [123 + i * 12345 for i in range(E)], K)
    for _ in range(warmup):
        b.step()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        b.step()
    e.record()
    torch.cuda.synchronize()
    b.close()
    return s.elapsed_time(e) / steps


def time_single(raw, P, H, lam, cov, steps, warmup, K=0):
    import torch
    from mjmpc_amd.control import MPPI
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, num_shards=max(K, 1))
    eng.on_env_reset = "ignore"
    if K:
        eng.randomize_dynamics(dyn_cfg(raw), 123)
        eng.set_real_env_model("nominal")
    c = MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, init_cov=cov, base_action="null", lam=lam,
             num_particles=P, step_size=1.0, alpha=1, gamma=1.0, n_iters=1, action_lows=eng.action_lows,
             action_highs=eng.action_highs, filter_coeffs=FILT, seed=123, noise_mode="device", noise_dtype="f64")
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda st: None
    c.enable_graph(post_step=eng.step_state)
    for _ in range(warmup):
        c.optimize(None)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        c.optimize(None)
    e.record()
    torch.cuda.synchronize()
    eng.close()
    return s.elapsed_time(e) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="half_cheetah,swimmer,sawyer")
    ap.add_argument("--E", default="1,4,16,64")
    ap.add_argument("--P", default="256,1024")
    ap.add_argument("--H", default="16,32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model-shards", type=int, default=0, help="randomized model shards per episode (0: no randomization)")
    args = ap.parse_args()
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    ms = models()
    rows = []
    for name in args.models.split(","):
        fn, lam, cov = ms[name]
        raw = fn()
        for H in [int(x) for x in args.H.split(",")]:
            for P in [int(x) for x in args.P.split(",")]:
                single = time_single(raw, P, H, lam, cov, args.steps, args.warmup, args.model_shards)
                for E in [int(x) for x in args.E.split(",")]:
                    batch = time_batch(raw, E, P, H, lam, cov, args.steps, args.warmup, args.model_shards)
                    row = dict(model=name, E=E, P=P, H=H, model_shards=args.model_shards, batch_ms_per_step=round(batch, 4),
                               batch_episode_steps_per_s=round(1e3 * E / batch, 1), single_ms_per_step=round(single, 4),
                               sequential_ms_per_step=round(E * single, 4), speedup=round(E * single / batch, 2))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    print("%-13s %3s %5s %3s %10s %10s %12s %8s" % ("model", "E", "P", "H", "batch ms", "single ms", "E x single", "speedup"))
    for r in rows:
        print("%-13s %3d %5d %3d %10.3f %10.3f %12.3f %8.2f" % (r["model"], r["E"], r["P"], r["H"], r["batch_ms_per_step"],
                                                             r["single_ms_per_step"], r["sequential_ms_per_step"], r["speedup"]))


if __name__ == "__main__":
    main()
