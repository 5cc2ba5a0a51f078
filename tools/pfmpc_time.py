"""Control-step time of PFMPC in host and device mode (profiles/r08_pfmpc.txt):
    python tools/pfmpc_time.py [--particles 4096,65536] [--horizon 32] [--modes host,device] [--steps 20] [--warmup 5]
reacher (arm engine) and HalfCheetah (tree engine), f64.  Device events around ``--steps`` closed-loop control steps after
``--warmup``: ms per ``optimize()`` (the host's work between launches is inside the window: it is what a control loop
waits for).  Device mode then runs the same steps again with an event pair around every library launch of the step: the
per-kernel split, and what the non-rollout launches add to the rollout kernel's time."""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mjmpc_amd import _lib                                                                  # noqa: E402
from mjmpc_amd.control import PFMPC                                                         # noqa: E402
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn, make_rollout_fn   # noqa: E402

SPLIT = ("mjmpc_pf_delta", "mjmpc_arm_rollout_fused", "mjmpc_tree_rollout_fused", "mjmpc_pf_weights", "mjmpc_pf_resample",
         "mjmpc_pf_gather_shift", "mjmpc_pf_finish")


def make(model, mode, P, H):
    if model == "reacher":
        from mjmpc_amd.models.reacher7dof import reacher7dof_raw
        eng = ArmRolloutEngine(reacher7dof_raw(), dtype="f64")
        eng.set_env_state(dict(qp=np.zeros(7), qv=np.zeros(7), target_pos=np.array([0.1, 0.1, 0.1])))
        kw = dict(cov_shift=0.05, cov_resample=1.0, lam=0.05)
    else:
        from mjmpc_amd.envs.locomotion_env import HalfCheetahEnv
        from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
        from mjmpc_amd.models.half_cheetah import half_cheetah_raw
        eng = TreeRolloutEngine(half_cheetah_raw(), dtype="f64")
        env = HalfCheetahEnv(dtype="f64")
        env.reset(seed=123)
        eng.set_env_state(env.get_env_state())
        kw = dict(cov_shift=0.02, cov_resample=0.3, lam=0.5)
    c = PFMPC(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, base_action="null", num_particles=P,
              gamma=1.0, n_iters=1, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0],
              seed=123, noise_mode=mode, **kw)
    c.rollout_fn = make_device_rollout_fn(eng) if mode == "device" else make_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None                 # the engine keeps the real env's state: step_state advances it
    return c, eng


def run(c, eng, steps):
    for _ in range(steps):
        a, _ = c.optimize({})
        eng.step_state(a)


def timed(c, eng, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    run(c, eng, steps)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def split(c, eng, steps):
    """ms per step of every library launch of the device step (an event pair around each call)."""
    lib, saved, spans = _lib.load(), {}, OrderedDict()
    for name in SPLIT:
        fn = saved[name] = getattr(lib, name)

        def wrapper(*args, _fn=fn, _name=name):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = _fn(*args)
            e1.record()
            spans.setdefault(_name, []).append((e0, e1))
            return rc
        setattr(lib, name, wrapper)
    try:
        run(c, eng, steps)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)
    return OrderedDict((n, sum(a.elapsed_time(b) for a, b in ev) / steps) for n, ev in spans.items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="4096")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--modes", default="host,device")
    ap.add_argument("--models", default="reacher,half_cheetah")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    print("PFMPC control step, f64, %d steps after %d, device events; %s" % (args.steps, args.warmup, torch.cuda.get_device_name(0)))
    for model in args.models.split(","):
        for P in (int(p) for p in args.particles.split(",")):
            for mode in args.modes.split(","):
                c, eng = make(model, mode, P, args.horizon)
                run(c, eng, args.warmup)
                ms = timed(c, eng, args.steps)
                print("%-12s %6d x %d  %-6s  %10.3f ms per control step" % (model, P, args.horizon, mode, ms), flush=True)
                if mode == "device":
                    parts = split(c, eng, args.steps)
                    roll = sum(v for n, v in parts.items() if "rollout" in n)
                    for n, v in parts.items():
                        print("    %-28s %9.1f us" % (n, 1e3 * v))
                    print("    rollout kernel %.1f us, the other launches add %.1f us" % (1e3 * roll, 1e3 * (sum(parts.values()) - roll)),
                          flush=True)
                eng.close()


if __name__ == "__main__":
    main()
