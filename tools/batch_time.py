#!/usr/bin/env python
"""Episode batches (BatchedMPPI / BatchedCEM / BatchedPFMPC / BatchedDMDMPC / BatchedRandomShooting / BatchedMPPIQ): ms per batched control step and episode-steps/s, against the sequential loop.

For every model x E x P x H: one ``BatchedMPPI`` of E episodes of P particles (f64), timed with device events over
--steps control steps after --warmup; in the same process the single-episode device path on its own engine (MPPI,
noise_mode='device', graph replay, the env step on the device: what each episode of the reference's loop would run), timed
the same way.  The sequential loop of E episodes costs E times that per control step (the episodes are independent runs of
the same shape).  One JSON line per configuration, then a table.

    python tools/batch_time.py [--models half_cheetah,swimmer,sawyer] [--E 1,4,16,64] [--P 256,1024] [--H 16,32]
        [--model-shards K] [--controller mppi|cem|pfmpc|dmd|random_shooting|mppiq] [--repeats R] [--engine tree|arm]
        [--cost-terms]

--engine arm: the batch runs on ``ArmRolloutEngine`` (``engine="arm"``; the models the arm kernels run: sawyer) and
the sequential baseline is the single-episode loop on that engine, as ``make_engine`` gives it to a user: the same controller on
``make_device_rollout_fn(ArmRolloutEngine)`` - for MPPI the fused two-launch step where the engine supports the shape.  The
per-launch split names the arm entry points.  No dynamics randomization (--model-shards) on this engine.

--controller cem: ``BatchedCEM`` (full covariance, elite_frac 0.1, beta 0.45) against the single-episode fused CEM
step (CEM, noise_mode='device', graph replay).  --repeats R: every configuration is timed R times, batch and single runs
alternating; the medians are reported with the single path's own spread (max - min over its repeats, ``single_spread_ms``).

--controller pfmpc: ``BatchedPFMPC`` (cov_shift 0.02, cov_resample = the model's init_cov, lam 1.0) against the
single-episode device path of particle-filter MPC (PFMPC, noise_mode='device', the resident real env stepped by
``set_post_step(engine.step_state)``; its ``optimize()`` waits for the action once per step, as that loop does).  After the
table: the per-launch split of one batched step (device events around every launch, so their sum exceeds the step's time).

--controller dmd: ``BatchedDMDMPC`` (full covariance, update_cov, beta 0.05) against the single-episode captured
DMD-MPC loop (DMDMPC, update_cov=True, noise_mode='device', graph replay: the general step of about ten launches), with the
per-launch split of one batched step as for pfmpc.

--controller random_shooting: ``BatchedRandomShooting`` (step_size 1.0, the model's init_cov) against the
single-episode captured random-shooting loop (RandomShooting, noise_mode='device', graph replay: draw, fused rollout, argmin,
record, combine, tail, env step), with the per-launch split of one batched step as for pfmpc.

--controller mppiq: ``BatchedMPPIQ`` (alpha 1, time-based weights, td_lam 0.9, beta = the model's lam) against the
single-episode captured MPPIQ loop (MPPIQ, noise_mode='device', graph replay: draw, rollout, TD(lambda) returns, weights,
maxima, partial moments, record, combine, tail, env step), with the per-launch split of one batched step as for pfmpc.

--cost-terms: instead of the comparison with the sequential loop, every configuration's batch is timed without
and with user-defined cost terms (``set_cost_terms``: ``CostTerms.builtin_reach`` for sawyer, ``keep_builtin`` plus four rows for
the forward-task models), the two batches alive in one process and their windows of --steps steps alternating, --repeats windows
each (median, min, max).  Then ``mjmpc_cost_terms_batch`` (with its cost-to-go) alone against ``mjmpc_cost_terms`` alone and
against a minimal launch (``mjmpc_cost_terms`` on one element) on the same buffers, 4096 x 32 and 2048 x 32 with the reacher's
widths, the six-row and the 32-row table of profiles/r16_cost_terms.txt, windows of 200 launches alternating.

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


ELITE_FRAC, BETA = 0.1, 0.45       # (--controller cem)
COV_SHIFT, PF_LAM, PF_GAMMA = 0.02, 1.0, 0.99       # (--controller pfmpc)
DMD_BETA = 0.05                     # (--controller dmd)
TD_LAM = 0.9                        # (--controller mppiq)

# --controller -> ``batch``: the batch class and, from (lam, cov), its arguments between num_particles and filter_coeffs;
# ``single``: the single-episode class and its own keywords; ``took``: whether that controller ran the intended branch, and the
# complaint if not; ``launches``: the library calls of one batched step that the split times (none: no split); ``resident``:
# the single path is the resident real env, no state is uploaded and the env step rides behind the finish launch.
CONTROLLERS = {
    "mppi": dict(
        batch=("BatchedMPPI", lambda lam, cov: (lam, 1.0, cov, 1.0)),
        single=("MPPI", lambda lam, cov: dict(init_cov=cov, lam=lam, step_size=1.0, alpha=1, gamma=1.0, noise_dtype="f64"))),
    "cem": dict(
        batch=("BatchedCEM", lambda lam, cov: (cov, ELITE_FRAC, 1.0, BETA, 1.0)),
        single=("CEM", lambda lam, cov: dict(init_cov=cov, elite_frac=ELITE_FRAC, step_size=1.0, gamma=1.0, beta=BETA,
                                             cov_type="full", noise_dtype="f64")),
        took=(lambda c: c._cem_fused(), "the single-episode CEM path did not take its fused step at {P} x {H}")),
    "pfmpc": dict(
        batch=("BatchedPFMPC", lambda lam, cov: (COV_SHIFT, cov, PF_LAM, PF_GAMMA)),
        single=("PFMPC", lambda lam, cov: dict(cov_shift=COV_SHIFT, cov_resample=cov, lam=PF_LAM, gamma=PF_GAMMA)),
        resident=True,
        launches=("mjmpc_pf_delta_batch", "mjmpc_tree_rollout_fused_batch", "mjmpc_pf_weights_batch", "mjmpc_pf_resample_batch",
                  "mjmpc_pf_gather_shift_batch", "mjmpc_pf_finish_batch", "mjmpc_tree_step_shard_states")),
    "dmd": dict(
        batch=("BatchedDMDMPC", lambda lam, cov: (lam, 1.0, cov, DMD_BETA, 1.0)),
        single=("DMDMPC", lambda lam, cov: dict(init_cov=cov, beta=DMD_BETA, lam=lam, step_size=1.0, gamma=1.0, update_cov=True,
                                                cov_type="full", noise_dtype="f64")),
        took=(lambda c: not c._fused_capable() and c._device_cov(),
              "the single-episode DMD-MPC path did not take its covariance-adapting step"),
        # (mjmpc_sample_noise_cov_batch is the draw and the filter launch, mjmpc_dmd_update_batch the three update launches)
        launches=("mjmpc_cholesky_lower_batch", "mjmpc_sample_noise_cov_batch", "mjmpc_tree_rollout_fused_batch",
                  "mjmpc_dmd_update_batch", "mjmpc_tree_step_shard_states")),
    "random_shooting": dict(
        batch=("BatchedRandomShooting", lambda lam, cov: (1.0, cov, 1.0)),
        single=("RandomShooting", lambda lam, cov: dict(init_cov=cov, step_size=1.0, gamma=1.0, noise_dtype="f64")),
        took=(lambda c: c._wants_q0() and hasattr(c._rollout_fn, "fused"),
              "the single-episode random-shooting path did not take its q0-from-rollout step"),
        launches=("mjmpc_sample_noise_batch", "mjmpc_tree_rollout_fused_batch", "mjmpc_rs_update_batch",
                  "mjmpc_tree_step_shard_states")),
    "mppiq": dict(
        batch=("BatchedMPPIQ", lambda lam, cov: (lam, 1.0, cov, TD_LAM, 1.0)),
        single=("MPPIQ", lambda lam, cov: dict(init_cov=cov, beta=lam, step_size=1.0, alpha=1, gamma=1.0, td_lam=TD_LAM,
                                               time_based_weights=True, noise_dtype="f64")),
        took=(lambda c: not c._fused_capable() and not c._wants_q0() and c._static_cov() and c._graph is not None,
              "the single-episode MPPIQ path did not run its captured general step"),
        # (mjmpc_sample_noise_cov_batch is the draw and the filter launch, mjmpc_mppiq_update_batch the three update launches)
        launches=("mjmpc_sample_noise_cov_batch", "mjmpc_tree_rollout_fused_batch", "mjmpc_mppiq_update_batch",
                  "mjmpc_tree_step_shard_states")),
}
LAUNCHES = {name: c["launches"] for name, c in CONTROLLERS.items() if "launches" in c}


def make_batch(raw, E, P, H, lam, cov, controller, engine="tree"):
    from mjmpc_amd import control
    cls, args = CONTROLLERS[controller]["batch"]
    return getattr(control, cls)(raw, E, H, P, *args(lam, cov), FILT, "null", [123 + i * 12345 for i in range(E)], engine=engine)


class _TimedLib:
    """The library with device events around the launches named in ``names``."""

    def __init__(self, lib, names):
        import torch
        self._lib, self._names, self._torch, self.events = lib, set(names), torch, {n: [] for n in names}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._names:
            return fn

        def timed(*a):
            s, e = self._torch.cuda.Event(enable_timing=True), self._torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn(*a)
            e.record()
            self.events[name].append((s, e))
            return rc
        return timed


def launch_names(controller, engine="tree"):
    """The library calls the split times: the rollout and the env step are the engine kind's."""
    return tuple(n.replace("mjmpc_tree_", "mjmpc_%s_" % engine) for n in LAUNCHES[controller])


def launch_split(raw, E, P, H, lam, cov, steps, warmup, controller="pfmpc", engine="tree"):
    """ms per library call of one batched PFMPC / DMD-MPC / random-shooting / MPPIQ step (mean over ``steps`` steps)."""
    import torch
    names = launch_names(controller, engine)
    b = make_batch(raw, E, P, H, lam, cov, controller, engine)
    b.on_env_reset = "ignore"
    for _ in range(warmup):
        b.step()
    b.lib = timed = _TimedLib(b.lib, names)
    for _ in range(steps):
        b.step()
    torch.cuda.synchronize()
    b.lib = timed._lib
    b.close()
    return {n: sum(s.elapsed_time(e) for s, e in timed.events[n]) / steps for n in names}


def time_batch(raw, E, P, H, lam, cov, steps, warmup, K=0, controller="mppi", engine="tree"):
    import torch
    b = make_batch(raw, E, P, H, lam, cov, controller, engine)
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


def time_single(raw, P, H, lam, cov, steps, warmup, K=0, controller="mppi", engine="tree"):
    import torch
    from mjmpc_amd import control
    from mjmpc_amd.control.controller import resident_state
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = (ArmRolloutEngine if engine == "arm" else TreeRolloutEngine)(raw, num_shards=max(K, 1))
    eng.on_env_reset = "ignore"
    if K:
        eng.randomize_dynamics(dyn_cfg(raw), 123)
        eng.set_real_env_model("nominal")
    cls, kw = CONTROLLERS[controller]["single"]
    c = getattr(control, cls)(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, base_action="null",
                              num_particles=P, n_iters=1, action_lows=eng.action_lows, action_highs=eng.action_highs,
                              filter_coeffs=FILT, seed=123, noise_mode="device", **kw(lam, cov))
    c.rollout_fn = make_device_rollout_fn(eng)
    if CONTROLLERS[controller].get("resident"):
        c.set_sim_state_fn = resident_state
        c.set_post_step(eng.step_state)
    else:
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
    took, complaint = CONTROLLERS[controller].get("took", (None, ""))
    if engine == "arm":         # (the arm engine's single path takes its own branches - the fused iteration where it has one)
        took = None
    if took is not None and not took(c):
        raise SystemExit(complaint.format(P=P, H=H))
    eng.close()
    return s.elapsed_time(e) / steps


def batch_terms(name, b):
    """--cost-terms: the table a model's batch is timed with."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    if name == "sawyer":
        return CostTerms.builtin_reach(b.engine)
    t = CostTerms(b.engine, keep_builtin=True)
    t.square(obs="qvel", index=0, weight=0.1, target=1.0)
    t.abs(obs="qpos", index=1, weight=0.5)
    t.square(action=0, weight=0.01)
    t.square(obs="qvel", index=2, weight=0.2, terminal=True)
    return t


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def time_with_and_without_terms(raw, name, E, P, H, lam, cov, steps, warmup, repeats, controller, engine):
    """ms per batched step -> {variant: [windows]}: one batch without and one with terms, windows alternating."""
    import torch
    batches = {}
    for variant in ("builtin", "terms"):
        b = batches[variant] = make_batch(raw, E, P, H, lam, cov, controller, engine)
        b.on_env_reset = "ignore"
        if variant == "terms":
            b.set_cost_terms(batch_terms(name, b))
        for _ in range(warmup):
            b.step()
    torch.cuda.synchronize()
    out = {v: [] for v in batches}
    for _ in range(repeats):
        for variant, b in batches.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(steps):
                b.step()
            e.record()
            torch.cuda.synchronize()
            out[variant].append(s.elapsed_time(e) / steps)
    for b in batches.values():
        b.close()
    return out


def time_terms_kernels(E=16, windows=7, launches=200):
    """us per launch -> {table: {variant: [windows]}} at E x 256 particles, H 32, d_obs 20, A 7 (f64), the variants alternating."""
    import ctypes
    import numpy as np
    import torch
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    lib = _lib.require_gpu()
    host = ArmRolloutEngine.host_only(reacher7dof_raw())
    mixed = CostTerms(host).square(obs="qvel", weight=0.01).square(action=True, weight=0.001).cos(obs="qpos", weight=0.1)
    mixed.abs(obs="site_minus_target").norm(obs="site_minus_target", weight=5.0).square(obs="qvel", index=[0, 1, 2, 3, 4],
                                                                                         weight=1.0, terminal=True)
    P, H, D, A = 256, 32, 20, 7
    N = E * P
    rng = np.random.default_rng(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()        # noqa: E731
    nobs, act, costs = dev(rng.uniform(-1, 1, (N, H, D))), dev(rng.uniform(-1, 1, (N, H, A))), dev(rng.uniform(0, 1, (N, H)))
    gseq, q0 = dev(np.cumprod([1.0] + [0.99] * (H - 1))), torch.empty(N, dtype=torch.float64, device="cuda")
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())     # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}
    for label, terms in (("builtin_reach (6 rows)", CostTerms.builtin_reach(host)), ("mixed (32 rows)", mixed)):
        table = terms.table()
        per_episode = dev(np.stack([table] * E))
        tab, K = dev(table), len(table)
        a = act if np.any(table[:, 1] != 0) else None
        variants = {
            "mjmpc_cost_terms": lambda: lib.mjmpc_cost_terms(_lib.F64, N, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 1, vp(costs), stream),
            "minimal launch (mjmpc_cost_terms on one element)":
                lambda: lib.mjmpc_cost_terms(_lib.F64, 1, 1, D, A, vp(nobs), vp(a), vp(tab), K, 0, 1, vp(costs), stream),
            "mjmpc_cost_terms_batch, no q0":
                lambda: lib.mjmpc_cost_terms_batch(_lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 0, 1, vp(costs), None, None, stream),
            "mjmpc_cost_terms_batch + q0":
                lambda: lib.mjmpc_cost_terms_batch(_lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(tab), K, 0, 0, 1, vp(costs), vp(gseq), vp(q0), stream),
            "mjmpc_cost_terms_batch + q0, a table per episode":
                lambda: lib.mjmpc_cost_terms_batch(_lib.F64, E, P, H, D, A, vp(nobs), vp(a), vp(per_episode), K, 1, 0, 1, vp(costs), vp(gseq), vp(q0), stream),
        }
        for fn in variants.values():
            for _ in range(50):
                _lib.check(fn())
        torch.cuda.synchronize()
        res = out[label] = {v: [] for v in variants}
        for _ in range(windows):
            for v, fn in variants.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(launches):
                    fn()
                e.record()
                torch.cuda.synchronize()
                res[v].append(1e3 * s.elapsed_time(e) / launches)
    return out


def main_cost_terms(args):
    ms = models()
    for name in args.models.split(","):
        fn, lam, cov = ms[name]
        raw = fn()
        for H in [int(x) for x in args.H.split(",")]:
            for P in [int(x) for x in args.P.split(",")]:
                for E in [int(x) for x in args.E.split(",")]:
                    w = time_with_and_without_terms(raw, name, E, P, H, lam, cov, args.steps, args.warmup, max(args.repeats, 3),
                                                    args.controller, args.engine)
                    row = dict(model=name, controller=args.controller, engine=args.engine, E=E, P=P, H=H)
                    for v, xs in w.items():
                        row[v + "_ms_per_step"] = dict(median=round(_median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4))
                    row["terms_over_builtin"] = round(_median(w["terms"]) / _median(w["builtin"]), 4)
                    print(json.dumps(row), flush=True)
    # (16 x 256 x 32 elements are 8 workgroups per CU on 256 CUs, 8 x 256 x 32 are 4: one round of workgroups for both kernels)
    for E in (16, 8):
        for label, res in time_terms_kernels(E).items():
            for v, xs in res.items():
                print("%5d x 32  %-24s %-52s median %8.2f us  (min %8.2f, max %8.2f)"
                      % (E * 256, label, v, _median(xs), min(xs), max(xs)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="half_cheetah,swimmer,sawyer")
    ap.add_argument("--E", default="1,4,16,64")
    ap.add_argument("--P", default="256,1024")
    ap.add_argument("--H", default="16,32")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model-shards", type=int, default=0, help="randomized model shards per episode (0: no randomization)")
    ap.add_argument("--controller", default="mppi", choices=["mppi", "cem", "pfmpc", "dmd", "random_shooting", "mppiq"])
    ap.add_argument("--repeats", type=int, default=1, help="timings per configuration, batch and single runs alternating")
    ap.add_argument("--engine", default="tree", choices=["tree", "arm"], help="the engine of the batch and of the single-episode loop")
    ap.add_argument("--cost-terms", action="store_true", help="time every batch without and with user-defined cost terms, "
                    "then mjmpc_cost_terms_batch alone (DESIGN 10.8)")
    args = ap.parse_args()
    if args.cost_terms:
        from mjmpc_amd import _lib
        _lib.require_gpu()
        return main_cost_terms(args)
    if args.engine == "arm" and args.model_shards:
        raise SystemExit("--model-shards needs --engine tree (an arm batch rolls out one model block)")
    from mjmpc_amd import _lib
    _lib.require_gpu()          # (no GPU: no numbers)
    ms = models()
    rows, splits = [], []
    for name in args.models.split(","):
        fn, lam, cov = ms[name]
        raw = fn()
        for H in [int(x) for x in args.H.split(",")]:
            for P in [int(x) for x in args.P.split(",")]:
                if args.repeats <= 1:
                    single = time_single(raw, P, H, lam, cov, args.steps, args.warmup, args.model_shards, args.controller,
                                         args.engine)
                for E in [int(x) for x in args.E.split(",")]:
                    spread = None
                    if args.repeats > 1:        # batch, single, batch, single, ...: medians, and the single path's own spread
                        bs, ss = [], []
                        for _ in range(args.repeats):
                            bs.append(time_batch(raw, E, P, H, lam, cov, args.steps, args.warmup, args.model_shards, args.controller,
                                                 args.engine))
                            ss.append(time_single(raw, P, H, lam, cov, args.steps, args.warmup, args.model_shards, args.controller,
                                                  args.engine))
                        batch, single, spread = sorted(bs)[len(bs) // 2], sorted(ss)[len(ss) // 2], max(ss) - min(ss)
                    else:
                        batch = time_batch(raw, E, P, H, lam, cov, args.steps, args.warmup, args.model_shards, args.controller,
                                           args.engine)
                    row = dict(model=name, controller=args.controller, engine=args.engine, E=E, P=P, H=H,
                               model_shards=args.model_shards,
                               batch_ms_per_step=round(batch, 4),
                               batch_episode_steps_per_s=round(1e3 * E / batch, 1), single_ms_per_step=round(single, 4),
                               sequential_ms_per_step=round(E * single, 4), speedup=round(E * single / batch, 2))
                    if spread is not None:
                        row.update(repeats=args.repeats, single_spread_ms=round(spread, 4))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    if args.controller in LAUNCHES and not args.model_shards:
                        split = launch_split(raw, E, P, H, lam, cov, args.steps, args.warmup, args.controller, args.engine)
                        splits.append((name, E, P, H, split))
                        print(json.dumps(dict(model=name, controller=args.controller, E=E, P=P, H=H,
                                              launch_ms={k: round(v, 4) for k, v in split.items()})), flush=True)
    print("%-13s %3s %5s %3s %10s %10s %12s %8s" % ("model", "E", "P", "H", "batch ms", "single ms", "E x single", "speedup"))
    for r in rows:
        print("%-13s %3d %5d %3d %10.3f %10.3f %12.3f %8.2f" % (r["model"], r["E"], r["P"], r["H"], r["batch_ms_per_step"],
                                                             r["single_ms_per_step"], r["sequential_ms_per_step"], r["speedup"]))
    if any("single_spread_ms" in r for r in rows):
        print("single path, max - min over its repeats (ms): "
              + ", ".join("%d x %d: %.3f" % (r["E"], r["P"], r["single_spread_ms"]) for r in rows))
    if splits:
        names = launch_names(args.controller, args.engine)
        short = [n.replace("mjmpc_", "").replace("_batch", "") for n in names]
        print("per-launch split of one batched step (ms, device events around each library call)")
        print("%-13s %3s %5s %3s " % ("model", "E", "P", "H") + " ".join("%18s" % n for n in short))
        for name, E, P, H, split in splits:
            print("%-13s %3d %5d %3d " % (name, E, P, H) + " ".join("%18.4f" % split[n] for n in names))


if __name__ == "__main__":
    main()
