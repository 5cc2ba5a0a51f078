#!/usr/bin/env python
"""The config's ``n_episodes`` MPPI, CEM, PFMPC, DMD-MPC, random-shooting or MPPIQ episodes as ONE batch on the tree engine
(``BatchedMPPI`` / ``BatchedCEM`` / ``BatchedPFMPC`` / ``BatchedDMDMPC`` / ``BatchedRandomShooting`` / ``BatchedMPPIQ``).

    python examples/example_mpc_batched.py --config examples/configs/half_cheetah_gpu.yml
        [--controller mppi|cem|pfmpc|dmd|random_shooting|mppiq]
        [--dtype f64|f32] [--episodes N] [--dyn_randomize_config FILE [--num_cpu K] [--dyn_per_episode]]
        [--update_cov] [--cov_type diagonal|full] [--engine tree|arm]

examples/example_mpc.py runs the episodes one after another (as the reference's job_script.py:80-99): episode i with seed
``seed + i*12345`` from the env class's ``reset(seed=...)``.  This driver takes the same seeds and start states and runs all
episodes side by side - one sampling launch, one rollout launch, one update launch and one env-step launch per control
step of the whole batch.  Each episode computes exactly what the single-episode device path (``noise_mode='device'``,
``--graph``) computes for it on the tree engine.

``--dyn_randomize_config`` (the reference's example_mpc.py option; examples/configs/*_dyn_randomize.yml): every episode's
particles are split into the config's ``num_cpu`` shards and each shard rolls out its own randomized model, drawn once for
all episodes from the config's ``seed`` as the reference does before its episode loop (``--dyn_per_episode``: from every
episode's own seed), while the real envs keep the nominal model - still one batch.

The ``mppi``, ``cem``, ``pfmpc``, ``dmd``, ``random_shooting`` and ``mppiq`` blocks run here (``--controller cem``: ``BatchedCEM``, DESIGN 10.2 - the rollout, selection +
moments, refit + next samples and env-step launches per control step; ``--controller pfmpc``: ``BatchedPFMPC``, DESIGN 10.3 -
deviations, rollout, weights, resampling, gather + shift, mean + action and env step, e.g. examples/configs/reacher_gpu.yml;
``--controller dmd``: with ``update_cov: true`` ``BatchedDMDMPC``, DESIGN 10.4 - factors, draw, filter, rollout, weights, partial
moments, update + tail and env step -, with ``update_cov: false`` ``BatchedMPPI`` with the block's ``lam``, ``step_size`` and
``init_cov``, which is that arithmetic; the class that ran is printed; ``--controller random_shooting``:
``BatchedRandomShooting``, DESIGN 10.5 - draw, rollout, selection + blend + tail and env step; ``--controller mppiq``:
``BatchedMPPIQ``, DESIGN 10.6 - draw, filter, rollout, returns + weights, partial moments, update + tail and env step, with the
block's ``alpha`` and ``time_based_weights``); other controller blocks are refused.  The reacher configs run on the TREE engine here
(sawyer.xml compiled as a tree), while example_mpc.py steps them on the serial-chain arm engine: the two drivers' reacher
rewards are not expected to be equal.

A config's ``cost_terms`` block (examples/configs/cartpole_terms_batch_gpu.yml) replaces the built-in cost
of the plans and the real envs, as in example_mpc.py; a term's ``weight`` or ``target`` that lists ``n_episodes`` values gives
every episode its own table - a goal per episode, or a sweep of a weight over the batch.

``--engine arm`` runs the reacher configs' batch on the arm engine instead (``engine="arm"``: the arm kernels'
episode-batch launches, ``num_particles`` a multiple of 8, start states from the env class on the arm engine); the other
environments and ``--dyn_randomize_config`` need the default, ``--engine tree``.
"""
import argparse
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from example_mpc import ENVS, TREE_MODELS                           # noqa: E402
from mjmpc_amd.control import (BatchedCEM, BatchedDMDMPC, BatchedMPPI, BatchedMPPIQ, BatchedPFMPC,  # noqa: E402
                               BatchedRandomShooting)
from mjmpc_amd.envs.cost_terms import cost_terms_from_config        # noqa: E402
from mjmpc_amd.envs.tree_engine import TreeRolloutEngine            # noqa: E402
from mjmpc_amd.models.reacher7dof import reacher7dof_raw            # noqa: E402


# controller block -> the batch class, the block's settings it takes between num_particles and gamma, and the optional ones
# with the values they take where the block has none
BATCHES = {
    "mppi": (BatchedMPPI, ("lam", "step_size", "init_cov"), dict(alpha=1, time_based_weights=False)),
    "cem": (BatchedCEM, ("init_cov", "elite_frac", "step_size", "beta"), dict(cov_type="diagonal", sample_mode="mean")),
    "pfmpc": (BatchedPFMPC, ("cov_shift", "cov_resample", "lam"), dict(sample_mode="mean")),
    "dmd": (BatchedDMDMPC, ("lam", "step_size", "init_cov", "beta"), dict(cov_type="diagonal", sample_mode="mean")),
    "dmd_static": (BatchedMPPI, ("lam", "step_size", "init_cov"), dict()),
    "random_shooting": (BatchedRandomShooting, ("step_size", "init_cov"), dict(sample_mode="mean")),
    "mppiq": (BatchedMPPIQ, ("beta", "step_size", "init_cov", "td_lam"), dict(alpha=1, time_based_weights=True)),
}


def main():
    ap = argparse.ArgumentParser(description="Run a config's MPPI, CEM, PFMPC, DMD-MPC, random-shooting or MPPIQ episodes as one batch")
    ap.add_argument("--config", required=True, help="yaml file with experiment parameters")
    ap.add_argument("--controller", default="mppi", choices=["mppi", "cem", "pfmpc", "dmd", "random_shooting", "mppiq"],
                    help="controller block of the config to run")
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--episodes", type=int, help="override n_episodes")
    ap.add_argument("--dyn_randomize_config", help="yaml file with dynamics randomization parameters")
    ap.add_argument("--num_cpu", type=int, help="override the config's num_cpu (the model shards of --dyn_randomize_config)")
    ap.add_argument("--dyn_per_episode", action="store_true", help="a set of randomized models per episode (from its seed)")
    ap.add_argument("--update_cov", action="store_true", help="--controller dmd: adapt the covariance whatever the block says")
    ap.add_argument("--cov_type", choices=["diagonal", "full"], help="--controller dmd / cem: override the block's cov_type")
    ap.add_argument("--engine", default="tree", choices=["tree", "arm"], help="the engine the batch runs on (arm: the reacher configs)")
    args = ap.parse_args()
    with open(args.config) as f:
        exp = yaml.safe_load(f)
    if exp["env_name"] not in ENVS:
        raise SystemExit("environment %r is not built (have: %s)" % (exp["env_name"], ", ".join(ENVS)))
    if not isinstance(exp.get(args.controller), dict):
        raise SystemExit("the config has no %r controller block" % args.controller)
    if args.engine == "arm" and (exp["env_name"] in TREE_MODELS or args.dyn_randomize_config):
        raise SystemExit("--engine arm runs the reacher configs without dynamics randomization; use --engine tree")
    params = dict(exp[args.controller])
    num_cpu = args.num_cpu or params.pop("num_cpu", 1)
    params.pop("num_cpu", None)
    if args.update_cov:
        params["update_cov"] = True
    if args.cov_type:
        params["cov_type"] = args.cov_type
    if "particles_per_cpu" in params:
        params["num_particles"] = num_cpu * params.pop("particles_per_cpu")
    E = args.episodes or exp["n_episodes"]
    T = exp["max_ep_length"]
    seeds = [exp["seed"] + i * 12345 for i in range(E)]            # consistent episodes, as in the reference
    raw = TREE_MODELS[exp["env_name"]]() if exp["env_name"] in TREE_MODELS else reacher7dof_raw()

    # the start states: the env class's reset(seed) per episode (the reacher's env class on the tree engine)
    env_cls = ENVS[exp["env_name"]]
    if exp["env_name"] in TREE_MODELS or args.engine == "arm":
        env = env_cls(dtype=args.dtype)
    else:
        env = env_cls(engine=TreeRolloutEngine(raw, dtype=args.dtype))
    states = []
    for s in seeds:
        env.reset(seed=s)
        states.append(env.get_env_state())
    env.engine.close()

    base_action = params.get("base_action", exp.get("base_action", "null"))
    # (without covariance adaptation DMD-MPC is MPPI with alpha = 1, gaussian_dmd.py:65-104, and its static covariance is
    # diag(init_cov) for any cov_type)
    name = "dmd_static" if args.controller == "dmd" and not params.get("update_cov", False) else args.controller
    cls, names, optional = BATCHES[name]
    params.setdefault("beta", 0.0)
    batch = cls(raw, E, params["horizon"], params["num_particles"], *[params[n] for n in names], params["gamma"],
                params["filter_coeffs"], base_action, seeds, dtype=args.dtype, n_iters=params.get("n_iters", 1), engine=args.engine,
                **{k: params.get(k, default) for k, default in optional.items()})
    if args.controller == "dmd":
        print("the dmd block (update_cov: %s) runs as %s" % (bool(params.get("update_cov", False)), type(batch).__name__))
    if args.dyn_randomize_config:
        with open(args.dyn_randomize_config) as f:
            default_params, randomized = batch.randomize_dynamics(yaml.safe_load(f), seeds if args.dyn_per_episode else exp["seed"],
                                                                  num_shards=num_cpu)
        print("default params   :", default_params[0][0] if args.dyn_per_episode else default_params[0])
        print("randomized params:", randomized)
    if exp.get("cost_terms"):
        # user-defined cost terms: the plans and the real envs of every episode are costed by the config's table; a weight or
        # target that lists n_episodes values gives every episode its own
        terms = cost_terms_from_config(exp["cost_terms"], batch.engine, num_episodes=E)
        batch.set_cost_terms(terms)
        print("cost terms: %s" % ("one table per episode" if isinstance(terms, list) else "one table for every episode"))
    batch.set_states(states)
    batch.run(1)                        # warm-up step (code objects, allocations), then back to the start
    batch.reset()
    batch.set_states(states)
    t0 = time.perf_counter()
    actions, costs, nobs = batch.run(T)     # (ends in a device-to-host copy: the clock covers the work)
    dt = time.perf_counter() - t0
    final = batch.get_states()
    batch.close()

    rewards = -costs.astype(np.float64).sum(axis=0)
    for i in range(E):
        if exp["env_name"] in ("Swimmer-v0", "HalfCheetah-v0", "HalfCheetah_state-v0"):
            print("episode %d: reward %.3f, forward progress %.3f m" % (i, rewards[i], final[i]["qpos"][0]))
        else:
            print("episode %d: reward %.3f, final distance to target %.4f"
                  % (i, rewards[i], np.linalg.norm(nobs[-1, i, -3:])))
    print("Avg. reward = %.4f, Std. Reward = %.4f" % (rewards.mean(), rewards.std()))
    print("%s batch on the %s engine: %d episodes x %d particles x H%d%s, %.3f ms per batched control step (%.0f episode-steps/s)"
          % (args.controller, args.engine, E, params["num_particles"], params["horizon"],
             ", %d randomized model shards" % num_cpu if args.dyn_randomize_config else "", 1e3 * dt / T, E * T / dt))


if __name__ == "__main__":
    main()
