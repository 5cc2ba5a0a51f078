"""What the tests of the episode batches share (tests/test_batched_*.py).

GPU side: the start states, the single-episode reference run, the batch run and the comparison of the two.  A controller is
described by a ``case``: its two classes, its per-episode hyperparameters in the order the batch constructor takes them (the
single controller takes them by the same names), the wiring of its single path, the assertion that this path took the
intended branch, and the extra array it compares.  The single-episode reference is the device path of a fresh
``TreeRolloutEngine`` per episode: the controller with ``noise_mode='device', seed=seed_e``, ``make_device_rollout_fn(engine)``
and the engine's device-resident real env behind every step.  Every comparison is ``np.array_equal``.

CPU side: the ``no_engine`` fixture, the settings every batch refuses, and the checks every batch's file makes of its export,
its entry points and its broadcasting.
"""
import ctypes
import dataclasses
import os
import re
import types

import numpy as np
import pytest

FILT = [0.25, 0.8, 0.0]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _per(v, e):
    return v[e] if np.ndim(v) > 0 else v


def _qpos_qvel(st):
    return (st["qpos"], st["qvel"]) if "qpos" in st else (st["qp"], st["qv"])


def _host(x):
    return x.cpu().numpy().copy() if hasattr(x, "cpu") else np.array(x)


# ---------------------------------------------------------------------------------------------------------- start states
_CHEETAH = []


def _cheetah_states(E, copy=False):
    """Start states of the env class's seeded resets (state i does not depend on E), made once and shared, read-only;
    ``copy=True``: copies the caller may edit."""
    if len(_CHEETAH) < E:
        from mjmpc_amd.envs.locomotion_env import HalfCheetahEnv
        env = HalfCheetahEnv()
        for i in range(len(_CHEETAH), E):
            env.reset(seed=123 + i * 12345)
            _CHEETAH.append(env.get_env_state())
        env.engine.close()
    if copy:
        return [dict(qpos=s["qpos"].copy(), qvel=s["qvel"].copy()) for s in _CHEETAH[:E]]
    return _CHEETAH[:E]


def cheetah():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    return half_cheetah_raw()


def synthetic_states(name, E, seed=0):
    """The env class's start state with a small per-episode velocity offset (the synthetic envs start from one state)."""
    from mjmpc_amd.envs.synthetic_env import start_state
    from mjmpc_amd.models.synthetic import synthetic_raw
    raw = synthetic_raw(name)
    st = start_state(name, raw)
    rng = np.random.RandomState(seed)
    return raw, [dict(qp=st["qp"].copy(), qv=st["qv"] + 0.05 * rng.randn(st["qv"].size), target_pos=st["target_pos"].copy())
                 for _ in range(E)]


# ---------------------------------------------------------------------------------------------------------- the descriptions
def case(batch, single, hyper, single_kw, gamma=1.0, resident=False, before=None, during=None, extra=None, guards=True,
         solver=False):
    """``batch`` / ``single``: the class names in ``mjmpc_amd.control``; ``hyper``: the per-episode settings, in the batch
    constructor's order between ``num_particles`` and ``gamma``; ``single_kw(dtype)``: the single controller's other keywords;
    ``gamma``: the discount where a test gives none; ``resident``: the single path keeps its real env resident
    (``resident_state`` + ``set_post_step``, ``optimize({"resident": True}, hotstart=True)``) instead of replaying a graph
    (``enable_graph(post_step=...)``, ``optimize(None)``); ``before(c)`` / ``during(c)``: assert that the single path takes the
    intended branch, before the loop / after every step; ``extra``: the attribute names (single, batch) of a further array
    to compare; ``guards``: no real env may reset on either side and the single run is finite; ``solver``: no solver may
    fail on either side."""
    return types.SimpleNamespace(batch=batch, single=single, hyper=hyper, single_kw=single_kw, gamma=gamma, resident=resident,
                                 before=before, during=during, extra=extra, guards=guards, solver=solver)


# ---------------------------------------------------------------------------------------------------------- the two runs
_SINGLES = {}


def single(case, raw, state, seed, P, H, T, hyper, dtype, gamma=None, base_action="null", init_mean=None, cov_type=None, K=1,
           cfg=None, dyn_seed=None, key=None):
    """One episode on the single-episode device path -> dict(acts [T][A], costs [T], nobs [T][d_obs], mean, extra, state,
    blobs: the engine's shard blocks).  ``hyper``: this episode's values.  ``key``: names the model and the start state;
    runs with a key are kept and shared, read-only."""
    gamma = case.gamma if gamma is None else gamma
    full_key = None if key is None else (case.single, key, seed, P, H, T, tuple(float(v) for v in hyper), dtype, gamma,
                                         base_action, init_mean is None, cov_type, K, repr(cfg), dyn_seed)
    if full_key in _SINGLES:
        return _SINGLES[full_key]
    torch = _torch()
    from mjmpc_amd import control
    from mjmpc_amd.control.controller import resident_state
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, dtype=dtype, num_shards=K)
    if cfg is not None:
        eng.randomize_dynamics(cfg, dyn_seed)
        eng.set_real_env_model("nominal")
    eng.set_env_state(dict(state))
    kw = dict(zip(case.hyper, hyper), **case.single_kw(dtype))
    if cov_type is not None:
        kw["cov_type"] = cov_type
    c = getattr(control, case.single)(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H,
                                      base_action=base_action, num_particles=P, gamma=gamma, n_iters=1,
                                      action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed,
                                      noise_mode="device", **kw)
    c.rollout_fn = make_device_rollout_fn(eng)
    if case.resident:
        c.set_sim_state_fn = resident_state
        c.set_post_step(eng.step_state)
    else:
        c.set_sim_state_fn = lambda s: None
        if init_mean is not None:
            c.mean_action = np.array(init_mean, np.float64)
        c.enable_graph(post_step=eng.step_state)
    if case.before is not None:
        case.before(c)
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize({"resident": True}, hotstart=True) if case.resident else c.optimize(None)
        torch.cuda.synchronize()
        if case.during is not None:
            case.during(c)
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), mean=_host(c.mean_action),
               extra=None if case.extra is None else _host(getattr(c, case.extra[0])), state=eng.get_state_device(),
               blobs=getattr(eng, "shard_blobs", None))
    if case.guards:
        assert eng.env_resets() == 0, "the single path's real env reset"
    if case.solver:
        assert eng.solver_failures() == 0
    eng.close()
    if full_key is not None:
        _SINGLES[full_key] = out
    return out


def make_batch(case, raw, states, seeds, P, H, hyper, dtype, gamma=None, base_action="null", K=1, cfg=None, dyn_seed=None, **kw):
    """The batch on ``states``; ``hyper``: one value for every episode or one per episode, each; ``kw``: the batch class's own
    keywords (``cov_type``, ``init_mean``)."""
    from mjmpc_amd import control
    kw = {k: v for k, v in kw.items() if v is not None}
    b = getattr(control, case.batch)(raw, len(states), H, P, *hyper, case.gamma if gamma is None else gamma, FILT, base_action,
                                     seeds, dtype=dtype, **kw)
    b.set_states([dict(s) for s in states])
    if cfg is not None:
        b.randomize_dynamics(cfg, dyn_seed, K)
    return b


def run_batch(case, b, T):
    """``T`` steps of a fresh batch, then closed -> dict(acts [T][E][A], costs [T][E], nobs [T][E][d_obs], mean [E], extra [E],
    state: E state dicts)."""
    acts, costs, nobs = b.run(T)
    out = dict(acts=acts, costs=costs, nobs=nobs, mean=b.mean_action,
               extra=None if case.extra is None else getattr(b, case.extra[1]), state=b.get_states())
    assert b.num_steps == T
    if case.guards:
        assert b.engine.env_resets() == 0, "a real env of the batch reset"
    if case.solver:
        assert b.engine.solver_failures() == 0
    b.close()
    return out


def batch(case, raw, states, seeds, P, H, T, hyper, dtype, **kw):
    return run_batch(case, make_batch(case, raw, states, seeds, P, H, hyper, dtype, **kw), T)


# ---------------------------------------------------------------------------------------------------------- the comparisons
def check_against_singles(case, raw, states, seeds, P, H, T, hyper, dtype, keys=None, out=None, **kw):
    """Episode e of the batch against the single run of state e, seed e and the e-th hyperparameters (``init_mean`` and a list
    ``dyn_seed`` are per episode too).  ``out``: a batch result made elsewhere.  Returns it with the single runs under
    ``'singles'``."""
    E = len(states)
    out = batch(case, raw, states, seeds, P, H, T, hyper, dtype, **kw) if out is None else out
    acts, costs = out["acts"], out["costs"]
    assert acts.shape[:2] == (T, E) and costs.shape == (T, E) and out["mean"].shape[0] == E and len(out["state"]) == E
    assert case.extra is None or out["extra"].shape[0] == E
    assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs))
    out["singles"] = []
    for e in range(E):
        skw = dict(kw)
        if isinstance(skw.get("dyn_seed"), (list, tuple)):
            skw["dyn_seed"] = skw["dyn_seed"][e]
        if np.ndim(skw.get("init_mean")) == 3:
            skw["init_mean"] = skw["init_mean"][e]
        one = single(case, raw, states[e], seeds[e], P, H, T, [_per(v, e) for v in hyper], dtype,
                     key=None if keys is None else keys[e], **skw)
        out["singles"].append(one)
        if case.guards:
            assert np.all(np.isfinite(one["acts"])) and np.all(np.isfinite(one["costs"]))
        assert np.array_equal(acts[:, e], one["acts"]), \
            "episode %d: actions differ (max %.3g)" % (e, np.abs(acts[:, e] - one["acts"]).max())
        assert np.array_equal(costs[:, e], one["costs"]), "episode %d: real-env costs differ" % e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), "episode %d: next observations differ" % e
        assert np.array_equal(out["mean"][e], one["mean"]), "episode %d: final mean differs" % e
        if case.extra is not None:
            assert np.array_equal(out["extra"][e], one["extra"]), \
                "episode %d: final %s differs (max %.3g)" % (e, case.extra[1], np.abs(out["extra"][e] - one["extra"]).max())
        for x, y in zip(_qpos_qvel(out["state"][e]), _qpos_qvel(one["state"])):
            assert np.array_equal(x, y), "episode %d: final state differs" % e
    return out


def check_permutation(case, raw, states, seeds, P, H, T, hyper, dtype, perm):
    """Permuting the episodes (states, seeds, per-episode ``hyper`` arrays) permutes the results."""
    base = batch(case, raw, states, seeds, P, H, T, hyper, dtype)
    got = batch(case, raw, [states[k] for k in perm], [seeds[k] for k in perm], P, H, T, [v[perm] for v in hyper], dtype)
    for k in ("acts", "costs", "nobs"):
        assert np.array_equal(got[k], base[k][:, perm]), k
    assert np.array_equal(got["mean"], base["mean"][perm])
    assert case.extra is None or np.array_equal(got["extra"], base["extra"][perm])
    for k, e in enumerate(perm):
        for x, y in zip(_qpos_qvel(got["state"][k]), _qpos_qvel(base["state"][e])):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------- the CPU side
@pytest.fixture
def no_engine(monkeypatch):
    """Making an engine fails the test: every refusal must come first."""
    from mjmpc_amd.envs import tree_engine

    def refuse(*a, **k):
        raise AssertionError("an engine was created before the settings were checked")
    monkeypatch.setattr(tree_engine.TreeRolloutEngine, "__init__", refuse)


def rk4_hand():
    """A model the tree engine refuses: RK4 beyond 16 dofs."""
    from mjmpc_amd.models.hand24 import hand24_raw
    return dataclasses.replace(hand24_raw(), integrator="RK4")


# what _check_common refuses of every batch (use_zero_control_seq is no setting of BatchedPFMPC), and what _check_seeds does
COMMON_REFUSED = [
    dict(n_iters=2), dict(sample_mode="sample"), dict(gamma=0.0), dict(base_action="random"), dict(base_action="zeros"),
    dict(dtype="f16"), dict(num_episodes=0), dict(num_episodes=65536), dict(horizon=0), dict(num_particles=0),
    dict(filter_coeffs=[1.0, 0.0]), dict(seeds=[1, 2, 3]), dict(seeds=7), dict(seeds=[1, 2, 3, -4]),
]


def refused_id(by_type=("raw_model",)):
    """The id of an override of the settings: ``name=value``, with the value's type for the settings in ``by_type``."""
    return lambda d: ",".join("%s=%s" % (k, type(v).__name__ if k in by_type else v) for k, v in d.items())


def check_reaches_the_engine(cls, settings):
    """Every one of ``settings`` passes the checks (and then gets as far as making the engine; needs ``no_engine``)."""
    for kw in settings:
        with pytest.raises(AssertionError, match="engine was created"):
            cls(**kw)


def stop_at_setup(monkeypatch):
    """``_EpisodeBatch._setup`` stops the constructor ('far enough') -> the dict that then holds its E, H, P and init_mean."""
    from mjmpc_amd.control import batched
    seen = {}

    def stop(self, raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean):
        seen.update(E=E, H=H, P=P, init_mean=init_mean)
        raise RuntimeError("far enough")
    monkeypatch.setattr(batched._EpisodeBatch, "_setup", stop)
    return seen


def check_stops_at_setup(cls, kw, seen, E, H, P):
    with pytest.raises(RuntimeError, match="far enough"):
        cls(**kw)
    assert (seen["E"], seen["H"], seen["P"]) == (E, H, P)


def check_per_episode(name, one, each):
    """``_per_episode``: one value for every episode, or one per episode -> float64 [E]."""
    from mjmpc_amd.control import batched
    a = batched._per_episode(name, one, len(each))
    assert a.shape == (len(each),) and a.dtype == np.float64 and np.all(a == one)
    assert batched._per_episode(name, each, len(each)).tolist() == list(each)


def check_exported(name, methods, inherited):
    """The class is exported, a subclass of ``_EpisodeBatch``, has ``methods`` and has ``inherited`` from the base class
    unchanged -> the class."""
    import mjmpc_amd.control as control
    from mjmpc_amd.control.batched import _EpisodeBatch
    cls = getattr(control, name)
    assert name in control.__all__
    assert issubclass(cls, _EpisodeBatch)
    for n in methods:
        assert hasattr(cls, n), n
    for n in inherited:
        assert getattr(cls, n) is getattr(_EpisodeBatch, n), n
    return cls


def check_entry_points(symbols, abi=None):
    """Declared in the header, bound in ``_lib.SIGNATURES``, built into the library; ``abi``: the ABI version of all three."""
    from mjmpc_amd import _lib
    with open(os.path.join(ROOT, "include", "mjmpc_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in symbols:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    if abi is not None:                                         # (additions do not move the version)
        assert re.search(r"#define\s+MJMPC_ABI_VERSION\s+%d\b" % abi, header)
        assert _lib.ABI_VERSION == abi and lib.mjmpc_abi_version() == abi
    return header
