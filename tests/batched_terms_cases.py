"""What tests/test_batched_terms_gpu.py shares: the models with their start states, the tables (one for the
batch or one per episode), the single-episode reference with terms on its own engine, the raw calls of the six cost-term
entry points (tests/test_tracking_gpu.py and tests/test_rate_terms_gpu.py use them too) and the reference batch whose two
engine launches are rebuilt from ``mjmpc_cost_terms`` per episode and a numpy cost-to-go."""
import ctypes

import numpy as np

import batched_cases as bc
from batched_cases import FILT, _torch, _vp

_REACHER = []


def reacher_states(E):
    """``Reacher7DOFEnv``'s seeded resets with their own targets, made once."""
    if len(_REACHER) < E:
        from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
        env = Reacher7DOFEnv()
        for i in range(len(_REACHER), E):
            env.reset(seed=123 + i * 12345)
            st = env.get_env_state()
            _REACHER.append(dict(qp=st["qp"].copy(), qv=st["qv"].copy(), target_pos=st["target_pos"].copy()))
        env.engine.close()
    return [dict(qp=s["qp"].copy(), qv=s["qv"].copy(), target_pos=s["target_pos"].copy()) for s in _REACHER[:E]]


def model(name, E):
    """-> (raw model, E start states, engine kind) of 'cheetah', 'cartpole' (tree) or 'reacher' (arm)."""
    if name == "cheetah":
        return bc.cheetah(), bc._cheetah_states(E), "tree"
    if name == "cartpole":
        raw, states = bc.synthetic_states("cartpole", E)
        return raw, states, "tree"
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    return reacher7dof_raw(), reacher_states(E), "arm"


def engine(raw, kind, dtype, **kw):
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    return (ArmRolloutEngine if kind == "arm" else TreeRolloutEngine)(raw, dtype=dtype, **kw)


# ---------------------------------------------------------------------------------------------------------- the tables
def reach_terms(eng, e=None):
    """cost_terms_cases.mixed_terms (ABS, SQUARE on an action, NORM, COS, one terminal row) for a reach-task engine; ``e``:
    episode e's weights and targets (e = 0 or None: mixed_terms itself)."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    w, g = 1.0 + 0.25 * (e or 0), 0.05 * (e or 0)
    t = CostTerms(eng)
    t.abs(obs="site_minus_target", index=0, weight=0.7 * w, target=g)
    t.square(action=0, weight=0.05 * w)
    t.norm(obs="site_minus_target", weight=4.0 / w, target=[g, -g, 0.5 * g])
    t.cos(obs="qpos", index=0, weight=0.3, target=0.2 + g)
    t.square(obs="qvel", index=0, weight=0.5 * w, terminal=True)
    return t


def forward_terms(eng, e=None):
    """``keep_builtin`` and four rows over a forward-task engine (HalfCheetah): a speed goal, the torso's pitch, control effort
    and a terminal row; ``e``: episode e's weights and targets."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    w, g = 1.0 + 0.25 * (e or 0), 0.1 * (e or 0)
    t = CostTerms(eng, keep_builtin=True)
    t.square(obs="qvel", index=0, weight=0.1 * w, target=1.0 + g)
    t.abs(obs="qpos", index=1, weight=0.5, target=g)
    t.square(action=0, weight=0.01 * w)
    t.square(obs="qvel", index=2, weight=0.2, terminal=True)
    return t


def terms_for(name, eng, E, per_episode):
    make = forward_terms if name == "cheetah" else reach_terms
    return [make(eng, e) for e in range(E)] if per_episode else make(eng)


# ---------------------------------------------------------------------------------------------------------- the single episode
def single(case, raw, state, seed, P, H, T, hyper, dtype, make_terms, gamma=None, cov_type=None):
    """``batched_cases.single`` with ``engine.set_cost_terms(make_terms(engine))`` before ``make_device_rollout_fn``: one
    episode on the single-episode device path over an engine of its own with terms."""
    torch = _torch()
    from mjmpc_amd import control
    from mjmpc_amd.control.controller import resident_state
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, dtype=dtype)
    eng.set_env_state(dict(state))
    eng.set_cost_terms(make_terms(eng))
    kw = dict(zip(case.hyper, hyper), **case.single_kw(dtype))
    if cov_type is not None:
        kw["cov_type"] = cov_type
    c = getattr(control, case.single)(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H,
                                      base_action="null", num_particles=P, gamma=case.gamma if gamma is None else gamma,
                                      n_iters=1, action_lows=eng.action_lows, action_highs=eng.action_highs,
                                      filter_coeffs=FILT, seed=seed, noise_mode="device", **kw)
    c.rollout_fn = make_device_rollout_fn(eng)
    if case.resident:
        c.set_sim_state_fn = resident_state
        c.set_post_step(eng.step_state)
    else:
        c.set_sim_state_fn = lambda s: None
        c.enable_graph(post_step=eng.step_state)
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize({"resident": True}, hotstart=True) if case.resident else c.optimize(None)
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), mean=bc._host(c.mean_action),
               state=eng.get_state_device())
    assert eng.env_resets() == 0, "the single path's real env reset"
    eng.close()
    return out


def assert_same_runs(got, want, what=""):
    """Two batch results (``batched_cases.run_batch``), bit for bit."""
    for k in ("acts", "costs", "nobs", "mean"):
        assert np.array_equal(got[k], want[k]), "%s %s differ (max %.3g)" % (what, k, np.abs(got[k] - want[k]).max())
    assert (got["extra"] is None) == (want["extra"] is None)
    assert got["extra"] is None or np.array_equal(got["extra"], want["extra"]), what
    for a, b in zip(got["state"], want["state"]):
        for x, y in zip(bc._qpos_qvel(a), bc._qpos_qvel(b)):
            assert np.array_equal(x, y), what


# ---------------------------------------------------------------------------------------------------------- the entry points
def tdtype(f32):
    torch = _torch()
    return torch.float32 if f32 else torch.float64


def stream():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cost_terms(tables, nobs, act, costs, keep, terminal, f32):
    """``mjmpc_cost_terms`` on device tensors ([P][H][..]), in place in ``costs``; ``tables``: [K][8] on the device."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    Pn, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms(_lib.F32 if f32 else _lib.F64, Pn, Hn, d_obs, 0 if act is None else act.shape[2], _vp(nobs),
                                    _vp(act), _vp(tables), tables.shape[0], int(keep), int(terminal), _vp(costs), stream()))


def cost_terms_batch(tables, E, nobs, act, costs, keep, terminal, f32, gseq=None, q0=None, A=None):
    """``mjmpc_cost_terms_batch`` on device tensors ([E P][H][..]), in place in ``costs``; ``tables``: [1 or E][K][8]."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    N, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_batch(_lib.F32 if f32 else _lib.F64, E, N // E, Hn, d_obs,
                                          (0 if act is None else act.shape[2]) if A is None else A, _vp(nobs), _vp(act),
                                          _vp(tables), tables.shape[1], int(tables.shape[0] > 1), int(keep), int(terminal),
                                          _vp(costs), _vp(gseq), _vp(q0), stream()))


def cost_terms_track(d_tab, d_ref, periodic, counter, bias, advance, nobs, act, costs, keep, terminal, f32):
    """``mjmpc_cost_terms_track`` on device tensors ([P][H][..]), in place in ``costs``."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    Pn, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_track(_lib.F32 if f32 else _lib.F64, Pn, Hn, d_obs, 0 if act is None else act.shape[2],
                                          _vp(nobs), _vp(act), _vp(d_tab), d_tab.shape[0], int(keep), int(terminal), _vp(d_ref),
                                          d_ref.shape[0], d_ref.shape[1], int(periodic), _vp(counter), int(bias), int(advance),
                                          _vp(costs), stream()))


def cost_terms_track_batch(d_tabs, d_refs, periodic, counter, bias, E, nobs, act, costs, keep, terminal, f32, gseq=None, q0=None,
                           A=None):
    """``mjmpc_cost_terms_track_batch`` on device tensors ([E P][H][..]); ``d_tabs``: [1 or E][K][8], ``d_refs``: [1 or E][N][R]."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    N, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_track_batch(
        _lib.F32 if f32 else _lib.F64, E, N // E, Hn, d_obs, (0 if act is None else act.shape[2]) if A is None else A, _vp(nobs),
        _vp(act), _vp(d_tabs), d_tabs.shape[1], int(d_tabs.shape[0] > 1), int(keep), int(terminal), _vp(d_refs), d_refs.shape[1],
        d_refs.shape[2], int(d_refs.shape[0] > 1), int(periodic), _vp(counter), int(bias), _vp(costs), _vp(gseq), _vp(q0),
        stream()))


def cost_terms_rate(d_tab, d_ref, periodic, counter, bias, advance, prev, nobs, act, costs, keep, terminal, f32):
    """``mjmpc_cost_terms_rate`` on device tensors ([P][H][..]), in place in ``costs``; ``d_ref`` / ``counter`` / ``prev`` may
    be ``None``."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    Pn, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_rate(
        _lib.F32 if f32 else _lib.F64, Pn, Hn, d_obs, act.shape[2], _vp(nobs), _vp(act), _vp(d_tab), d_tab.shape[0], int(keep),
        int(terminal), _vp(d_ref), 0 if d_ref is None else d_ref.shape[0], 0 if d_ref is None else d_ref.shape[1], int(periodic),
        _vp(counter), int(bias), int(advance), _vp(prev), _vp(costs), stream()))


def cost_terms_rate_batch(d_tabs, d_refs, periodic, counter, bias, E, prevs, advance_prev, nobs, act, costs, keep, terminal, f32,
                          gseq=None, q0=None):
    """``mjmpc_cost_terms_rate_batch`` on device tensors ([E P][H][..]); ``d_tabs``: [1 or E][K][8], ``d_refs``: [1 or E][N][R] or
    ``None``, ``prevs``: [E][A] or ``None``."""
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    N, Hn, d_obs = nobs.shape
    _lib.check(lib.mjmpc_cost_terms_rate_batch(
        _lib.F32 if f32 else _lib.F64, E, N // E, Hn, d_obs, act.shape[2], _vp(nobs), _vp(act), _vp(d_tabs), d_tabs.shape[1],
        int(d_tabs.shape[0] > 1), int(keep), int(terminal), _vp(d_refs), 0 if d_refs is None else d_refs.shape[1],
        0 if d_refs is None else d_refs.shape[2], int(d_refs is not None and d_refs.shape[0] > 1), int(periodic), _vp(counter),
        int(bias), _vp(prevs), int(advance_prev), _vp(costs), _vp(gseq), _vp(q0), stream()))


def numpy_q0(costs, gseq):
    """The forward loop ``q = q + g[t] * c[t]`` in float64 over stored costs [N][H]; +inf where it is not finite."""
    c = np.asarray(costs).astype(np.float64)
    q = np.zeros(c.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(c.shape[1]):
            q = q + gseq[t] * c[:, t]
    return np.where(np.isfinite(q), q, np.inf)


# ---------------------------------------------------------------------------------------------------------- the reference batch
def as_separate_launches(b):
    """Replace the batch's two engine launches by their restatement from the parts: ``_rollout`` by the ``_obs`` rollout entry
    without a cost-to-go, ``mjmpc_cost_terms`` per episode with that episode's table and the cost-to-go from numpy;
    ``_env_step`` by ``step_shard_states`` and ``mjmpc_cost_terms`` per episode.  The sampler and the update launches stay
    the batch's own.  (Synchronises every step: a reference, not a fast path.)"""
    torch = _torch()
    from mjmpc_amd import _lib
    tables, K, per_episode, keep, reads = b._terms
    E, P, H = b.num_episodes, b.num_particles, b.horizon
    f32 = b.dtype == "f32"
    gseq_h = b._gseq.cpu().numpy()

    def table(e):
        return tables[e if per_episode else 0]

    def rollout(s, noise=None, filtered=True, gseq=True, q0=True):
        nobs = torch.empty((E * P, H, b.d_obs), dtype=b._tdtype, device=b.device)
        _lib.check(b._fn("rollout_fused_batch_obs")(
            b.engine._h, b._code, E * P, H, _vp(b._means), _vp(b._noise if noise is None else noise),
            _vp(b._coeffs) if filtered else None, None, _vp(b._costs), _vp(b._actions), None, _vp(nobs), s))
        for e in range(E):
            rows = slice(e * P, (e + 1) * P)
            cost_terms(table(e), nobs[rows], b._actions[rows] if reads else None, b._costs[rows], keep, 1, f32)
        if q0:
            torch.cuda.synchronize()
            b._q0.copy_(torch.from_numpy(numpy_q0(b._costs.cpu().numpy(), gseq_h)))

    def env_step(act, cost, nobs, s):
        _lib.check(b._fn("step_shard_states")(b.engine._h, b._code, _vp(act), _vp(cost), _vp(nobs), s))
        act_t = act.to(b._tdtype).contiguous()
        for e in range(E):
            cost_terms(table(e), nobs[e:e + 1].view(1, 1, -1), act_t[e:e + 1].view(1, 1, -1) if reads else None,
                       cost[e:e + 1].view(1, 1), keep, 0, f32)
    b._rollout = rollout
    b._env_step = env_step
    return b
