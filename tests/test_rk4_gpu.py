"""GPU: MuJoCo's RK4 integrator on the tree engine (tree_rollout_rk4.hip) against the RK4 step composed from the FP64 C
oracle's forward evaluations (tests/rk4_ref.py; the oracle itself steps with Euler).  One env step from random states at
1e-9 on every kind of model the RK4 instantiations run (fluid forces, plane contacts with pyramids, slides with friction
loss, free and ball joints, equalities and tendons, round 5's record kinds, random models), rollouts, every launch mode,
wave-mate independence, MuJoCo's reset on instability, f32 against f64 and a closed loop on the double pendulum."""
import numpy as np
import pytest

import rk4_ref

pytestmark = pytest.mark.gpu

NAMES = ["swimmer", "cheetah", "cartpole", "tray", "fourbar", "gripper:pyramidal", "double_pendulum"]


def _raw(name):
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    from mjmpc_amd.models.swimmer import swimmer_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    base, _, cone = name.partition(":")
    raw = dict(swimmer=swimmer_raw, cheetah=half_cheetah_raw).get(base, lambda: synthetic_raw(base))()
    if cone:
        raw.cone, raw.impratio = cone, 1.0
    raw.integrator = "RK4"
    return raw


def _state(name, raw, rs):
    from mjmpc_amd.models.raw import TASK_FORWARD
    from test_general_models_gpu import random_state
    base = name.partition(":")[0]
    if raw.task == TASK_FORWARD:
        q, v = 0.15 * rs.standard_normal(raw.nv), 0.5 * rs.standard_normal(raw.nv)
        if base == "cheetah":
            q[1] = rs.uniform(-0.12, 0.05)
        return q, v
    if base == "double_pendulum":
        return (np.array([rs.uniform(-1.5, 1.5), rs.uniform(-0.6, 0.6), rs.uniform(-0.6, 0.6)]),
                rs.standard_normal(3) * [0.5, 2.0, 2.0])
    return random_state(base, raw, rs)


def _set(eng, raw, q, v):
    eng.set_env_state(dict(qp=q, qv=v, qpos=q, qvel=v, target_pos=np.asarray(raw.target_pos, float)))


_RIGS = {}


def _rig(name, dtype="f64"):
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    if (name, dtype) not in _RIGS:
        raw = _raw(name)
        _RIGS[name, dtype] = (raw, TreeRolloutEngine(raw, dtype=dtype), RefArm(raw.to_flat()))
    return _RIGS[name, dtype]


def _one_step_worst(raw, eng, ref, states, actions):
    worst = 0.0
    tgt = np.asarray(raw.target_pos, float)
    for (q, v), u in zip(states, actions):
        _set(eng, raw, q, v)
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        q1, v1, r1, o1, _ = rk4_ref.env_step(ref, raw, q, v, u, tgt)
        scale = max(1.0, np.abs(o1).max())
        worst = max(worst, np.abs(nobs[0, 0] - o1).max() / scale, abs(rew[0, 0] - r1) / max(1.0, abs(r1)))
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_one_env_step_matches_composed_rk4(name):
    """32 random states and actions per model: next observation (qpos, qvel, the last stage's site) and reward at 1e-9."""
    raw, eng, ref = _rig(name)
    rs = np.random.RandomState(11)
    span = (eng.action_highs - eng.action_lows) / 2
    states = [_state(name, raw, rs) for _ in range(32)]
    actions = [rs.uniform(-1.2, 1.2, eng.d_action) * span for _ in range(32)]
    worst = _one_step_worst(raw, eng, ref, states, actions)
    print("%s RK4: one env step from 32 random states, worst relative error %.2e" % (name, worst))
    assert worst < 1e-9, worst
    assert eng.solver_failures() == 0


def test_random_models_match_composed_rk4():
    """16 seeds of tests/test_random_models_gpu.py's generator, redrawn until the model has at most 16 dofs and pyramidal
    cones, switched to RK4."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    from test_random_models_gpu import random_model, random_state
    done, k, worst = 0, 0, 0.0
    while done < 16:
        assert k < 400, "too few random models fit the RK4 kernels"
        raw = random_model(k)
        k += 1
        if raw.nv > 16 or raw.cone != "pyramidal":
            continue
        raw.integrator = "RK4"
        try:
            eng = TreeRolloutEngine(raw, dtype="f64")
            ref = RefArm(raw.to_flat())
        except (ValueError, NotImplementedError, AssertionError):
            continue
        rs = np.random.RandomState(k + 77)
        states = [random_state(raw, rs) for _ in range(4)]
        actions = [rs.uniform(-1.5, 1.5, eng.d_action) for _ in range(4)]
        w = _one_step_worst(raw, eng, ref, states, actions)
        assert w < 1e-9, (k - 1, w)
        worst = max(worst, w)
        eng.close()
        done += 1
    print("RK4 random models: 16 models (seeds 0..%d), worst relative error %.2e" % (k - 1, worst))


ROLLOUT_TOL = dict(swimmer=1e-9, cheetah=1e-7, cartpole=1e-9, tray=1e-7, fourbar=1e-8, double_pendulum=1e-9)
ROLLOUT_TOL["gripper:pyramidal"] = 1e-7


@pytest.mark.parametrize("name", NAMES)
def test_rollouts_match_composed_rk4(name):
    """8 particles x 12 env steps of noisy actions from one random state."""
    raw, eng, ref = _rig(name)
    rs = np.random.RandomState(5)
    P, H, A = 8, 12, eng.d_action
    q, v = _state(name, raw, rs)
    span = (eng.action_highs - eng.action_lows) / 2
    mean = 0.2 * rs.standard_normal((H, A)) * span
    eps = 0.4 * rs.standard_normal((P, H, A)) * span
    _set(eng, raw, q, v)
    _, rew, act, _, _, nobs = eng.rollout(P, H, mean, eps, "open_loop")
    tol = ROLLOUT_TOL[name]
    for p in range(P):
        o_rew, o_nobs, _ = rk4_ref.rollout(ref, raw, q, v, raw.target_pos, act[p])
        scale = max(1.0, np.abs(o_nobs).max())
        assert np.abs(nobs[p] - o_nobs).max() <= tol * scale, (p, np.abs(nobs[p] - o_nobs).max())
        assert np.abs(rew[p] - o_rew).max() <= tol * max(1.0, np.abs(o_rew).max())
    assert eng.solver_failures() == 0


@pytest.mark.parametrize("name", ["cartpole", "swimmer", "double_pendulum"])
def test_not_silently_euler(name):
    """The same model and state under Euler differ from RK4 by more than 1e-6 after one env step."""
    from mjmpc_amd.envs import make_engine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    raw = _raw(name)
    euler = _raw(name)
    euler.integrator = "Euler"
    rk4 = make_engine(raw)
    assert isinstance(rk4, TreeRolloutEngine) and rk4.model.integrator == "RK4"
    eu = TreeRolloutEngine(euler)
    rs = np.random.RandomState(2)
    q, v = _state(name, raw, rs)
    u = 0.3 * np.ones(rk4.d_action)
    outs = []
    for eng in (rk4, eu):
        _set(eng, raw, q, v)
        outs.append(eng.rollout(1, 1, u[None], None, "open_loop")[5][0, 0])
    assert np.abs(outs[0] - outs[1]).max() > 1e-6


def test_device_env_and_graph_replay_match_composed_rk4():
    """step_state / get_state_device and a captured, replayed env step against the composed reference."""
    import torch
    raw, eng, ref = _rig("tray")
    rs = np.random.RandomState(21)
    q, v = _state("tray", raw, rs)
    tgt = np.asarray(raw.target_pos, float)
    us = [rs.uniform(-0.3, 0.3, eng.d_action) for _ in range(4)]
    _set(eng, raw, q, v)
    qo, vo = q.copy(), v.copy()
    for u in us[:2]:
        cost, nobs = eng.step_state(u)
        qo, vo, r, o, _ = rk4_ref.env_step(ref, raw, qo, vo, u, tgt)
        np.testing.assert_allclose(nobs.cpu().numpy(), o, rtol=0, atol=1e-9 * max(1.0, np.abs(o).max()))
        assert abs(-float(cost.cpu()[0]) - r) <= 1e-9 * max(1.0, abs(r))
    st = eng.get_state_device()
    np.testing.assert_allclose(st["qp"], qo, rtol=0, atol=1e-9)
    np.testing.assert_allclose(st["qv"], vo, rtol=0, atol=1e-9 * max(1.0, np.abs(vo).max()))
    a_d = torch.tensor(us[2], dtype=torch.float64, device=eng.device)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.step_state(a_d)                         # (warm-up: buffers allocated outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    qo, vo, _, _, _ = rk4_ref.env_step(ref, raw, qo, vo, us[2], tgt)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        eng.step_state(a_d)
    for u in us[2:]:
        a_d.copy_(torch.tensor(u, dtype=torch.float64))
        g.replay()
        qo, vo, _, _, _ = rk4_ref.env_step(ref, raw, qo, vo, u, tgt)
    torch.cuda.synchronize()
    st = eng.get_state_device()
    np.testing.assert_allclose(st["qp"], qo, rtol=0, atol=1e-9)
    np.testing.assert_allclose(st["qv"], vo, rtol=0, atol=1e-9 * max(1.0, np.abs(vo).max()))


def test_closed_loop_and_fused_launches_mirror_the_rollout():
    """rollout_cl against the composed reference driven by the same linear policy; rollout_fused's costs and actions are
    the open-loop rollout's bits for the same filtered samples."""
    import torch
    raw, eng, ref = _rig("double_pendulum")
    rs = np.random.RandomState(8)
    q, v = _state("double_pendulum", raw, rs)
    tgt = np.asarray(raw.target_pos, float)
    P, H, A, D = 4, 6, eng.d_action, eng.d_obs
    W = 0.05 * rs.standard_normal((D + 1, A))
    eps = 0.2 * rs.standard_normal((P, H, A))
    _set(eng, raw, q, v)
    obs, rew, act, _, _, nobs = eng.rollout(P, H, W, eps, "closed_loop_linear")
    for p in range(P):
        qq, vv = q.copy(), v.copy()
        o = obs[p, 0]
        for t in range(H):
            u = W.T @ np.append(o, 1.0) + eps[p, t]
            np.testing.assert_allclose(act[p, t], u, rtol=0, atol=1e-9)
            qq, vv, r, o, _ = rk4_ref.env_step(ref, raw, qq, vv, u, tgt)
            np.testing.assert_allclose(nobs[p, t], o, rtol=0, atol=1e-9 * max(1.0, np.abs(o).max()))
            assert abs(rew[p, t] - r) <= 1e-9 * max(1.0, abs(r))
    # the fused launch: filter + cost-to-go; the open-loop launch from the filtered samples gives the same bits
    mean = 0.1 * rs.standard_normal((H, A))
    filt = np.array([0.25, 0.8, 0.0])
    raw_eps = 0.3 * rs.standard_normal((P, H, A))
    f_eps = raw_eps.copy()
    for t in range(2, H):
        f_eps[:, t] = filt[0] * raw_eps[:, t] + filt[1] * f_eps[:, t - 1] + filt[2] * f_eps[:, t - 2]
    dev = eng.device
    gseq = torch.ones(H, dtype=torch.float64, device=dev)
    costs, fact, q0 = eng.rollout_fused(P, H, torch.tensor(mean, device=dev), torch.tensor(raw_eps, device=dev),
                                        torch.tensor(filt, device=dev), gseq)
    costs, fact, q0 = costs.cpu().numpy(), fact.cpu().numpy(), q0.cpu().numpy()
    _, rew2, act2, _, _, _ = eng.rollout(P, H, mean, fact - mean[None], "open_loop")
    np.testing.assert_array_equal(act2, fact)
    np.testing.assert_array_equal(-rew2, costs)
    np.testing.assert_allclose(q0, costs.sum(axis=1), rtol=1e-12, atol=0)


def test_randomized_shards_match_their_oracles():
    """randomize_dynamics with 3 shards: every shard against the composed reference on an oracle edited through its setters."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    raw = _raw("cartpole")
    eng = TreeRolloutEngine(raw, dtype="f64", num_shards=3)
    _, rnd = eng.randomize_dynamics({"dof_damping": {"slider": [0.5, 0.0], "hinge": [0.5, 0.0]},
                                     "body_mass": {"pole": [0.3, 0.0]}}, 17)
    rs = np.random.RandomState(4)
    q, v = _state("cartpole", raw, rs)
    tgt = np.asarray(raw.target_pos, float)
    P, H, A = 6, 3, eng.d_action
    mean, eps = np.zeros((H, A)), 0.5 * rs.standard_normal((P, H, A))
    _set(eng, raw, q, v)
    _, rew, act, _, _, nobs = eng.rollout(P, H, mean, eps, "open_loop")
    for s in range(3):
        ref = RefArm(raw.to_flat())
        d = rnd[s]
        bodies = [b.name for b in raw.bodies]
        for jn, val in d.get("dof_damping", {}).items():
            ref.set_dof_damping(raw.dof_of_joint(jn), float(val))
        for bn, val in d.get("body_mass", {}).items():
            ref.set_body_mass(bodies.index(bn) + 1, float(val))
        for p in range(2 * s, 2 * s + 2):
            o_rew, o_nobs, _ = rk4_ref.rollout(ref, raw, q, v, tgt, act[p])
            np.testing.assert_allclose(nobs[p], o_nobs, rtol=0, atol=1e-9 * max(1.0, np.abs(o_nobs).max()))
            np.testing.assert_allclose(rew[p], o_rew, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_wave_mates_do_not_change_a_particles_bits(dtype):
    """A particle's RK4 costs and observations are the same bits alone (P = 1), in a permuted batch and among 256."""
    raw, eng, _ = _rig("cheetah", dtype)
    rs = np.random.RandomState(31)
    q, v = _state("cheetah", raw, rs)
    H, A = 4, eng.d_action
    mean, eps = 0.2 * rs.standard_normal((H, A)), 1.5 * rs.standard_normal((256, H, A))
    _set(eng, raw, q, v)
    _, rew, _, _, _, nobs = eng.rollout(256, H, mean, eps, "open_loop")
    perm = rs.permutation(256)
    _, rew_p, _, _, _, nobs_p = eng.rollout(256, H, mean, eps[perm], "open_loop")
    np.testing.assert_array_equal(rew_p, rew[perm])
    np.testing.assert_array_equal(nobs_p, nobs[perm])
    for p in (0, 7, 100, 255):
        _, r1, _, _, _, n1 = eng.rollout(1, H, mean, eps[p:p + 1], "open_loop")
        np.testing.assert_array_equal(r1[0], rew[p])
        np.testing.assert_array_equal(n1[0], nobs[p])


@pytest.mark.parametrize("kind", ["nan", "acc"])
def test_reset_follows_composed_rk4(kind):
    """A start state holding a NaN (mj_checkVel) and one whose stage-0 acceleration is beyond 1e10 (mj_checkAcc): reset,
    then RK4 from qpos0 with zero controls, as the composed reference; the env-reset counter of the device env moves."""
    raw, eng, ref = _rig("cartpole")
    rs = np.random.RandomState(3)
    q, v = _state("cartpole", raw, rs)
    if kind == "nan":
        v[1] = np.nan
    else:
        v[:] = [0.0, 2e5]                               # (the pole's centripetal terms: qacc ~ 1e10 and beyond)
    tgt = np.asarray(raw.target_pos, float)
    u = np.array([0.7])
    n0 = ref.resets()
    q1, v1, r1, o1, n = rk4_ref.env_step(ref, raw, q, v, u, tgt)
    assert n >= 1
    if kind == "acc":
        assert ref.resets() > n0                        # (the oracle's mj_checkAcc fired at stage 0)
    d0 = eng.diverged_substeps()
    _set(eng, raw, q, v)
    _, rew, _, _, _, nobs = eng.rollout(3, 1, np.tile(u, (1, 1)), np.zeros((3, 1, 1)), "open_loop")
    for p in range(3):
        np.testing.assert_allclose(nobs[p, 0], o1, rtol=0, atol=1e-9 * max(1.0, np.abs(o1).max()))
        assert abs(rew[p, 0] - r1) <= 1e-9 * max(1.0, abs(r1))
    assert eng.diverged_substeps() - d0 >= 3
    eng.on_env_reset = "ignore"
    e0 = eng.env_resets()
    _set(eng, raw, q, v)
    eng.step_state(u)
    st = eng.get_state_device()
    assert eng.env_resets() > e0
    np.testing.assert_allclose(st["qp"], q1, rtol=0, atol=1e-9)
    np.testing.assert_allclose(st["qv"], v1, rtol=0, atol=1e-9 * max(1.0, np.abs(v1).max()))
    eng.set_reset_returns("inf")
    _set(eng, raw, q, v)
    _, rew, _, _, _, _ = eng.rollout(2, 1, np.tile(u, (1, 1)), np.zeros((2, 1, 1)), "open_loop")
    assert np.isinf(rew).all()
    eng.set_reset_returns("finite")
    eng.on_env_reset = "raise"


@pytest.mark.parametrize("name", ["swimmer", "double_pendulum"])
def test_f32_stays_close_to_f64(name):
    raw, e64, _ = _rig(name)
    _, e32, _ = _rig(name, "f32")
    rs = np.random.RandomState(6)
    q, v = _state(name, raw, rs)
    H, A = 8, e64.d_action
    mean, eps = 0.2 * rs.standard_normal((H, A)), 0.5 * rs.standard_normal((256, H, A))
    outs = []
    for eng in (e64, e32):
        _set(eng, raw, q, v)
        outs.append(eng.rollout(256, H, mean, eps, "open_loop"))
    assert np.abs(outs[1][5][:, 0] - outs[0][5][:, 0]).max() < 2e-3
    ret64, ret32 = outs[0][1].sum(axis=1), outs[1][1].sum(axis=1)
    assert abs(ret64.mean() - ret32.mean()) < 0.02 * ret64.std() + 1e-3
    assert np.corrcoef(ret64, ret32)[0, 1] > 0.999


def test_mppi_keeps_the_double_pendulum_upright():
    """make_engine routes the RK4 model to the tree engine; MPPI through the controller keeps the poles up for 20 control
    steps from the model's start state (lower pole tilted by 0.1 rad), without a reset."""
    from mjmpc_amd.envs import make_engine
    from mjmpc_amd.envs.arm_engine import make_rollout_fn
    from mjmpc_amd.envs.synthetic_env import DoublePendulumEnv
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.policies import MPCPolicy
    raw = _raw("double_pendulum")
    sim = make_engine(raw)
    assert isinstance(sim, TreeRolloutEngine) and sim.model.integrator == "RK4"
    env = DoublePendulumEnv()
    env.real_env_step(True)
    env.reset(seed=0)
    params = dict(horizon=32, init_cov=0.3, lam=0.1, step_size=1.0, alpha=1, gamma=1.0, n_iters=1, num_particles=1024,
                  filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seed=0, d_obs=env.d_obs, d_state=env.d_state,
                  d_action=env.d_action, action_lows=env.action_lows, action_highs=env.action_highs)
    policy = MPCPolicy(controller_type="mppi", param_dict=params, batch_size=1)
    policy.controller.set_sim_state_fn = sim.set_env_state
    policy.controller.rollout_fn = make_rollout_fn(sim)
    d0 = env.engine.diverged_substeps()
    for _ in range(20):
        action, _ = policy.get_action(env.get_env_state(), calc_val=False)
        env.step(action)
        qp = env.get_env_state()["qp"]
        assert abs(qp[1]) < 0.5 and abs(qp[1] + qp[2]) < 0.5, qp
    assert env.engine.diverged_substeps() == d0
    assert np.linalg.norm(env._hand - env._target) < 0.3
    sim.close()
