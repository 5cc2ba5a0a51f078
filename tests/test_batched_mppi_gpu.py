"""GPU: an episode batch (``BatchedMPPI``) reproduces E separate single-episode runs to the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``MPPI(...,
noise_mode='device', seed=seed_e)``, ``make_device_rollout_fn(engine)``, ``enable_graph(post_step=engine.step_state)``
(tests/test_baseline_sizes_gpu.py's pattern), whose iteration runs ``mjmpc_tree_rollout_fused`` + the fused MPPI update
and steps the engine's device-resident real env.  Unless a test says otherwise every comparison is ``np.array_equal``:
the actions, real-env costs and next observations of every step, the final mean and the final state.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILT = [0.25, 0.8, 0.0]


def _torch():
    import torch
    return torch


def _single(raw, state, seed, P, H, T, lam, step_size, init_cov, dtype, gamma=1.0, base_action="null", init_mean=None):
    """One episode on the single-episode device path -> (actions [T][A], costs [T], next obs [T][d_obs], mean, state)."""
    torch = _torch()
    from mjmpc_amd.control import MPPI
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, dtype=dtype)
    eng.set_env_state(dict(state))
    A = eng.d_action
    c = MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=A, horizon=H, init_cov=init_cov, base_action=base_action, lam=lam,
             num_particles=P, step_size=step_size, alpha=1, gamma=gamma, n_iters=1, action_lows=eng.action_lows,
             action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed, noise_mode="device", noise_dtype=dtype)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    if init_mean is not None:
        c.mean_action = np.array(init_mean, np.float64)
    c.enable_graph(post_step=eng.step_state)
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize(None)
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    mean = np.array(c.mean_action)
    st = eng.get_state_device()
    eng.close()
    return np.array(acts), np.array(costs), np.array(nobs), mean, st


def _batch(raw, states, seeds, P, H, T, lam, step_size, init_cov, dtype, gamma=1.0, base_action="null", init_mean=None):
    from mjmpc_amd.control import BatchedMPPI
    b = BatchedMPPI(raw, len(states), H, P, lam, step_size, init_cov, gamma, FILT, base_action, seeds, init_mean=init_mean,
                    dtype=dtype)
    b.set_states([dict(s) for s in states])
    acts, costs, nobs = b.run(T)
    out = acts, costs, nobs, b.mean_action, b.get_states()
    b.close()
    return out


def _qpos_qvel(st):
    return (st["qpos"], st["qvel"]) if "qpos" in st else (st["qp"], st["qv"])


def _check_against_singles(raw, states, seeds, P, H, T, lam, step_size, init_cov, dtype, **kw):
    E = len(states)
    per = lambda v, e: v[e] if np.ndim(v) > 0 else v          # noqa: E731
    acts, costs, nobs, means, fin = _batch(raw, states, seeds, P, H, T, lam, step_size, init_cov, dtype, **kw)
    assert acts.shape[:2] == (T, E) and costs.shape == (T, E) and means.shape[0] == E and len(fin) == E
    assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs))
    for e in range(E):
        im = kw.get("init_mean")
        skw = dict(kw, init_mean=None if im is None else (im[e] if np.ndim(im) == 3 else im))
        a1, c1, o1, m1, s1 = _single(raw, states[e], seeds[e], P, H, T, per(lam, e), per(step_size, e), per(init_cov, e), dtype,
                                     **skw)
        assert np.array_equal(acts[:, e], a1), "episode %d: actions differ (max %.3g)" % (e, np.abs(acts[:, e] - a1).max())
        assert np.array_equal(costs[:, e], c1), "episode %d: real-env costs differ" % e
        assert np.array_equal(nobs[:, e], o1), "episode %d: next observations differ" % e
        assert np.array_equal(means[e], m1), "episode %d: final mean differs" % e
        for x, y in zip(_qpos_qvel(fin[e]), _qpos_qvel(s1)):
            assert np.array_equal(x, y), "episode %d: final state differs" % e
    return acts, costs


def _cheetah_states(E):
    from mjmpc_amd.envs.locomotion_env import HalfCheetahEnv
    env = HalfCheetahEnv()
    out = []
    for i in range(E):
        env.reset(seed=123 + i * 12345)
        out.append(env.get_env_state())
    env.engine.close()
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_single_episodes(dtype):
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    E = 4
    acts, _ = _check_against_singles(half_cheetah_raw(), _cheetah_states(E), [123 + i * 12345 for i in range(E)], 256, 16, 20,
                                     0.2, 1.0, 0.3, dtype)
    assert not np.array_equal(acts[:, 0], acts[:, 1])          # (the episodes are different episodes)


def test_per_episode_hyperparameters():
    """Different lam, step_size and init_cov (and initial mean) per episode, base_action 'repeat'."""
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    E, H = 4, 16
    init_mean = np.random.RandomState(5).uniform(-0.3, 0.3, (E, H, 6))
    _check_against_singles(half_cheetah_raw(), _cheetah_states(E), [7 + 3 * i for i in range(E)], 256, H, 20,
                           np.array([0.05, 0.2, 1.0, 0.5]), np.array([1.0, 0.8, 0.5, 0.9]), np.array([0.1, 0.3, 0.6, 1.0]),
                           "f64", base_action="repeat", init_mean=init_mean)


def _synthetic_states(name, E, seed=0):
    """The env class's start state with a small per-episode velocity offset (the synthetic envs start from one state)."""
    from mjmpc_amd.envs.synthetic_env import start_state
    from mjmpc_amd.models.synthetic import synthetic_raw
    raw = synthetic_raw(name)
    st = start_state(name, raw)
    rng = np.random.RandomState(seed)
    return raw, [dict(qp=st["qp"].copy(), qv=st["qv"] + 0.05 * rng.randn(st["qv"].size), target_pos=st["target_pos"].copy())
                 for _ in range(E)]


def test_free_joint_model_round_trips_quaternions():
    """A GEN model with a free joint (the tray's glass): the quaternion goes through the state shards and back."""
    raw, states = _synthetic_states("tray", 3)
    assert raw_has_free(raw)
    _check_against_singles(raw, states, [11, 12, 13], 256, 16, 10, 0.5, 1.0, 0.3, "f64")


def raw_has_free(raw):
    from mjmpc_amd.models.compile_tree import compile_tree
    m = compile_tree(raw)
    return m.nq > m.nv


def test_rk4_double_pendulum():
    raw, states = _synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    _check_against_singles(raw, states, [21, 22], 256, 16, 10, 0.2, 1.0, 0.3, "f64")


def test_permuting_the_episodes_permutes_the_results():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw, E = half_cheetah_raw(), 4
    states, seeds = _cheetah_states(E), [5, 6, 7, 8]
    lam, step, cov = np.array([0.1, 0.2, 0.3, 0.4]), np.array([1.0, 0.9, 0.8, 0.7]), np.array([0.2, 0.3, 0.4, 0.5])
    base = _batch(raw, states, seeds, 256, 16, 10, lam, step, cov, "f64")
    perm = [2, 0, 3, 1]
    got = _batch(raw, [states[k] for k in perm], [seeds[k] for k in perm], 256, 16, 10, lam[perm], step[perm], cov[perm], "f64")
    assert np.array_equal(got[0], base[0][:, perm]) and np.array_equal(got[1], base[1][:, perm])
    assert np.array_equal(got[2], base[2][:, perm]) and np.array_equal(got[3], base[3][perm])
    for k, e in enumerate(perm):
        for x, y in zip(_qpos_qvel(got[4][k]), _qpos_qvel(base[4][e])):
            assert np.array_equal(x, y)


def test_one_episode_equals_the_single_path():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    _check_against_singles(half_cheetah_raw(), _cheetah_states(1), [123], 512, 16, 15, 0.2, 1.0, 0.3, "f64")


def test_reacher_on_the_tree_engine_with_per_episode_targets():
    """sawyer.xml (the reference's reacher) on the tree engine, eight episodes with their own targets, 512 x H32."""
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    raw, E = reacher7dof_raw(), 8
    env = Reacher7DOFEnv(engine=TreeRolloutEngine(raw))
    states = []
    for i in range(E):
        env.reset(seed=123 + i * 12345)
        st = env.get_env_state()
        states.append(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
    env.engine.close()
    assert len({tuple(s["target_pos"]) for s in states}) == E
    _check_against_singles(raw, states, [123 + i * 12345 for i in range(E)], 512, 32, 8, 0.01, 1.0, 1.0, "f64")


def test_batched_env_step_equals_single_steps_with_resets():
    """One launch steps E real envs as mjmpc_tree_step_state steps E single-state engines - bits and env-reset counts -
    including a start state already beyond MuJoCo's 1e10 bound (the kernel's emulation of mj_resetData)."""
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw, E = half_cheetah_raw(), 4
    states = _cheetah_states(E)
    states[2] = dict(qpos=states[2]["qpos"].copy(), qvel=states[2]["qvel"].copy())
    states[2]["qvel"][3] = 3e10
    rng = np.random.RandomState(0)
    actions = [rng.uniform(-1, 1, (E, 6)) for _ in range(3)]
    for dtype in ("f64", "f32"):
        # the batch: one engine, E state shards
        eng = TreeRolloutEngine(raw, dtype=dtype)
        eng.on_env_reset = "ignore"
        nq, nv, D = eng.model.nq, eng.model.nv, eng.d_obs
        arr = np.zeros((E, 78))
        for k, s in enumerate(states):
            arr[k, :nq], arr[k, 40:40 + nv], arr[k, 72:75] = s["qpos"], s["qvel"], eng.model.target_default
        lib, strm = eng._lib, eng._stream()
        _lib.check(lib.mjmpc_tree_set_shard_states(eng._h, arr.ctypes.data_as(_lib._dp), E, strm))
        tdt = torch.float32 if dtype == "f32" else torch.float64
        bc, bo = [], []
        for a in actions:
            ad = torch.from_numpy(a).cuda()
            cost, obs = torch.empty(E, dtype=tdt, device="cuda"), torch.empty((E, D), dtype=tdt, device="cuda")
            _lib.check(lib.mjmpc_tree_step_shard_states(eng._h, eng._code, ctypes.c_void_p(ad.data_ptr()),
                                                        ctypes.c_void_p(cost.data_ptr()), ctypes.c_void_p(obs.data_ptr()), strm))
            torch.cuda.synchronize()
            bc.append(cost.cpu().numpy())
            bo.append(obs.cpu().numpy())
        qp, qv = np.zeros((E, nq)), np.zeros((E, nv))
        _lib.check(lib.mjmpc_tree_get_shard_states(eng._h, qp.ctypes.data_as(_lib._dp), qv.ctypes.data_as(_lib._dp), strm))
        batch_resets = eng.env_resets()
        eng.close()
        # E single-state engines, mjmpc_tree_step_state
        single_resets = 0
        for e in range(E):
            s = TreeRolloutEngine(raw, dtype=dtype)
            s.on_env_reset = "ignore"
            s.set_env_state(dict(states[e]))
            for k, a in enumerate(actions):
                cost, obs = s.step_state(a[e])
                torch.cuda.synchronize()
                assert np.array_equal(cost.cpu().numpy()[0], bc[k][e]), (dtype, e, k)
                assert np.array_equal(obs.cpu().numpy(), bo[k][e]), (dtype, e, k)
            st = s.get_state_device()
            assert np.array_equal(st["qpos"], qp[e]) and np.array_equal(st["qvel"], qv[e]), (dtype, e)
            single_resets += s.env_resets()
            s.close()
        assert single_resets >= 1 and batch_resets == single_resets, (dtype, batch_resets, single_resets)
        assert np.all(np.isfinite(qp)) and np.all(np.abs(qv) < 1e10)


def test_env_reset_policy_is_checked_where_run_synchronises():
    """A real env that resets raises at the end of run() under the default policy (SimulationUnstableError)."""
    from mjmpc_amd.control import BatchedMPPI
    from mjmpc_amd.envs.tree_engine import SimulationUnstableError
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    states = _cheetah_states(2)
    bad = dict(qpos=states[1]["qpos"].copy(), qvel=states[1]["qvel"].copy())
    bad["qvel"][3] = 3e10
    b = BatchedMPPI(half_cheetah_raw(), 2, 8, 64, 0.2, 1.0, 0.3, 1.0, FILT, "null", [1, 2])
    b.set_states([states[0], bad])
    with pytest.raises(SimulationUnstableError):
        b.run(2)
    b.on_env_reset = "ignore"
    acts, _, _ = b.run(2)
    assert np.all(np.isfinite(acts))
    b.close()
