"""GPU: a random-shooting episode batch (``BatchedRandomShooting``) reproduces E separate single-episode runs to
the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``RandomShooting(...,
noise_mode='device', noise_dtype=dtype, seed=seed_e)``, ``make_device_rollout_fn(engine)``,
``enable_graph(post_step=engine.step_state)``, whose iteration runs the Philox draw, ``mjmpc_tree_rollout_fused`` (filter +
rollout + q0), ``mjmpc_rs_best`` + ``mjmpc_rs_combine`` and ``mjmpc_step_tail`` and steps the engine's device-resident real env;
``_single`` asserts that it took that q0-from-rollout branch.  Every comparison is ``np.array_equal``: the actions, real-env
costs and next observations of every step, the final mean and the final state.  No real env may reset on either side and
every action and cost is finite, so that two all-``inf`` runs cannot pass for equal.  A single run is computed once per
setting and shared, read-only, by the tests that compare against it.
"""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILT = [0.25, 0.8, 0.0]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _per(v, e):
    return v[e] if np.ndim(v) > 0 else v


_SINGLES = {}


def _single(raw, state, seed, P, H, T, step_size, init_cov, dtype, base_action="null", K=1, cfg=None, dyn_seed=None, key=None):
    """One episode on the single-episode device path -> (actions [T][A], costs [T], next obs [T][d_obs], mean, state).
    ``key``: names the model and the start state; runs with a key are kept and shared."""
    full_key = None if key is None else (key, seed, P, H, T, float(step_size), float(init_cov), dtype, base_action, K,
                                         repr(cfg), dyn_seed)
    if full_key in _SINGLES:
        return _SINGLES[full_key]
    torch = _torch()
    from mjmpc_amd.control import RandomShooting
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, dtype=dtype, num_shards=K)
    if cfg is not None:
        eng.randomize_dynamics(cfg, dyn_seed)
        eng.set_real_env_model("nominal")
    eng.set_env_state(dict(state))
    A = eng.d_action
    c = RandomShooting(d_state=eng.d_state, d_obs=eng.d_obs, d_action=A, horizon=H, init_cov=init_cov, base_action=base_action,
                       num_particles=P, step_size=step_size, gamma=1.0, n_iters=1, action_lows=eng.action_lows,
                       action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed, noise_mode="device", noise_dtype=dtype)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    c.enable_graph(post_step=eng.step_state)
    # the branch of the device iteration that takes q0 from the rollout launch (draw, fused rollout, rs_best + rs_combine, tail)
    assert c._wants_q0() and c.noise_mode == "device" and hasattr(c._rollout_fn, "fused")
    assert not c.dev.gamma_zero and not c.use_zero_control_seq
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize(None)
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    mean = np.array(c.mean_action)
    st = eng.get_state_device()
    assert eng.env_resets() == 0, "the single path's real env reset"
    eng.close()
    out = np.array(acts), np.array(costs), np.array(nobs), mean, st
    if full_key is not None:
        _SINGLES[full_key] = out
    return out


def _batch(raw, states, seeds, P, H, T, step_size, init_cov, dtype, base_action="null", K=1, cfg=None, dyn_seed=None):
    from mjmpc_amd.control import BatchedRandomShooting
    b = BatchedRandomShooting(raw, len(states), H, P, step_size, init_cov, 1.0, FILT, base_action, seeds, dtype=dtype)
    b.set_states([dict(s) for s in states])
    if cfg is not None:
        b.randomize_dynamics(cfg, dyn_seed, K)
    acts, costs, nobs = b.run(T)
    out = acts, costs, nobs, b.mean_action, b.get_states()
    assert b.engine.env_resets() == 0, "a real env of the batch reset"
    b.close()
    return out


def _qpos_qvel(st):
    return (st["qpos"], st["qvel"]) if "qpos" in st else (st["qp"], st["qv"])


def _check_against_singles(raw, states, seeds, P, H, T, step_size, init_cov, dtype, keys=None, **kw):
    E = len(states)
    acts, costs, nobs, means, fin = _batch(raw, states, seeds, P, H, T, step_size, init_cov, dtype, **kw)
    assert acts.shape[:2] == (T, E) and costs.shape == (T, E) and means.shape[0] == E and len(fin) == E
    assert np.all(np.isfinite(acts)) and np.all(np.isfinite(costs))
    for e in range(E):
        skw = dict(kw)
        if isinstance(skw.get("dyn_seed"), (list, tuple)):
            skw["dyn_seed"] = skw["dyn_seed"][e]
        a1, c1, o1, m1, s1 = _single(raw, states[e], seeds[e], P, H, T, _per(step_size, e), _per(init_cov, e), dtype,
                                     key=None if keys is None else keys[e], **skw)
        assert np.all(np.isfinite(a1)) and np.all(np.isfinite(c1))
        assert np.array_equal(acts[:, e], a1), "episode %d: actions differ (max %.3g)" % (e, np.abs(acts[:, e] - a1).max())
        assert np.array_equal(costs[:, e], c1), "episode %d: real-env costs differ" % e
        assert np.array_equal(nobs[:, e], o1), "episode %d: next observations differ" % e
        assert np.array_equal(means[e], m1), "episode %d: final mean differs" % e
        for x, y in zip(_qpos_qvel(fin[e]), _qpos_qvel(s1)):
            assert np.array_equal(x, y), "episode %d: final state differs" % e
    return acts, costs


_CHEETAH = {}


def _cheetah_states(E):
    """Start states of the env class's seeded resets (state i does not depend on E), made once and shared (read-only)."""
    if E not in _CHEETAH:
        from mjmpc_amd.envs.locomotion_env import HalfCheetahEnv
        env = HalfCheetahEnv()
        out = []
        for i in range(E):
            env.reset(seed=123 + i * 12345)
            out.append(env.get_env_state())
        env.engine.close()
        _CHEETAH[E] = out
    return _CHEETAH[E]


def _cheetah_keys(E):
    return [("half_cheetah", i) for i in range(E)]


def _cheetah():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    return half_cheetah_raw()


SEEDS = [123 + i * 12345 for i in range(3)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_single_episodes(dtype):
    """E = 3, P = 64, H = 8, T = 6; step_size 0.7: the blend is a blend and not a copy of the best sequence."""
    E = 3
    acts, _ = _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS, 64, 8, 6, 0.7, 0.3, dtype, keys=_cheetah_keys(E))
    assert not np.array_equal(acts[:, 0], acts[:, 1])           # (the episodes are different episodes)


def test_per_episode_hyperparameters():
    """A step size of 1 (the copy), two below it; three covariances."""
    E = 3
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS, 64, 8, 6, np.array([1.0, 0.7, 0.4]), np.array([0.2, 0.3, 0.5]),
                           "f64", keys=_cheetah_keys(E))


def test_base_action_repeat():
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 64, 8, 6, 0.7, 0.3, "f64", base_action="repeat",
                           keys=_cheetah_keys(E))


def test_particles_not_a_multiple_of_the_block_or_a_wave():
    """P = 50: the scan's last stride is partial, and row e + 1's cost-to-go lies right behind row e's."""
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 50, 8, 6, 0.7, 0.3, "f64", keys=_cheetah_keys(E))


def test_one_episode():
    _check_against_singles(_cheetah(), _cheetah_states(1), SEEDS[:1], 64, 8, 6, 0.7, 0.3, "f64", keys=_cheetah_keys(1))


def test_permuting_the_episodes_permutes_the_results():
    raw, E = _cheetah(), 3
    states = _cheetah_states(E)
    step, cov = np.array([1.0, 0.7, 0.4]), np.array([0.2, 0.3, 0.5])
    base = _batch(raw, states, SEEDS, 64, 8, 6, step, cov, "f64")
    perm = [2, 0, 1]
    got = _batch(raw, [states[k] for k in perm], [SEEDS[k] for k in perm], 64, 8, 6, step[perm], cov[perm], "f64")
    for i in range(3):
        assert np.array_equal(got[i], base[i][:, perm])
    assert np.array_equal(got[3], base[3][perm])
    for k, e in enumerate(perm):
        for x, y in zip(_qpos_qvel(got[4][k]), _qpos_qvel(base[4][e])):
            assert np.array_equal(x, y)


def test_free_joint_model():
    """A general instantiation of the rollout kernel: the tray, whose glass has a free joint."""
    from mjmpc_amd.envs.synthetic_env import start_state
    from mjmpc_amd.models.compile_tree import compile_tree
    from mjmpc_amd.models.synthetic import synthetic_raw
    raw = synthetic_raw("tray")
    m = compile_tree(raw)
    assert m.nq > m.nv
    st = start_state("tray", raw)
    rng = np.random.RandomState(0)
    states = [dict(qp=st["qp"].copy(), qv=st["qv"] + 0.05 * rng.randn(st["qv"].size), target_pos=st["target_pos"].copy())
              for _ in range(2)]
    _check_against_singles(raw, states, [11, 12], 32, 4, 3, 0.7, 0.3, "f64")


@pytest.mark.parametrize("dyn_seed", [5, [3, 4]], ids=["shared_seed", "per_episode_seeds"])
def test_randomized_dynamics_two_shards(dyn_seed):
    """K = 2 shards of 32 particles roll out their own model blocks (the parameters of
    examples/configs/half_cheetah_gpu_dyn_randomize.yml); the real envs stay nominal."""
    import yaml
    with open(os.path.join(ROOT, "examples", "configs", "half_cheetah_gpu_dyn_randomize.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) == {"body_mass", "dof_damping", "geom_friction"}
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 64, 8, 6, 0.7, 0.3, "f64", K=2, cfg=cfg, dyn_seed=dyn_seed)


def test_best_particle_is_the_argmin_of_the_cost_to_go():
    from mjmpc_amd.control import BatchedRandomShooting
    E, P = 3, 64
    b = BatchedRandomShooting(_cheetah(), E, 8, P, 0.7, 0.3, 1.0, FILT, "null", SEEDS)
    b.set_states([dict(s) for s in _cheetah_states(E)])
    b.step()
    best = b.best_particle
    q0 = b._q0.cpu().numpy().reshape(E, P)
    b.close()
    assert best.shape == (E,) and best.dtype == np.int64
    assert np.all(np.isfinite(q0.min(axis=1)))
    assert np.array_equal(best, np.argmin(q0, axis=1))
    assert len(set(best.tolist())) > 1                          # (not one index for every episode)


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shift_mode", [0, 1])
def test_update_launch_on_hand_made_rows(shift_mode, dtype):
    """E = 4 rows of P = 300 (two strides of the block, the second partial), H = 3, A = 2: the minimum in the last entry; three
    tied minima, two in the two strides of one thread and one in another wavefront (the lowest index wins); a row of +inf
    (particle 0, never index P); a row of equal values.  Means and actions against a numpy evaluation to 1e-15 relative: means, actions and step sizes are
    positive, so neither the blend nor its fused-multiply-add form cancels and both are within two roundings (1.1e-16
    relative each) of the exact value of their common operands, at most 4.4e-16 apart - bitwise equality is not asserted, the
    contraction is not numpy's."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, P, H, A = 4, 300, 3, 2
    code = _lib.F32 if dtype == "f32" else _lib.F64
    npt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.RandomState(4)
    q0 = rng.uniform(1.0, 2.0, (E, P))
    q0[0, 299] = 0.5
    q0[1, [7, 64, 263]] = 0.25
    q0[2, :] = np.inf
    q0[3, :] = 1.5
    expect = np.array([299, 7, 0, 0])
    assert np.array_equal(np.argmin(q0, axis=1), expect)
    actions = rng.uniform(0.1, 1.0, (E, P, H, A)).astype(npt)
    means0 = rng.uniform(0.1, 1.0, (E, H, A))
    step = np.array([0.7, 1.0, 0.4, 0.25])
    # -- numpy: blend, read the action out, shift
    blended = np.stack([(1.0 - step[e]) * means0[e] + step[e] * actions[e, expect[e]].astype(np.float64) for e in range(E)])
    ref_out = blended[:, 0].copy()
    ref_means = np.concatenate([blended[:, 1:], blended[:, -1:] if shift_mode == 1 else np.zeros((E, 1, A))], axis=1)

    dev = "cuda"
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_q0, d_act, d_step = d(q0), d(actions), d(step)
    step0 = 3
    for with_outputs in (True, False):
        d_means = d(means0)
        d_out = torch.zeros((E, A), dtype=torch.float64, device=dev) if with_outputs else None
        d_counter = torch.full((1,), step0, dtype=torch.int64, device=dev) if with_outputs else None
        d_best = torch.full((E,), -1, dtype=torch.int64, device=dev) if with_outputs else None
        _lib.check(lib.mjmpc_rs_update_batch(code, E, P, H, A, _vp(d_q0), _vp(d_act), _vp(d_step), shift_mode, _vp(d_means),
                                             _vp(d_out), _vp(d_counter), _vp(d_best), s))
        torch.cuda.synchronize()
        np.testing.assert_allclose(d_means.cpu().numpy(), ref_means, rtol=1e-15, atol=0)
        if with_outputs:
            assert np.array_equal(d_best.cpu().numpy(), expect)
            np.testing.assert_allclose(d_out.cpu().numpy(), ref_out, rtol=1e-15, atol=0)
            assert int(d_counter.item()) == step0 + 1           # advanced once, by row 0
    assert np.array_equal(d_q0.cpu().numpy(), q0) and np.array_equal(d_act.cpu().numpy(), actions)      # inputs untouched
