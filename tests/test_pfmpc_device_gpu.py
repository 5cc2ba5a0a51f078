"""GPU: the device-resident mode of PFMPC (``noise_mode='device'``, csrc/pfmpc.hip).

A closed loop cannot be compared end to end with a numpy restatement: the device's Philox normals match
tests/philox_ref.py to ``philox_ref.TOL``, not to the bit, and resampling is discrete - one near-tie would send the two runs
apart.  So every stage is checked against the restatement FED WITH THE DEVICE'S OWN OUTPUT of the stage before it
(``PFMPC.last_device_step()``): the weights against ``oracle.controllers_ref.pf_weights`` on the costs the rollout returned,
the indices against ``systematic_resample_indices`` on the device's weights and pointer (bit for bit), the gathered set
against ``samples[idx]`` (bit for bit), the mean against ``np.mean`` within the forward-error bound of two summations of M
terms, the shifted set against the reference's ``_shift`` with the jitter of ``philox_ref.sample_ref`` within
``philox_ref.error_bound``.  tests/test_pfmpc_device_cpu.py holds the resampling inputs used here to the serial walk."""
import ctypes

import numpy as np
import pytest

import pfmpc_cases as pc

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)      # the controller-update tolerance of tests/test_controllers_gpu.py


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(x, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).cuda()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _resample_on_device(w, first):
    import torch
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    M = w.shape[0]
    idx = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty((lib.mjmpc_pf_workspace_bytes(M, 1, 1) + 7) // 8, dtype=torch.float64, device="cuda")
    d_w, d_first = _dev(w), _dev(np.array([first]))     # (named: a temporary's memory is free for the next allocation)
    _lib.check(lib.mjmpc_pf_resample(M, _vp(d_w), _vp(d_first), _vp(idx), _vp(ws), _stream()))
    torch.cuda.synchronize()
    return idx.cpu().numpy()


@pytest.mark.parametrize("M", pc.SIZES)
@pytest.mark.parametrize("kind", pc.WEIGHT_KINDS)
def test_resampling_kernel_returns_the_indices_of_the_host_search(kind, M):
    from mjmpc_amd.control.particle_filter_controller import systematic_resample_indices
    w = pc.weights(kind, M)
    for pk in pc.POINTER_KINDS:
        first = pc.pointer(pk, M)
        want = systematic_resample_indices(w, first)
        got = _resample_on_device(w, first)
        assert np.array_equal(got, want), (kind, M, pk, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("seed,offset,step", [(0, 0, None), (123, 7, None), (2 ** 63 + 12345, 0, 3), (2 ** 64 - 1, 2, 41),
                                              (77, 2 ** 33, 5)])
def test_first_pointer_is_the_uniform_of_its_own_philox_block(seed, offset, step):
    import torch
    from mjmpc_amd import _lib
    from oracle import controllers_ref as cr
    lib = _lib.require_gpu()
    for M in (8, 1000, 4096):
        rs = np.random.RandomState(M)
        q0 = 30.0 * rs.rand(M)
        q0[M // 2] = np.inf                 # (a diverged rollout weighs nothing)
        w, first = torch.empty(M, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        d_step = None if step is None else torch.full((1,), step, dtype=torch.int64, device="cuda")
        d_q0 = _dev(q0)
        _lib.check(lib.mjmpc_pf_weights(M, _vp(d_q0), 0.7, seed, offset, _vp(d_step), _vp(w), _vp(first), _stream()))
        torch.cuda.synchronize()
        k = offset + (step or 0)
        assert first.item() == pc.first_pointer_ref(seed, k, M), (seed, k, M)
        finite = np.isfinite(q0)
        want = np.zeros(M)
        want[finite] = cr.softmax0((-1.0 / 0.7) * q0[finite])
        np.testing.assert_allclose(w.cpu().numpy(), want, **TOL)


def _check_stages(rec, cov_shift, filter_coeffs, seed, base_action, shifted=True):
    """The resampling, gather-and-mean and shift checks on one step's recorded stages (numpy arrays)."""
    from mjmpc_amd.control.particle_filter_controller import systematic_resample_indices
    M = rec["w"].shape[0]
    k = rec["step"]
    assert rec["first"][0] == pc.first_pointer_ref(seed, k, M)
    assert np.array_equal(rec["idx"], systematic_resample_indices(rec["w"], rec["first"][0]))
    assert np.array_equal(rec["resampled"], rec["samples"][rec["idx"]])
    bound = 2.0 * (M - 1) * 2.0 ** -53 * np.abs(rec["samples"]).max()
    err = np.abs(rec["mean"] - np.mean(rec["resampled"], axis=0)).max()
    print("mean: error %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    if not shifted:
        assert np.array_equal(rec["shifted"], rec["resampled"])
        return
    want, allowed = pc.shift_ref(rec["resampled"], cov_shift, filter_coeffs, seed, k, base_action)
    excess = np.abs(rec["shifted"] - want) - allowed
    print("shift: largest error %.3e, largest error over its bound %.3e" % (np.abs(rec["shifted"] - want).max(), excess.max()))
    assert (excess <= 0.0).all()
    if base_action == "null":
        assert (rec["shifted"][:, -1] == 0.0).all()
    else:
        assert np.array_equal(rec["shifted"][:, -1], rec["shifted"][:, -2])
    # the jitter is there at all: the shifted rows are not the moved rows
    if want.shape[1] > 1:
        assert np.abs(rec["shifted"][:, :-1] - rec["resampled"][:, 1:]).max() > 0.1 * np.sqrt(cov_shift)


@pytest.mark.parametrize("M,H,A,base,coeffs,seed,step", [
    (100, 7, 5, "null", [0.25, 0.8, 0.1], 2 ** 63 + 9, 6),          # H % 4 != 0, a partial last workgroup, 64-bit seed
    (100, 7, 5, "repeat", [0.25, 0.8, 0.1], 11, 0),
    (64, 8, 3, "repeat", [1.0, 0.0, 0.0], 3, 2),                    # no filter
    (1000, 2, 1, "repeat", [0.25, 0.8, 0.0], 5, 1),                 # the shortest horizon 'repeat' has
    (37, 1, 2, "null", [0.25, 0.8, 0.0], 5, 1),
    (4096, 32, 7, "null", [0.25, 0.8, 0.0], 123, 4)])
def test_gather_mean_and_shift_kernels(M, H, A, base, coeffs, seed, step):
    import torch
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    rs = np.random.RandomState(M + H)
    samples, q0, cov_shift, lam = rs.randn(M, H, A), 5.0 * rs.rand(M), 0.3, 0.4
    f64 = dict(dtype=torch.float64, device="cuda")
    d_set, d_out, d_gath = _dev(samples), torch.zeros((M, H, A), **f64), torch.zeros((M, H, A), **f64)
    w, first, mean, act = torch.empty(M, **f64), torch.zeros(1, **f64), torch.zeros((H, A), **f64), torch.zeros(A, **f64)
    idx = torch.empty(M, dtype=torch.int32, device="cuda")
    ws = torch.empty((lib.mjmpc_pf_workspace_bytes(M, H, A) + 7) // 8, **f64)
    d_step = torch.full((1,), step, dtype=torch.int64, device="cuda")
    fc = np.asarray(coeffs, np.float64)
    d_co = None if tuple(fc) == (1.0, 0.0, 0.0) else _dev(fc)
    d_q0, d_chol = _dev(q0), _dev(np.sqrt(cov_shift) * np.eye(A))
    s = _stream()
    _lib.check(lib.mjmpc_pf_weights(M, _vp(d_q0), lam, seed, 0, _vp(d_step), _vp(w), _vp(first), s))
    _lib.check(lib.mjmpc_pf_resample(M, _vp(w), _vp(first), _vp(idx), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_gather_shift(M, H, A, _vp(d_set), _vp(idx), {"null": 0, "repeat": 1}[base],
                                         _vp(d_chol), _vp(d_co), seed, 1, _vp(d_step), _vp(d_out), _vp(d_gath), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_finish(M, H, A, _vp(ws), _vp(mean), _vp(act), _vp(d_step), s))
    torch.cuda.synchronize()
    rec = dict(samples=samples, w=w.cpu().numpy(), first=first.cpu().numpy(), idx=idx.cpu().numpy(),
               resampled=d_gath.cpu().numpy(), mean=mean.cpu().numpy(), shifted=d_out.cpu().numpy(), step=step)
    assert np.array_equal(d_set.cpu().numpy(), samples)                 # the source set is only read
    _check_stages(rec, cov_shift, coeffs, seed, base)
    assert np.array_equal(act.cpu().numpy(), rec["mean"][0]) and int(d_step.item()) == step + 1
    # the deviations the next rollout takes, in both storage types
    for code, tdt in ((_lib.F64, torch.float64), (_lib.F32, torch.float32)):
        delta = torch.empty((M, H, A), dtype=tdt, device="cuda")
        _lib.check(lib.mjmpc_pf_delta(code, M, H, A, _vp(d_out), _vp(mean), _vp(delta), s))
        torch.cuda.synchronize()
        assert np.array_equal(delta.cpu().numpy(), (rec["shifted"] - rec["mean"][None]).astype(delta.cpu().numpy().dtype))
    # shift_mode < 0: the plain gather
    _lib.check(lib.mjmpc_pf_gather_shift(M, H, A, _vp(d_set), _vp(idx), -1, None, None, seed, 1, None, _vp(d_out), None,
                                         _vp(ws), s))
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), samples[rec["idx"]])


# ---- closed loops -----------------------------------------------------------------------------------------------
REACHER_START = dict(qp=np.array([0.1, 0.2, 0.0, -0.5, 0.0, -0.3, 0.0]), qv=np.zeros(7), target_pos=np.array([0.2, -0.1, 0.2]))
CFG = dict(reacher=dict(horizon=12, num_particles=1000, cov_shift=0.05, cov_resample=0.6, lam=0.5, gamma=0.98,
                        filter_coeffs=[0.25, 0.8, 0.1], base_action="repeat"),
           cheetah=dict(horizon=10, num_particles=512, cov_shift=0.02, cov_resample=0.3, lam=1.0, gamma=0.99,
                        filter_coeffs=[0.25, 0.8, 0.0], base_action="null"))


def _make(model, dtype, seed, n_iters=1, **over):
    from mjmpc_amd.control import PFMPC
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    if model == "reacher":
        from mjmpc_amd.models.reacher7dof import reacher7dof_raw
        eng = ArmRolloutEngine(reacher7dof_raw(), dtype=dtype)
        eng.set_env_state(REACHER_START)
    else:
        from mjmpc_amd.envs.locomotion_env import HalfCheetahEnv
        from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
        from mjmpc_amd.models.half_cheetah import half_cheetah_raw
        eng = TreeRolloutEngine(half_cheetah_raw(), dtype=dtype)
        env = HalfCheetahEnv(dtype=dtype)
        env.reset(seed=123)
        eng.set_env_state(env.get_env_state())
    kw = dict(CFG[model], d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, action_lows=eng.action_lows,
              action_highs=eng.action_highs, n_iters=n_iters, seed=seed, noise_mode="device")
    kw.update(over)
    c = PFMPC(**kw)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    return c, eng


def _numpy(rec):
    return {k: (v if isinstance(v, int) else v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64))
            for k, v in rec.items()}


def _closed_loop(model, dtype, seed, n_iters=1, steps=10, check=True):
    import torch
    from oracle import controllers_ref as cr
    c, eng = _make(model, dtype, seed, n_iters)
    cfg = CFG[model]
    acts = []
    for k in range(steps):
        a, _ = c.optimize({})
        rec = _numpy(c.last_device_step())
        assert rec["step"] == k and c.num_steps == k + 1
        assert np.array_equal(a, rec["mean"][0])
        if check:
            assert np.isfinite(rec["costs"]).all()
            want_w = cr.pf_weights(rec["costs"], cr.gamma_seq(cfg["gamma"], cfg["horizon"]), cfg["lam"])
            np.testing.assert_allclose(rec["w"], want_w, **TOL)
            _check_stages(rec, cfg["cov_shift"], cfg["filter_coeffs"], seed, cfg["base_action"])
        eng.step_state(a)
        acts.append(a)
    torch.cuda.synchronize()
    assert eng.solver_failures() == 0
    return np.array(acts)


@pytest.mark.parametrize("model,dtype,n_iters", [("reacher", "f64", 1), ("reacher", "f32", 1), ("cheetah", "f64", 1),
                                                 ("reacher", "f64", 2)])
def test_closed_loop_stage_by_stage(model, dtype, n_iters):
    seed = 2 ** 31 + 17         # (Controller.seed() takes what numpy's RandomState takes: below 2^32)
    acts = _closed_loop(model, dtype, seed, n_iters)
    assert np.isfinite(acts).all() and np.abs(acts).max() > 0.0
    again = _closed_loop(model, dtype, seed, n_iters, check=False)
    assert np.array_equal(acts, again)                                  # same seed: the same actions, bit for bit
    other = _closed_loop(model, dtype, seed + 1, n_iters, check=False)
    assert not np.array_equal(acts, other)


def test_first_step_rolls_out_the_philox_counterpart_of_the_fresh_samples():
    import philox_ref as pr
    c, eng = _make("reacher", "f64", 31)
    cfg = CFG["reacher"]
    M, H, A = cfg["num_particles"], cfg["horizon"], 7
    ref, scale = pr.sample_ref(M, H, A, np.sqrt(cfg["cov_resample"]) * np.eye(A), 31, 0, 0, True, cfg["filter_coeffs"],
                               np.float64, True)
    got = c.sample_actions().cpu().numpy()
    assert (np.abs(got - ref) <= pr.error_bound(ref, scale, cfg["filter_coeffs"])).all()
    assert not c.mean_action.cpu().numpy().any()
    c.optimize({})
    c.reset()
    assert c.num_steps == 0 and np.array_equal(c.sample_actions().cpu().numpy(), got)
    assert not c.mean_action.cpu().numpy().any()


def test_no_hotstart_leaves_the_resampled_set():
    c, eng = _make("reacher", "f64", 8)
    c.optimize({}, hotstart=False)
    rec = _numpy(c.last_device_step())
    _check_stages(rec, 0.0, [1.0, 0.0, 0.0], 8, "null", shifted=False)
    assert c.num_steps == 1


def test_resident_loop_equals_the_loop_through_the_host():
    """``resident_state`` + ``set_post_step(engine.step_state)``: no state is uploaded, and the actions are those of the
    loop that reads the state back and hands it to ``optimize()`` - the real env is stepped by ``step_state`` in both."""
    import torch
    from mjmpc_amd.control.controller import resident_state

    def run(resident, steps=8):
        c, eng = _make("cheetah", "f64", 5)
        uploads = []
        real_set = eng.set_env_state
        eng.set_env_state = lambda s: (uploads.append(1), real_set(s))[1]
        if resident:
            c.set_sim_state_fn = resident_state
            c.set_post_step(eng.step_state)
        else:
            c.set_sim_state_fn = eng.set_env_state
        acts = []
        for _ in range(steps):
            if resident:
                a, _ = c.optimize({"resident": True})
            else:
                a, _ = c.optimize(eng.get_state_device())
                eng.step_state(a)
            acts.append(a)
        torch.cuda.synchronize()
        return np.array(acts), eng.get_state_device(), len(uploads)

    a_h, s_h, n_h = run(False)
    a_r, s_r, n_r = run(True)
    assert n_h == 8 and n_r == 0
    assert np.array_equal(a_r, a_h)
    assert np.array_equal(s_r["qpos"], s_h["qpos"]) and np.array_equal(s_r["qvel"], s_h["qvel"])


def test_device_mode_on_an_engine_without_a_fused_rollout():
    """The analytic engines offer no fused launch: the cost-to-go comes from the update's own kernel instead."""
    from mjmpc_amd.control import PFMPC
    from mjmpc_amd.envs.analytic_engine import AnalyticRolloutEngine
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from oracle import controllers_ref as cr
    eng = AnalyticRolloutEngine.pendulum()
    eng.set_env_state({"state": np.array([2.5, 0.3])})
    c = PFMPC(d_state=2, d_obs=3, d_action=1, horizon=9, cov_shift=0.1, cov_resample=1.0, base_action="null", lam=0.8,
              num_particles=200, gamma=0.97, n_iters=1, action_lows=np.array([-2.0]), action_highs=np.array([2.0]),
              filter_coeffs=[0.25, 0.8, 0.0], seed=4, noise_mode="device")
    fn = make_device_rollout_fn(eng)
    assert not hasattr(fn, "fused")
    c.rollout_fn = fn
    c.set_sim_state_fn = lambda s: None
    for k in range(3):
        a, _ = c.optimize({})
        rec = _numpy(c.last_device_step())
        np.testing.assert_allclose(rec["w"], cr.pf_weights(rec["costs"], cr.gamma_seq(0.97, 9), 0.8), **TOL)
        _check_stages(rec, 0.1, [0.25, 0.8, 0.0], 4, "null")
        assert np.array_equal(a, rec["mean"][0])


def test_host_mode_is_the_default_and_unchanged():
    from mjmpc_amd.control import PFMPC
    from oracle import envs_ref as er
    from oracle.envs_ref import PendulumRef
    env = PendulumRef()

    def one_step(**kw):
        state = {}

        def rollout_fn(num_particles, horizon, mean, noise, mode):
            obs, rew, act, done, nobs = er.rollout(env, state["cur"], num_particles, horizon, mean, noise)
            return dict(observations=obs, actions=act, costs=-rew, dones=done, next_observations=nobs)

        c = PFMPC(d_state=2, d_obs=3, d_action=1, horizon=10, cov_shift=0.1, cov_resample=1.0, base_action="repeat", lam=0.3,
                  num_particles=48, gamma=0.99, n_iters=1, action_lows=np.array([-2.0]), action_highs=np.array([2.0]),
                  filter_coeffs=[0.25, 0.8, 0.0], seed=123, **kw)
        c.set_sim_state_fn = lambda s: state.update(cur=np.asarray(s["state"], float).copy())
        c.rollout_fn = rollout_fn
        a, _ = c.optimize({"state": np.array([2.0, 0.5])})
        return a, c.action_samples.copy(), c.noise_mode

    a0, s0, m0 = one_step()
    a1, s1, m1 = one_step(noise_mode="host")
    assert m0 == m1 == "host"
    assert isinstance(s0, np.ndarray) and np.array_equal(a0, a1) and np.array_equal(s0, s1)


def test_assigning_a_host_rollout_fn_in_device_mode_is_refused():
    c, eng = _make("reacher", "f64", 1)
    with pytest.raises(ValueError, match="rollout_fn"):
        c.rollout_fn = lambda *a, **k: None
