"""GPU: episode batches on the arm engine (``engine="arm"``).

The arm kernels choose their launch shape from the grid, and a particle's bits depend on its group of 8 and on that shape.  The
exact reference of a batch launch is therefore a plain ``mjmpc_arm_rollout_fused`` launch OF THE SAME SIZE (all ``E * P``
particles) under episode e's state and mean, of which rows ``[e P, (e + 1) P)`` are episode e's; the exact reference of the
batched env step is ``mjmpc_arm_step_state`` on a single-state engine.  Every comparison is ``np.array_equal`` except the
one against the C oracle (1e-9, the project's f64 gate).
"""
import ctypes
import types

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, _torch, _vp

pytestmark = pytest.mark.gpu

A = 7
E_BADARG = -1       # MJMPC_E_BADARG
_STATES = []


def _raw():
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    return reacher7dof_raw()


def _states(E):
    """Start states of ``Reacher7DOFEnv``'s seeded resets with their own targets (state i does not depend on E), made once."""
    if len(_STATES) < E:
        from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
        env = Reacher7DOFEnv()
        for i in range(len(_STATES), E):
            env.reset(seed=123 + i * 12345)
            st = env.get_env_state()
            _STATES.append(dict(qp=st["qp"].copy(), qv=st["qv"].copy(), target_pos=st["target_pos"].copy()))
        env.engine.close()
        assert len({tuple(s["target_pos"]) for s in _STATES}) == len(_STATES)
    return [dict(qp=s["qp"].copy(), qv=s["qv"].copy(), target_pos=s["target_pos"].copy()) for s in _STATES[:E]]


def _engine(dtype):
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    return ArmRolloutEngine(_raw(), dtype=dtype)


def _inputs(E, P, H, dtype, seed):
    """Means [E][H][A], raw noise [E P][H][A] in the dtype, filter coefficients and a discount sequence, on the device."""
    torch = _torch()
    rng = np.random.RandomState(seed)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    means = torch.from_numpy(rng.uniform(-0.3, 0.3, (E, H, A))).cuda()
    noise = torch.from_numpy(rng.standard_normal((E * P, H, A))).to(tdt).cuda()
    coeffs = torch.tensor(FILT, dtype=torch.float64).cuda()
    gseq = torch.from_numpy(np.cumprod([1.0] + [0.97] * (H - 1))).cuda()
    return means, noise, coeffs, gseq


def _batch_rollout(eng, E, P, H, means, noise, coeffs, gseq):
    """One ``mjmpc_arm_rollout_fused_batch`` launch on the engine's state shards -> costs, actions, q0 (host)."""
    torch = _torch()
    from mjmpc_amd import _lib
    costs = torch.empty((E * P, H), dtype=noise.dtype, device="cuda")
    acts = torch.empty((E * P, H, A), dtype=noise.dtype, device="cuda")
    q0 = None if gseq is None else torch.empty(E * P, dtype=torch.float64, device="cuda")
    _lib.check(eng._lib.mjmpc_arm_rollout_fused_batch(eng._h, eng._code, E * P, H, _vp(means), _vp(noise), _vp(coeffs), _vp(gseq),
                                                      _vp(costs), _vp(acts), _vp(q0), eng._stream()))
    torch.cuda.synchronize()
    return costs.cpu().numpy(), acts.cpu().numpy(), None if q0 is None else q0.cpu().numpy()


def _check_rollout_against_plain_launches(dtype, E, P, H, seed):
    states = _states(E)
    means, noise, coeffs, gseq = _inputs(E, P, H, dtype, seed)
    eng = _engine(dtype)
    eng.set_shard_states_raw([eng._unpack(s) for s in states])
    costs, acts, q0 = _batch_rollout(eng, E, P, H, means, noise, coeffs, gseq)
    assert eng.solver_failures() == 0
    eng.close()
    assert np.all(np.isfinite(costs)) and np.all(np.isfinite(q0))
    ref = _engine(dtype)
    for e in range(E):
        ref.set_env_state(states[e])
        c, a, q = (x.cpu().numpy() for x in ref.rollout_fused(E * P, H, means[e], noise, coeffs, gseq))
        rows = slice(e * P, (e + 1) * P)
        assert np.array_equal(costs[rows], c[rows]), (dtype, E * P, e, np.abs(costs[rows] - c[rows]).max())
        assert np.array_equal(acts[rows], a[rows]), (dtype, E * P, e)
        assert np.array_equal(q0[rows], q[rows]), (dtype, E * P, e)
        other = slice(((e + 1) % E) * P, ((e + 1) % E + 1) * P)        # (another episode's rows follow ITS state and mean)
        assert not np.array_equal(costs[other], c[other])
    ref.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_batch_rollout_equals_plain_launches_of_the_same_size(dtype):
    """E = 3 episodes of two particle groups each (the four-wave flag shape on any MI300-class device)."""
    _check_rollout_against_plain_launches(dtype, 3, 16, 3, 1)


# (shape, smallest total above the shape's lower threshold in SIMDs, dtypes) - launch_arm_rollout's choices from the grid
# (three waves per SIMD fit in f32 only: in f64 the last total runs the two-wave instantiation again)
SHAPES = [("duo", 2, ("f64",)), ("solo_1_wave", 4, ("f64",)), ("solo_2_waves", 8, ("f64", "f32")),
          ("solo_3_waves", 16, ("f64", "f32"))]


@pytest.mark.parametrize("shape,dtype", [(s[0], d) for s in SHAPES for d in s[2]])
def test_every_launch_shape(shape, dtype):
    """Totals just above each threshold (2064, 4112, 8208 and - f32 - 16400 particles on 256 CUs): with the test above every
    twin instantiation has run."""
    simds = 4 * _torch().cuda.get_device_properties(0).multi_processor_count
    total = dict((s[0], s[1]) for s in SHAPES)[shape] * simds + 16
    _check_rollout_against_plain_launches(dtype, 2, total // 2, 2, 2)


def test_batch_rollout_against_the_oracle(ref_arm):
    """Two particles of every episode against the C restatement of the physics (f64, 1e-9)."""
    E, P, H = 3, 16, 4
    states = _states(E)
    means, noise, _, _ = _inputs(E, P, H, "f64", 3)
    eng = _engine("f64")
    eng.set_shard_states_raw([eng._unpack(s) for s in states])
    costs, acts, _ = _batch_rollout(eng, E, P, H, means, noise, None, None)         # (no filter: the noise as it is)
    assert eng.solver_failures() == 0
    eng.close()
    means_h, noise_h = means.cpu().numpy(), noise.cpu().numpy()
    for e in range(E):
        pick = [e * P + 3, e * P + 12]
        _, rew, act, _, _ = ref_arm.rollout(states[e]["qp"], states[e]["qv"], states[e]["target_pos"], means_h[e], noise_h[pick])
        assert np.array_equal(acts[pick], act)
        np.testing.assert_allclose(costs[pick], -rew, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_batched_env_step_equals_single_steps_with_a_reset(dtype):
    """One launch steps E real envs as ``mjmpc_arm_step_state`` steps E single-state engines - costs, observations, final
    states and env-reset counts - with a start state already beyond MuJoCo's 1e10 bound (the kernel's mj_resetData)."""
    torch = _torch()
    from mjmpc_amd import _lib
    E = 4
    states = _states(E)
    states[2]["qv"][3] = 3e10
    rng = np.random.RandomState(0)
    actions = [rng.uniform(-1, 1, (E, A)) for _ in range(3)]
    eng = _engine(dtype)
    eng.on_env_reset = "ignore"
    eng.set_shard_states_raw([eng._unpack(s) for s in states])
    tdt = torch.float32 if dtype == "f32" else torch.float64
    D = eng.d_obs
    b_cost, b_obs = [], []
    for a in actions:
        ad = torch.from_numpy(a).cuda()
        cost, obs = torch.empty(E, dtype=tdt, device="cuda"), torch.empty((E, D), dtype=tdt, device="cuda")
        _lib.check(eng._lib.mjmpc_arm_step_shard_states(eng._h, eng._code, _vp(ad), _vp(cost), _vp(obs), eng._stream()))
        torch.cuda.synchronize()
        b_cost.append(cost.cpu().numpy())
        b_obs.append(obs.cpu().numpy())
    qp, qv = eng.get_shard_states()
    batch_resets = eng.env_resets()
    eng.close()
    single_resets = 0
    for e in range(E):
        s = _engine(dtype)
        s.on_env_reset = "ignore"
        s.set_env_state(states[e])
        for k, a in enumerate(actions):
            cost, obs = s.step_state(a[e])
            torch.cuda.synchronize()
            assert np.array_equal(cost.cpu().numpy()[0], b_cost[k][e]), (dtype, e, k)
            assert np.array_equal(obs.cpu().numpy(), b_obs[k][e]), (dtype, e, k)
        st = s.get_state_device()
        assert np.array_equal(st["qp"], qp[e]) and np.array_equal(st["qv"], qv[e]), (dtype, e)
        single_resets += s.env_resets()
        s.close()
    assert single_resets >= 1 and batch_resets == single_resets, (dtype, batch_resets, single_resets)
    assert np.all(np.isfinite(qp)) and np.all(np.abs(qv) < 1e10)
    assert np.all(np.isfinite(np.array(b_cost)))


# ---------------------------------------------------------------------------------------------------------- the closed loop
E3 = 3
CASES = dict(
    BatchedMPPI=(bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), None),
                 (np.array([0.01, 0.05, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedCEM=(bc.case("BatchedCEM", "CEM", ("init_cov", "elite_frac", "step_size", "beta"), None, extra=("cov_action", "cov")),
                (np.array([1.0, 0.5, 0.3]), np.array([0.25, 0.125, 0.5]), np.array([1.0, 0.9, 0.8]), np.array([0.1, 0.2, 0.0]))),
    BatchedPFMPC=(bc.case("BatchedPFMPC", "PFMPC", ("cov_shift", "cov_resample", "lam"), None, gamma=0.99,
                          extra=("action_samples", "action_samples")),
                  (np.array([0.3, 0.2, 0.5]), np.array([0.1, 0.3, 0.2]), np.array([0.05, 0.2, 0.1]))),
    BatchedDMDMPC=(bc.case("BatchedDMDMPC", "DMDMPC", ("lam", "step_size", "init_cov", "beta"), None, extra=("cov_action", "cov")),
                   (np.array([0.05, 0.1, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]), np.array([0.1, 0.0, 0.2]))),
    BatchedRandomShooting=(bc.case("BatchedRandomShooting", "RandomShooting", ("step_size", "init_cov"), None),
                           (np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedMPPIQ=(bc.case("BatchedMPPIQ", "MPPIQ", ("beta", "step_size", "init_cov", "td_lam"), None),
                  (np.array([0.2, 0.1, 0.5]), np.array([1.0, 0.8, 0.5]), np.array([0.3, 0.2, 0.5]), np.array([0.9, 0.0, 1.0]))),
)


def _as_plain_launches(b):
    """Replace the batch's two engine-specific launches by their references: ``_rollout`` by E plain full-size
    ``mjmpc_arm_rollout_fused`` launches on a single-state engine (episode e's rows of launch e are kept), ``_env_step`` by
    ``set_state`` / ``mjmpc_arm_step_state`` / ``get_state`` per episode.  The sampler and the update launches stay the batch's
    own (the tree batches' tests hold them to the single-episode controllers)."""
    torch = _torch()
    from mjmpc_amd import _lib
    E, P, H = b.num_episodes, b.num_particles, b.horizon
    ref = _engine(b.dtype)
    ref.on_env_reset = "ignore"
    host = dict(states=None)

    def states():
        if host["states"] is None:
            qp, qv = b.engine.get_shard_states()
            host["states"] = [dict(qp=qp[e].copy(), qv=qv[e].copy(), target_pos=b._targets[e].copy()) for e in range(E)]
        return host["states"]

    def rollout(self, s, noise=None, filtered=True, gseq=True, q0=True):
        noise = self._noise if noise is None else noise
        c, a = torch.empty_like(self._costs), torch.empty_like(self._actions)
        q = torch.empty_like(self._q0) if q0 else None
        for e, st in enumerate(states()):
            ref.set_env_state(st)
            _lib.check(ref._lib.mjmpc_arm_rollout_fused(ref._h, ref._code, E * P, H, _vp(self._means[e]), _vp(noise),
                                                        _vp(self._coeffs) if filtered else None, _vp(self._gseq) if gseq else None,
                                                        _vp(c), _vp(a), _vp(q), s))
            rows = slice(e * P, (e + 1) * P)
            self._costs[rows].copy_(c[rows])
            self._actions[rows].copy_(a[rows])
            if q0:
                self._q0[rows].copy_(q[rows])

    def env_step(self, act, cost, nobs, s):
        new = []
        for e, st in enumerate(states()):
            ref.set_env_state(st)
            c, o = ref.step_state(act[e])
            cost[e:e + 1].copy_(c)
            nobs[e].copy_(o)
            after = ref.get_state_device()
            new.append(dict(qp=after["qp"], qv=after["qv"], target_pos=st["target_pos"]))
        host["states"] = new
        self.engine.set_shard_states_raw([self.engine._unpack(st) for st in new])

    b._rollout, b._env_step = types.MethodType(rollout, b), types.MethodType(env_step, b)
    return ref


@pytest.mark.parametrize("name,dtype", [(n, "f64") for n in sorted(CASES)] + [("BatchedMPPI", "f32")])
def test_closed_loop_equals_the_loop_of_plain_launches(name, dtype):
    case, hyper = CASES[name]
    P, H, T = 64, 8, 5
    seeds = [123 + i * 12345 for i in range(E3)]
    got = bc.run_batch(case, bc.make_batch(case, _raw(), _states(E3), seeds, P, H, hyper, dtype, engine="arm"), T)
    b = bc.make_batch(case, _raw(), _states(E3), seeds, P, H, hyper, dtype, engine="arm")
    ref = _as_plain_launches(b)
    want = bc.run_batch(case, b, T)
    assert ref.env_resets() == 0 and ref.solver_failures() == 0
    ref.close()
    assert np.all(np.isfinite(got["acts"])) and np.all(np.isfinite(got["costs"]))
    for k in ("acts", "costs", "nobs", "mean"):
        assert np.array_equal(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())
    if case.extra is not None:
        assert np.array_equal(got["extra"], want["extra"]), case.extra[1]
    for x, y in zip(got["state"], want["state"]):
        assert np.array_equal(x["qp"], y["qp"]) and np.array_equal(x["qv"], y["qv"]) and np.array_equal(x["target_pos"], y["target_pos"])
    assert not np.array_equal(got["acts"][:, 0], got["acts"][:, 1])         # (the episodes are different episodes)
    assert not np.array_equal(got["state"][0]["qp"], _states(1)[0]["qp"])    # (and their real envs have moved)


@pytest.mark.parametrize("name", ["BatchedMPPI", "BatchedCEM"])
def test_permuting_the_episodes_permutes_the_results(name):
    case = CASES[name][0]
    hyper = dict(BatchedMPPI=(np.array([0.01, 0.05, 0.2, 0.1]), np.array([1.0, 0.9, 0.8, 0.7]), np.array([1.0, 0.3, 0.4, 0.5])),
                 BatchedCEM=(np.array([1.0, 0.3, 0.4, 0.5]), np.array([0.25, 0.125, 0.5, 0.25]), np.array([1.0, 0.9, 0.8, 0.7]),
                             np.array([0.1, 0.2, 0.0, 0.3])))[name]
    perm = [2, 0, 3, 1]
    states, seeds, P, H, T = _states(4), [5, 6, 7, 8], 32, 8, 5

    def run(order):
        return bc.run_batch(case, bc.make_batch(case, _raw(), [states[k] for k in order], [seeds[k] for k in order], P, H,
                                                [v[order] for v in hyper], "f64", engine="arm"), T)
    base, got = run([0, 1, 2, 3]), run(perm)
    for k in ("acts", "costs", "nobs"):
        assert np.array_equal(got[k], base[k][:, perm]), k
    assert np.array_equal(got["mean"], base["mean"][perm])
    assert case.extra is None or np.array_equal(got["extra"], base["extra"][perm])
    for k, e in enumerate(perm):
        assert np.array_equal(got["state"][k]["qp"], base["state"][e]["qp"])
        assert np.array_equal(got["state"][k]["qv"], base["state"][e]["qv"])


def test_refusals_on_the_device():
    """Twelve particles per episode (a group would straddle two episodes) and an engine with two model blocks:
    MJMPC_E_BADARG with a message, before any launch."""
    torch = _torch()
    from mjmpc_amd import _lib
    E, H = 2, 2
    eng = _engine("f64")
    lib = eng._lib
    eng.set_shard_states_raw([eng._unpack(s) for s in _states(E)])
    means, noise, coeffs, gseq = _inputs(E, 16, H, "f64", 4)
    out = torch.zeros((E * 16, H), dtype=torch.float64, device="cuda")

    def launch(P_total):
        return lib.mjmpc_arm_rollout_fused_batch(eng._h, eng._code, P_total, H, _vp(means), _vp(noise), _vp(coeffs), None,
                                                 _vp(out), None, None, eng._stream())
    assert launch(24) == E_BADARG and b"multiple of 8" in lib.mjmpc_last_error()
    assert launch(17) == E_BADARG and len(lib.mjmpc_last_error()) > 0
    assert launch(32) == 0
    blobs = np.ascontiguousarray(np.stack([eng.model.blob, eng.model.blob]), np.float64)
    _lib.check(lib.mjmpc_arm_set_shard_models(eng._h, blobs.ctypes.data_as(_lib._dp), 2))
    assert launch(32) == E_BADARG and b"one model block" in lib.mjmpc_last_error()
    cost = torch.zeros(E, dtype=torch.float64, device="cuda")
    assert lib.mjmpc_arm_step_shard_states(eng._h, eng._code, _vp(means), _vp(cost), None, eng._stream()) == E_BADARG
    torch.cuda.synchronize()
    assert eng.env_resets() == 0
    eng.close()
    plain = _engine("f64")          # no state shards: the batch entry points require them, also for one episode
    assert plain._lib.mjmpc_arm_rollout_fused_batch(plain._h, plain._code, 16, H, _vp(means), _vp(noise), None, None, _vp(out),
                                                    None, None, plain._stream()) == E_BADARG
    qp = np.zeros((1, A))
    assert plain._lib.mjmpc_arm_get_shard_states(plain._h, qp.ctypes.data_as(_lib._dp), qp.ctypes.data_as(_lib._dp),
                                                 ctypes.c_void_p(0)) == E_BADARG
    plain.close()
