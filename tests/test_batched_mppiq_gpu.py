"""GPU: an MPPIQ episode batch (``BatchedMPPIQ``) reproduces E separate single-episode runs to the bit.

Kernel level: ``mjmpc_mppiq_update_batch`` on random arrays against the single sequence called on every row's slices -
``mjmpc_td_lambda_returns`` (no Q estimates), ``mjmpc_softmax_stats`` on the returns (``gamma_zero = 1``, ``alpha = 1``, no
covariance), ``mjmpc_softmax_combine`` (one record), ``mjmpc_step_tail`` - with ``np.array_equal``, and against
``oracle.controllers_ref.mppiq_update`` with the tolerances of
``test_controllers_gpu.py::test_mppiq_matches_oracle_at_larger_size_and_f32``.

Closed loop: the single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``MPPIQ(...,
noise_mode='device', noise_dtype=dtype, seed=seed_e)`` and ``make_device_rollout_fn(engine)`` - captured with
``enable_graph(post_step=engine.step_state)`` for ``alpha = 1`` (``batched_cases.single``), eager for ``alpha = 0`` (``_eager``:
that path uploads ``cov^-1`` per update and cannot be captured).  Every comparison is ``np.array_equal``: the actions, real-env
costs and next observations of every step, the final mean and the final state.
"""
import ctypes
import os

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, ROOT, _cheetah_states, _torch, _vp
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu

HYPER = ("beta", "step_size", "init_cov", "td_lam")


def _runs_the_captured_general_step(c):
    # draw + filter, plain rollout, MPPIQ._device_update, step_tail - captured; not the fused MPPI step, not q0 from the rollout
    assert c._graph_capable() and not c._host_uploads_per_step() and c._static_cov()
    assert not c._fused_capable() and not c._wants_q0() and not c._cem_fused()


MPPIQ1 = bc.case("BatchedMPPIQ", "MPPIQ", HYPER, lambda dtype: dict(alpha=1, time_based_weights=True, noise_dtype=dtype),
                 before=_runs_the_captured_general_step)

SEEDS = [123 + i * 12345 for i in range(3)]
BETA, STEP, COV, TDL = np.array([0.2, 0.1, 0.5]), np.array([1.0, 0.8, 0.5]), np.array([0.3, 0.2, 0.5]), np.array([0.9, 0.0, 1.0])
P, H, T = 48, 8, 3


def _keys(E):
    return [("half_cheetah", i) for i in range(E)]


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
_KERNEL = {}


def _kernel_case(E, P, H, A, tbw, alpha, dtype, shift_mode=0, inf_particle=True):
    """The batch launch and the single sequence per row on the same random arrays (made once per setting, shared, read-only)
    -> dict of the inputs (host), and per side the shifted means, the actions and the step counter."""
    key = (E, P, H, A, tbw, alpha, dtype, shift_mode, inf_particle)
    if key in _KERNEL:
        return _KERNEL[key]
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    code = _lib.F32 if dtype == "f32" else _lib.F64
    npt = np.float32 if dtype == "f32" else np.float64
    rs = np.random.RandomState(8)
    beta, step, td_lam = np.array([0.4, 0.15, 1.0])[:E], np.array([0.8, 1.0, 0.3])[:E], np.array([0.85, 0.0, 1.0])[:E]
    init_cov, gamma = np.array([0.9, 0.5, 1.3])[:E], 0.97
    # (the ranges of test_mppiq_matches_oracle_at_larger_size_and_f32)
    means0 = 0.2 * rs.randn(E, H, A)
    actions = (means0[:, None] + 0.5 * rs.randn(E, P, H, A)).astype(npt)
    costs = (rs.rand(E, P, H) * 2).astype(npt)
    if inf_particle:
        costs[1, 5, :] = np.inf             # a rollout of episode 1 that diverged at its first step
    wseq = np.stack([np.cumprod([1.0] + [gamma * l] * (H - 2)) if H > 1 else np.array([1.0]) for l in td_lam])
    wzero = np.array([int(bool(np.any(w == 0))) for w in wseq], np.int32)
    covinv = np.stack([np.linalg.inv(np.diag(np.full(A, c))) for c in init_cov])

    dev = "cuda"
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_costs, d_act, d_beta, d_step, d_tdl, d_wseq, d_wz, d_cinv = (d(x) for x in (costs, actions, beta, step, td_lam, wseq, wzero,
                                                                                  covinv))
    step0 = 3
    # -- the batch
    b_means, b_out = d(means0), torch.zeros((E, A), dtype=torch.float64, device=dev)
    b_counter = torch.full((1,), step0, dtype=torch.int64, device=dev)
    nbytes = lib.mjmpc_mppiq_batch_workspace_bytes(E, P, H, A, tbw)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    _lib.check(lib.mjmpc_mppiq_update_batch(code, E, P, H, A, _vp(d_costs), _vp(d_act), _vp(d_beta), _vp(d_step), _vp(d_tdl),
                                            _vp(d_wseq), _vp(d_wz), gamma, alpha, _vp(d_cinv) if alpha == 0 else None, tbw,
                                            shift_mode, _vp(b_means), _vp(b_out), _vp(b_counter), _vp(ws), s))
    torch.cuda.synchronize()
    # -- the single sequence on every row's slices
    s_means, s_out = d(means0), torch.zeros((E, A), dtype=torch.float64, device=dev)
    s_counter = torch.full((1,), step0, dtype=torch.int64, device=dev)
    ws1 = torch.empty((lib.mjmpc_update_workspace_bytes(P, H, A) + 7) // 8, dtype=torch.float64, device=dev)
    rec = torch.empty(lib.mjmpc_softmax_record_len(H, A, tbw), dtype=torch.float64, device=dev)
    ret = torch.empty((P, H), dtype=d_costs.dtype, device=dev)
    gseq = torch.ones(H, dtype=torch.float64, device=dev)                  # (not read: gamma_zero = 1)
    for e in range(E):
        _lib.check(lib.mjmpc_td_lambda_returns(code, P, H, A, _vp(d_costs[e]), _vp(d_act[e]), None, _vp(s_means[e]),
                                               _vp(d_cinv[e]), _vp(d_wseq[e]), int(wzero[e]), float(beta[e]), alpha, gamma,
                                               float(td_lam[e]), _vp(ret), _vp(ws1), s))
        _lib.check(lib.mjmpc_softmax_stats(code, P, H, A, _vp(ret), _vp(d_act[e]), _vp(s_means[e]), _vp(d_cinv[e]), _vp(gseq), 1,
                                           float(beta[e]), 1, tbw, 0, _vp(rec), _vp(ws1), s))
        _lib.check(lib.mjmpc_softmax_combine(_vp(rec), 1, H, A, tbw, float(beta[e]), float(step[e]), 0, float(P), _vp(s_means[e]),
                                             None, None, None, s))
        _lib.check(lib.mjmpc_step_tail(_vp(s_means[e]), H, A, shift_mode, None, _vp(s_out[e]), None,
                                       _vp(s_counter) if e == 0 else None, None, None, 0.0, s))
    torch.cuda.synchronize()
    out = dict(means0=means0, actions=actions, costs=costs, beta=beta, step=step, td_lam=td_lam, init_cov=init_cov, gamma=gamma,
               step0=step0, batch=(b_means.cpu().numpy(), b_out.cpu().numpy(), int(b_counter.item())),
               single=(s_means.cpu().numpy(), s_out.cpu().numpy(), int(s_counter.item())),
               inputs_untouched=np.array_equal(d_costs.cpu().numpy(), costs, equal_nan=True)
               and np.array_equal(d_act.cpu().numpy(), actions))
    _KERNEL[key] = out
    return out


KERNEL_SHAPE = (3, 1040, 5, 3)         # 65 chunks of 16 (the merge's lane loop wraps), a ragged particle loop, H != A, both odd


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("tbw", [0, 1])
@pytest.mark.parametrize("shift_mode", [0, 1])
def test_update_launch_equals_the_single_sequence(shift_mode, tbw, alpha, dtype):
    """(a) the means, actions, shifted means and step counter of row e are the bits of the single sequence on row e's slices."""
    r = _kernel_case(*KERNEL_SHAPE, tbw, alpha, dtype, shift_mode)
    (bm, bo, bc_), (sm, so, sc) = r["batch"], r["single"]
    assert np.all(np.isfinite(sm)) and np.all(np.isfinite(so))
    for e in range(KERNEL_SHAPE[0]):
        assert np.array_equal(bo[e], so[e]), "row %d: actions differ (max %.3g)" % (e, np.abs(bo[e] - so[e]).max())
        assert np.array_equal(bm[e], sm[e]), "row %d: shifted means differ (max %.3g)" % (e, np.abs(bm[e] - sm[e]).max())
    assert bc_ == sc == r["step0"] + 1                          # advanced once, by row 0
    assert r["inputs_untouched"]
    assert not np.array_equal(bo[0], bo[1]) and not np.array_equal(bo[1], bo[2])


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 2e-5)])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("tbw", [0, 1])
def test_update_launch_matches_the_oracle(tbw, alpha, dtype, tol):
    """(b) the updated mean before the shift (``shift_mode = 0``: the action, then the shifted rows) against
    ``controllers_ref.mppiq_update(..., qvals=None, ...)``.  Particle 5 of episode 1 carries +inf costs at every step (a rollout
    that diverged at once): its weight is zero in every column, which is the oracle WITHOUT that particle - the oracle itself
    turns ``td_lam * inf`` into NaN for ``td_lam = 0``, episode 1's.  (One +inf step alone would leave that particle's other
    weight columns finite with ``td_lam = 0``: the returns pass through step by step.)"""
    from oracle import controllers_ref as cr
    E, P, H, A = KERNEL_SHAPE
    r = _kernel_case(E, P, H, A, tbw, alpha, dtype, 0)
    bm, bo, _ = r["batch"]
    assert np.all(np.isfinite(bm)) and np.all(np.isfinite(bo))
    for e in range(E):
        updated = np.concatenate([bo[e][None], bm[e][:H - 1]], axis=0)
        assert not bm[e][H - 1].any()                            # ('null': the new last row)
        keep = np.ones(P, bool)
        if e == 1:
            keep[5] = False
        want = cr.mppiq_update(r["costs"][e][keep].astype(np.float64), r["actions"][e][keep].astype(np.float64), None,
                               r["means0"][e], r["init_cov"][e] * np.eye(A), r["beta"][e], alpha, r["gamma"], r["td_lam"][e],
                               r["step"][e], bool(tbw))
        assert np.all(np.isfinite(want))
        err = np.abs(updated - want).max()
        print("episode %d: max |mean - oracle| = %.3g (tolerance %g)" % (e, err, tol))
        np.testing.assert_allclose(updated, want, rtol=tol, atol=tol)


@pytest.mark.parametrize("dtype,tol", [("f64", 1e-12), ("f32", 2e-5)])
@pytest.mark.parametrize("alpha", [0, 1])
@pytest.mark.parametrize("tbw", [0, 1])
def test_horizon_of_one(tbw, alpha, dtype, tol):
    """(c) H = 1, P = 17, A = 2, E = 2: the returns are the total cost, the table is [1.0], one partial chunk is ragged."""
    from oracle import controllers_ref as cr
    E, P, H, A = 2, 17, 1, 2
    r = _kernel_case(E, P, H, A, tbw, alpha, dtype, 0, inf_particle=False)
    (bm, bo, bc_), (sm, so, sc) = r["batch"], r["single"]
    assert np.array_equal(bm, sm) and np.array_equal(bo, so) and bc_ == sc == r["step0"] + 1
    assert np.all(np.isfinite(bo)) and not bm.any()             # (the shifted horizon of one step is the 'null' row)
    for e in range(E):
        want = cr.mppiq_update(r["costs"][e].astype(np.float64), r["actions"][e].astype(np.float64), None, r["means0"][e],
                               r["init_cov"][e] * np.eye(A), r["beta"][e], alpha, r["gamma"], r["td_lam"][e], r["step"][e],
                               bool(tbw))
        np.testing.assert_allclose(bo[e][None], want, rtol=tol, atol=tol)


# ---------------------------------------------------------------------------------------------------------- closed loop
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_captured_single_episodes(dtype):
    """E = 3, P = 48 (three chunks), H = 8, T = 3; alpha = 1, a softmax per horizon step, per-episode hyperparameters (a td_lam
    of 0 and of 1 among them)."""
    E = 3
    out = bc.check_against_singles(MPPIQ1, _cheetah(), _cheetah_states(E), SEEDS, P, H, T, (BETA, STEP, COV, TDL), dtype,
                                   keys=_keys(E))
    acts = out["acts"]
    assert not np.array_equal(acts[:, 0], acts[:, 1]) and not np.array_equal(acts[:, 1], acts[:, 2])


def _eager(raw, state, seed, hyper, dtype, alpha, tbw, base_action="null"):
    """One episode on the EAGER single-episode device path (what ``batched_cases.single`` cannot express: ``MPPIQ(alpha=0)``
    uploads ``cov^-1`` per update and is not captured): per step ``optimize(None)``, then ``engine.step_state`` with the action
    uploaded as float64 -> the dict ``batched_cases.single`` returns."""
    torch = _torch()
    from mjmpc_amd.control import MPPIQ
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    eng = TreeRolloutEngine(raw, dtype=dtype)
    eng.set_env_state(dict(state))
    c = MPPIQ(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, base_action=base_action, num_particles=P,
              gamma=1.0, n_iters=1, action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed,
              noise_mode="device", noise_dtype=dtype, alpha=alpha, time_based_weights=tbw, **dict(zip(HYPER, hyper)))
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    assert not c._graph_on and (alpha == 1 or not c._graph_capable())
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize(None)
        a = np.array(a, np.float64)
        eng.step_state(torch.from_numpy(a.copy()).to("cuda"))
        torch.cuda.synchronize()
        acts.append(a)
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), mean=np.array(c.mean_action),
               state=eng.get_state_device())
    assert eng.env_resets() == 0, "the single path's real env reset"
    eng.close()
    return out


def test_control_cost_batch_equals_eager_single_episodes():
    """alpha = 0 (the control cost with cov^-1 = diag(1 / init_cov_e)), one weight per particle, f64, E = 2."""
    E = 2
    hyper = (BETA[:E], STEP[:E], COV[:E], np.array([0.9, 1.0]))
    raw, states = _cheetah(), _cheetah_states(E)
    out = bc.batch(MPPIQ1, raw, states, SEEDS[:E], P, H, T, hyper, "f64", alpha=0, time_based_weights=False)
    assert np.all(np.isfinite(out["acts"])) and np.all(np.isfinite(out["costs"]))
    for e in range(E):
        one = _eager(raw, states[e], SEEDS[e], [v[e] for v in hyper], "f64", 0, False)
        assert np.all(np.isfinite(one["acts"])) and np.all(np.isfinite(one["costs"]))
        assert np.array_equal(out["acts"][:, e], one["acts"]), \
            "episode %d: actions differ (max %.3g)" % (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), "episode %d: real-env costs differ" % e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), "episode %d: next observations differ" % e
        assert np.array_equal(out["mean"][e], one["mean"]), "episode %d: final mean differs" % e
        for x, y in zip(bc._qpos_qvel(out["state"][e]), bc._qpos_qvel(one["state"])):
            assert np.array_equal(x, y), "episode %d: final state differs" % e
    assert not np.array_equal(out["acts"][:, 0], out["acts"][:, 1])


def test_permuting_the_episodes_permutes_the_results():
    bc.check_permutation(MPPIQ1, _cheetah(), _cheetah_states(3), SEEDS, P, H, T, (BETA, STEP, COV, TDL), "f64", [2, 0, 1])


def test_one_episode():
    bc.check_against_singles(MPPIQ1, _cheetah(), _cheetah_states(1), SEEDS[:1], P, H, T, (BETA[0], STEP[0], COV[0], TDL[0]),
                             "f64", keys=_keys(1))


def test_base_action_repeat():
    E = 2
    bc.check_against_singles(MPPIQ1, _cheetah(), _cheetah_states(E), SEEDS[:E], P, H, T, (0.2, 0.8, 0.3, 0.9), "f64",
                             base_action="repeat", keys=_keys(E))


def test_randomized_dynamics_two_shards():
    """K = 2 shards of 24 particles roll out their own model blocks (the parameters of
    examples/configs/half_cheetah_gpu_dyn_randomize.yml); the real envs stay nominal."""
    import yaml
    with open(os.path.join(ROOT, "examples", "configs", "half_cheetah_gpu_dyn_randomize.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) == {"body_mass", "dof_damping", "geom_friction"}
    E = 2
    bc.check_against_singles(MPPIQ1, _cheetah(), _cheetah_states(E), SEEDS[:E], P, H, T, (0.2, 0.8, 0.3, 0.9), "f64", K=2, cfg=cfg,
                             dyn_seed=5)


def test_reset_and_set_states_reproduce_the_run():
    """Two steps, then ``reset()`` and ``set_states``, then the same two steps: the same actions, costs, observations, mean."""
    E = 2
    states = _cheetah_states(E)
    b = bc.make_batch(MPPIQ1, _cheetah(), states, SEEDS[:E], P, H, (BETA[:E], STEP[:E], COV[:E], TDL[:E]), "f64")
    first = b.run(2)
    mean1 = b.mean_action
    assert b.num_steps == 2 and np.any(mean1 != 0)
    b.reset()
    assert b.num_steps == 0 and not b.mean_action.any()
    b.set_states([dict(s) for s in states])
    second = b.run(2)
    mean2 = b.mean_action
    assert b.engine.env_resets() == 0
    b.close()
    for x, y in zip(first, second):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    assert np.array_equal(mean1, mean2)
