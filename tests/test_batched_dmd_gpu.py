"""GPU: a DMD-MPC episode batch (``BatchedDMDMPC``) reproduces E separate single-episode runs to the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``DMDMPC(..., update_cov=True,
cov_type=..., noise_mode='device', noise_dtype=dtype, seed=seed_e)``, ``make_device_rollout_fn(engine)``,
``enable_graph(post_step=engine.step_state)``, whose iteration is the general branch of ``OLGaussianMPC._device_iteration`` -
``mjmpc_cholesky_lower`` + ``mjmpc_sample_noise``, the plain rollout, ``mjmpc_softmax_stats`` + ``mjmpc_softmax_combine``,
``mjmpc_step_tail`` - and steps the engine's device-resident real env; every test asserts that it did NOT take a fused branch.
Every comparison is ``np.array_equal``: the actions, real-env costs and next observations of every step, the final mean, the
final covariance and the final state.  No real env may reset (``mjmpc_tree_env_resets`` == 0 on both sides) and every action
and cost is finite, so that two all-``inf`` runs cannot pass for equal.  The C-ABI tests compare rows of the batch entry
points with the single entry points on the row slices, on synthetic inputs and without a rollout.
"""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, _cheetah_states, _per, _torch, _vp
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu


def _is_the_general_step(c):
    assert not c._fused_capable() and c._device_cov(), "the single path is not the general covariance-adapting step"


def _took_no_fused_branch(c):
    assert not c._fused_capable() and c._device_cov() and not c._cem_fused() and not c._mono


DMD = bc.case("BatchedDMDMPC", "DMDMPC", ("lam", "step_size", "init_cov", "beta"),
              lambda dtype: dict(update_cov=True, noise_dtype=dtype), before=_is_the_general_step, during=_took_no_fused_branch,
              extra=("cov_action", "cov"))


def _make_batch(raw, states, seeds, P, H, lam, step_size, init_cov, beta, dtype, cov_type="full", **kw):
    return bc.make_batch(DMD, raw, states, seeds, P, H, (lam, step_size, init_cov, beta), dtype, cov_type=cov_type, **kw)


def _check_against_singles(raw, states, seeds, P, H, T, lam, step_size, init_cov, beta, dtype, cov_type="full", **kw):
    E = len(states)
    out = bc.check_against_singles(DMD, raw, states, seeds, P, H, T, (lam, step_size, init_cov, beta), dtype, cov_type=cov_type,
                                   **kw)
    acts, covs = out["acts"], out["extra"]
    A = acts.shape[2]
    assert covs.shape == (E, A, A) and np.all(np.isfinite(covs))
    for e in range(E):
        # adaptation happened: the final covariance is not the initial one
        assert not np.array_equal(covs[e], np.diag(np.full(A, _per(init_cov, e)))), "episode %d: covariance never moved" % e
        if cov_type == "full" and A > 1:
            assert np.count_nonzero(covs[e] - np.diag(np.diag(covs[e]))) > 0, "episode %d: no off-diagonal entries" % e
        else:
            assert np.count_nonzero(covs[e] - np.diag(np.diag(covs[e]))) == 0
    if E > 1:
        assert not np.array_equal(acts[:, 0], acts[:, 1])           # (the episodes are different episodes)
    return acts, out["costs"], covs


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cov_type", ["full", "diagonal"])
def test_half_cheetah_batch_equals_single_episodes(cov_type, dtype):
    """E = 3, P = 64, H = 8, T = 6: from step 2 on a covariance re-estimated from the weighted samples colours the draw."""
    E = 3
    _check_against_singles(_cheetah(), _cheetah_states(E), [123 + i * 12345 for i in range(E)], 64, 8, 6, 0.2, 1.0, 0.3, 0.05,
                           dtype, cov_type=cov_type)


def test_per_episode_hyperparameters():
    """Different lam, step_size (0.7 and 0.5: the old covariance enters the blend), beta (one of them 0) and init_cov."""
    E = 3
    _check_against_singles(_cheetah(), _cheetah_states(E), [7, 10, 13], 64, 8, 6, np.array([0.1, 0.2, 0.5]),
                           np.array([0.7, 1.0, 0.5]), np.array([0.2, 0.3, 0.5]), np.array([0.05, 0.0, 0.2]), "f64")


def test_particles_not_a_multiple_of_the_chunk():
    """P = 50: a row's last partial holds 2 particles and ends where the next row's particles begin."""
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 50, 8, 6, 0.2, 1.0, 0.3, 0.05, "f64")


def test_one_episode_and_permuted_episodes():
    raw = _cheetah()
    _check_against_singles(raw, _cheetah_states(1), [123], 64, 8, 6, 0.2, 1.0, 0.3, 0.05, "f64")
    lam, step, cov, beta = np.array([0.1, 0.2, 0.4]), np.array([1.0, 0.9, 0.8]), np.array([0.2, 0.3, 0.4]), np.array([0.05, 0.1, 0.0])
    bc.check_permutation(DMD, raw, _cheetah_states(3), [5, 6, 7], 64, 8, 6, (lam, step, cov, beta), "f64", [2, 0, 1])


def test_base_action_repeat():
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 64, 8, 6, 0.2, 0.9, 0.3, 0.05, "f64",
                           base_action="repeat")


def test_rk4_double_pendulum():
    """A non-HalfCheetah instantiation of the rollout kernel (RK4) with one actuator: A = 1, a 1 x 1 covariance."""
    raw, states = bc.synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    _check_against_singles(raw, states, [21, 22], 32, 6, 4, 0.2, 1.0, 0.3, 0.05, "f64")


def test_randomized_dynamics_two_shards():
    """K = 2 shards of 24 particles roll out their own model blocks; the real envs stay nominal."""
    cfg = {"body_mass": {"torso": [0.3, 0.1], "ffoot": [0.5, 0.0]}, "dof_damping": {"bshin": [0.4, 0.2]},
           "geom_friction": {"bfoot": [0.5, 0.5]}}
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 48, 8, 6, 0.2, 1.0, 0.3, 0.05, "f64",
                           K=2, cfg=cfg, dyn_seed=[3, 4])


def test_reset_reproduces_the_first_run():
    E, T = 2, 4
    states = _cheetah_states(E)
    b = _make_batch(_cheetah(), states, [123, 12468], 64, 8, 0.2, 0.8, 0.3, 0.05, "f64")
    first = b.run(T)
    mean1, cov1 = b.mean_action, b.cov
    assert not np.array_equal(cov1[0], np.diag(np.full(6, 0.3))) and b.num_steps == T
    b.reset()
    assert b.num_steps == 0 and not b.mean_action.any()
    assert np.array_equal(b.cov, np.stack([np.diag(np.full(6, 0.3))] * E))
    b.set_states([dict(s) for s in states])
    second = b.run(T)
    for x, y in zip(first, second):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y)
    assert np.array_equal(b.mean_action, mean1) and np.array_equal(b.cov, cov1)
    assert b.engine.env_resets() == 0
    b.close()


def test_batched_dmdmpc_reports_the_indefinite_episode_once():
    from mjmpc_amd import _lib
    torch = _torch()
    E = 3
    b = _make_batch(_cheetah(), _cheetah_states(E), [1, 2, 3], 64, 8, 0.2, [1.0, 0.0, 1.0], 0.3, 0.0, "f64")
    bad = np.diag(np.full(6, 0.3))
    bad[2, 2] = -1.0
    b._covs[1].copy_(torch.from_numpy(bad))                     # step_size 0 and beta 0: the update keeps this covariance
    with pytest.raises(_lib.MjmpcError, match=r"episode 1\b"):
        b.run(1)
    assert np.array_equal(b.cov[1], bad)                        # reported once: the flag was cleared, nothing ran since
    b.mean_action
    b.get_states()
    b.close()


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
def _dev(a, t=None):
    x = _torch().from_numpy(np.ascontiguousarray(a)).to("cuda")
    return x if t is None else x.to(t)


def _spd(rng, A, scale):
    m = rng.uniform(-1, 1, (A, A))
    return scale * (m @ m.T / A + 0.5 * np.eye(A))


_UPDATE = {}


def _update_case(P, H, A, shift_mode, cov_mode, dtype, nan_row=None):
    """E = 3 rows of ``mjmpc_dmd_update_batch`` and the three single calls (``mjmpc_softmax_stats``, ``mjmpc_softmax_combine``,
    ``mjmpc_step_tail``) on the row slices, on synthetic costs (one of them +inf) and actions.  Computed once per case."""
    key = (P, H, A, shift_mode, cov_mode, dtype, nan_row)
    if key in _UPDATE:
        return _UPDATE[key]
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, step0 = 3, 7
    code = _lib.F32 if dtype == "f32" else _lib.F64
    tdt = torch.float32 if dtype == "f32" else torch.float64
    rng = np.random.RandomState(P + 10 * H + 100 * A)
    costs = rng.uniform(0.0, 2.0, (E, P, H))
    costs[0, 3, H - 1] = np.inf                                 # (a rollout that diverged: zero weight)
    actions = rng.uniform(-1, 1, (E, P, H, A))
    means0 = rng.uniform(-0.2, 0.2, (E, H, A))
    covs0 = np.stack([_spd(rng, A, c) for c in (0.3, 0.2, 0.5)])
    lam, step, beta = np.array([0.2, 1.0, 0.05]), np.array([1.0, 0.7, 0.5]), np.array([0.05, 0.0, 0.3])
    gseq = np.cumprod([1.0] + [0.97] * (H - 1))
    if nan_row is not None:
        costs[nan_row], actions[nan_row], means0[nan_row], covs0[nan_row] = np.nan, np.nan, np.nan, np.nan
        lam[nan_row] = step[nan_row] = beta[nan_row] = np.nan
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_costs, d_act, d_gseq = _dev(costs, tdt), _dev(actions, tdt), _dev(gseq)
    # -- the batch
    b = dict(means=_dev(means0), covs=_dev(covs0), out=torch.zeros((E, A), dtype=torch.float64, device="cuda"),
             counter=torch.full((1,), step0, dtype=torch.int64, device="cuda"))
    nbytes = lib.mjmpc_dmd_batch_workspace_bytes(E, P, H, A)
    assert nbytes > 0
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device="cuda")
    d_lam, d_stepsz, d_beta = _dev(lam), _dev(step), _dev(beta)
    _lib.check(lib.mjmpc_dmd_update_batch(code, E, P, H, A, _vp(d_costs), _vp(d_act), _vp(d_gseq), _vp(d_lam), _vp(d_stepsz),
                                          cov_mode, _vp(d_beta), shift_mode, _vp(b["means"]), _vp(b["covs"]), _vp(b["out"]),
                                          _vp(b["counter"]), _vp(ws), s))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in b.items()}
    # -- three single calls on the row slices
    ref = dict(means=[], covs=[], out=[])
    ws1 = torch.zeros((lib.mjmpc_update_workspace_bytes(P, H, A) + 7) // 8, dtype=torch.float64, device="cuda")
    rec = torch.zeros(lib.mjmpc_softmax_record_len(H, A, 0), dtype=torch.float64, device="cuda")
    wnorm = torch.zeros(2, dtype=torch.float64, device="cuda")
    for e in range(E):
        if e == nan_row:            # (mjmpc_softmax_stats refuses a lam that is not positive: the row has no single result)
            for k, shape in (("means", (H, A)), ("covs", (A, A)), ("out", (A,))):
                ref[k].append(np.full(shape, np.nan))
            continue
        mean, cov = _dev(means0[e]), _dev(covs0[e])
        out = torch.zeros(A, dtype=torch.float64, device="cuda")
        counter = torch.full((1,), step0, dtype=torch.int64, device="cuda")
        _lib.check(lib.mjmpc_softmax_stats(code, P, H, A, _vp(d_costs[e]), _vp(d_act[e]), _vp(mean), None, _vp(d_gseq), 0,
                                           float(lam[e]), 1, 0, 1, _vp(rec), _vp(ws1), s))
        _lib.check(lib.mjmpc_softmax_combine(_vp(rec), 1, H, A, 0, float(lam[e]), float(step[e]), cov_mode, float(P), _vp(mean),
                                             _vp(cov), None, _vp(wnorm), s))
        _lib.check(lib.mjmpc_step_tail(_vp(mean), H, A, shift_mode, None, _vp(out), None, _vp(counter), _vp(cov), None,
                                       float(beta[e]), s))
        torch.cuda.synchronize()
        assert int(counter.item()) == step0 + 1
        for k, v in (("means", mean), ("covs", cov), ("out", out)):
            ref[k].append(v.cpu().numpy())
    assert int(got["counter"][0]) == step0 + 1                  # advanced once, by row 0: 7 -> 8, not 7 + E
    _UPDATE[key] = got, {k: np.stack(v) for k, v in ref.items()}, means0, covs0
    return _UPDATE[key]


# P = 50: a last chunk of 2 of 16; P = 1043: 66 partials, wave_entry_sum's lane-strided loop runs twice
_UPDATE_SHAPES = [(50, 7, 6, 0), (1043, 7, 9, 0), (50, 1, 1, 1), (50, 7, 6, 1)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cov_mode", [2, 1])
@pytest.mark.parametrize("shape", _UPDATE_SHAPES, ids=lambda s: "P%d-H%d-A%d-%s" % (s[0], s[1], s[2], ("null", "repeat")[s[3]]))
def test_update_rows_equal_single_calls(shape, cov_mode, dtype):
    P, H, A, shift_mode = shape
    got, ref, means0, covs0 = _update_case(P, H, A, shift_mode, cov_mode, dtype)
    for k in ("means", "covs", "out"):
        assert np.all(np.isfinite(got[k])), k
        assert np.array_equal(got[k], ref[k]), "%s differ (max %.3g)" % (k, np.abs(got[k] - ref[k]).max())
    assert not np.array_equal(got["out"][0], got["out"][1]) and np.abs(got["out"]).max() > 0
    # the shift: rows move up, the last row is 0 ('null') or the row that was last ('repeat'; H = 1: the action)
    last = got["means"][:, H - 1]
    if shift_mode == 0:
        assert not last.any()
    else:
        assert np.array_equal(last, got["means"][:, H - 2] if H >= 2 else got["out"])
    for e in range(3):
        off = got["covs"][e] - np.diag(np.diag(got["covs"][e]))
        if cov_mode == 2 and A > 1:
            assert np.count_nonzero(off) > 0
        # cov_mode 1 with step_size < 1 keeps (1 - step) of the old off-diagonal entries; with step_size 1 none is left
        if cov_mode == 1 and e == 0:
            assert np.count_nonzero(off) == 0


def test_update_rows_are_isolated_from_a_nan_row():
    """Row 1's costs, actions, mean, covariance and hyperparameters are NaN: rows 0 and 2 still equal their single results."""
    got, ref, _, _ = _update_case(50, 7, 6, 0, 2, "f64", nan_row=1)
    clean, _, _, _ = _update_case(50, 7, 6, 0, 2, "f64")
    for e in (0, 2):
        for k in ("means", "covs", "out"):
            assert np.all(np.isfinite(got[k][e])), (k, e)
            assert np.array_equal(got[k][e], ref[k][e]), (k, e)
            assert np.array_equal(got[k][e], clean[k][e]), (k, e)
    assert np.all(np.isnan(got["out"][1]))


def _draw_case(H, A, kind, filt, dtype, bad_row=None):
    """E = 3 rows of ``mjmpc_cholesky_lower_batch`` + ``mjmpc_sample_noise_cov_batch`` and ``mjmpc_cholesky_lower`` +
    ``mjmpc_sample_noise`` on the row slices: P = 50, seeds beyond 2^63, the step counter at 5."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, P = 3, 50
    code = _lib.F32 if dtype == "f32" else _lib.F64
    tdt = torch.float32 if dtype == "f32" else torch.float64
    rng = np.random.RandomState(H + 10 * A)
    if kind == "general":
        covs = np.stack([_spd(rng, A, c) for c in (0.3, 0.2, 0.5)])
    else:
        covs = np.stack([np.diag(rng.uniform(0.1, 0.6, A)) for _ in range(E)])
    if bad_row is not None:
        covs[bad_row, A // 2, A // 2] = -1.0
    diag = int(kind == "diagonal")
    seeds = np.array([2 ** 63 + 9, 11, 2 ** 64 - 3], np.uint64)
    identity = list(filt) == [1.0, 0.0, 0.0]
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_covs, d_coeffs, d_step = _dev(covs), _dev(np.array(filt, np.float64)), _dev(np.array([5], np.int64))
    chols = torch.zeros((E, A, A), dtype=torch.float64, device="cuda")
    status = torch.zeros(E, dtype=torch.int32, device="cuda")
    noise = torch.zeros((E, P, H, A), dtype=tdt, device="cuda")
    _lib.check(lib.mjmpc_cholesky_lower_batch(E, _vp(d_covs), A, _vp(chols), _vp(status), s))
    # (an identity filter: the batch class hands NULL - no filter launch -, the single path its coefficients)
    d_seeds = _dev(seeds.view(np.int64))
    _lib.check(lib.mjmpc_sample_noise_cov_batch(code, E, _vp(noise), P, H, A, _vp(chols), None if identity else _vp(d_coeffs),
                                                _vp(d_seeds), 0, _vp(d_step), diag, s))
    torch.cuda.synchronize()
    got = dict(chols=chols.cpu().numpy(), status=status.cpu().numpy(), noise=noise.cpu().numpy())
    ref = dict(chols=[], status=[], noise=[])
    for e in range(E):
        chol = torch.zeros((A, A), dtype=torch.float64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.zeros((P, H, A), dtype=tdt, device="cuda")
        _lib.check(lib.mjmpc_cholesky_lower(_vp(d_covs[e]), A, _vp(chol), _vp(st), s))
        _lib.check(lib.mjmpc_sample_noise(code, _vp(out), P, H, A, _vp(chol), _vp(d_coeffs), int(seeds[e]), 0, 0, _vp(d_step), diag, s))
        torch.cuda.synchronize()
        for k, v in (("chols", chol), ("status", st), ("noise", out)):
            ref[k].append(v.cpu().numpy())
    # the flags are sticky and per row: factoring good covariances afterwards leaves them as they are
    good = _dev(np.stack([np.eye(A)] * E))
    _lib.check(lib.mjmpc_cholesky_lower_batch(E, _vp(good), A, _vp(chols), _vp(status), s))
    torch.cuda.synchronize()
    got["status_after"] = status.cpu().numpy()
    return got, {k: np.stack(v) for k, v in ref.items()}


# A = 6, H = 8: noise_full_kernel's staged store; H = 6: its direct store; A = 9: the per-element kernel
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("filt", [[1.0, 0.0, 0.0], FILT], ids=["identity", "filtered"])
@pytest.mark.parametrize("kind", ["general", "diagonal"])
@pytest.mark.parametrize("shape", [(8, 6), (6, 6), (7, 9)], ids=lambda s: "H%d-A%d" % s)
def test_draw_rows_equal_single_calls(shape, kind, filt, dtype):
    H, A = shape
    got, ref = _draw_case(H, A, kind, filt, dtype)
    assert not got["status"].any() and not ref["status"].any() and not got["status_after"].any()
    assert np.all(np.isfinite(got["noise"])) and np.abs(got["noise"]).max() > 0
    assert np.array_equal(got["chols"], ref["chols"])
    assert np.array_equal(got["noise"], ref["noise"])
    assert not np.array_equal(got["noise"][0], got["noise"][1])
    if kind == "general":
        assert np.count_nonzero(np.tril(got["chols"][0], -1)) > 0


@pytest.mark.parametrize("shape", [(8, 6), (7, 9)], ids=lambda s: "H%d-A%d" % s)
def test_status_is_raised_for_the_indefinite_row_only(shape):
    H, A = shape
    got, ref = _draw_case(H, A, "general", FILT, "f64", bad_row=1)
    assert got["status"].tolist() == [0, 1, 0] and ref["status"][:, 0].tolist() == [0, 1, 0]
    assert got["status_after"].tolist() == [0, 1, 0]
    for e in (0, 2):
        assert np.array_equal(got["chols"][e], ref["chols"][e]) and np.array_equal(got["noise"][e], ref["noise"][e])
        assert np.all(np.isfinite(got["noise"][e]))
