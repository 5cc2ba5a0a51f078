"""GPU: a PFMPC episode batch (``BatchedPFMPC``) reproduces E separate single-episode runs to the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``PFMPC(...,
noise_mode='device', seed=seed_e)``, ``make_device_rollout_fn(engine)``, ``set_sim_state_fn = resident_state`` and
``set_post_step(engine.step_state)``, ``optimize()`` with ``hotstart=True``.  Every comparison with it is ``np.array_equal``:
at the C ABI row by row against the single launches on the row's slices, and in closed loops the actions, real-env costs and
next observations of every step, the final mean, the final set and the final state.  No real env may reset and no solver may
fail, on either side.  The stage checks (``last_step()``) use the numpy restatements and bounds of tests/pfmpc_cases.py and
tests/philox_ref.py, as tests/test_pfmpc_device_gpu.py does for the single path.
"""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
import pfmpc_cases as pc
from batched_cases import FILT, _cheetah_states, _torch, _vp
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-12, atol=1e-12)      # the controller-update tolerance of tests/test_controllers_gpu.py
MODES = {"null": 0, "repeat": 1}


def _dev(x):
    return _torch().from_numpy(np.ascontiguousarray(x)).cuda()


def _stream():
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
def _abi_inputs(E, M, H, A, salt=0):
    rs = np.random.RandomState(1000 * salt + M + H)
    sets, q0, means = rs.randn(E, M, H, A), 5.0 * rs.rand(E, M), 0.1 * rs.randn(E, H, A)
    q0[E // 2, M // 2] = np.inf                 # (a diverged rollout weighs nothing)
    return sets, q0, means


def _abi_batch(sets, q0, means, lams, seeds, cov_shifts, coeffs, mode, step):
    """The five batched launches (and the deviations of the shifted sets in both storage types) -> numpy arrays."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, M, H, A = sets.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    d_sets, d_q0, d_means0 = _dev(sets), _dev(q0), _dev(means)
    d_lams, d_seeds = _dev(np.asarray(lams, np.float64)), _dev(np.array(seeds, np.uint64).view(np.int64))
    d_chols = _dev(np.stack([np.sqrt(c) * np.eye(A) for c in cov_shifts]))
    d_co = None if tuple(coeffs) == (1.0, 0.0, 0.0) else _dev(np.asarray(coeffs, np.float64))
    out, gath = torch.zeros((E, M, H, A), **f64), torch.zeros((E, M, H, A), **f64)
    w, first = torch.zeros((E, M), **f64), torch.zeros(E, **f64)
    idx = torch.full((E, M), -7, dtype=torch.int32, device="cuda")
    mean, act = torch.zeros((E, H, A), **f64), torch.zeros((E, A), **f64)
    counter = torch.full((1,), step, dtype=torch.int64, device="cuda")
    nbytes = lib.mjmpc_pf_batch_workspace_bytes(E, M, H, A)
    assert nbytes == E * lib.mjmpc_pf_workspace_bytes(M, H, A) > 0
    ws = torch.zeros(nbytes // 8, **f64)
    s = _stream()
    _lib.check(lib.mjmpc_pf_weights_batch(E, M, _vp(d_q0), _vp(d_lams), _vp(d_seeds), 0, _vp(counter), _vp(w), _vp(first), s))
    _lib.check(lib.mjmpc_pf_resample_batch(E, M, _vp(w), _vp(first), _vp(idx), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_gather_shift_batch(E, M, H, A, _vp(d_sets), _vp(idx), mode, _vp(d_chols), _vp(d_co), _vp(d_seeds), 1,
                                               _vp(counter), _vp(out), _vp(gath), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_finish_batch(E, M, H, A, _vp(ws), _vp(mean), _vp(act), _vp(counter), s))
    got = {}
    for name, code, tdt in (("delta64", _lib.F64, torch.float64), ("delta32", _lib.F32, torch.float32)):
        delta = torch.zeros((E, M, H, A), dtype=tdt, device="cuda")
        _lib.check(lib.mjmpc_pf_delta_batch(code, E, M, H, A, _vp(out), _vp(mean), _vp(delta), s))
        got[name] = delta
    # the deviations of the SOURCE sets from the given means (what a control step's first launch forms)
    delta0 = torch.zeros((E, M, H, A), **f64)
    _lib.check(lib.mjmpc_pf_delta_batch(_lib.F64, E, M, H, A, _vp(d_sets), _vp(d_means0), _vp(delta0), s))
    plain = torch.zeros((E, M, H, A), **f64)     # shift_mode < 0: the plain gather (no factors, no survivors kept)
    _lib.check(lib.mjmpc_pf_gather_shift_batch(E, M, H, A, _vp(d_sets), _vp(idx), -1, None, None, _vp(d_seeds), 1, None,
                                               _vp(plain), None, _vp(ws), s))
    torch.cuda.synchronize()
    got.update(w=w, first=first, idx=idx, gathered=gath, shifted=out, mean=mean, act=act, counter=counter, delta0=delta0,
               plain=plain, source=d_sets)
    return {k: v.cpu().numpy() for k, v in got.items()}


def _abi_single(sets, q0, means, lam, seed, cov_shift, coeffs, mode, step):
    """The five single launches on one row's slices, with a step tensor of their own."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    M, H, A = sets.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    d_set, d_q0, d_mean0 = _dev(sets), _dev(q0), _dev(means)
    d_chol = _dev(np.sqrt(cov_shift) * np.eye(A))
    d_co = None if tuple(coeffs) == (1.0, 0.0, 0.0) else _dev(np.asarray(coeffs, np.float64))
    out, gath = torch.zeros((M, H, A), **f64), torch.zeros((M, H, A), **f64)
    w, first, idx = torch.zeros(M, **f64), torch.zeros(1, **f64), torch.full((M,), -7, dtype=torch.int32, device="cuda")
    mean, act = torch.zeros((H, A), **f64), torch.zeros(A, **f64)
    counter = torch.full((1,), step, dtype=torch.int64, device="cuda")
    ws = torch.zeros((lib.mjmpc_pf_workspace_bytes(M, H, A) + 7) // 8, **f64)
    s = _stream()
    _lib.check(lib.mjmpc_pf_weights(M, _vp(d_q0), float(lam), int(seed), 0, _vp(counter), _vp(w), _vp(first), s))
    _lib.check(lib.mjmpc_pf_resample(M, _vp(w), _vp(first), _vp(idx), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_gather_shift(M, H, A, _vp(d_set), _vp(idx), mode, _vp(d_chol), _vp(d_co), int(seed), 1, _vp(counter),
                                         _vp(out), _vp(gath), _vp(ws), s))
    _lib.check(lib.mjmpc_pf_finish(M, H, A, _vp(ws), _vp(mean), _vp(act), _vp(counter), s))
    got = {}
    for name, code, tdt in (("delta64", _lib.F64, torch.float64), ("delta32", _lib.F32, torch.float32)):
        delta = torch.zeros((M, H, A), dtype=tdt, device="cuda")
        _lib.check(lib.mjmpc_pf_delta(code, M, H, A, _vp(out), _vp(mean), _vp(delta), s))
        got[name] = delta
    delta0 = torch.zeros((M, H, A), **f64)
    _lib.check(lib.mjmpc_pf_delta(_lib.F64, M, H, A, _vp(d_set), _vp(d_mean0), _vp(delta0), s))
    torch.cuda.synchronize()
    got.update(w=w, first=first, idx=idx, gathered=gath, shifted=out, mean=mean, act=act, counter=counter, delta0=delta0)
    return {k: v.cpu().numpy() for k, v in got.items()}


ROW_KEYS = ("w", "first", "idx", "gathered", "shifted", "mean", "act", "delta64", "delta32", "delta0")


@pytest.mark.parametrize("M,H,A,base,coeffs", [
    (100, 7, 5, "null", [0.25, 0.8, 0.1]),          # a partial last chunk, H % 4 != 0
    (37, 1, 2, "null", [0.25, 0.8, 0.0]),
    (64, 2, 1, "repeat", [1.0, 0.0, 0.0]),          # the shortest horizon 'repeat' has; no filter
    (4100, 3, 2, "null", [0.25, 0.8, 0.0]),         # two tiles of the running sum, nb = 129 > 64 partials per row
])
def test_rows_equal_the_single_launches_at_the_c_abi(M, H, A, base, coeffs):
    E, step = 3, 6
    lams, seeds, cov_shifts = [0.4, 1.3, 0.07], [11, 2 ** 63 + 9, 2 ** 40 + 5], [0.3, 0.0, 0.05]
    sets, q0, means = _abi_inputs(E, M, H, A)
    assert np.isinf(q0[1]).sum() == 1
    got = _abi_batch(sets, q0, means, lams, seeds, cov_shifts, coeffs, MODES[base], step)
    assert int(got["counter"][0]) == step + 1                  # advanced once, by row 0: not step + E
    assert np.array_equal(got["source"], sets)                  # the source sets are only read
    for e in range(E):
        ref = _abi_single(sets[e], q0[e], means[e], lams[e], seeds[e], cov_shifts[e], coeffs, MODES[base], step)
        assert int(ref["counter"][0]) == step + 1
        for k in ROW_KEYS:
            want = ref[k][0] if k == "first" else ref[k]
            assert np.array_equal(got[k][e], want), (k, e)
        assert np.all(np.isfinite(got["shifted"][e])) and np.all(np.isfinite(got["mean"][e]))
        assert np.array_equal(got["act"][e], got["mean"][e][0])
        i = got["idx"][e].astype(np.int64)
        assert np.array_equal(got["gathered"][e], sets[e][i]) and np.array_equal(got["plain"][e], sets[e][i])
        assert got["w"][e][np.isinf(q0[e])].tolist() == [0.0] * int(np.isinf(q0[e]).sum())
        if H > 1:                                               # a zero variance is a zero jitter, not an error
            moved = got["shifted"][e][:, :-1] - got["gathered"][e][:, 1:]
            assert (np.abs(moved).max() > 0) == (cov_shifts[e] > 0), e
    assert not np.array_equal(got["first"][0], got["first"][1])  # (per-row seeds: different pointers)
    # row isolation: other data in rows 0 and 2 leaves row 1's outputs as they were
    sets2, q02, means2 = _abi_inputs(E, M, H, A, salt=1)
    sets2[1], q02[1], means2[1] = sets[1], q0[1], means[1]
    assert not np.array_equal(sets2[0], sets[0]) and not np.array_equal(q02[2], q0[2])
    got2 = _abi_batch(sets2, q02, means2, [2.0, lams[1], 0.9], [5, seeds[1], 6], [0.1, cov_shifts[1], 0.2], coeffs, MODES[base],
                      step)
    for k in ROW_KEYS + ("plain",):
        assert np.array_equal(got2[k][1], got[k][1]), k
    for k in ("w", "first", "gathered", "mean", "delta0"):      # (and the other rows did change)
        assert not np.array_equal(got2[k][0], got[k][0]) and not np.array_equal(got2[k][2], got[k][2]), k


def test_resampling_rows_return_the_indices_of_the_host_search():
    """One weight kind per row (E = 7), M = 4096: every row's indices are ``systematic_resample_indices`` of ITS weights."""
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.control.particle_filter_controller import systematic_resample_indices
    lib = _lib.require_gpu()
    M, E = 4096, len(pc.WEIGHT_KINDS)
    assert E == 7
    w = np.stack([pc.weights(kind, M) for kind in pc.WEIGHT_KINDS])
    d_w = _dev(w)
    ws = torch.zeros(lib.mjmpc_pf_batch_workspace_bytes(E, M, 1, 1) // 8, dtype=torch.float64, device="cuda")
    kinds = list(pc.POINTER_KINDS)
    for r in range(len(kinds)):
        # (the pointer kinds rotate over the rows, so that a launch mixes them)
        first = np.array([pc.pointer(kinds[(e + r) % len(kinds)], M) for e in range(E)])
        d_first = _dev(first)
        idx = torch.full((E, M), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.mjmpc_pf_resample_batch(E, M, _vp(d_w), _vp(d_first), _vp(idx), _vp(ws), _stream()))
        torch.cuda.synchronize()
        got = idx.cpu().numpy()
        for e in range(E):
            want = systematic_resample_indices(w[e], first[e])
            assert np.array_equal(got[e], want), (pc.WEIGHT_KINDS[e], kinds[(e + r) % len(kinds)])


# ---------------------------------------------------------------------------------------------------------- closed loops
PF = bc.case("BatchedPFMPC", "PFMPC", ("cov_shift", "cov_resample", "lam"), lambda dtype: dict(), gamma=0.99, resident=True,
             extra=("action_samples", "action_samples"), solver=True)


def _check_against_singles(raw, states, seeds, P, H, T, cov_shift, cov_resample, lam, dtype, **kw):
    out = bc.check_against_singles(PF, raw, states, seeds, P, H, T, (cov_shift, cov_resample, lam), dtype, **kw)
    assert out["extra"].shape[:3] == (len(states), P, H)
    assert np.abs(out["acts"]).max() > 0
    return out["acts"]


SEEDS3 = [123 + i * 12345 for i in range(3)]
LAM3, SHIFT3, RESAMPLE3 = np.array([1.0, 0.3, 2.5]), np.array([0.02, 0.0, 0.05]), np.array([0.3, 0.2, 0.5])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_single_episodes(dtype):
    """E = 3, P = 100 (a partial last chunk of the gather), H = 6, T = 5, per-episode lam, cov_shift (one zero), cov_resample."""
    acts = _check_against_singles(_cheetah(), _cheetah_states(3), SEEDS3, 100, 6, 5, SHIFT3, RESAMPLE3, LAM3, dtype)
    assert not np.array_equal(acts[:, 0], acts[:, 1])           # (the episodes are different episodes)


def test_base_action_repeat():
    _check_against_singles(_cheetah(), _cheetah_states(3), SEEDS3, 100, 6, 5, SHIFT3, RESAMPLE3, LAM3, "f64",
                           base_action="repeat")


def test_one_episode_and_permuted_episodes():
    raw = _cheetah()
    _check_against_singles(raw, _cheetah_states(1), [123], 100, 6, 5, 0.02, 0.3, 1.0, "f64")
    bc.check_permutation(PF, raw, _cheetah_states(3), SEEDS3, 100, 6, 5, (SHIFT3, RESAMPLE3, LAM3), "f64", [2, 0, 1])


def test_rk4_double_pendulum():
    raw, states = bc.synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    _check_against_singles(raw, states, [21, 22], 64, 4, 3, [0.02, 0.05], 0.3, [1.0, 0.5], "f64")


def test_free_joint_tray():
    """The general instantiation of the rollout kernel: a model with a free joint (the tray's glass)."""
    from mjmpc_amd.models.compile_tree import compile_tree
    raw, states = bc.synthetic_states("tray", 2)
    m = compile_tree(raw)
    assert m.nq > m.nv
    _check_against_singles(raw, states, [11, 12], 64, 4, 3, [0.02, 0.05], 0.3, [1.0, 0.5], "f64")


def test_randomized_dynamics_two_shards():
    """K = 2 shards of 24 particles roll out their own model blocks (per-episode base seeds); the real envs stay nominal."""
    cfg = {"body_mass": {"torso": [0.3, 0.1], "ffoot": [0.5, 0.0]}, "dof_damping": {"bshin": [0.4, 0.2]},
           "geom_friction": {"bfoot": [0.5, 0.5]}}
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 48, 6, 5, [0.02, 0.05], 0.3, [1.0, 0.5], "f64",
                           K=2, cfg=cfg, dyn_seed=[3, 4])


# ---------------------------------------------------------------------------------------------------------- stages and reset
def _check_stages(rec, cov_shift, filter_coeffs, seed, base_action):
    """``_check_stages`` of tests/test_pfmpc_device_gpu.py: the resampling, gather-and-mean and shift checks on one
    episode's recorded stages (numpy arrays)."""
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
    want, allowed = pc.shift_ref(rec["resampled"], cov_shift, filter_coeffs, seed, k, base_action)
    excess = np.abs(rec["shifted"] - want) - allowed
    print("shift: largest error %.3e, largest error over its bound %.3e" % (np.abs(rec["shifted"] - want).max(), excess.max()))
    assert (excess <= 0.0).all()
    assert (rec["shifted"][:, -1] == 0.0).all() if base_action == "null" else \
        np.array_equal(rec["shifted"][:, -1], rec["shifted"][:, -2])
    assert np.abs(rec["shifted"][:, :-1] - rec["resampled"][:, 1:]).max() > 0.1 * np.sqrt(cov_shift)


def test_stages_of_one_step_stand_on_their_own():
    from mjmpc_amd.control import BatchedPFMPC
    from oracle import controllers_ref as cr
    E, P, H, gamma = 2, 100, 6, 0.99
    seeds, lam, cov_shift = [2 ** 31 + 17, 5], [1.0, 0.4], [0.02, 0.05]
    b = BatchedPFMPC(_cheetah(), E, H, P, cov_shift, 0.3, lam, gamma, FILT, "null", seeds, keep_stages=True)
    with pytest.raises(ValueError):
        b.last_step()                                           # (no step yet)
    b.set_states([dict(s) for s in _cheetah_states(E)])
    first_sets = b.action_samples
    acts, _, _ = b.run(1)
    rec = b.last_step()
    assert rec["step"] == 0 and b.num_steps == 1
    host = {k: (v if isinstance(v, int) else v.cpu().numpy().astype(np.float64 if v.is_floating_point() else np.int64))
            for k, v in rec.items()}
    assert host["samples"].shape == (E, P, H, 6) and host["costs"].shape == (E, P, H) and host["w"].shape == (E, P)
    assert host["first"].shape == (E,) and host["idx"].shape == (E, P) and host["mean"].shape == (E, H, 6)
    assert np.array_equal(host["samples"], first_sets) and np.array_equal(host["shifted"], b.action_samples)
    assert np.array_equal(host["mean"], b.mean_action)
    for e in range(E):
        one = {k: (v if k == "step" else (v[e:e + 1] if k == "first" else v[e])) for k, v in host.items()}
        assert np.isfinite(one["costs"]).all()
        np.testing.assert_allclose(one["w"], cr.pf_weights(one["costs"], cr.gamma_seq(gamma, H), lam[e]), **TOL)
        _check_stages(one, cov_shift[e], FILT, seeds[e], "null")
        assert np.array_equal(acts[0, e], one["mean"][0])
    assert b.engine.env_resets() == 0 and b.engine.solver_failures() == 0
    b.close()
    plain = BatchedPFMPC(_cheetah(), 1, H, 32, 0.02, 0.3, 1.0, gamma, FILT, "null", [1])
    plain.run(1)
    with pytest.raises(ValueError, match="keep_stages"):
        plain.last_step()
    plain.close()


def test_reset_restores_the_initial_sets_and_the_run():
    import philox_ref as pr
    from mjmpc_amd.control import BatchedPFMPC
    E, P, H, A = 2, 64, 6, 6
    seeds, cov_resample = [31, 32], [0.3, 0.6]
    states = [dict(s) for s in _cheetah_states(E)]
    b = BatchedPFMPC(_cheetah(), E, H, P, 0.02, cov_resample, 1.0, 0.99, FILT, "null", seeds)
    sets0 = b.action_samples
    for e in range(E):              # the Philox counterpart of the reference's fresh samples, row by row
        ref, scale = pr.sample_ref(P, H, A, np.sqrt(cov_resample[e]) * np.eye(A), seeds[e], 0, 0, True, FILT, np.float64, True)
        assert (np.abs(sets0[e] - ref) <= pr.error_bound(ref, scale, FILT)).all()
    assert not b.mean_action.any() and b.num_steps == 0
    b.set_states(states)
    first = b.run(3)
    assert not np.array_equal(b.action_samples, sets0) and b.mean_action.any()
    b.reset()
    assert b.num_steps == 0 and int(b._step_dev.item()) == 0
    assert np.array_equal(b.action_samples, sets0) and not b.mean_action.any()
    b.set_states(states)
    again = b.run(3)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    assert b.engine.env_resets() == 0
    b.close()
