"""GPU: a CEM episode batch (``BatchedCEM``) reproduces E separate single-episode runs to the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``CEM(...,
noise_mode='device', noise_dtype=dtype, seed=seed_e)``, ``make_device_rollout_fn(engine)``,
``enable_graph(post_step=engine.step_state)`` (``_single`` of tests/test_batched_mppi_gpu.py), whose iteration runs
``mjmpc_tree_rollout_fused`` + ``mjmpc_cem_select_moments`` + ``mjmpc_cem_finish`` and steps the engine's device-resident real
env; every test asserts that it took that fused branch.  Every comparison is ``np.array_equal``: the actions, real-env
costs and next observations of every step, the final mean, the final covariance and the final state.  No real env may
reset (``mjmpc_tree_env_resets`` == 0 on both sides) and every action and cost is finite, so that two all-``inf`` runs
cannot pass for equal.
"""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, _cheetah_states, _torch, _vp
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu


def _took_the_fused_step(c):
    assert c._cem_fused(), "the single path did not take its fused CEM step"


CEM = bc.case("BatchedCEM", "CEM", ("init_cov", "elite_frac", "step_size", "beta"), lambda dtype: dict(noise_dtype=dtype),
              during=_took_the_fused_step, extra=("cov_action", "cov"))


def _check_against_singles(raw, states, seeds, P, H, T, init_cov, elite_frac, step_size, beta, dtype, cov_type="full", **kw):
    out = bc.check_against_singles(CEM, raw, states, seeds, P, H, T, (init_cov, elite_frac, step_size, beta), dtype,
                                   cov_type=cov_type, **kw)
    return out["acts"], out["costs"], out["extra"]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("cov_type", ["full", "diagonal"])
def test_half_cheetah_batch_equals_single_episodes(cov_type, dtype):
    """E = 3, P = 64, H = 8, T = 6, k = 6: by step 3 a covariance refitted from elites has coloured a draw."""
    E = 3
    acts, _, covs = _check_against_singles(_cheetah(), _cheetah_states(E), [123 + i * 12345 for i in range(E)], 64, 8, 6,
                                           0.3, 0.1, 1.0, 0.45, dtype, cov_type=cov_type)
    assert not np.array_equal(acts[:, 0], acts[:, 1])           # (the episodes are different episodes)
    if cov_type == "full":
        assert np.count_nonzero(covs[0] - np.diag(np.diag(covs[0]))) > 0        # (the refit has filled the covariance)


def test_per_episode_hyperparameters():
    """k = 1 (the H k = 8-row np.cov edge), 6 and 32; different beta, step_size (one below 1) and init_cov; 'repeat'."""
    E, P = 3, 64
    elite_frac = np.array([1.0 / P, 0.1, 0.5])
    assert [int(P * f) for f in elite_frac] == [1, 6, 32]
    _check_against_singles(_cheetah(), _cheetah_states(E), [7, 10, 13], P, 8, 6, np.array([0.2, 0.3, 0.5]), elite_frac,
                           np.array([1.0, 0.8, 0.9]), np.array([0.45, 0.2, 0.6]), "f64", base_action="repeat")


def test_particles_not_a_multiple_of_the_tiles():
    """P = 50: a row's last partial and its selection tile end inside the next row's particles' address range."""
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 50, 8, 6, 0.3, 0.1, 1.0, 0.45, "f64")


def test_one_episode_and_permuted_episodes():
    raw = _cheetah()
    _check_against_singles(raw, _cheetah_states(1), [123], 64, 8, 6, 0.3, 0.1, 1.0, 0.45, "f64")
    cov, frac, step, beta = np.array([0.2, 0.3, 0.4]), np.array([0.1, 0.2, 0.3]), np.array([1.0, 0.9, 0.8]), np.array([0.45, 0.3, 0.1])
    bc.check_permutation(CEM, raw, _cheetah_states(3), [5, 6, 7], 64, 8, 6, (cov, frac, step, beta), "f64", [2, 0, 1])


def test_rk4_double_pendulum():
    """A non-HalfCheetah instantiation of the rollout kernel (RK4, one actuator... A <= H + 1 holds)."""
    raw, states = bc.synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    _check_against_singles(raw, states, [21, 22], 32, 6, 4, 0.3, 0.25, 1.0, 0.45, "f64")


def test_randomized_dynamics_two_shards():
    """K = 2 shards of 24 particles roll out their own model blocks; the real envs stay nominal."""
    cfg = {"body_mass": {"torso": [0.3, 0.1], "ffoot": [0.5, 0.0]}, "dof_damping": {"bshin": [0.4, 0.2]},
           "geom_friction": {"bfoot": [0.5, 0.5]}}
    _check_against_singles(_cheetah(), _cheetah_states(2), [123, 12468], 48, 8, 6, 0.3, 0.125, 1.0, 0.45, "f64",
                           K=2, cfg=cfg, dyn_seed=[3, 4])


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
def _abi_case(dtype, full, covs0, step_sizes, seed=0):
    """E = 3 rows of P = 50 particles, H = 8, A = 6, k = (1, 6, 25): hand-made q0 with duplicates across the k-th rank and
    +inf entries, random actions.  Returns what the batch entries and three single calls on the row slices leave behind."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, P, H, A = 3, 50, 8, 6
    ks = [1, 6, 25]
    code = _lib.F32 if dtype == "f32" else _lib.F64
    tdt = torch.float32 if dtype == "f32" else torch.float64
    rng = np.random.RandomState(seed)
    q0 = rng.uniform(1.0, 2.0, (E, P))
    q0[0, [3, 17, 40]] = q0[0].min() - 0.5              # k = 1: three tied minima, the lowest index wins
    q0[1, [2, 9, 11, 30]] = np.sort(q0[1])[5]           # k = 6: four more copies of the 6th smallest value
    q0[2, 10:40] = 1.5                                  # k = 25: the rank lies inside a run of 30 equal values
    q0[:, [0, 7, 49]] = np.inf
    q0[2, 45:] = np.inf
    actions = rng.uniform(-1, 1, (E, P, H, A))
    means0 = rng.uniform(-0.2, 0.2, (E, H, A))
    grow_diag = rng.uniform(0.1, 0.5, (E, A))
    grow_scale = np.array([0.45, 0.0, 0.2])
    seeds = np.array([11, 2 ** 40 + 5, 2 ** 63 + 9], np.uint64)
    dev = "cuda"
    d = lambda a, t=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if t is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(t)   # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_act = d(actions, tdt)
    step0 = 3
    # -- the batch
    b = dict(means=d(means0), covs=d(covs0), chols=torch.zeros((E, A, A), dtype=torch.float64, device=dev),
             status=torch.zeros(E, dtype=torch.int32, device=dev), out=torch.zeros((E, A), dtype=torch.float64, device=dev),
             counter=torch.full((1,), step0, dtype=torch.int64, device=dev), noise=torch.zeros((E, P, H, A), dtype=tdt, device=dev))
    nbytes = lib.mjmpc_cem_batch_workspace_bytes(E, P, max(ks), H, A)
    assert nbytes > 0
    ws = torch.zeros(nbytes // 8, dtype=torch.float64, device=dev)
    d_q0, d_k, d_step = d(q0), d(np.array(ks, np.int64)), d(np.array(step_sizes, np.float64))
    d_gd, d_gs, d_seeds = d(grow_diag), d(grow_scale), d(seeds.view(np.int64))
    _lib.check(lib.mjmpc_cem_select_moments_batch(code, E, P, H, A, _vp(d_act), _vp(d_q0), _vp(d_k), _vp(b["means"]),
                                                  _vp(b["covs"]), _vp(b["counter"]), _vp(ws), s))
    _lib.check(lib.mjmpc_cem_finish_batch(code, E, P, H, A, _vp(d_k), full, _vp(d_step), 0, _vp(b["means"]), _vp(b["covs"]),
                                          _vp(b["chols"]), _vp(b["status"]), _vp(d_gd), _vp(d_gs), _vp(b["out"]),
                                          _vp(b["counter"]), _vp(b["noise"]), _vp(d_seeds), 0, _vp(ws), s))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in b.items()}
    # -- three single calls on the row slices, and the sampler kernel for the next step's samples
    ref = dict(means=[], covs=[], chols=[], status=[], out=[], noise=[], drawn=[])
    ws1 = torch.zeros((lib.mjmpc_update_workspace_bytes(P, H, A) + 7) // 8, dtype=torch.float64, device=dev)
    addr = lib.mjmpc_workspace_q0(_vp(ws1), P, H, A)
    q0_view = ws1[(addr - ws1.data_ptr()) // 8:][:P]
    for e in range(E):
        mean, cov = d(means0[e]), d(covs0[e])
        chol, status = torch.zeros((A, A), dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        out, counter = torch.zeros(A, dtype=torch.float64, device=dev), torch.full((1,), step0, dtype=torch.int64, device=dev)
        noise = torch.zeros((P, H, A), dtype=tdt, device=dev)
        q0_view.copy_(d_q0[e])
        _lib.check(lib.mjmpc_cem_select_moments(code, P, H, A, _vp(d_act[e]), None, P, 0, ks[e], _vp(mean), _vp(cov),
                                                _vp(counter), _vp(ws1), s))
        _lib.check(lib.mjmpc_cem_finish(code, P, H, A, ks[e], None, 1, float(ks[e]), full, float(step_sizes[e]), 0, _vp(mean),
                                        _vp(cov), _vp(chol), _vp(status), _vp(d_gd[e]), float(grow_scale[e]), _vp(out), None,
                                        _vp(counter), _vp(noise), int(seeds[e]), 0, 0, _vp(ws1), s))
        drawn = torch.zeros((P, H, A), dtype=tdt, device=dev)
        _lib.check(lib.mjmpc_sample_noise(code, _vp(drawn), P, H, A, _vp(b["chols"][e]), None, int(seeds[e]), 0, 0,
                                          _vp(b["counter"]), 0, s))
        torch.cuda.synchronize()
        assert int(counter.item()) == step0 + 1
        for k, v in (("means", mean), ("covs", cov), ("chols", chol), ("status", status), ("out", out), ("noise", noise),
                     ("drawn", drawn)):
            ref[k].append(v.cpu().numpy())
    assert int(got["counter"][0]) == step0 + 1                  # advanced once, by row 0
    return got, {k: np.stack(v) for k, v in ref.items()}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("full", [1, 0])
def test_ties_and_inf_at_the_c_abi(full, dtype):
    A = 6
    covs0 = np.stack([np.diag(np.full(A, c)) for c in (0.3, 0.2, 0.5)])
    got, ref = _abi_case(dtype, full, covs0, [1.0, 0.8, 0.9])
    assert not got["status"].any() and not ref["status"].any()
    for k in ("means", "covs", "chols", "out"):
        assert np.all(np.isfinite(got[k])), k
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["noise"], ref["noise"])           # the single finish launch's draw
    assert np.array_equal(got["noise"], ref["drawn"])           # mjmpc_sample_noise(..., chol_is_diagonal = 0) of the new step
    assert np.abs(got["noise"]).max() > 0 and not np.array_equal(got["noise"][0], got["noise"][1])


def test_status_is_raised_for_the_indefinite_row_only():
    A = 6
    covs0 = np.stack([np.diag(np.full(A, c)) for c in (0.3, 0.2, 0.5)])
    covs0[1, 2, 2] = -1.0                                       # indefinite, and step_size 0 keeps it
    got, ref = _abi_case("f64", 1, covs0, [1.0, 0.0, 0.9])
    assert got["status"].tolist() == [0, 1, 0] and ref["status"][:, 0].tolist() == [0, 1, 0]
    for e in (0, 2):
        for k in ("means", "covs", "chols", "out", "noise"):
            assert np.array_equal(got[k][e], ref[k][e]), (k, e)


def test_batched_cem_reports_the_indefinite_episode_once():
    from mjmpc_amd import _lib
    from mjmpc_amd.control import BatchedCEM
    torch = _torch()
    E = 3
    b = BatchedCEM(_cheetah(), E, 8, 64, 0.3, 0.1, [1.0, 0.0, 1.0], 0.0, 1.0, FILT, "null", [1, 2, 3])
    b.set_states([dict(s) for s in _cheetah_states(E)])
    bad = np.diag(np.full(6, 0.3))
    bad[2, 2] = -1.0
    b._covs[1].copy_(torch.from_numpy(bad))                     # step_size 0 and beta 0: the refit keeps this covariance
    with pytest.raises(_lib.MjmpcError, match=r"episode 1\b"):
        b.run(1)
    assert np.array_equal(b.cov[1], bad)                        # reported once: the flag was cleared, nothing ran since
    b.mean_action
    b.get_states()
    b.close()
