"""GPU: user-defined cost terms in the episode batches.

1. the ``_obs`` rollout entries: costs, actions and q0 of ``rollout_fused_batch``, next observations of the single-state
   engine (tree) / of the plain full-size launch (arm); 2. ``mjmpc_cost_terms_batch`` against ``mjmpc_cost_terms`` per episode
   and its q0 against the numpy loop; 3. closed loops, bit for bit, against the single-episode controllers over engines with
   terms and against the batch rebuilt from separate launches; 4. the terms act.  Every comparison is ``np.array_equal``
   except the anchor to the built-in reach cost (8 eps, DESIGN 12's).
"""
import numpy as np
import pytest

import batched_cases as bc
import batched_terms_cases as tc
from batched_cases import FILT, _torch, _vp
from cost_terms_cases import random_table

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]
CHEETAH_CFG = {"body_mass": {"torso": [0.3, 0.1], "ffoot": [0.5, 0.0]}, "body_inertia": {"bthigh": [0.3, 0.0]}}


# ---- 1. the _obs rollout entries ---------------------------------------------------------------------------------------
def _inputs(E, P, H, A, dtype, seed):
    torch = _torch()
    rng = np.random.RandomState(seed)
    means = torch.from_numpy(rng.uniform(-0.3, 0.3, (E, H, A))).cuda()
    noise = torch.from_numpy(0.5 * rng.standard_normal((E * P, H, A))).to(tc.tdtype(dtype == "f32")).cuda()
    coeffs = torch.tensor(FILT, dtype=torch.float64).cuda()
    gseq = torch.from_numpy(np.cumprod([1.0] + [0.97] * (H - 1))).cuda()
    return means, noise, coeffs, gseq


def _launch(eng, kind, name, N, H, means, noise, coeffs, gseq, want_q0, nobs="none"):
    """One batch rollout launch -> costs, actions, q0, next observations (host; None where not asked for)."""
    torch = _torch()
    from mjmpc_amd import _lib
    A = eng.d_action
    costs = torch.full((N, H), -1.0, dtype=noise.dtype, device="cuda")
    acts = torch.empty((N, H, A), dtype=noise.dtype, device="cuda")
    q0 = torch.empty(N, dtype=torch.float64, device="cuda") if want_q0 else None
    args = [eng._h, eng._code, N, H, _vp(means), _vp(noise), _vp(coeffs), _vp(gseq) if want_q0 else None, _vp(costs), _vp(acts),
            _vp(q0)]
    d_nobs = None
    if name.endswith("_obs"):
        d_nobs = torch.full((N, H, eng.d_obs), np.nan, dtype=noise.dtype, device="cuda") if nobs == "want" else None
        args.append(_vp(d_nobs))
    _lib.check(getattr(eng._lib, "mjmpc_%s_%s" % (kind, name))(*args, eng._stream()))
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (costs, acts, q0, d_nobs))


def _check_obs_entry(eng, kind, single_engine, states, E, P, H, dtype, seed, full_size):
    """``eng``: the batch's engine with its state shards set.  ``single_engine()``: a fresh single-state engine of the
    reference; ``full_size``: the reference launch holds all E P particles (arm) or episode e's P (tree)."""
    means, noise, coeffs, gseq = _inputs(E, P, H, eng.d_action, dtype, seed)
    N = E * P
    c0, a0, q0, _ = _launch(eng, kind, "rollout_fused_batch", N, H, means, noise, coeffs, gseq, True)
    c1, a1, q1, n1 = _launch(eng, kind, "rollout_fused_batch_obs", N, H, means, noise, coeffs, gseq, True, "want")
    c2, a2, q2, _ = _launch(eng, kind, "rollout_fused_batch_obs", N, H, means, noise, coeffs, gseq, True)   # NULL: the old entry
    assert np.all(np.isfinite(c0)) and np.all(np.isfinite(q0)) and np.all(np.isfinite(n1))
    for c, a, q in ((c1, a1, q1), (c2, a2, q2)):
        assert np.array_equal(c, c0) and np.array_equal(a, a0) and np.array_equal(q, q0), (dtype, E, P, H)
    # the next observations: pre-filtered noise (no filter in either launch) against the single-state engine
    c3, a3, _, n3 = _launch(eng, kind, "rollout_fused_batch_obs", N, H, means, noise, None, None, False, "want")
    ref = single_engine()
    for e in range(E):
        ref.set_env_state(dict(states[e]))
        rows = slice(e * P, (e + 1) * P)
        if full_size:
            c, a, _, n = ref.rollout_device(N, H, means[e], noise, want_obs=True)
            c, a, n = (x.cpu().numpy()[rows] for x in (c, a, n))
        else:
            c, a, _, n = (None if x is None else x.cpu().numpy() for x in ref.rollout_device(P, H, means[e], noise[rows], want_obs=True))
        assert np.array_equal(n3[rows], n), (dtype, e, np.abs(n3[rows] - n).max())
        assert np.array_equal(c3[rows], c) and np.array_equal(a3[rows], a), (dtype, e)
    ref.close()
    # (the filter acts from the third step on: the two comparisons above are then of different launches)
    assert H < 3 or not np.array_equal(a3, a0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E,P,H", [(3, 5, 3), (2, 64, 8)])
@pytest.mark.parametrize("name", ["cheetah", "cartpole"])
def test_tree_obs_entry(name, E, P, H, dtype):
    raw, states, kind = tc.model(name, E)
    eng = tc.engine(raw, kind, dtype)
    eng.set_shard_states_raw([eng._unpack(dict(s)) for s in states])
    _check_obs_entry(eng, kind, lambda: tc.engine(raw, kind, dtype), states, E, P, H, dtype, 1, False)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_tree_obs_entry_with_randomized_dynamics(dtype):
    """K = 2 model shards per episode on HalfCheetah: the rows are those of a two-shard engine with the same blocks."""
    from mjmpc_amd.control import BatchedMPPI
    E, P, H, K = 3, 8, 3, 2
    raw, states, kind = tc.model("cheetah", E)
    b = BatchedMPPI(raw, E, H, P, 0.2, 1.0, 0.3, 1.0, FILT, "null", [1, 2, 3], dtype=dtype)
    b.set_states([dict(s) for s in states])
    b.randomize_dynamics(CHEETAH_CFG, 321, K)

    def two_shards():
        ref = tc.engine(raw, kind, dtype, num_shards=K)
        ref.randomize_dynamics(CHEETAH_CFG, 321)
        return ref
    _check_obs_entry(b.engine, kind, two_shards, states, E, P, H, dtype, 2, False)
    b.close()


def _check_arm_obs_entry(dtype, E, P, H, seed):
    raw, states, kind = tc.model("reacher", E)
    eng = tc.engine(raw, kind, dtype)
    eng.set_shard_states_raw([eng._unpack(s) for s in states])
    _check_obs_entry(eng, kind, lambda: tc.engine(raw, kind, dtype), states, E, P, H, dtype, seed, True)
    assert eng.solver_failures() == 0
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_arm_obs_entry(dtype):
    _check_arm_obs_entry(dtype, 3, 16, 3, 3)


# (shape, smallest total above the shape's lower threshold in SIMDs, dtypes): launch_arm_rollout's choices from the grid, as
# tests/test_batched_arm_gpu.py derives them (with the test above - the four-wave flag shape - every twin has stored)
ARM_SHAPES = [("duo", 2, ("f64",)), ("solo_1_wave", 4, ("f64",)), ("solo_2_waves", 8, ("f64", "f32")),
              ("solo_3_waves", 16, ("f32",))]


@pytest.mark.parametrize("shape,dtype", [(s[0], d) for s in ARM_SHAPES for d in s[2]])
def test_arm_obs_entry_in_every_launch_shape(shape, dtype):
    simds = 4 * _torch().cuda.get_device_properties(0).multi_processor_count
    total = dict((s[0], s[1]) for s in ARM_SHAPES)[shape] * simds + 16
    _check_arm_obs_entry(dtype, 2, total // 2, 2, 4)


# ---- 2. mjmpc_cost_terms_batch against mjmpc_cost_terms ------------------------------------------------------------------
# (E, P, H): one element; tiles that hold several particles and episodes; H = the tile, beyond it, no divisor of it
KERNEL_SHAPES = [(1, 1, 1), (3, 5, 3), (2, 8, 8), (3, 1, 64), (2, 3, 100), (4, 67, 7)]


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
@pytest.mark.parametrize("d_obs,A,K", [(10, 1, 1), (10, 7, 128), (43, 1, 128), (43, 7, 1), (43, 7, 37)])
def test_batch_kernel_equals_the_single_kernel_per_episode(d_obs, A, K, f32):
    torch = _torch()
    rng = np.random.default_rng(2000 * d_obs + 20 * A + K)
    tdt = tc.tdtype(f32)
    for E, P, H in KERNEL_SHAPES:
        N = E * P
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (N, H, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (N, H, A))).to(tdt).cuda()
        gseq_h = np.cumprod([1.0] + [0.93] * (H - 1))
        gseq = torch.from_numpy(gseq_h).cuda()
        for per_episode in (False, True):
            first = random_table(rng, K, d_obs, A)
            tables = np.stack([first] * (E if per_episode else 1))
            if per_episode:                         # the rows of episode 0 with weights and targets redrawn per episode
                tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
                tables[1:, :, 4] = rng.uniform(-5.0, 5.0, (E - 1, K))
            d_tab = torch.from_numpy(np.ascontiguousarray(tables)).cuda()
            reads = bool(np.any(first[:, 1] != 0))
            for keep, terminal in ((0, 1), (1, 0), (1, 1), (0, 0)):
                cin = rng.uniform(-3.0, 3.0, (N, H))
                bad = []
                if N * H >= 15:                     # an incoming +inf and an incoming NaN: both leave as +inf
                    cin.reshape(-1)[4], cin.reshape(-1)[N * H - 2] = np.inf, np.nan
                    bad = [4 // H, (N * H - 2) // H]
                d_cin = torch.from_numpy(cin).to(tdt).cuda()
                want = d_cin.clone()
                for e in range(E):
                    rows = slice(e * P, (e + 1) * P)
                    tc.cost_terms(d_tab[e if per_episode else 0], nobs[rows], act[rows] if reads else None, want[rows], keep,
                                  terminal, f32)
                got, q0 = d_cin.clone(), torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
                tc.cost_terms_batch(d_tab, E, nobs, act if reads else None, got, keep, terminal, f32, gseq, q0, A=A)
                torch.cuda.synchronize()
                got_h, want_h, q0_h = got.cpu().numpy(), want.cpu().numpy(), q0.cpu().numpy()
                where = (E, P, H, per_episode, keep, terminal)
                assert np.array_equal(got_h, want_h), where
                assert np.array_equal(q0_h, tc.numpy_q0(got_h, gseq_h)), where
                flat = got_h.reshape(-1)
                ok = np.ones(N * H, bool)
                if bad:
                    ok[[4, N * H - 2]] = False
                    assert np.all(np.isposinf(flat[~ok])) and np.all(np.isposinf(q0_h[bad])), where
                assert np.all(np.isfinite(flat[ok])), where                 # (the neighbours are untouched)
                assert np.all(np.isfinite(np.delete(q0_h, bad))), where
                if keep == terminal:                # without a cost-to-go the costs are the same
                    alone = d_cin.clone()
                    tc.cost_terms_batch(d_tab, E, nobs, act if reads else None, alone, keep, terminal, f32, A=A)
                    torch.cuda.synchronize()
                    assert np.array_equal(alone.cpu().numpy(), got_h), where


# ---- 3. closed loops ----------------------------------------------------------------------------------------------------
SEEDS = [123 + i * 12345 for i in range(3)]
DMD = bc.case("BatchedDMDMPC", "DMDMPC", ("lam", "step_size", "init_cov", "beta"),
              lambda dtype: dict(update_cov=True, noise_dtype=dtype), extra=("cov_action", "cov"))
MPPIQ = bc.case("BatchedMPPIQ", "MPPIQ", ("beta", "step_size", "init_cov", "td_lam"),
                lambda dtype: dict(alpha=1, time_based_weights=True, noise_dtype=dtype))
# every class with per-episode settings (tests/test_batched_arm_gpu.py's values)
CASES = dict(
    BatchedMPPI=(bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), None),
                 (np.array([0.01, 0.05, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedCEM=(bc.case("BatchedCEM", "CEM", ("init_cov", "elite_frac", "step_size", "beta"), None, extra=("cov_action", "cov")),
                (np.array([1.0, 0.5, 0.3]), np.array([0.25, 0.125, 0.5]), np.array([1.0, 0.9, 0.8]), np.array([0.1, 0.2, 0.0]))),
    BatchedPFMPC=(bc.case("BatchedPFMPC", "PFMPC", ("cov_shift", "cov_resample", "lam"), None, gamma=0.99,
                          extra=("action_samples", "action_samples")),
                  (np.array([0.3, 0.2, 0.5]), np.array([0.1, 0.3, 0.2]), np.array([0.05, 0.2, 0.1]))),
    BatchedDMDMPC=(DMD, (np.array([0.05, 0.1, 0.2]), np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]), np.array([0.1, 0.0, 0.2]))),
    BatchedRandomShooting=(bc.case("BatchedRandomShooting", "RandomShooting", ("step_size", "init_cov"), None),
                           (np.array([1.0, 0.8, 0.9]), np.array([1.0, 0.5, 0.3]))),
    BatchedMPPIQ=(MPPIQ, (np.array([0.2, 0.1, 0.5]), np.array([1.0, 0.8, 0.5]), np.array([0.3, 0.2, 0.5]), np.array([0.9, 0.0, 1.0]))),
)


def _make(case, hyper, name, E, P, H, dtype, terms="shared", **kw):
    """A batch of model ``name`` on its engine kind with its start states; ``terms``: None, 'shared', 'per_episode' or a
    function of the batch."""
    raw, states, kind = tc.model(name, E)
    b = bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, dtype, engine=kind, **kw)
    if callable(terms):
        b.set_cost_terms(terms(b))
    elif terms is not None:
        b.set_cost_terms(tc.terms_for(name, b.engine, E, terms == "per_episode"))
    return b


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@pytest.mark.parametrize("name", ["cartpole", "cheetah"])
@pytest.mark.parametrize("cls", ["BatchedDMDMPC", "BatchedMPPIQ"])
def test_batch_with_terms_equals_single_episodes_with_terms(cls, name, per_episode):
    """(a) episode e against the single-episode controller on an engine of its own after ``set_cost_terms`` (table e)."""
    E, P, H, T, dtype = 3, 64, 8, 5, "f64"
    case, hyper = CASES[cls]
    raw, states, _ = tc.model(name, E)
    cov_type = "full" if cls == "BatchedDMDMPC" else None       # (both sides adapt a full covariance)
    b = _make(case, hyper, name, E, P, H, dtype, "per_episode" if per_episode else "shared", cov_type=cov_type)
    out = bc.run_batch(case, b, T)
    assert np.all(np.isfinite(out["acts"])) and np.all(np.isfinite(out["costs"])) and np.abs(out["acts"]).max() > 0
    make = tc.forward_terms if name == "cheetah" else tc.reach_terms
    for e in range(E):
        one = tc.single(case, raw, states[e], SEEDS[e], P, H, T, [v[e] for v in hyper], dtype,
                        lambda eng, e=e: make(eng, e if per_episode else None), cov_type=cov_type)
        assert np.array_equal(out["acts"][:, e], one["acts"]), (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), e
        assert np.array_equal(out["mean"][e], one["mean"]), e
        for x, y in zip(bc._qpos_qvel(out["state"][e]), bc._qpos_qvel(one["state"])):
            assert np.array_equal(x, y), e


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cls,name", [(c, "cartpole") for c in sorted(CASES)]
                         + [(c, "reacher") for c in ("BatchedMPPI", "BatchedCEM", "BatchedPFMPC")])
def test_batch_with_terms_equals_its_separate_launches(cls, name, dtype):
    """(b) the fused path against the same batch with the ``_obs`` rollout, ``mjmpc_cost_terms`` per episode and a numpy
    cost-to-go in ``_rollout``'s place, ``step_shard_states`` and ``mjmpc_cost_terms`` per episode in ``_env_step``'s."""
    E, P, H, T = 3, 16, 8, 3
    case, hyper = CASES[cls]
    got = bc.run_batch(case, _make(case, hyper, name, E, P, H, dtype, "per_episode"), T)
    want = bc.run_batch(case, tc.as_separate_launches(_make(case, hyper, name, E, P, H, dtype, "per_episode")), T)
    assert np.all(np.isfinite(got["acts"])) and np.abs(got["acts"]).max() > 0
    tc.assert_same_runs(got, want, "%s %s %s" % (cls, name, dtype))


def test_batch_with_terms_and_randomized_dynamics():
    """(b) with K = 2 model shards per episode (HalfCheetah)."""
    E, P, H, T = 3, 16, 8, 3
    case, hyper = CASES["BatchedMPPI"]
    runs = []
    for separate in (False, True):
        b = _make(case, hyper, "cheetah", E, P, H, "f64", "per_episode")
        b.randomize_dynamics(CHEETAH_CFG, 321, 2)
        runs.append(bc.run_batch(case, tc.as_separate_launches(b) if separate else b, T))
    tc.assert_same_runs(runs[0], runs[1], "randomized dynamics")


@pytest.mark.parametrize("cls", ["BatchedMPPI", "BatchedDMDMPC"])
def test_set_cost_terms_none_restores_the_builtin_cost(cls):
    """(c) after terms and ``set_cost_terms(None)`` the run is that of a batch that never had terms."""
    E, P, H, T = 3, 16, 8, 3
    case, hyper = CASES[cls]
    never = bc.run_batch(case, _make(case, hyper, "cartpole", E, P, H, "f64", None), T)
    b = _make(case, hyper, "cartpole", E, P, H, "f64", "per_episode")
    with_terms = b.run(2)
    assert b._terms_nobs is not None
    b.set_cost_terms(None)
    assert b._terms is None and b._terms_nobs is None and b._terms_env is None    # (the buffers live only while terms are set)
    b.reset()
    b.num_steps = 0
    b.set_states([dict(s) for s in tc.model("cartpole", E)[1]])
    again = bc.run_batch(case, b, T)
    tc.assert_same_runs(again, never, "after set_cost_terms(None)")
    assert not np.array_equal(with_terms[1], never["costs"][:2])


@pytest.mark.parametrize("name", ["cartpole", "cheetah"])
def test_a_zero_weight_row_on_top_of_the_builtin_cost_changes_nothing(name):
    """(d) ``keep_builtin`` and one SQUARE row of weight 0: the rollouts' per-step costs and a ``BatchedDMDMPC`` run (it reads
    the per-step costs) are those of the batch without terms, exactly."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    E, P, H, T = 3, 16, 8, 3
    case, hyper = CASES["BatchedDMDMPC"]

    def zero_row(b):
        return CostTerms(b.engine, keep_builtin=True).square(obs="qvel", index=0, weight=0.0, target=0.3)
    step_costs = []
    for terms in (None, zero_row):
        b = _make(case, hyper, name, E, P, H, "f64", terms)
        b.step()
        _torch().cuda.synchronize()
        step_costs.append(b._costs.cpu().numpy().copy())
        b.close()
    assert np.array_equal(step_costs[0], step_costs[1]) and np.all(np.isfinite(step_costs[0]))
    plain = bc.run_batch(case, _make(case, hyper, name, E, P, H, "f64", None), T)
    zero = bc.run_batch(case, _make(case, hyper, name, E, P, H, "f64", zero_row), T)
    tc.assert_same_runs(zero, plain, "zero-weight row")


@pytest.mark.parametrize("dtype", DTYPES)
def test_builtin_reach_terms_equal_the_arm_kernels_cost(dtype):
    """(e) the anchor of DESIGN 12 for the batch: one rollout launch of the reacher on the arm engine costed by
    ``builtin_reach`` against the kernel's own cost, within 8 eps (and twice it with ``keep_builtin``)."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    E, P, H = 3, 16, 8
    eps = np.finfo(np.float32 if dtype == "f32" else np.float64).eps
    case, hyper = CASES["BatchedMPPI"]
    costs = {}
    for keep in (None, False, True):
        terms = None if keep is None else (lambda b, keep=keep: CostTerms.builtin_reach(b.engine, keep_builtin=keep))
        b = _make(case, hyper, "reacher", E, P, H, dtype, terms)
        s = b._stream()
        b._draw(s)
        b._rollout(s)
        _torch().cuda.synchronize()
        costs[keep] = b._costs.cpu().numpy().astype(np.float64)
        q0 = b._q0.cpu().numpy()
        assert np.array_equal(q0, tc.numpy_q0(b._costs.cpu().numpy(), b._gseq.cpu().numpy())) or keep is None
        assert b.engine.solver_failures() == 0
        b.close()
    builtin = costs[None]
    assert np.all(np.isfinite(builtin)) and np.all(builtin > 0)
    for keep, factor in ((False, 1.0), (True, 2.0)):
        err = np.abs(costs[keep] - factor * builtin)
        assert np.all(err <= 8 * eps * builtin), "keep_builtin %s: %.3g eps" % (keep, (err / (eps * builtin)).max())


# ---- 4. the terms act ---------------------------------------------------------------------------------------------------
def _goal_terms(b, goals):
    """The cart's rest position as each episode's own goal."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    return [CostTerms(b.engine).square(obs="qpos", index=0, weight=2.0, target=g).cos(obs="qpos", index=1, weight=1.0)
            .square(action=0, weight=0.01) for g in goals]


def test_per_episode_targets_move_the_episodes_apart():
    """Two episodes with one seed and one start state and different targets end with different means; with the same target
    they are the same episode."""
    case, _ = CASES["BatchedMPPI"]
    raw, states, _ = tc.model("cartpole", 1)
    out = {}
    for goals in ((-0.5, 0.5), (0.5, 0.5)):
        b = bc.make_batch(case, raw, [states[0], states[0]], [7, 7], 64, 8, (0.05, 1.0, 0.5), "f64")
        b.set_cost_terms(_goal_terms(b, goals))
        out[goals] = bc.run_batch(case, b, 5)
    same, apart = out[(0.5, 0.5)], out[(-0.5, 0.5)]
    assert np.array_equal(same["mean"][0], same["mean"][1]) and np.array_equal(same["acts"][:, 0], same["acts"][:, 1])
    assert not np.array_equal(apart["mean"][0], apart["mean"][1])
    assert np.array_equal(apart["mean"][1], same["mean"][1])            # (episode 1 is the same episode in both batches)
    assert np.all(np.isfinite(apart["mean"]))


@pytest.mark.parametrize("cls", ["BatchedMPPI", "BatchedMPPIQ"])
def test_permuting_the_episodes_with_their_tables_permutes_the_results(cls):
    E, P, H, T = 3, 16, 8, 3
    case, hyper = CASES[cls]
    raw, states, _ = tc.model("cartpole", E)
    perm = np.array([2, 0, 1])
    base = bc.run_batch(case, _make(case, hyper, "cartpole", E, P, H, "f64", "per_episode"), T)
    b = bc.make_batch(case, raw, [states[k] for k in perm], [SEEDS[k] for k in perm], P, H, [v[perm] for v in hyper], "f64")
    b.set_cost_terms([tc.reach_terms(b.engine, int(k)) for k in perm])
    got = bc.run_batch(case, b, T)
    for k in ("acts", "costs", "nobs"):
        assert np.array_equal(got[k], base[k][:, perm]), k
    assert np.array_equal(got["mean"], base["mean"][perm])
    assert case.extra is None or np.array_equal(got["extra"], base["extra"][perm])
    for k, e in enumerate(perm):
        for x, y in zip(bc._qpos_qvel(got["state"][k]), bc._qpos_qvel(base["state"][e])):
            assert np.array_equal(x, y)
