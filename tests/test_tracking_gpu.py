"""GPU: cost terms that track a reference trajectory.

1. ``mjmpc_cost_terms_track`` against the numpy restatement of the contract (tests/tracking_cases.py) within the derived
   bound of tests/cost_terms_cases.py, the counter with and without ``advance``; ``mjmpc_cost_terms_track_batch`` against the
   single entry per episode, bit for bit; 2. a reference that is constant in time against the same constant target, bit for
   bit, through ``rollout_device``; 3. closed loops: eager, hipGraph replay and launch tape give the same bits, the real cost
   of step s is the restatement's with reference row s + 1, a host-driven loop with ``set_track_step`` gives the same actions;
   4. the env classes advance by one per step; 5. the episode batches against the sequential captured single-episode loop and
   against themselves rebuilt from ``mjmpc_cost_terms_track`` per episode with the env time counted on the host; 6. untracked
   terms and ``None`` cost what they cost without this feature."""

import numpy as np
import pytest

import batched_cases as bc
import batched_terms_cases as btc
import tracking_cases as tc
from batched_cases import FILT, _torch, _vp
from cost_terms_cases import H, P, _engine, _mppi, _noise, bound, random_table

pytestmark = pytest.mark.gpu

DTYPES = ["f64", "f32"]


# ---- 1. the entry points ------------------------------------------------------------------------------------------------
# (P, H): two workgroups, the last partial; one step per particle; the controlled env's step
SHAPES = [(24, 5), (8, 1), (1, 1)]


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
@pytest.mark.parametrize("d_obs,A,K", [(10, 1, 5), (43, 7, 37), (43, 7, 128)])
def test_track_kernel_matches_the_restatement(d_obs, A, K, f32):
    """N = 3 < H: clamp and wrap both occur inside one rollout; N = 40; counters 0, N - 2 and 10 N + 1, bias 0 and -1 (at counter
    0 a base of -1: before the first row)."""
    torch = _torch()
    rng = np.random.default_rng(3000 * d_obs + 30 * A + K)
    tdt = btc.tdtype(f32)
    settings = [(0, 1), (1, 0), (1, 1), (0, 0)]                 # (keep_builtin, terminal), taken in turn
    turn = 0
    for Pn, Hn in SHAPES:
        nobs_h = rng.uniform(-5.0, 5.0, (Pn, Hn, d_obs))
        act_h = rng.uniform(-5.0, 5.0, (Pn, Hn, A))
        nobs, act = torch.from_numpy(nobs_h).to(tdt).cuda(), torch.from_numpy(act_h).to(tdt).cuda()
        nobs_seen, act_seen = nobs.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        for N in (3, 40):
            table, ref = tc.track_rows(rng, random_table(rng, K, d_obs, A), N)
            d_tab, d_ref = torch.from_numpy(table).cuda(), torch.from_numpy(ref).cuda()
            for now in (0, N - 2, 10 * N + 1):
                for bias in (0, -1):
                    for periodic in (0, 1):
                        keep, terminal = settings[turn % 4]
                        turn += 1
                        advance = int((Pn, Hn) == (1, 1) and turn % 2 == 0)
                        cin = rng.uniform(-3.0, 3.0, (Pn, Hn))
                        if Pn * Hn >= 15:               # an incoming +inf and an incoming NaN: both leave as +inf
                            cin.reshape(-1)[4], cin.reshape(-1)[Pn * Hn - 2] = np.inf, np.nan
                        costs = torch.from_numpy(cin).to(tdt).cuda()
                        cin_seen = costs.cpu().numpy().astype(np.float64)
                        counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
                        btc.cost_terms_track(d_tab, d_ref, periodic, counter, bias, advance, nobs, act, costs, keep, terminal, f32)
                        torch.cuda.synchronize()
                        where = (Pn, Hn, N, now, bias, periodic, keep, terminal, advance)
                        assert int(counter.item()) == now + advance, where
                        got = costs.cpu().numpy().astype(np.float64)
                        want, mag = tc.restate(table, ref, periodic, now + bias, nobs_seen, act_seen, cin_seen, keep, terminal)
                        bad = ~np.isfinite(cin_seen)
                        assert np.all(np.isposinf(got[bad])) and np.all(np.isposinf(want[bad])), where
                        err = np.abs(got[~bad] - want[~bad])
                        tol = bound(table, want, mag, f32)[~bad]
                        assert np.all(err <= tol), "%s: error %.3g over the bound by %.3g" % (where, err.max(), (err - tol).max())


def test_track_kernel_reads_the_row_the_contract_names():
    """One ABS row of weight 1 on a zero observation and one on a zero action: the cost IS the goal that was read."""
    torch = _torch()
    N, Hn = 3, 7
    ref = np.array([[1.0, 100.0], [2.0, 200.0], [4.0, 400.0]])
    table = np.array([[0, 0, 0, 1.0, 1.0, 0, 0, 1], [0, 1, 0, 1.0, 100.0, 0, 0, 2]], np.float64)
    d_tab, d_ref = torch.from_numpy(table).cuda(), torch.from_numpy(ref).cuda()
    nobs, act = torch.zeros((2, Hn, 1), dtype=torch.float64, device="cuda"), torch.zeros((2, Hn, 1), dtype=torch.float64, device="cuda")
    for now, periodic, obs_rows, act_rows in [
        (0, 0, [1, 2, 2, 2, 2, 2, 2], [0, 1, 2, 2, 2, 2, 2]),
        (0, 1, [1, 2, 0, 1, 2, 0, 1], [0, 1, 2, 0, 1, 2, 0]),
        (-3, 0, [0, 0, 0, 1, 2, 2, 2], [0, 0, 0, 0, 1, 2, 2]),
        (-3, 1, [1, 2, 0, 1, 2, 0, 1], [0, 1, 2, 0, 1, 2, 0]),
        (31, 1, [2, 0, 1, 2, 0, 1, 2], [1, 2, 0, 1, 2, 0, 1]),
        (2 ** 40 + 1, 0, [2] * 7, [2] * 7),
        (-2 ** 40, 0, [0] * 7, [0] * 7),
        (3 * 2 ** 40 + 2, 1, [0, 1, 2, 0, 1, 2, 0], [2, 0, 1, 2, 0, 1, 2]),
    ]:
        costs = torch.zeros((2, Hn), dtype=torch.float64, device="cuda")
        counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
        btc.cost_terms_track(d_tab, d_ref, periodic, counter, 0, 0, nobs, act, costs, 0, 1, False)
        want = ref[obs_rows, 0] + ref[act_rows, 1]
        assert np.array_equal(costs.cpu().numpy(), np.stack([want, want])), (now, periodic)


# (E, P, H): workgroups that straddle episodes; H above the 64-element chunk; several particles per workgroup and episodes of
# fewer particles than a workgroup holds; one particle per episode
BATCH_KERNEL_SHAPES = [(3, 8, 5), (2, 8, 70), (4, 3, 7), (3, 1, 64)]


@pytest.mark.parametrize("f32", [False, True], ids=DTYPES)
def test_track_batch_kernel_equals_the_single_kernel_per_episode(f32):
    torch = _torch()
    rng = np.random.default_rng(77)
    tdt = btc.tdtype(f32)
    d_obs, A, K, N = 11, 2, 9, 6
    for E, Pn, Hn in BATCH_KERNEL_SHAPES:
        n = E * Pn
        nobs = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, d_obs))).to(tdt).cuda()
        act = torch.from_numpy(rng.uniform(-5.0, 5.0, (n, Hn, A))).to(tdt).cuda()
        gseq_h = np.cumprod([1.0] + [0.93] * (Hn - 1))
        gseq = torch.from_numpy(gseq_h).cuda()
        first, ref0 = tc.track_rows(rng, random_table(rng, K, d_obs, A), N)
        for tab_pe, ref_pe, periodic, now, bias in [(0, 0, 0, 0, 0), (1, 1, 1, 4, -1), (0, 1, 0, 3, 0), (1, 0, 1, 61, 0)]:
            tables = np.stack([first] * (E if tab_pe else 1))
            refs = np.stack([ref0] * (E if ref_pe else 1))
            if tab_pe:
                tables[1:, :, 3] = rng.uniform(-2.0, 2.0, (E - 1, K))
                tables[1:, :, 4] = rng.uniform(-5.0, 5.0, (E - 1, K))
            if ref_pe:
                refs[1:] = rng.uniform(-5.0, 5.0, (E - 1,) + ref0.shape)
            d_tabs, d_refs = torch.from_numpy(np.ascontiguousarray(tables)).cuda(), torch.from_numpy(np.ascontiguousarray(refs)).cuda()
            counter = torch.full((1,), now, dtype=torch.int64, device="cuda")
            cin = rng.uniform(-3.0, 3.0, (n, Hn))
            cin.reshape(-1)[4], cin.reshape(-1)[n * Hn - 2] = np.inf, np.nan
            d_cin = torch.from_numpy(cin).to(tdt).cuda()
            want = d_cin.clone()
            for e in range(E):
                rows = slice(e * Pn, (e + 1) * Pn)
                btc.cost_terms_track(d_tabs[e if tab_pe else 0], d_refs[e if ref_pe else 0], periodic, counter, bias, 0, nobs[rows],
                                     act[rows], want[rows], 1, 1, f32)
            got, q0 = d_cin.clone(), torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            btc.cost_terms_track_batch(d_tabs, d_refs, periodic, counter, bias, E, nobs, act, got, 1, 1, f32, gseq, q0)
            torch.cuda.synchronize()
            where = (E, Pn, Hn, tab_pe, ref_pe, periodic, now, bias)
            got_h = got.cpu().numpy()
            assert int(counter.item()) == now, where                # (the batch entry never advances)
            assert np.array_equal(got_h, want.cpu().numpy()), where
            assert np.array_equal(q0.cpu().numpy(), btc.numpy_q0(got_h, gseq_h)), where
            assert np.isposinf(got_h.reshape(-1)[4]) and np.isposinf(got_h.reshape(-1)[n * Hn - 2]), where
            assert np.sum(~np.isfinite(got_h)) == 2, where


# ---- 2. a constant reference is a constant target -------------------------------------------------------------------------
def _constant_pair(eng, N, periodic):
    from mjmpc_amd.envs.cost_terms import CostTerms
    goal = [0.03, -0.02, 0.05]
    a = CostTerms(eng)
    a.square(obs="qpos", index=0, weight=2.0, target=0.3)
    a.norm(obs="site_minus_target", weight=4.0, target=goal)
    a.abs(action=0, weight=0.05, target=0.1)
    a.cos(obs="qpos", index=0, weight=0.3, target=0.2)
    a.square(obs="qvel", index=0, weight=0.5, terminal=True, target=-0.25)
    b = CostTerms(eng)
    b.square(obs="qpos", index=0, weight=2.0, reference=np.full(N, 0.3), periodic=periodic)
    b.norm(obs="site_minus_target", weight=4.0, reference=np.tile(goal, (N, 1)), periodic=periodic)
    b.abs(action=0, weight=0.05, reference=np.full(N, 0.1), periodic=periodic)
    b.cos(obs="qpos", index=0, weight=0.3, reference=np.full(N, 0.2), periodic=periodic)
    b.square(obs="qvel", index=0, weight=0.5, terminal=True, reference=np.full(N, -0.25), periodic=periodic)
    return a, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_a_constant_reference_equals_the_constant_target_bit_for_bit(model, dtype):
    eng = _engine(model, dtype)
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    for N, periodic, now in ((1, False, 0), (3, True, 0), (5, False, 2), (5, True, 1001)):
        constant, tracked = _constant_pair(eng, N, periodic)
        eng.set_cost_terms(constant)
        want = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
        eng.set_cost_terms(tracked)
        eng.set_track_step(now)
        got = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy()
        assert eng.track_step() == now                          # (a plan does not advance the env time)
        assert np.all(np.isfinite(want)) and np.all(want > 0)
        assert np.array_equal(got, want), (N, periodic, now, np.abs(got - want).max())
    eng.close()


# ---- 3. closed loops ------------------------------------------------------------------------------------------------------
def _loop(model, dtype, make_terms, mode, T=6):
    """``T`` control steps of MPPI on an engine that is its own real env: ``mode`` 'eager', 'graph' (hipGraph replay) or 'tape'.
    -> actions [T][A], real costs [T], real next observations [T][d_obs], final env time, launch_mode, the terms."""
    torch = _torch()
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    eng = _engine(model, dtype)
    terms = make_terms(eng)
    eng.set_cost_terms(terms)
    c = _mppi(eng)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    if mode != "eager":
        c.enable_graph(post_step=eng.step_state, tape=mode == "tape")
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize({})
        if mode == "eager":
            eng.step_state(np.array(a, np.float64))
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    if mode != "eager":
        assert c._graph is not None and not getattr(c, "graph_fallback", False) and not c._mono
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), now=eng.track_step(),
               launch_mode=getattr(c, "launch_mode", None), table=terms.table(), ref=terms.reference_table(),
               periodic=terms.periodic)
    assert eng.env_resets() == 0
    eng.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_eager_graph_and_tape_loops_agree_and_cost_the_row_of_their_step(model, dtype):
    T = 6

    def make(eng):                  # N = 5 < T + H: the plans run off the end of the reference; observation and action rows
        return tc.tracked_reach_terms(eng, periodic=model == "reacher", N=5)
    eager, graph, tape = (_loop(model, dtype, make, mode, T) for mode in ("eager", "graph", "tape"))
    assert np.all(np.isfinite(eager["acts"])) and np.abs(eager["acts"]).max() > 0
    for other in (graph, tape):
        for k in ("acts", "costs", "nobs"):
            assert np.array_equal(other[k], eager[k]), (k, np.abs(other[k].astype(float) - eager[k].astype(float)).max())
    assert eager["now"] == graph["now"] == tape["now"] == T
    assert graph["launch_mode"] == "hipGraph replay"
    # the real cost of step s: reference row s + 1 for the observation, row s for the action, no terminal rows
    table, ref, f32 = eager["table"], eager["ref"], dtype == "f32"
    seen = np.float32 if f32 else np.float64
    for s in range(T):
        o = eager["nobs"][s].astype(np.float64).reshape(1, 1, -1)
        a = eager["acts"][s].astype(seen).astype(np.float64).reshape(1, 1, -1)
        want, mag = tc.restate(table, ref, eager["periodic"], s, o, a, np.zeros((1, 1)), False, False)
        assert abs(float(eager["costs"][s]) - want[0, 0]) <= bound(table, want, mag, f32)[0, 0], s
    # ... and it is not the cost of a goal that stands still
    # (step 4 of N = 5: rows 4 / 4 clamped and 0 / 4 periodic, against rows 1 / 0 at time 0)
    frozen, _ = tc.restate(table, ref, eager["periodic"], 0, eager["nobs"][4].astype(np.float64).reshape(1, 1, -1),
                           eager["acts"][4].astype(np.float64).reshape(1, 1, -1), np.zeros((1, 1)), False, False)
    assert abs(float(eager["costs"][4]) - frozen[0, 0]) > 1e-3 * abs(frozen[0, 0])


def test_the_tape_survives_tracked_terms_without_action_rows():
    """No row reads an action: ``step_state`` issues no torch op, the captured iteration is library calls only - the advance
    of the env time among them - and runs from its launch tape."""
    def make(eng):
        return tc.tracked_reach_terms(eng, N=5, actions=False)
    tape, eager = _loop("cartpole", "f64", make, "tape"), _loop("cartpole", "f64", make, "eager")
    assert tape["launch_mode"].startswith("launch tape"), tape["launch_mode"]
    assert tape["now"] == 6 and np.array_equal(tape["acts"], eager["acts"]) and np.array_equal(tape["costs"], eager["costs"])


@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_a_host_driven_loop_with_set_track_step_gives_the_same_actions(model):
    """The controlled env is another engine: the rollout engine cannot see its steps and is told the env time."""
    torch = _torch()
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    T = 6

    def make(eng):
        return tc.tracked_reach_terms(eng, N=5)
    own = _loop(model, "f64", make, "eager", T)
    real, sim = _engine(model), _engine(model)
    for eng in (real, sim):
        eng.set_cost_terms(make(eng))
    c = _mppi(sim)
    c.rollout_fn = make_device_rollout_fn(sim)
    c.set_sim_state_fn = sim.set_env_state
    acts, costs = [], []
    for k in range(T):
        sim.set_track_step(k)
        a, _ = c.optimize(real.get_state_device())
        real.step_state(np.array(a, np.float64))
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(real._buf["step_cost"].cpu().numpy()[0])
    assert real.track_step() == T and sim.track_step() == T - 1    # (the sim engine only planned)
    assert np.array_equal(np.array(acts), own["acts"]) and np.array_equal(np.array(costs), own["costs"])
    real.close()
    sim.close()


# ---- 4. the env classes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_env_steps_advance_the_env_time_by_one(model):
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.synthetic_env import CartPoleEnv
    eng = _engine(model)
    terms = tc.tracked_reach_terms(eng, N=4, periodic=True)
    table, ref = terms.table(), terms.reference_table()
    eng.set_cost_terms(terms)
    env = (Reacher7DOFEnv if model == "reacher" else CartPoleEnv)(engine=eng)
    env.reset(seed=1)
    assert eng.track_step() == 0                                    # (making and resetting an env plans, it does not step)
    a = 0.3 * np.ones(eng.d_action)
    for s in range(6):
        ob, rew, _, _ = env.step(a)
        assert eng.track_step() == s + 1
        want, mag = tc.restate(table, ref, True, s, np.asarray(ob, float).reshape(1, 1, -1), a.reshape(1, 1, -1), np.zeros((1, 1)),
                               False, False)
        assert abs(-rew - want[0, 0]) <= bound(table, want, mag, False)[0, 0], s
    # a plan in between leaves the time alone; a guarded rollout of another shape cannot be one env step
    eng.rollout_device(P, H, np.zeros((H, eng.d_action)), _noise(eng))
    assert eng.track_step() == 6
    with pytest.raises(ValueError, match="one particle and one step"):
        with eng.real_step_guard("test"):
            eng.rollout_device(2, 1, np.zeros((1, eng.d_action)), None)
    assert eng.track_step() == 6
    if model == "cartpole":                                         # the tree engine's own step
        eng.step(a)
        assert eng.track_step() == 7
    # set_env_state leaves the time alone, set_cost_terms starts it over
    eng.set_env_state(eng.get_env_state()[0])
    assert eng.track_step() == (7 if model == "cartpole" else 6)
    eng.set_track_step(123)
    assert eng.track_step() == 123
    eng.set_cost_terms(terms)
    assert eng.track_step() == 0
    eng.set_cost_terms(None)
    with pytest.raises(RuntimeError, match="tracked"):
        eng.track_step()
    with pytest.raises(RuntimeError, match="tracked"):
        eng.set_track_step(1)
    eng.close()


# ---- 5. the episode batches -----------------------------------------------------------------------------------------------
SEEDS = [123 + i * 12345 for i in range(3)]
DMD = bc.case("BatchedDMDMPC", "DMDMPC", ("lam", "step_size", "init_cov", "beta"),
              lambda dtype: dict(update_cov=True, noise_dtype=dtype), extra=("cov_action", "cov"))
MPPIQ = bc.case("BatchedMPPIQ", "MPPIQ", ("beta", "step_size", "init_cov", "td_lam"),
                lambda dtype: dict(alpha=1, time_based_weights=True, noise_dtype=dtype))
# every class with per-episode settings (tests/test_batched_terms_gpu.py's values)
CASES = dict(
    BatchedMPPI=(bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype)),
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
N_REF = 6


def _episode_terms(eng, e, periodic):
    """Episode e's tracked terms: the rows of every episode, goals of its own."""
    return tc.tracked_reach_terms(eng, ref_scale=1.0 + 0.5 * e, periodic=periodic, N=N_REF)


def _make(cls, name, E, Pn, Hn, dtype, per_episode, periodic, now=None, cov_type=None):
    case, hyper = CASES[cls]
    raw, states, kind = btc.model(name, E)
    b = bc.make_batch(case, raw, states, SEEDS[:E], Pn, Hn, [v[:E] for v in hyper], dtype, engine=kind, cov_type=cov_type)
    b.set_cost_terms([_episode_terms(b.engine, e, periodic) for e in range(E)] if per_episode
                     else _episode_terms(b.engine, 0, periodic))
    if now is not None:
        b.set_track_step(now)
    return case, b


def _single(case, kind, raw, state, seed, Pn, Hn, T, hyper, dtype, make_terms, now, cov_type=None):
    """The sequential single-episode loop: an engine of its own with the same tracked terms, ``make_device_rollout_fn`` and
    ``enable_graph(post_step=engine.step_state)``, the env time set to ``now``."""
    torch = _torch()
    from mjmpc_amd import control
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    eng = btc.engine(raw, kind, dtype)
    eng.set_env_state(dict(state))
    eng.set_cost_terms(make_terms(eng))
    if now:
        eng.set_track_step(now)
    kw = dict(zip(case.hyper, hyper), **case.single_kw(dtype))
    if cov_type is not None:
        kw["cov_type"] = cov_type
    c = getattr(control, case.single)(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=Hn,
                                      base_action="null", num_particles=Pn, gamma=case.gamma, n_iters=1,
                                      action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=seed,
                                      noise_mode="device", **kw)
    c.rollout_fn = make_device_rollout_fn(eng)
    c.set_sim_state_fn = lambda s: None
    c.enable_graph(post_step=eng.step_state)
    acts, costs, nobs = [], [], []
    for _ in range(T):
        a, _ = c.optimize(None)
        torch.cuda.synchronize()
        acts.append(np.array(a, np.float64))
        costs.append(eng._buf["step_cost"].cpu().numpy()[0])
        nobs.append(eng._buf["step_obs"].cpu().numpy().copy())
    out = dict(acts=np.array(acts), costs=np.array(costs), nobs=np.array(nobs), mean=bc._host(c.mean_action),
               state=eng.get_state_device(), now=eng.track_step())
    assert eng.env_resets() == 0, "the single path's real env reset"
    eng.close()
    return out


def _check_batch_against_sequential_loops(cls, name, E, Pn, Hn, now, per_episode, cov_type=None):
    """Episode e of the batch against the sequential captured single-episode loop, bit for bit, over T = 4 steps; a case with
    ``now`` starts at that env time (``set_track_step``) and is periodic."""
    T, dtype, periodic = 4, "f64", now != 0
    case, b = _make(cls, name, E, Pn, Hn, dtype, per_episode, periodic, now or None, cov_type=cov_type)
    hyper = CASES[cls][1]
    out = bc.run_batch(case, b, T)
    assert np.all(np.isfinite(out["acts"])) and np.all(np.isfinite(out["costs"])) and np.abs(out["acts"]).max() > 0
    raw, states, kind = btc.model(name, E)
    for e in range(E):
        one = _single(case, kind, raw, states[e], SEEDS[e], Pn, Hn, T, [v[e] for v in hyper], dtype,
                      lambda eng, e=e: _episode_terms(eng, e if per_episode else 0, periodic), now, cov_type=cov_type)
        assert one["now"] == now + T
        print("%s %s E%d P%d H%d episode %d: actions differ by at most %.3g, real costs by %.3g"
              % (cls, name, E, Pn, Hn, e, np.abs(out["acts"][:, e] - one["acts"]).max(),
                 np.abs(out["costs"][:, e] - one["costs"]).max()))
        assert np.array_equal(out["acts"][:, e], one["acts"]), (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), e
        assert np.array_equal(out["mean"][e], one["mean"]), e
        for x, y in zip(bc._qpos_qvel(out["state"][e]), bc._qpos_qvel(one["state"])):
            assert np.array_equal(x, y), e


BATCH_CASES = pytest.mark.parametrize("E,Pn,Hn,now", [(3, 8, 5, 0), (2, 8, 70, 4)], ids=["3x8x5", "2x8x70"])


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@BATCH_CASES
@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batched_mppi_equals_the_sequential_captured_loop(name, E, Pn, Hn, now, per_episode):
    """With tracked terms the batch's step is the single-episode MPPI's general iteration in batch form - draw + filter, plain
    rollout, the terms, the general softmax update (``BatchedMPPI._launches_tracked``) - so the pair is identical on both
    engines.  (With constant terms the batch keeps its fused update and differs from that loop in the last bits: 3e-14 on
    the cart-pole, 3e-13 on the reacher, measured.)"""
    _check_batch_against_sequential_loops("BatchedMPPI", name, E, Pn, Hn, now, per_episode)


@pytest.mark.parametrize("per_episode", [False, True], ids=["shared", "per_episode"])
@BATCH_CASES
@pytest.mark.parametrize("cls", ["BatchedDMDMPC", "BatchedMPPIQ"])
def test_batches_that_sum_in_their_update_equal_the_sequential_captured_loop(cls, E, Pn, Hn, now, per_episode):
    """DMD-MPC and MPPIQ read the per-step costs and sum them in their update kernels on both paths: the classes
    whose batch with constant terms is the single-episode loop bit for bit are so with tracked terms."""
    _check_batch_against_sequential_loops(cls, "cartpole", E, Pn, Hn, now, per_episode,
                                          cov_type="full" if cls == "BatchedDMDMPC" else None)


def _as_separate_tracked_launches(b):
    """Replace the batch's two engine launches by their restatement from the parts, the env time counted ON THE HOST:
    ``_rollout`` by the ``_obs`` rollout entry without a cost-to-go, ``mjmpc_cost_terms_track`` per episode with that episode's
    table and reference at env time ``num_steps + _track_bias``, and the cost-to-go from numpy; ``_env_step`` by
    ``step_shard_states`` and ``mjmpc_cost_terms_track`` per episode at the same env time.  So the batch's own device counter
    must stand at ``num_steps`` behind the draw and at ``num_steps + 1`` behind the update, in every class."""
    torch = _torch()
    from mjmpc_amd import _lib
    tables, K, per_episode, keep, reads = b._terms
    refs, N, R, ref_per_episode, periodic = b._track
    E, Pn, Hn = b.num_episodes, b.num_particles, b.horizon
    f32 = b.dtype == "f32"
    gseq_h = b._gseq.cpu().numpy()
    counter = torch.zeros(1, dtype=torch.int64, device=b.device)

    def track(e, nobs, act, costs, terminal):
        counter.fill_(b.num_steps + b._track_bias)
        btc.cost_terms_track(tables[e if per_episode else 0], refs[e if ref_per_episode else 0], periodic, counter, 0, 0, nobs,
                             act if reads else None, costs, keep, terminal, f32)

    def rollout(s, noise=None, filtered=True, gseq=True, q0=True):
        nobs = torch.empty((E * Pn, Hn, b.d_obs), dtype=b._tdtype, device=b.device)
        _lib.check(b._fn("rollout_fused_batch_obs")(
            b.engine._h, b._code, E * Pn, Hn, _vp(b._means), _vp(b._noise if noise is None else noise),
            _vp(b._coeffs) if filtered else None, None, _vp(b._costs), _vp(b._actions), None, _vp(nobs), s))
        for e in range(E):
            rows = slice(e * Pn, (e + 1) * Pn)
            track(e, nobs[rows], b._actions[rows], b._costs[rows], 1)
        if q0:
            torch.cuda.synchronize()
            b._q0.copy_(torch.from_numpy(btc.numpy_q0(b._costs.cpu().numpy(), gseq_h)))

    def env_step(act, cost, nobs, s):
        _lib.check(b._fn("step_shard_states")(b.engine._h, b._code, _vp(act), _vp(cost), _vp(nobs), s))
        act_t = act.to(b._tdtype).contiguous()
        for e in range(E):
            track(e, nobs[e:e + 1].view(1, 1, -1), act_t[e:e + 1].view(1, 1, -1), cost[e:e + 1].view(1, 1), 0)
    b._rollout = rollout
    b._env_step = env_step
    return b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cls,name", [(c, "cartpole") for c in sorted(CASES)] + [("BatchedMPPI", "reacher")])
def test_every_batch_class_equals_its_separate_tracked_launches(cls, name, dtype):
    E, Pn, Hn, T = 3, 8, 5, 3
    runs = []
    for separate in (False, True):
        case, b = _make(cls, name, E, Pn, Hn, dtype, True, True, now=2)
        runs.append(bc.run_batch(case, _as_separate_tracked_launches(b) if separate else b, T))
    assert np.all(np.isfinite(runs[0]["acts"])) and np.abs(runs[0]["acts"]).max() > 0
    btc.assert_same_runs(runs[0], runs[1], "%s %s %s" % (cls, name, dtype))


def test_batch_set_track_step_and_reset():
    """``set_track_step(n)``: the next plan is made at env time n; ``reset()``: env time = step count again."""
    E, Pn, Hn, T = 3, 8, 5, 3
    raw, states, _ = btc.model("cartpole", E)

    def fresh(now=None):
        return _make("BatchedMPPI", "cartpole", E, Pn, Hn, "f64", True, False, now)[1]
    b = fresh()
    first = b.run(T)
    assert b._track_bias == 0 and b.num_steps == T
    # rewound to env time 0 while the step count (the noise key) goes on; reset() with the start states is the fresh batch again
    b.set_track_step(0)
    assert b._track_bias == -T
    b.run(1)
    b.reset()
    assert b._track_bias == 0 and b.num_steps == 0
    b.set_states([dict(s) for s in states])
    again = b.run(T)
    for x, y in zip(again, first):
        assert np.array_equal(x, y)
    b.close()
    # a batch that starts at env time 3 costs its first real step with reference row 4, not row 1
    late = fresh(now=3)
    assert late._track_bias == 3
    out = late.run(T)
    late.close()
    assert not np.array_equal(out[1], first[1]) and np.all(np.isfinite(out[1]))


# ---- 6. costs unchanged without tracking ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("model", ["cartpole", "reacher"])
def test_untracked_terms_and_none_cost_what_they_did(model, dtype):
    torch = _torch()
    from cost_terms_cases import mixed_terms
    from mjmpc_amd.envs.cost_terms import CostTerms
    eng = _engine(model, dtype)
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    builtin = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    eng.set_cost_terms(tc.tracked_reach_terms(eng))
    tracked = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().copy()
    assert eng._track_step is not None and eng._track_ref is not None
    # untracked terms behind tracked ones: the existing entry's costs on the same observations and actions
    plain = mixed_terms(eng, CostTerms)
    eng.set_cost_terms(plain)
    assert eng._track_step is None and eng._track_ref is None
    costs, act, _, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
    got = costs.cpu().numpy().copy()
    want = torch.zeros_like(costs)
    btc.cost_terms(torch.from_numpy(plain.table()).cuda(), nobs, act, want, False, True, dtype == "f32")
    torch.cuda.synchronize()
    assert np.array_equal(got, want.cpu().numpy()) and not np.array_equal(got, tracked)
    cost, step_obs = eng.step_state(np.zeros(eng.d_action))           # (no counter to advance: the old launch)
    torch.cuda.synchronize()
    assert np.isfinite(float(cost.cpu()[0]))
    eng.close()
    # None: the built-in cost, exactly
    eng = _engine(model, dtype)
    eng.set_cost_terms(tc.tracked_reach_terms(eng))
    eng.set_cost_terms(None)
    assert eng._track_step is None and eng._terms_dev is None
    assert np.array_equal(eng.rollout_device(P, H, mean, noise)[0].cpu().numpy(), builtin)
    eng.close()
