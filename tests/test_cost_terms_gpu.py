"""GPU: user-defined cost terms - ``mjmpc_cost_terms`` against the numpy restatement of the row semantics
(tests/cost_terms_cases.py) within the derived bound, the anchor to the built-in reach cost of both engines, real steps
without terminal rows, every controller over an engine with terms, and the guards on the fused launches."""
import ctypes

import numpy as np
import pytest

from cost_terms_cases import H, P, _engine, _noise, bound, mixed_terms, random_table, restate

pytestmark = pytest.mark.gpu

FILT = [0.25, 0.8, 0.0]


def _torch():
    import torch
    return torch


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- 1. the kernel against the restatement ------------------------------------------------------------------------------
def _run_kernel(table, nobs, act, cin, keep, terminal, f32):
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    tdt = torch.float32 if f32 else torch.float64
    d_nobs = torch.from_numpy(nobs).to("cuda", tdt)
    d_act = None if act is None else torch.from_numpy(act).to("cuda", tdt)
    d_cost = torch.from_numpy(cin).to("cuda", tdt)
    d_tab = torch.from_numpy(np.ascontiguousarray(table)).cuda()
    Pn, Hn, d_obs = nobs.shape
    A = 0 if act is None else act.shape[2]
    _lib.check(lib.mjmpc_cost_terms(_lib.F32 if f32 else _lib.F64, Pn, Hn, d_obs, A, _vp(d_nobs), _vp(d_act), _vp(d_tab),
                                    len(table), int(keep), int(terminal), _vp(d_cost),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    # what the kernel saw: the inputs in its storage type
    return (d_cost.cpu().numpy().astype(np.float64), d_nobs.cpu().numpy().astype(np.float64),
            None if act is None else d_act.cpu().numpy().astype(np.float64))


# (P, H): below, at and just above one workgroup's 64 elements, not a multiple of the wavefront; several workgroups
SHAPES = [(1, 1), (5, 3), (8, 8), (13, 5), (67, 7)]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("d_obs,A,K", [(10, 1, 1), (10, 7, 128), (43, 1, 128), (43, 7, 1), (43, 7, 37)])
def test_kernel_matches_the_restatement(d_obs, A, K, f32):
    rng = np.random.default_rng(1000 * d_obs + 10 * A + K)
    for Pn, Hn in SHAPES:
        for kind0 in range(4 if K == 1 else 1):         # K = 1: every kind once
            table = random_table(rng, K, d_obs, A)
            if K == 1:
                table[0, 0], table[0, 5] = kind0, float(kind0 == 2)
            nobs = rng.uniform(-5.0, 5.0, (Pn, Hn, d_obs))              # |r| <= 10 with targets in [-5, 5]
            act = rng.uniform(-5.0, 5.0, (Pn, Hn, A))
            for keep, terminal in ((0, 1), (1, 0), (1, 1), (0, 0)):
                cin = rng.uniform(-3.0, 3.0, (Pn, Hn))
                if f32:
                    cin = cin.astype(np.float32).astype(np.float64)
                bad = []
                if Pn * Hn >= 15:                       # an incoming +inf and an incoming NaN: both leave as +inf
                    cin.reshape(-1)[4], cin.reshape(-1)[Pn * Hn - 2] = np.inf, np.nan
                    bad = [4, Pn * Hn - 2]
                got, nobs_seen, act_seen = _run_kernel(table, nobs, act, cin, keep, terminal, f32)
                want, mag = restate(table, nobs_seen, act_seen, cin, keep, terminal)
                tol = bound(table, want, mag, f32)
                ok = np.ones(Pn * Hn, bool)
                ok[np.array(bad, int)] = False
                g, w = got.reshape(-1), want.reshape(-1)
                assert np.all(np.isposinf(g[~ok])) and np.all(np.isposinf(w[~ok]))
                assert np.all(np.isfinite(g[ok]))                       # (the neighbours are untouched)
                err = np.abs(g[ok] - w[ok])
                assert np.all(err <= tol.reshape(-1)[ok]), \
                    "(%d, %d) d_obs %d A %d K %d keep %d terminal %d: error %.3g over the bound by %.3g" % (
                        Pn, Hn, d_obs, A, K, keep, terminal, err.max(), (err - tol.reshape(-1)[ok]).max())


def test_kernel_terminal_rows_and_a_closing_norm_group():
    """Terminal rows with ``terminal`` 0 and 1, also at H = 1 (every step is the last), and a norm group as the table's last
    rows: the rows change the result exactly where they should."""
    rng = np.random.default_rng(7)
    d_obs, A = 10, 1
    table = np.array([[1, 0, 2, 0.5, 0.1, 0, 0, 0],
                      [0, 1, 0, 3.0, 0.0, 0, 1, 0],                     # terminal
                      [2, 0, 7, 2.0, 0.2, 1, 1, 0], [2, 0, 8, 9.0, 0.0, 1, 1, 0],       # a terminal group (weight: the first row's)
                      [2, 0, 4, 1.5, 0.0, 2, 0, 0], [2, 0, 5, 1.5, 1.0, 2, 0, 0]], float)  # the closing group
    for Pn, Hn in ((6, 1), (9, 4)):
        nobs, act = rng.uniform(-5, 5, (Pn, Hn, d_obs)), rng.uniform(-5, 5, (Pn, Hn, A))
        cin = np.zeros((Pn, Hn))
        out = {}
        for terminal in (0, 1):
            got, _, _ = _run_kernel(table, nobs, act, cin, 0, terminal, False)
            want, mag = restate(table, nobs, act, cin, 0, terminal)
            assert np.all(np.abs(got - want) <= bound(table, want, mag, False))
            out[terminal] = got
        plain = 0.5 * (nobs[..., 2] - 0.1) ** 2 + 1.5 * np.sqrt(nobs[..., 4] ** 2 + (nobs[..., 5] - 1.0) ** 2)
        last = 3.0 * np.abs(act[..., 0]) + 2.0 * np.sqrt((nobs[..., 7] - 0.2) ** 2 + nobs[..., 8] ** 2)
        np.testing.assert_allclose(out[0], plain, rtol=1e-14)
        np.testing.assert_allclose(out[1][:, -1], (plain + last)[:, -1], rtol=1e-14)
        assert np.array_equal(out[1][:, :-1], out[0][:, :-1])
        assert np.all(out[1][:, -1] > out[0][:, -1])


# ---- 2. the anchor: builtin_reach() against the oracle-checked built-in cost ---------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("model", ["reacher", "cartpole", "tray"])
def test_builtin_reach_terms_equal_the_builtin_cost(model, dtype):
    from mjmpc_amd.envs.cost_terms import CostTerms
    eps = np.finfo(np.float32 if dtype == "f32" else np.float64).eps
    eng = _engine(model, dtype)
    mean, noise = np.zeros((H, eng.d_action)), _noise(eng)
    builtin = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().astype(np.float64)
    assert eng.diverged_substeps() == 0
    assert np.all(np.isfinite(builtin)) and np.all(builtin > 0)
    for keep, factor in ((False, 1.0), (True, 2.0)):
        eng.set_cost_terms(CostTerms.builtin_reach(eng, keep_builtin=keep))
        costs, act, obs, nobs = eng.rollout_device(P, H, mean, noise)            # (no observations asked for: the engine's own)
        assert obs is None and nobs is None and act is not None
        got = costs.cpu().numpy().astype(np.float64)
        assert eng.diverged_substeps() == 0
        err = np.abs(got - factor * builtin)
        assert np.all(err <= 8 * eps * builtin), "keep_builtin %s: %.3g eps" % (keep, (err / (eps * builtin)).max())
    eng.set_cost_terms(None)                                    # today's behaviour, exactly
    again = eng.rollout_device(P, H, mean, noise)[0].cpu().numpy().astype(np.float64)
    assert np.array_equal(again, builtin)
    # the reference-shaped rollout carries the term costs as rewards and its observations are untouched
    eng.set_cost_terms(CostTerms(eng).square(obs="qvel", weight=0.5).abs(action=True, weight=0.1))
    o, rew, a, _, _, no = eng.rollout(P, H, mean, noise)
    want, mag = restate(eng._cost_terms.table(), no, a, np.zeros((P, H)), False, True)
    tol = bound(eng._cost_terms.table(), want, mag, dtype == "f32")
    assert np.all(np.abs(-rew - want) <= tol)
    eng.close()


def test_closed_loop_rollouts_are_costed_by_the_terms():
    """``rollout_device(mode="closed_loop_linear")`` takes the second launch too."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    eng = _engine("reacher")
    terms = mixed_terms(eng, CostTerms)
    eng.set_cost_terms(terms)
    w = 0.01 * np.random.default_rng(5).standard_normal((eng.d_obs + 1, eng.d_action))
    costs, act, _, nobs = eng.rollout_device(P, H, w, _noise(eng), mode="closed_loop_linear", want_obs=True)
    got, act, nobs = (x.cpu().numpy() for x in (costs, act, nobs))
    want, mag = restate(terms.table(), nobs, act, np.zeros((P, H)), False, True)
    assert np.all(np.abs(got - want) <= bound(terms.table(), want, mag, False))
    eng.close()


# ---- 3. real steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["reacher", "cartpole"])
def test_real_steps_leave_terminal_rows_out(model):
    torch = _torch()
    from mjmpc_amd.envs.cost_terms import CostTerms
    from mjmpc_amd.envs.reacher_env import Reacher7DOFEnv
    from mjmpc_amd.envs.synthetic_env import CartPoleEnv
    eng = _engine(model)
    terms = CostTerms.builtin_reach(eng)
    terms.square(action=0, weight=0.1)
    terms.square(obs="qvel", weight=1e6, terminal=True)         # would swamp everything
    table = terms.table()
    eng.set_cost_terms(terms)
    env = (Reacher7DOFEnv if model == "reacher" else CartPoleEnv)(engine=eng)
    env.reset(seed=1)
    a = 0.5 * np.ones(eng.d_action)
    zero = np.zeros((1, 1))

    def check(cost, nobs, terminal):
        want, mag = restate(table, np.asarray(nobs, float).reshape(1, 1, -1), a.reshape(1, 1, -1), zero, False, terminal)
        assert abs(cost - want[0, 0]) <= bound(table, want, mag, False)[0, 0]
        return want[0, 0]

    for mode in ("raise", "ignore"):                            # the guard marks the step in the "ignore" mode too
        eng.on_env_reset = mode
        ob, rew, _, _ = env.step(a)
        check(-rew, ob, terminal=False)
    # the same engine as a planner: a one-step plan's only step is its last
    eng.on_env_reset = "raise"
    costs, _, _, nobs = eng.rollout_device(1, 1, a.reshape(1, -1), None, want_obs=True)
    c_plan = float(costs.cpu()[0, 0])
    with_t = check(c_plan, nobs.cpu().numpy(), terminal=True)
    without_t, _ = restate(table, nobs.cpu().numpy(), a.reshape(1, 1, -1), zero, False, False)
    # (the velocities are not zero after the step: the terminal row is most of the plan's cost and none of the real step's)
    assert with_t - without_t[0, 0] > 10 * without_t[0, 0]
    # the device-resident env
    cost, nobs = eng.step_state(a)
    torch.cuda.synchronize()
    check(float(cost.cpu()[0]), nobs.cpu().numpy(), terminal=False)
    eng.close()


# ---- 4. controllers -----------------------------------------------------------------------------------------------------
def _controller(kind, eng, **over):
    from mjmpc_amd import control
    kw = dict(d_state=eng.d_state, d_obs=eng.d_obs, d_action=eng.d_action, horizon=H, num_particles=P, n_iters=1, gamma=0.98,
              action_lows=eng.action_lows, action_highs=eng.action_highs, filter_coeffs=FILT, seed=11, base_action="null",
              noise_mode="device")
    if kind == "mppi":
        c = control.MPPI(init_cov=0.1, lam=0.05, step_size=0.8, alpha=1, **dict(kw, **over))
    elif kind == "cem":
        c = control.CEM(init_cov=0.1, elite_frac=0.25, step_size=0.8, beta=0.05, cov_type="diagonal", **dict(kw, **over))
    elif kind == "dmd":
        c = control.DMDMPC(init_cov=0.1, beta=0.05, lam=0.05, step_size=0.8, update_cov=False, cov_type="diagonal", **dict(kw, **over))
    elif kind == "rs":
        c = control.RandomShooting(init_cov=0.1, step_size=0.8, **dict(kw, **over))
    elif kind == "mppiq":
        c = control.MPPIQ(init_cov=0.1, beta=0.05, step_size=0.8, alpha=1, td_lam=0.9, time_based_weights=True,
                          noise_dtype="f64", **dict(kw, **over))
    else:
        kw.pop("base_action")
        c = control.PFMPC(cov_shift=0.05, cov_resample=0.1, base_action="null", lam=0.05, **dict(kw, **over))
    return c


def _attach(c, eng, spy=None):
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn
    fn = make_device_rollout_fn(eng)
    if spy is not None:
        inner = fn

        def fn(num_particles, horizon, mean, noise, mode):
            spy.append((mean.detach().cpu().numpy().copy(), noise.detach().cpu().numpy().astype(np.float64)))
            return inner(num_particles, horizon, mean, noise, mode)
        fn.accepts_device, fn.engine = True, eng
    c.rollout_fn = fn
    c.set_sim_state_fn = lambda s: None
    return c


def test_mppi_over_terms_matches_the_oracle_update_and_graph_equals_eager():
    torch = _torch()
    from oracle import controllers_ref as cr
    from mjmpc_amd.envs.cost_terms import CostTerms
    eng = _engine("reacher")
    terms = mixed_terms(eng, CostTerms)
    eng.set_cost_terms(terms)
    calls = []
    c = _attach(_controller("mppi", eng), eng, spy=calls)
    assert not hasattr(c.rollout_fn, "fused")
    for _ in range(2):
        c.optimize({})
    torch.cuda.synchronize()
    got = c.mean_action.copy()
    assert len(calls) == 2
    # the expected mean: the engine's own rollouts WITHOUT terms, their next observations and actions through the
    # restatement, then the oracle's MPPI update and shift
    plain = _engine("reacher")
    gseq = cr.gamma_seq(0.98, H)
    mean = np.zeros((H, eng.d_action))
    for mean_seen, noise in calls:
        np.testing.assert_allclose(mean_seen, mean, rtol=1e-9, atol=1e-12)
        _, _, act, _, _, nobs = plain.rollout(P, H, mean_seen, noise)
        costs, _ = restate(terms.table(), nobs, act, np.zeros((P, H)), False, True)
        mean = cr.mppi_update(costs, act, mean_seen, np.diag([0.1] * eng.d_action), gseq, 0.05, 1, 0.8)
        mean = cr.shift_mean(mean, "null")
    np.testing.assert_allclose(got, mean, rtol=1e-9, atol=1e-9)
    assert np.abs(got).max() > 1e-3
    plain.close()
    eng.close()

    def loop(graph, steps=3):
        e = _engine("reacher")
        e.set_cost_terms(mixed_terms(e, CostTerms))
        cc = _attach(_controller("mppi", e), e)
        if graph:
            cc.enable_graph()
        acts = [np.array(cc.optimize({})[0], np.float64) for _ in range(steps)]
        torch.cuda.synchronize()
        if graph:
            assert cc._graph is not None and not getattr(cc, "graph_fallback", False) and not cc._mono
        out = np.array(acts), cc.mean_action.copy()
        e.close()
        return out
    a_e, m_e = loop(False)
    a_g, m_g = loop(True)
    assert np.array_equal(a_g, a_e) and np.array_equal(m_g, m_e)


@pytest.mark.parametrize("kind", ["cem", "dmd", "rs", "mppiq", "pfmpc"])
def test_every_controller_runs_over_terms_and_the_terms_move_the_mean(kind):
    torch = _torch()
    from mjmpc_amd.envs.cost_terms import CostTerms

    def run(with_terms, graph):
        eng = _engine("cartpole")
        if with_terms:
            eng.set_cost_terms(mixed_terms(eng, CostTerms))
        c = _attach(_controller(kind, eng), eng)
        if graph:
            if not getattr(c, "_graph_capable", lambda: False)():
                eng.close()
                return None
            c.enable_graph()
        for _ in range(2):
            c.optimize({})
        torch.cuda.synchronize()
        assert eng.diverged_substeps() == 0
        mean = c.mean_action                                    # (PFMPC's device mode keeps it on the device)
        mean = np.array(mean.cpu().numpy() if hasattr(mean, "cpu") else mean, np.float64)
        eng.close()
        return mean

    eager = run(True, False)
    assert np.all(np.isfinite(eager))
    assert not np.array_equal(eager, run(False, False))
    graphed = run(True, True)                                   # (None: the class is not graph-capable)
    assert graphed is not None or kind == "pfmpc"
    if graphed is not None:
        assert np.all(np.isfinite(graphed))
        np.testing.assert_allclose(graphed, eager, rtol=1e-9, atol=1e-10)


# ---- 5. guards ----------------------------------------------------------------------------------------------------------
def test_mppi_that_would_take_the_one_launch_iteration_runs_the_generic_one():
    torch = _torch()
    from mjmpc_amd.envs.cost_terms import CostTerms
    eng = _engine("reacher")
    over = dict(num_particles=4096, horizon=32)
    probe = _attach(_controller("mppi", eng, **over), eng)
    probe.enable_graph()
    probe.optimize({})
    torch.cuda.synchronize()
    assert probe._mono                                          # without terms this configuration IS the one-launch iteration
    eng.close()

    eng = _engine("reacher")
    eng.set_cost_terms(CostTerms.builtin_reach(eng))
    c = _attach(_controller("mppi", eng, **over), eng)
    c.enable_graph()
    a, _ = c.optimize({})
    torch.cuda.synchronize()
    assert not c._mono and np.all(np.isfinite(a)) and np.abs(c.mean_action).max() > 0
    with pytest.raises(RuntimeError, match="set_cost_terms"):
        eng.mppi_step(4096, 32, *[None] * 12)
    with pytest.raises(RuntimeError, match="set_cost_terms"):
        eng.rollout_fused(4096, 32, None, None, None, None)
    eng.close()
