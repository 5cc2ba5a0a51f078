"""GPU: world positions of points as cost-term observations - ``mjmpc_points`` through both engines and the
episode batches.  The augmented rows keep the observation bit for bit; the points and differences are held to the C oracle's
kinematics at each row's own ``qpos`` (f64: 1e-9 absolute, the project's bound for observations; f32: the oracle is fed the f32
``qpos`` and one f32 ulp of the value is allowed on top, since the kernel computes in double and rounds once); the costs are
the restatement of the table over the augmented rows within its bound.

Measured on an MI355X over all cases and shapes (each case prints its own): worst |point - oracle| 2.1e-15 in f64 and 5.9e-8
in f32 (the door's points, about 1 m from the origin: half an f32 ulp)."""
import numpy as np
import pytest

import batched_terms_cases as tc
import points_cases as pc
import quad_cases as qc
from cost_terms_cases import REACHER_START, bound, restate

pytestmark = pytest.mark.gpu

# a lone row; ragged tiles inside a wavefront and across wavefronts; a full tile of two wavefronts' worth of rows
SHAPES = [(1, 1), (3, 5), (67, 3), (64, 8)]


def _torch():
    import torch
    return torch


def _engine(name, dtype="f64"):
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    raw, kind, points, differences = pc.case(name)
    eng = (ArmRolloutEngine if kind == "arm" else TreeRolloutEngine)(raw, dtype=dtype)
    if name == "reacher":
        eng.set_env_state(REACHER_START)
    elif name.startswith("random"):
        q = pc.random_qpos(raw, np.random.RandomState(77))
        eng.set_env_state(dict(qp=q, qv=np.zeros(raw.nv), target_pos=np.asarray(raw.target_pos, float)))
    else:
        from mjmpc_amd.models.synthetic import start_state
        st = start_state(name, raw)
        eng.set_env_state(dict(qp=st["qp"], qv=st["qv"], target_pos=st["target_pos"]))
    return eng, raw, points, differences


_ORACLES = {}


def _oracle(name):
    if name not in _ORACLES:
        raw, _, points, differences = pc.case(name)
        _ORACLES[name] = pc.Oracle(raw, *pc.resolved(raw, points, differences))
    return _ORACLES[name]


def _terms(eng, points, differences, keep_builtin=False):
    """The case's points and differences and rows of the kinds 0 .. 3 over them (what cost_terms_cases.restate states): a
    norm over the first difference, an ABS and a COS row on points, a row on an action and a terminal row on a point."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = pc.add_points(CostTerms(eng, keep_builtin=keep_builtin), points, differences)
    t.norm(obs=differences[0][0], index=[0, 1], weight=3.0, target=[0.01, -0.02])
    t.abs(obs=points[0][0], index=2, weight=0.7, target=0.3)
    t.cos(obs=points[1][0], index=0, weight=0.2)
    t.square(action=0, weight=0.05)
    t.square(obs="qvel", index=0, weight=0.01)
    t.square(obs=points[-1][0], weight=2.0, target=[0.1, 0.0, 0.2], terminal=True)
    return t


def _check_rows(name, eng, aug, nobs, f32):
    """The augmented rows ``aug`` [..][d_obs + n_extra] against the observations they came from and the oracle; -> worst error."""
    d, nq = eng.d_obs, eng._nq
    aug, nobs = aug.cpu().numpy(), nobs.cpu().numpy()
    assert aug.dtype == nobs.dtype == (np.float32 if f32 else np.float64)
    assert np.array_equal(aug[..., :d].view(np.uint8), nobs.view(np.uint8))             # bit for bit
    rows = aug.reshape(-1, aug.shape[-1]).astype(np.float64)
    oracle = _oracle(name)
    want = np.array([oracle(r[:nq]) for r in rows])
    got = rows[:, d:]
    assert got.shape == want.shape and np.all(np.isfinite(want))
    err = np.abs(got - want)
    tol = 2.0 ** -23 * np.abs(want) + 1e-9 if f32 else 1e-9
    assert np.all(err <= tol), "%s: worst %.3g (over the bound by %.3g)" % (name, err.max(), (err - tol).max())
    return err.max()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", pc.case_names())
def test_points_and_costs_against_the_oracle_and_the_restatement(name, dtype):
    torch = _torch()
    f32 = dtype == "f32"
    eng, raw, points, differences = _engine(name, dtype)
    A = eng.d_action
    rng = np.random.default_rng(5)
    worst = 0.0
    for P, H in SHAPES:
        mean, noise = np.zeros((H, A)), 0.3 * rng.standard_normal((P, H, A))
        eng.set_cost_terms(None)
        builtin = eng.rollout_device(P, H, mean, noise)[0].clone()
        terms = _terms(eng, points, differences)
        table = terms.table()
        eng.set_cost_terms(terms)
        costs, act, obs, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        torch.cuda.synchronize()
        assert nobs.shape == (P, H, eng.d_obs)                                  # the returned observations keep their width
        aug = eng.cost_observations()
        assert aug.shape == (P, H, eng.d_obs + terms.n_extra)
        worst = max(worst, _check_rows(name, eng, aug, nobs, f32))
        aug_h, act_h = aug.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        want, mag = restate(table, aug_h, act_h, np.zeros((P, H)), False, True)
        got = costs.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want) <= bound(table, want, mag, f32)), (P, H)
        # keep_builtin and incoming costs that are not finite, through the same launch path
        kept = _terms(eng, points, differences, keep_builtin=True)
        eng.set_cost_terms(kept)
        cin = builtin.clone()
        bad = [1, P * H - 2] if P * H >= 15 else []
        for k, v in zip(bad, (float("inf"), float("nan"))):
            cin.view(-1)[k] = v
        cin_h = cin.cpu().numpy().astype(np.float64)
        eng._launch_cost_terms(P, H, nobs, act, cin, terminal=False)
        torch.cuda.synchronize()
        assert np.array_equal(eng.cost_observations().cpu().numpy(), aug.cpu().numpy())
        want, mag = restate(table, aug_h, act_h, cin_h, True, False)
        got = cin.cpu().numpy().astype(np.float64).reshape(-1)
        ok = np.ones(P * H, bool)
        ok[bad] = False
        assert np.all(np.isposinf(got[~ok])) and np.all(np.isposinf(want.reshape(-1)[~ok]))
        assert np.all(np.abs(got[ok] - want.reshape(-1)[ok]) <= bound(table, want, mag, f32).reshape(-1)[ok]), (P, H)
    print("%s %s: worst |point - oracle| %.3g" % (name, dtype, worst))
    # set_cost_terms(None): the engine without terms, bit for bit
    P, H = SHAPES[-1]
    eng.set_cost_terms(None)
    again = eng.rollout_device(P, H, mean, noise)[0]
    assert np.array_equal(again.cpu().numpy(), builtin.cpu().numpy())
    with pytest.raises(RuntimeError, match="cost_observations"):
        eng.cost_observations()
    eng.close()


def _entry_terms(which, eng, points, differences):
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = pc.add_points(CostTerms(eng), points, differences)
    if which == "track":
        ref = np.stack([np.linspace(0.2, 0.5, 12), np.linspace(0.0, -0.2, 12), np.full(12, 0.3)], axis=1)
        t.square(obs=points[0][0], weight=2.0, reference=ref)
        t.abs(obs=differences[0][0], index=1, weight=0.5)
    elif which == "rate":
        t.outside(obs=points[1][0], index=2, low=0.35, high=0.45, weight=10.0)
        t.norm(obs=differences[0][0], weight=1.5)
    else:
        Q = np.array([[2.0, 0.3, -0.1, 0.0], [0.3, 1.0, 0.2, 0.1], [-0.1, 0.2, 3.0, 0.0], [0.0, 0.1, 0.0, 0.5]])
        t.quadratic(parts=[dict(obs=differences[0][0], target=[0.0, 0.0, 0.05]), dict(action=0)], matrix=Q, weight=1.5)
        t.linear(obs=points[0][0], index=2, weight=-0.4)
    return t


@pytest.mark.parametrize("which", ["track", "rate", "quad"])
@pytest.mark.parametrize("name", ["reacher", "tray"])
def test_every_cost_entry_reads_the_augmented_rows(name, which):
    """A tracked ``reference=`` on a point (``mjmpc_cost_terms_track``), an ``outside`` band (``_rate``) and a ``quadratic``
    over a difference (``_quad``), each held to quad_cases.restate over ``cost_observations()``."""
    torch = _torch()
    eng, raw, points, differences = _engine(name)
    terms = _entry_terms(which, eng, points, differences)
    table, pool, ref = terms.table(), terms.quad_table(), terms.reference_table()
    assert {"track": ref is not None, "rate": terms.needs_rate_entry and not terms.needs_quad_entry,
            "quad": terms.needs_quad_entry}[which]
    eng.set_cost_terms(terms)
    P, H, A = 13, 5, eng.d_action
    noise = 0.3 * np.random.default_rng(9).standard_normal((P, H, A))
    costs, act, _, nobs = eng.rollout_device(P, H, np.zeros((H, A)), noise, want_obs=True)
    torch.cuda.synchronize()
    aug = eng.cost_observations()
    _check_rows(name, eng, aug, nobs, False)
    want, mag = qc.restate(table, pool, aug.cpu().numpy(), act.cpu().numpy(), None, np.zeros((P, H)), False, True, ref=ref)
    got = costs.cpu().numpy()
    assert np.all(np.abs(got - want) <= qc.bound(table, want, mag, False)) and np.abs(want).max() > 1e-3
    eng.close()


@pytest.mark.parametrize("name", ["reacher", "gripper"])
def test_steps_of_the_controlled_env(name):
    """``step_state`` and a guarded ``(1, 1)`` rollout: one augmented row, no terminal rows, the points of the NEW state."""
    torch = _torch()
    eng, raw, points, differences = _engine(name)
    terms = _terms(eng, points, differences)
    table = terms.table()
    eng.set_cost_terms(terms)
    a = 0.3 * np.ones(eng.d_action)

    def check(cost, nobs, aug):
        assert aug.shape == (eng.d_obs + terms.n_extra,) or aug.shape == (1, 1, eng.d_obs + terms.n_extra)
        _check_rows(name, eng, aug.reshape(1, 1, -1), nobs.reshape(1, 1, -1), False)
        want, mag = restate(table, aug.cpu().numpy().reshape(1, 1, -1), a.reshape(1, 1, -1), np.zeros((1, 1)), False, False)
        assert abs(float(cost) - want[0, 0]) <= bound(table, want, mag, False)[0, 0]
        with_terminal, _ = restate(table, aug.cpu().numpy().reshape(1, 1, -1), a.reshape(1, 1, -1), np.zeros((1, 1)), False, True)
        assert with_terminal[0, 0] > want[0, 0]

    cost, nobs = eng.step_state(a)
    torch.cuda.synchronize()
    check(cost.cpu()[0], nobs, eng.cost_observations())
    with eng.real_step_guard("test"):
        costs, _, _, nobs = eng.rollout_device(1, 1, a.reshape(1, -1), None, want_obs=True)
    torch.cuda.synchronize()
    check(costs.cpu()[0, 0], nobs, eng.cost_observations())
    # a plan of the same shape without the guard: its only step is its last
    costs, act, _, nobs = eng.rollout_device(1, 1, a.reshape(1, -1), None, want_obs=True)
    want, mag = restate(table, eng.cost_observations().cpu().numpy(), act.cpu().numpy(), np.zeros((1, 1)), False, True)
    assert abs(float(costs.cpu()[0, 0]) - want[0, 0]) <= bound(table, want, mag, False)[0, 0]
    eng.close()


def test_captured_mppi_loop_equals_the_eager_loop():
    torch = _torch()
    from cost_terms_cases import _mppi
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn

    def loop(graph, steps=4):
        eng, raw, points, differences = _engine("tray")
        eng.set_cost_terms(_terms(eng, points, differences))
        c = _mppi(eng, num_particles=64, horizon=8, init_cov=0.01)
        c.rollout_fn = make_device_rollout_fn(eng)
        c.set_sim_state_fn = lambda s: None
        assert not hasattr(c.rollout_fn, "fused")
        if graph:
            c.enable_graph()
        acts = [np.array(c.optimize({})[0], np.float64) for _ in range(steps)]
        torch.cuda.synchronize()
        if graph:
            assert c._graph is not None and not getattr(c, "graph_fallback", False) and not c._mono
        out = np.array(acts), c.mean_action.copy()
        eng.close()
        return out

    a_e, m_e = loop(False)
    a_g, m_g = loop(True)
    assert np.all(np.isfinite(a_e)) and np.abs(m_e).max() > 0
    assert np.array_equal(a_g, a_e) and np.array_equal(m_g, m_e)


# ---- episode batches --------------------------------------------------------------------------------------------------
def _batch_terms(eng, points, differences, e):
    """Episode ``e``'s table: the shared points, its own weights and targets."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = pc.add_points(CostTerms(eng), points, differences)
    t.norm(obs=differences[0][0], index=[0, 1], weight=3.0 / (1 + e), target=[0.01 * e, -0.02])
    t.abs(obs=points[0][0], index=2, weight=0.7 + 0.1 * e, target=0.3 - 0.05 * e)
    t.square(action=0, weight=0.05)
    t.square(obs=points[-1][0], weight=2.0, target=[0.1, 0.0, 0.2 + 0.1 * e], terminal=True)
    return t


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batch_costs_are_the_single_engines_per_episode(name):
    """BatchedMPPI on the tree and on the arm engine, E = 3, P = 8, H = 4, a table per episode: every episode's costs and
    cost-to-go, and its real-env step's cost, are bit for bit the single engine's launches with that episode's table over the
    same rows."""
    torch = _torch()
    from test_batched_terms_gpu import CASES, SEEDS
    E, P, H = 3, 8, 4
    case, hyper = CASES["BatchedMPPI"]
    raw, states, kind = tc.model(name, E)
    _, _, points, differences = pc.case(name)
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, "f64", engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, points, differences, e) for e in range(E)])
    act, cost, nobs = b.step()
    torch.cuda.synchronize()
    r_nobs, r_act, r_costs, r_q0 = (x.clone() for x in (b._terms_nobs, b._actions, b._costs, b._q0))
    act, cost, nobs = act.clone(), cost.clone(), nobs.clone()
    gseq = b._gseq.cpu().numpy()
    assert b._points is not None and np.all(np.isfinite(r_costs.cpu().numpy()))
    eng = tc.engine(raw, kind, "f64")
    per_episode = []
    for e in range(E):
        eng.set_cost_terms(_batch_terms(eng, points, differences, e))
        rows = slice(e * P, (e + 1) * P)
        c = torch.zeros((P, H), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(P, H, r_nobs[rows].contiguous(), r_act[rows].contiguous(), c, terminal=True)
        torch.cuda.synchronize()
        assert np.array_equal(c.cpu().numpy(), r_costs[rows].cpu().numpy()), e
        assert np.array_equal(tc.numpy_q0(c.cpu().numpy(), gseq), r_q0[rows].cpu().numpy()), e
        assert np.array_equal(eng.cost_observations().cpu().numpy()[..., :eng.d_obs], r_nobs[rows].cpu().numpy())
        c1 = torch.zeros((1,), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(1, 1, nobs[e].contiguous(), act[e].contiguous(), c1, terminal=False)
        torch.cuda.synchronize()
        assert np.array_equal(c1.cpu().numpy()[0], cost[e].cpu().numpy()), e
        per_episode.append(c.cpu().numpy())
    assert not np.array_equal(per_episode[0], per_episode[1])                   # (the tables do differ)
    eng.close()
    # mismatched points between the episodes are refused, naming the episode
    moved = [(n, dict(kw, pos=(0.0, 0.0, 0.123)) if i == 0 and "body" in kw else kw) for i, (n, kw) in enumerate(points)]
    assert moved != points
    with pytest.raises(ValueError, match="episode 1's points"):
        b.set_cost_terms([_batch_terms(b.engine, moved if e == 1 else points, differences, e) for e in range(E)])
    with pytest.raises(ValueError, match="episode 2's points"):
        b.set_cost_terms([_batch_terms(b.engine, points, differences if e < 2 else differences[:1] + [("extra", points[0][0], points[1][0])], e)
                          for e in range(E)])
    b.set_cost_terms(None)
    assert b._points is None and b._terms is None
    b.close()


def test_batched_mppiq_with_points_equals_single_episodes():
    """A further batch class, closed loop: BatchedMPPIQ's episodes against the single-episode MPPIQ on an engine of its own with
    that episode's table (tests/batched_terms_cases.single)."""
    from test_batched_terms_gpu import CASES, SEEDS
    E, P, H, T, dtype = 3, 16, 8, 3, "f64"
    case, hyper = CASES["BatchedMPPIQ"]
    raw, states, kind = tc.model("cartpole", E)
    _, _, points, differences = pc.case("cartpole")
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, dtype, engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, points, differences, e) for e in range(E)])
    out = tc.bc.run_batch(case, b, T)
    assert np.all(np.isfinite(out["acts"])) and np.abs(out["acts"]).max() > 0
    for e in range(E):
        one = tc.single(case, raw, states[e], SEEDS[e], P, H, T, [v[e] for v in hyper], dtype,
                        lambda eng, e=e: _batch_terms(eng, points, differences, e))
        assert np.array_equal(out["acts"][:, e], one["acts"]), (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), e


def test_entry_refusals():
    import ctypes
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    p, s = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(dtype=_lib.F64, N=1, d_obs=4, nq=2, obs=p, prog=p, n_rows=1, n_points=1, n_diff=0, out=p)
    for over in (dict(obs=None), dict(prog=None), dict(out=None), dict(N=0), dict(d_obs=0), dict(nq=5), dict(nq=0),
                 dict(n_points=0), dict(n_points=17), dict(n_diff=17), dict(n_diff=-1), dict(n_rows=0), dict(n_rows=545),
                 dict(dtype=7), dict(d_obs=8000, nq=2)):
        kw = dict(good, **over)
        rc = lib.mjmpc_points(kw["dtype"], kw["N"], kw["d_obs"], kw["nq"], kw["obs"], kw["prog"], kw["n_rows"], kw["n_points"],
                              kw["n_diff"], kw["out"], s)
        assert rc == -1, over
