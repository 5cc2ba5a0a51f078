"""GPU: body axes and velocities as cost-term observations - ``mjmpc_points_motion`` through both engines and the
episode batches.  The augmented rows keep the observation bit for bit; every new entry is held to the numpy interpreter of
tests/motion_cases.py - which tests/test_motion_cpu.py holds to the C oracle - fed the row's own ``qpos`` and ``qvel`` as stored
(f64: 1e-9 absolute, the project's bound for observations; f32: ``2^-23 |ref| + 1e-9``, since the kernel computes in double and
rounds once), positions and axes also to the oracle directly at the same bounds; the costs are the restatement of the table over
the augmented rows within its bound.

Measured on an MI355X over all cases and shapes (each case prints its own; profiles/r26_motion.txt): worst |entry - interpreter|
2.4e-13 in f64 (random35, whose chain of 20 joints reaches large rates; 3.6e-15 at worst on the five fixed models) and 1.9e-6 in
f32 (random35 again: half an f32 ulp of an entry of that size; 9.0e-7 on the fixed models)."""
import numpy as np
import pytest

import batched_terms_cases as tc
import motion_cases as mc
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
    raw, kind, outputs, differences = mc.case(name)
    eng = (ArmRolloutEngine if kind == "arm" else TreeRolloutEngine)(raw, dtype=dtype)
    rs = np.random.RandomState(77)
    if name == "reacher":
        eng.set_env_state(dict(REACHER_START, qv=0.5 * rs.standard_normal(raw.nv)))
    elif name.startswith("random"):
        q = pc.random_qpos(raw, rs)
        eng.set_env_state(dict(qp=q, qv=0.5 * rs.standard_normal(raw.nv), target_pos=np.asarray(raw.target_pos, float)))
    else:
        from mjmpc_amd.models.synthetic import start_state
        st = start_state(name, raw)
        eng.set_env_state(dict(qp=st["qp"], qv=0.5 * rs.standard_normal(raw.nv), target_pos=st["target_pos"]))
    return eng, raw, outputs, differences


_ORACLES = {}


def _oracle(name):
    if name not in _ORACLES:
        raw, _, outputs, differences = mc.case(name)
        _ORACLES[name] = mc.Oracle(raw, *mc.resolved(raw, outputs, differences))
    return _ORACLES[name]


def _names(outputs):
    """-> (the first point, its velocity, the second point's velocity)."""
    return outputs[0][1], outputs[0][1] + "_vel", outputs[1][1] + "_vel"


def _terms(eng, outputs, differences, keep_builtin=False):
    """The case's outputs and differences and rows of the kinds 0 .. 3 over them (what cost_terms_cases.restate states): a norm
    over the difference of two velocities, an ABS row on an axis, a COS row on a point, a row on an action, a square on an
    angular velocity and a terminal row on a velocity."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    point, vel, _ = _names(outputs)
    t = mc.add_outputs(CostTerms(eng, keep_builtin=keep_builtin), outputs, differences)
    t.norm(obs="slip", weight=0.5, target=[0.01, -0.02, 0.0])
    t.abs(obs="up0", index=2, weight=0.7, target=1.0)
    t.cos(obs=point, index=0, weight=0.2)
    t.square(action=0, weight=0.05)
    t.square(obs="spin0", weight=0.01)
    t.abs(obs="tilt", index=1, weight=0.3)
    t.square(obs=vel, weight=0.2, target=[0.1, 0.0, -0.1], terminal=True)
    return t


def _check_rows(name, eng, terms, aug, nobs, f32):
    """The augmented rows ``aug`` [..][d_obs + n_extra] against the observations they came from, the interpreter and, for
    positions and axes, the oracle; -> worst error against the interpreter."""
    d, nq, nv = eng.d_obs, eng._nq, eng.model.nv
    aug, nobs = aug.cpu().numpy(), nobs.cpu().numpy()
    assert aug.dtype == nobs.dtype == (np.float32 if f32 else np.float64)
    assert np.array_equal(aug[..., :d].view(np.uint8), nobs.view(np.uint8))             # bit for bit
    rows = aug.reshape(-1, aug.shape[-1]).astype(np.float64)
    program, n_rows, n_out, n_diff, dofadr = terms.points_table()
    want = mc.interpret(program, n_rows, dofadr, n_out, rows[:, :nq], rows[:, nq:nq + nv])
    got = rows[:, d:]
    assert got.shape == want.shape and np.all(np.isfinite(want))
    err = np.abs(got - want)
    tol = 2.0 ** -23 * np.abs(want) + 1e-9 if f32 else 1e-9
    assert np.all(err <= tol), "%s: worst %.3g (over the bound by %.3g)" % (name, err.max(), (err - tol).max())
    oracle = _oracle(name)
    direct = np.array([oracle(r[:nq]) for r in rows])
    static = np.isfinite(direct[0])                                                     # positions, axes, their differences
    assert static.sum() >= 3 * 4 and np.all(np.isfinite(direct[:, static]))
    err_o = np.abs(got[:, static] - direct[:, static])
    tol_o = 2.0 ** -23 * np.abs(direct[:, static]) + 1e-9 if f32 else 1e-9
    assert np.all(err_o <= tol_o), "%s: worst against the oracle %.3g" % (name, err_o.max())
    return err.max()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", mc.case_names())
def test_entries_and_costs_against_the_interpreter_and_the_restatement(name, dtype):
    torch = _torch()
    f32 = dtype == "f32"
    eng, raw, outputs, differences = _engine(name, dtype)
    A = eng.d_action
    rng = np.random.default_rng(5)
    worst = 0.0
    for P, H in SHAPES:
        mean, noise = np.zeros((H, A)), 0.3 * rng.standard_normal((P, H, A))
        eng.set_cost_terms(None)
        builtin = eng.rollout_device(P, H, mean, noise)[0].clone()
        terms = _terms(eng, outputs, differences)
        table = terms.table()
        eng.set_cost_terms(terms)
        costs, act, obs, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        torch.cuda.synchronize()
        assert nobs.shape == (P, H, eng.d_obs)                                  # the returned observations keep their width
        aug = eng.cost_observations()
        assert aug.shape == (P, H, eng.d_obs + terms.n_extra)
        worst = max(worst, _check_rows(name, eng, terms, aug, nobs, f32))
        aug_h, act_h = aug.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        want, mag = restate(table, aug_h, act_h, np.zeros((P, H)), False, True)
        got = costs.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want) <= bound(table, want, mag, f32)), (P, H)
        last, _ = restate(table, aug_h, act_h, np.zeros((P, H)), False, False)
        assert np.all(want[:, -1] > last[:, -1]) and np.array_equal(want[:, :-1], last[:, :-1])     # the terminal row on a velocity
        # keep_builtin and incoming costs that are not finite, through the same launch path
        kept = _terms(eng, outputs, differences, keep_builtin=True)
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
    print("%s %s: worst |entry - interpreter| %.3g" % (name, dtype, worst))
    # set_cost_terms(None): the engine without terms, bit for bit
    P, H = SHAPES[-1]
    eng.set_cost_terms(None)
    again = eng.rollout_device(P, H, mean, noise)[0]
    assert np.array_equal(again.cpu().numpy(), builtin.cpu().numpy())
    with pytest.raises(RuntimeError, match="cost_observations"):
        eng.cost_observations()
    eng.close()


def _entry_terms(which, eng, outputs, differences):
    from mjmpc_amd.envs.cost_terms import CostTerms
    point, vel, vel1 = _names(outputs)
    t = mc.add_outputs(CostTerms(eng), outputs, differences)
    if which == "track":
        ref = np.stack([np.linspace(0.0, 0.5, 12), np.linspace(0.0, -0.2, 12), np.linspace(1.0, 0.8, 12)], axis=1)
        t.square(obs="up0", weight=2.0, reference=ref)
        t.abs(obs="slip", index=1, weight=0.5)
    elif which == "rate":
        t.outside(obs=vel, index=2, low=-0.05, high=0.05, weight=10.0)
        t.norm(obs="twist", weight=0.1)
    else:
        Q = np.array([[2.0, 0.3, -0.1, 0.0], [0.3, 1.0, 0.2, 0.1], [-0.1, 0.2, 3.0, 0.0], [0.0, 0.1, 0.0, 0.5]])
        t.quadratic(parts=[dict(obs=vel1, target=[0.0, 0.0, 0.05]), dict(obs="qvel", index=0)], matrix=Q, weight=0.5)
        t.linear(obs="up0", index=2, weight=-0.4)
    return t


@pytest.mark.parametrize("which", ["track", "rate", "quad"])
@pytest.mark.parametrize("name", ["reacher", "tray"])
def test_every_cost_entry_reads_the_augmented_rows(name, which):
    """A tracked ``reference=`` on an axis (``mjmpc_cost_terms_track``), an ``outside`` band on a velocity (``_rate``) and a
    ``quadratic`` whose parts mix a velocity block and ``qvel`` (``_quad``), each held to quad_cases.restate over
    ``cost_observations()``."""
    torch = _torch()
    eng, raw, outputs, differences = _engine(name)
    terms = _entry_terms(which, eng, outputs, differences)
    table, pool, ref = terms.table(), terms.quad_table(), terms.reference_table()
    assert {"track": ref is not None, "rate": terms.needs_rate_entry and not terms.needs_quad_entry,
            "quad": terms.needs_quad_entry}[which]
    eng.set_cost_terms(terms)
    P, H, A = 13, 5, eng.d_action
    noise = 0.3 * np.random.default_rng(9).standard_normal((P, H, A))
    costs, act, _, nobs = eng.rollout_device(P, H, np.zeros((H, A)), noise, want_obs=True)
    torch.cuda.synchronize()
    aug = eng.cost_observations()
    _check_rows(name, eng, terms, aug, nobs, False)
    want, mag = qc.restate(table, pool, aug.cpu().numpy(), act.cpu().numpy(), None, np.zeros((P, H)), False, True, ref=ref)
    got = costs.cpu().numpy()
    assert np.all(np.abs(got - want) <= qc.bound(table, want, mag, False)) and np.abs(want).max() > 1e-3
    eng.close()


@pytest.mark.parametrize("name", ["reacher", "gripper"])
def test_steps_of_the_controlled_env(name):
    """``step_state`` and a guarded ``(1, 1)`` rollout: one augmented row, no terminal rows, the entries of the NEW state."""
    torch = _torch()
    eng, raw, outputs, differences = _engine(name)
    terms = _terms(eng, outputs, differences)
    table = terms.table()
    eng.set_cost_terms(terms)
    a = 0.3 * np.ones(eng.d_action)

    def check(cost, nobs, aug):
        assert aug.shape == (eng.d_obs + terms.n_extra,) or aug.shape == (1, 1, eng.d_obs + terms.n_extra)
        _check_rows(name, eng, terms, aug.reshape(1, 1, -1), nobs.reshape(1, 1, -1), False)
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
        eng, raw, outputs, differences = _engine("tray")
        eng.set_cost_terms(_terms(eng, outputs, differences))
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
def _batch_terms(eng, outputs, differences, e):
    """Episode ``e``'s table: the shared outputs and differences, its own weights and targets."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    point, vel, _ = _names(outputs)
    t = mc.add_outputs(CostTerms(eng), outputs, differences)
    t.norm(obs="slip", weight=0.5 / (1 + e), target=[0.01 * e, -0.02, 0.0])
    t.abs(obs="up0", index=2, weight=0.7 + 0.1 * e, target=1.0 - 0.05 * e)
    t.square(action=0, weight=0.05)
    t.square(obs=vel, weight=0.2, target=[0.1, 0.0, 0.1 * e], terminal=True)
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
    _, _, outputs, differences = mc.case(name)
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, "f64", engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, outputs, differences, e) for e in range(E)])
    act, cost, nobs = b.step()
    torch.cuda.synchronize()
    r_nobs, r_act, r_costs, r_q0 = (x.clone() for x in (b._terms_nobs, b._actions, b._costs, b._q0))
    act, cost, nobs = act.clone(), cost.clone(), nobs.clone()
    gseq = b._gseq.cpu().numpy()
    assert b._points is not None and b._points[-1] is not None and np.all(np.isfinite(r_costs.cpu().numpy()))
    eng = tc.engine(raw, kind, "f64")
    per_episode = []
    for e in range(E):
        terms = _batch_terms(eng, outputs, differences, e)
        eng.set_cost_terms(terms)
        rows = slice(e * P, (e + 1) * P)
        c = torch.zeros((P, H), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(P, H, r_nobs[rows].contiguous(), r_act[rows].contiguous(), c, terminal=True)
        torch.cuda.synchronize()
        assert np.array_equal(c.cpu().numpy(), r_costs[rows].cpu().numpy()), e
        assert np.array_equal(tc.numpy_q0(c.cpu().numpy(), gseq), r_q0[rows].cpu().numpy()), e
        _check_rows(name, eng, terms, eng.cost_observations(), r_nobs[rows], False)
        c1 = torch.zeros((1,), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(1, 1, nobs[e].contiguous(), act[e].contiguous(), c1, terminal=False)
        torch.cuda.synchronize()
        assert np.array_equal(c1.cpu().numpy()[0], cost[e].cpu().numpy()), e
        per_episode.append(c.cpu().numpy())
    assert not np.array_equal(per_episode[0], per_episode[1])                   # (the tables do differ)
    eng.close()
    b.set_cost_terms(None)
    assert b._points is None and b._terms is None
    b.close()


def test_batched_mppiq_with_motion_equals_single_episodes():
    """A further batch class, closed loop: BatchedMPPIQ's episodes against the single-episode MPPIQ on an engine of its own with
    that episode's table (tests/batched_terms_cases.single)."""
    from test_batched_terms_gpu import CASES, SEEDS
    E, P, H, T, dtype = 3, 16, 8, 3, "f64"
    case, hyper = CASES["BatchedMPPIQ"]
    raw, states, kind = tc.model("cartpole", E)
    _, _, outputs, differences = mc.case("cartpole")
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, dtype, engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, outputs, differences, e) for e in range(E)])
    out = tc.bc.run_batch(case, b, T)
    assert np.all(np.isfinite(out["acts"])) and np.abs(out["acts"]).max() > 0
    for e in range(E):
        one = tc.single(case, raw, states[e], SEEDS[e], P, H, T, [v[e] for v in hyper], dtype,
                        lambda eng, e=e: _batch_terms(eng, outputs, differences, e))
        assert np.array_equal(out["acts"][:, e], one["acts"]), (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), e


def test_a_slot_no_closing_row_names_reads_as_zero_and_wild_tables_stay_inside():
    """The kernel's own guards: slots, qpos and dof addresses far outside are held inside (nothing is read or written out of
    bounds: the canaries around the output stay), and an unnamed slot is 0."""
    import ctypes
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    N, d_obs, nq, nv, n_out = 70, 7, 3, 3, 3
    program = np.zeros((3, 16))
    program[0, :3] = [mc.HINGE, 1000.0, 0.0]
    program[0, 6], program[0, 12] = 1.0, 1.0
    program[1, :6] = [mc.VELOCITY, 1.0, 2.0, 0.1, 0.0, 0.0]            # slot 2
    program[2, :6] = [mc.POINT, 0.0, 99.0, 0.1, 0.0, 0.0]              # a slot outside: written nowhere
    dofadr = np.array([-5, 0, 0], np.int32)
    obs = torch.from_numpy(np.random.default_rng(1).standard_normal((N, d_obs))).cuda()
    out = torch.full((N + 2, d_obs + 3 * n_out), 7.0, dtype=torch.float64, device="cuda")
    prog_d, dof_d = torch.from_numpy(program).cuda(), torch.from_numpy(dofadr).cuda()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(lib.mjmpc_points_motion(_lib.F64, N, d_obs, nq, nv, vp(obs), vp(prog_d), vp(dof_d), 3, n_out, 0, vp(out[1:]),
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got, rows = out.cpu().numpy(), obs.cpu().numpy()
    assert np.all(got[0] == 7.0) and np.all(got[-1] == 7.0)
    assert np.array_equal(got[1:-1, :d_obs], rows)
    assert np.all(got[1:-1, d_obs:d_obs + 6] == 0.0)                    # slots 0 and 1: no closing row names them
    # the hinge reads qpos[nq - 1] and qvel[0]: the point (0.1, 0, 0) turns about z at the rate qvel[0]
    ang, rate = rows[:, nq - 1], rows[:, nq]
    want = np.stack([-0.1 * np.sin(ang) * rate, 0.1 * np.cos(ang) * rate, np.zeros(N)], axis=1)
    assert np.abs(got[1:-1, d_obs + 6:] - want).max() <= 1e-12
