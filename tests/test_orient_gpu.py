"""GPU: orientation errors as cost-term observations - ``mjmpc_points_orient`` through both engines, the episode
batches and, with synthetic programs, at the C entry.  The augmented rows keep the observation bit for bit; an orientation entry is
held to the C oracle's rotation vector at the row's stored ``qpos`` (tests/orient_cases.py: rotation matrices from world points,
the angle from ``atan2(|vee|, trace)``) at the CPU test's bound - f32 rows with the one rounding of the stored entry,
``2^-23 |ref|``, beside it - and every new entry to the numpy interpreter fed the row's own ``qpos`` and ``qvel`` (f64: 1e-9; f32:
``2^-23 |ref| + 1e-9``).  Rows whose angle stands within 0.05 of pi (the oracle's route is ill-conditioned there and the sign of
``r`` flips) or whose ``|w|`` is below 1e-6 (the interpreter and the kernel may take different halves) are left out, at most 1 row
in 20.  The points, velocities and centres of mass of the same table are ``mjmpc_points_tree``'s to the bit; the costs are the
restatement of the table over the augmented rows within its bound."""
import ctypes

import numpy as np
import pytest

import batched_terms_cases as tc
import com_cases as cc
import orient_cases as oc
import points_cases as pc
import points_tile_cases as ptc
import quad_cases as qc
from cost_terms_cases import REACHER_START, bound, restate

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (67, 3), (64, 8)]
ORIENTATIONS = ("to_ancestor", "absolute", "across")


def _torch():
    import torch
    return torch


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


_ORACLES = {}


def _oracle(name):
    if name not in _ORACLES:
        _ORACLES[name] = oc.Oracle(oc.raw_model(name))
    return _ORACLES[name]


def _engine(name, dtype="f64"):
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    raw, kind, outputs, differences = oc.case(name)
    eng = (ArmRolloutEngine if kind == "arm" else TreeRolloutEngine)(raw, dtype=dtype)
    rs = np.random.RandomState(77)
    qv = 0.5 * rs.standard_normal(raw.nv)
    if name == "reacher":
        eng.set_env_state(dict(REACHER_START, qv=qv))
    elif eng.forward_task:
        eng.set_env_state(dict(qpos=np.asarray(raw.qpos0, float), qvel=qv))
    elif name in ("tray", "gripper"):
        from mjmpc_amd.models.synthetic import start_state
        st = start_state(name, raw)
        eng.set_env_state(dict(qp=st["qp"], qv=qv, target_pos=st["target_pos"]))
    elif name.startswith("random"):
        # (a random configuration whose angles start well below pi: the rollouts below are short)
        qp = oc.draw_states(raw, _oracle(name), oc.resolved(raw, outputs), 1, 77, band=0.5)[0][0]
        eng.set_env_state(dict(qp=qp, qv=qv, target_pos=np.asarray(raw.target_pos, float)))
    else:
        eng.set_env_state(dict(qp=np.asarray(raw.qpos0, float), qv=qv, target_pos=np.asarray(raw.target_pos, float)))
    return eng, raw, outputs, differences


def _terms(eng, outputs, differences, keep_builtin=False):
    """The case's outputs and rows of the kinds 0 .. 3 over them (what cost_terms_cases.restate states): a ``norm`` over an
    orientation - the angle -, a terminal row on another."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = oc.add_outputs(CostTerms(eng, keep_builtin=keep_builtin), outputs, differences)
    t.norm(obs="across", weight=0.5)
    t.abs(obs="absolute", index=2, weight=0.7, target=0.3)
    t.cos(obs="to_ancestor", index=0, weight=0.2)
    t.square(action=0, weight=0.05)
    t.square(obs="tip_vel", weight=0.01)
    t.norm(obs="spin", weight=0.02, target=[0.1, 0.0, -0.1])
    if differences:
        t.abs(obs="tip_from_whole", index=1, weight=0.3)
    t.square(obs="to_ancestor", weight=0.2, target=[0.1, 0.0, -0.1], terminal=True)
    return t


def _within_cap(left_out, what):
    assert 20 * int(np.sum(left_out)) <= left_out.size, "%s: %d of %d rows left out" % (what, np.sum(left_out), left_out.size)


def _check_rows(name, eng, terms, aug, nobs, f32, oracle=True):
    """The augmented rows against the observations they came from, the interpreter, the oracle's orientation errors and
    ``mjmpc_points_tree``'s other outputs; -> (worst error against the interpreter, worst against the oracle)."""
    torch = _torch()
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.cost_terms import CostTerms
    d, nq, nv = eng.d_obs, eng._nq, eng.model.nv
    nobs_d = nobs.reshape(-1, d).contiguous()
    aug, nobs = aug.cpu().numpy(), nobs.cpu().numpy()
    assert aug.dtype == nobs.dtype == (np.float32 if f32 else np.float64)
    assert np.array_equal(aug[..., :d].view(np.uint8), nobs.view(np.uint8))             # bit for bit
    rows = aug.reshape(-1, aug.shape[-1]).astype(np.float64)
    program, n_rows, n_out, n_diff, dofadr, n_levels, orient = terms.points_table()
    assert orient is True
    want, least = oc.interpret(program, n_rows, dofadr, n_out, n_levels, rows[:, :nq], rows[:, nq:nq + nv], with_w=True)
    got = rows[:, d:]
    assert got.shape == want.shape and np.all(np.isfinite(want)) and np.all(np.isfinite(got))
    unsettled = least < 1e-6
    _within_cap(unsettled, name + ", |w| below 1e-6")
    err = np.abs(got - want)[~unsettled]
    tol = (2.0 ** -23 * np.abs(want) + 1e-9 if f32 else np.full_like(want, 1e-9))[~unsettled]
    assert np.all(err <= tol), "%s: worst %.3g (over the bound by %.3g)" % (name, err.max(), (err - tol).max())
    layout = terms.points_layout()
    worst_o = 0.0
    if oracle:
        o, specs = _oracle(name), oc.resolved(eng.raw, oc.case(name)[2])
        direct = {k: np.array([o.error(specs[k], r[:nq]) for r in rows]) for k in ORIENTATIONS}
        band = np.any([np.linalg.norm(direct[k], axis=1) > np.pi - oc.BAND for k in ORIENTATIONS], axis=0)
        _within_cap(band, name + ", angles within 0.05 of pi")
        for k in ORIENTATIONS:
            err_o = np.abs(rows[:, layout[k]] - direct[k])[~band]
            tol_o = oc.ORIENT_BOUND + (2.0 ** -23 * np.abs(direct[k][~band]) if f32 else 0.0)
            print("%s %s %s: worst against the oracle %.3g" % (name, "f32" if f32 else "f64", k, err_o.max()))
            assert np.all(err_o <= tol_o), "%s %s: worst against the oracle %.3g" % (name, k, err_o.max())
            worst_o = max(worst_o, float(err_o.max()))
    # points, velocities and centres of mass: the same definitions without the orientations through mjmpc_points_tree, to the bit
    outputs, differences = oc.outputs_for(eng.raw, com="whole" in layout)
    plain = oc.add_outputs(CostTerms(eng), [x for x in outputs if x[0] != "orientation"], differences)
    table = plain.points_table()
    prog2, n_rows2, n_out2, n_diff2, dofadr2 = table[:5]
    levels2 = table[5] if len(table) > 5 else 0
    out2 = torch.empty((len(rows), d + plain.n_extra), dtype=nobs_d.dtype, device="cuda")
    prog_d, dof_d = torch.from_numpy(prog2).cuda(), torch.from_numpy(dofadr2).cuda()
    _lib.check(eng._lib.mjmpc_points_tree(eng._code, len(rows), d, nq, nv, _vp(nobs_d), _vp(prog_d), _vp(dof_d), n_rows2, n_out2,
                                          n_diff2, levels2, _vp(out2), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    old, flat = out2.cpu().numpy(), aug.reshape(-1, aug.shape[-1])
    for key, at in plain.points_layout().items():
        assert np.array_equal(flat[:, layout[key]].view(np.uint8), old[:, at].view(np.uint8)), key
    return float(err.max()), worst_o


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", oc.case_names())
def test_entries_and_costs_against_the_oracle_the_interpreter_and_the_restatement(name, dtype):
    torch = _torch()
    from mjmpc_amd.envs.cost_terms import CostTerms
    f32 = dtype == "f32"
    eng, raw, outputs, differences = _engine(name, dtype)
    A = eng.d_action
    rng = np.random.default_rng(5)
    worst = (0.0, 0.0)
    for P, H in SHAPES:
        mean, noise = np.zeros((H, A)), 0.3 * rng.standard_normal((P, H, A))
        eng.set_cost_terms(None)
        builtin = eng.rollout_device(P, H, mean, noise)[0].clone()
        terms = _terms(eng, outputs, differences)
        table = terms.table()
        eng.set_cost_terms(terms)
        assert eng._points_orient and (eng._points_levels or 0) == terms.points_table()[5]
        costs, act, obs, nobs = eng.rollout_device(P, H, mean, noise, want_obs=True)
        torch.cuda.synchronize()
        assert nobs.shape == (P, H, eng.d_obs)
        aug = eng.cost_observations()
        assert aug.shape == (P, H, eng.d_obs + terms.n_extra)
        worst = tuple(max(a, b) for a, b in zip(worst, _check_rows(name, eng, terms, aug, nobs, f32)))
        aug_h, act_h = aug.cpu().numpy().astype(np.float64), act.cpu().numpy().astype(np.float64)
        want, mag = restate(table, aug_h, act_h, np.zeros((P, H)), False, True)
        got = costs.cpu().numpy().astype(np.float64)
        assert np.all(np.abs(got - want) <= bound(table, want, mag, f32)), (P, H)
        last, _ = restate(table, aug_h, act_h, np.zeros((P, H)), False, False)
        assert np.all(want[:, -1] > last[:, -1]) and np.array_equal(want[:, :-1], last[:, :-1])     # the terminal row
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
        # a norm row over an orientation is the angle
        angle = oc.add_outputs(CostTerms(eng), outputs, differences).norm(obs="across")
        eng.set_cost_terms(angle)
        c = torch.zeros((P, H), dtype=costs.dtype, device="cuda")
        eng._launch_cost_terms(P, H, nobs, act, c, terminal=False)
        torch.cuda.synchronize()
        theta = np.linalg.norm(aug_h[..., terms.points_layout()["across"]], axis=-1)
        assert np.all(np.abs(c.cpu().numpy() - theta) <= (2.0 ** -22 if f32 else 1e-14) * np.maximum(theta, 1.0))
        assert theta.max() <= np.pi + 1e-6 and theta.max() > 0.1
    print("%s %s: worst |entry - interpreter| %.3g, worst |orientation - oracle| %.3g" % ((name, dtype) + worst))
    P, H = SHAPES[-1]
    eng.set_cost_terms(None)
    again = eng.rollout_device(P, H, mean, noise)[0]
    assert np.array_equal(again.cpu().numpy(), builtin.cpu().numpy())
    with pytest.raises(RuntimeError, match="cost_observations"):
        eng.cost_observations()
    eng.close()


def _entry_terms(which, eng, outputs, differences):
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = oc.add_outputs(CostTerms(eng), outputs, differences)
    if which == "track":
        ref = np.stack([np.linspace(0.0, 0.5, 12), np.linspace(0.0, -0.2, 12), np.linspace(0.5, 0.3, 12)], axis=1)
        t.square(obs="absolute", weight=2.0, reference=ref)
        t.abs(obs="across", index=1, weight=0.5)
    elif which == "rate":
        t.outside(obs="across", index=1, low=-0.1, high=0.1, weight=10.0)
        t.norm(obs="to_ancestor", weight=0.1)
    else:
        Q = np.diag([2.0, 1.0, 3.0, 0.5, 0.4, 0.3])
        Q[0, 3] = Q[3, 0] = 0.3
        Q[1, 4] = Q[4, 1] = -0.2
        Q[2, 5] = Q[5, 2] = 0.1
        t.quadratic(parts=[dict(obs="absolute", target=[0.0, 0.1, 0.05]), dict(obs="spin")], matrix=Q, weight=0.5)
        t.linear(obs="to_ancestor", index=0, weight=-0.4)
    return t


@pytest.mark.parametrize("which", ["track", "rate", "quad"])
@pytest.mark.parametrize("name", ["reacher", "tray"])
def test_every_cost_entry_reads_the_augmented_rows(name, which):
    """A ``reference=`` on an orientation block (``mjmpc_cost_terms_track``), an ``outside`` band on one component (``_rate``)
    and a ``quadratic`` mixing an orientation block with an ``angular_velocity`` block (``_quad``), each held to
    quad_cases.restate over ``cost_observations()``."""
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
    eng.close()


def test_captured_mppi_loop_equals_the_eager_loop():
    torch = _torch()
    from cost_terms_cases import _mppi
    from mjmpc_amd.envs.arm_engine import make_device_rollout_fn

    def loop(graph, steps=4):
        eng, raw, outputs, differences = _engine("cheetah")
        eng.set_cost_terms(_terms(eng, outputs, differences, keep_builtin=True))
        assert eng._points_orient and eng._points_levels > 0
        c = _mppi(eng, num_particles=64, horizon=8, init_cov=0.3)
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
def _batch_terms(eng, e):
    """Episode ``e``'s table: the shared outputs, its own weights and targets."""
    from mjmpc_amd.envs.cost_terms import CostTerms
    t = oc.add_outputs(CostTerms(eng), *oc.outputs_for(eng.raw))
    t.norm(obs="across", weight=0.5 / (1 + e), target=[0.01 * e, -0.02, 0.0])
    t.abs(obs="absolute", index=2, weight=0.7 + 0.1 * e, target=0.3 - 0.05 * e)
    t.square(action=0, weight=0.05)
    t.square(obs="to_ancestor", weight=0.2, target=[0.1, 0.0, 0.1 * e], terminal=True)
    return t


@pytest.mark.parametrize("name", ["cartpole", "reacher"])
def test_batch_costs_are_the_single_engines_per_episode(name):
    """BatchedMPPI on the tree and on the arm engine, E = 3, a table per episode: every episode's costs and cost-to-go, and its
    real-env step's cost, are bit for bit the single engine's launches with that episode's table over the same rows."""
    torch = _torch()
    from test_batched_terms_gpu import CASES, SEEDS
    E, P, H = 3, 8, 4
    case, hyper = CASES["BatchedMPPI"]
    raw, states, kind = tc.model(name, E)
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, "f64", engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, e) for e in range(E)])
    assert b._points_orient and b._points is not None
    act, cost, nobs = b.step()
    torch.cuda.synchronize()
    r_nobs, r_act, r_costs, r_q0 = (x.clone() for x in (b._terms_nobs, b._actions, b._costs, b._q0))
    act, cost, nobs = act.clone(), cost.clone(), nobs.clone()
    gseq = b._gseq.cpu().numpy()
    assert np.all(np.isfinite(r_costs.cpu().numpy()))
    eng = tc.engine(raw, kind, "f64")
    per_episode = []
    for e in range(E):
        terms = _batch_terms(eng, e)
        eng.set_cost_terms(terms)
        rows = slice(e * P, (e + 1) * P)
        c = torch.zeros((P, H), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(P, H, r_nobs[rows].contiguous(), r_act[rows].contiguous(), c, terminal=True)
        torch.cuda.synchronize()
        assert np.array_equal(c.cpu().numpy(), r_costs[rows].cpu().numpy()), e
        assert np.array_equal(tc.numpy_q0(c.cpu().numpy(), gseq), r_q0[rows].cpu().numpy()), e
        _check_rows(name, eng, terms, eng.cost_observations(), r_nobs[rows], False, oracle=False)
        c1 = torch.zeros((1,), dtype=torch.float64, device="cuda")
        eng._launch_cost_terms(1, 1, nobs[e].contiguous(), act[e].contiguous(), c1, terminal=False)
        torch.cuda.synchronize()
        assert np.array_equal(c1.cpu().numpy()[0], cost[e].cpu().numpy()), e
        per_episode.append(c.cpu().numpy())
    assert not np.array_equal(per_episode[0], per_episode[1])
    eng.close()
    b.set_cost_terms(None)
    assert b._points is None and b._terms is None and not b._points_orient
    b.close()


def test_batched_mppiq_with_an_orientation_equals_single_episodes():
    from test_batched_terms_gpu import CASES, SEEDS
    E, P, H, T, dtype = 3, 16, 8, 3, "f64"
    case, hyper = CASES["BatchedMPPIQ"]
    raw, states, kind = tc.model("cartpole", E)
    b = tc.bc.make_batch(case, raw, states, SEEDS[:E], P, H, hyper, dtype, engine=kind)
    b.set_cost_terms([_batch_terms(b.engine, e) for e in range(E)])
    out = tc.bc.run_batch(case, b, T)
    assert np.all(np.isfinite(out["acts"])) and np.abs(out["acts"]).max() > 0
    for e in range(E):
        one = tc.single(case, raw, states[e], SEEDS[e], P, H, T, [v[e] for v in hyper], dtype, lambda eng, e=e: _batch_terms(eng, e))
        assert np.array_equal(out["acts"][:, e], one["acts"]), (e, np.abs(out["acts"][:, e] - one["acts"]).max())
        assert np.array_equal(out["costs"][:, e], one["costs"]), e
        assert np.array_equal(out["nobs"][:, e], one["nobs"]), e


# ---- the C entry, synthetic programs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.synthetic_names())
def test_synthetic_programs_at_the_entry(name):
    """The log map's edges on the world frame (the identity: exactly 0; ``s`` on either side of 2^-26; ``theta = pi - 1e-6``;
    ``w`` exactly 0: ``(pi, 0, 0)``; ``w < 0``), ``rel = 1`` before any HOLD, two relative walks with a HOLD each, a HOLD inside a
    centre-of-mass walk, ``n_levels`` 0 and 2, N = 1, rows and rows + 1, slots outside: against the interpreter in
    ``np.longdouble`` with points_tile_cases' criteria, the observation bit for bit, the output between canaries."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    c = oc.synthetic_case(name)
    want80, _, b, settled = oc.synthetic_reference(name)
    tdt = torch.float32 if c.dtype == "f32" else torch.float64
    obs = torch.from_numpy(c.obs).cuda()
    out = torch.full((c.N + 2, c.d_aug), 7.0, dtype=tdt, device="cuda")
    prog_d, dof_d = torch.from_numpy(c.program).cuda(), torch.from_numpy(c.dofadr).cuda()
    code = _lib.F32 if c.dtype == "f32" else _lib.F64
    _lib.check(lib.mjmpc_points_orient(code, c.N, c.d_obs, c.nq, c.nv, _vp(obs), _vp(prog_d), _vp(dof_d), c.n_rows, c.n_out,
                                       c.n_diff, c.n_levels, _vp(out[1:]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[0] == 7.0) and np.all(got[-1] == 7.0)                              # the canaries
    word = np.uint32 if c.dtype == "f32" else np.uint64
    assert np.array_equal(got[1:-1, :c.d_obs].view(word), c.obs.view(word))              # bit for bit, NaN payloads included
    new = got[1:-1, c.d_obs:]
    assert np.all(np.isfinite(new))

    def block(tag, rows=slice(None)):
        return new[rows, 3 * c.slots[tag]:3 * c.slots[tag] + 3].astype(np.float64)
    assert np.all(block("identity") == 0.0)                                              # exactly, and no NaN
    tol = 2.0 ** -23 if c.dtype == "f32" else 4e-16
    assert np.all(np.abs(block("w zero") - [np.pi, 0.0, 0.0]) <= tol * np.pi)
    assert np.all(block("w negative")[:, 1] < 0) and np.all(block("under")[:, 0] > 0) and np.all(block("over")[:, 1] < 0)
    _within_cap(~settled, name)
    if c.dtype == "f32":
        excess, worst, ulps = ptc.excess_f32(new[settled], want80[settled], b)
    else:
        excess, worst = ptc.excess_f64(new[settled], want80[settled], b)
    print("%s: tile %d, worst %.3g, bound %.3g" % (name, c.tile, worst, b))
    assert excess <= 0.0, (name, worst, b)
    # the second relative walk read its own HOLD's frame, not the first's
    assert np.abs(block("relative") - block("after com")).max() > 1e-3
