"""GPU parity of the designed models of tests/tree_shape_cases.py: every instantiation of the tree rollout kernel at its exact
fill (nv == DN on a path of DP links, the last link on the particle's last lane), the model one dof and one link over every
class boundary, and the edge models (31 / 32 dofs, ball joints on lanes 13..15, 16..18 and 29..31, a free joint on lanes 0..5,
nq == 40, 16 contact records with the last on link 31) against the C oracle.  Bounds: the project's 1e-9 per env step (SURVEY
8d), 1e-7 over a short rollout as tests/test_random_models_gpu.py bounds its own; f32 by that file's statistic (median below
1e-4).  MJMPC_TREE_SHAPES_RECORD=<file> in the environment appends one JSON line per case with the measured
errors (profiles/r24_tree_shapes.txt was made from it)."""
import dataclasses
import json
import os

import numpy as np
import pytest

import tree_shape_cases as tsc

pytestmark = pytest.mark.gpu

EULER = [c for c in tsc.CASES if not c.integrator]
RK4 = [c for c in tsc.CASES if c.integrator]
P, H = 19, 4            # 19 particles: no multiple of a workgroup's 2 / 4 / 8 / 16 - the ragged last workgroup and wave run


def _ids(cases):
    return [c.name for c in cases]


def _record(**kw):
    print(" ".join("%s %s" % (k, ("%.2e" % v) if isinstance(v, float) else v) for k, v in kw.items()))
    if os.environ.get("MJMPC_TREE_SHAPES_RECORD"):
        with open(os.environ["MJMPC_TREE_SHAPES_RECORD"], "a") as f:
            f.write(json.dumps(kw) + "\n")


_REF = {}


def _reference(case):
    """Model, oracle, states and the oracle's results for a case - made once per model, shared by every test, read-only."""
    key = (case.chains, case.family, case.integrator, case.records)
    if key in _REF:
        return _REF[key]
    import rk4_ref
    from oracle.physics_ref import RefArm
    raw = tsc.build(case)
    ref = RefArm(raw.to_flat())
    rs = np.random.RandomState(len(key[0]) * 100 + case.nv)
    tgt = np.asarray(raw.target_pos, float)
    sts = tsc.states(case, rs, raw)
    if case.integrator:
        steps = [rk4_ref.env_step(ref, raw, q, v, u, tgt)[:4] for q, v, u in sts]
    else:
        steps = [ref.env_step(q, v, u, tgt) for q, v, u in sts]
    for q1, v1, r1, o1 in steps:
        assert np.isfinite(o1).all() and np.isfinite(r1), "%s: the oracle left a non-finite step" % case.name
    A = len(raw.actuators)
    # the rollouts start from the designed state, moving: the last link beyond its limit, its sphere on the floor
    q, v = tsc.designed_q(raw), 0.3 * rs.standard_normal(raw.nv)
    out = dict(raw=raw, ref=ref, tgt=tgt, states=sts, steps=steps, start=(q, v), mean=0.2 * rs.standard_normal((H, A)),
               eps=0.5 * rs.standard_normal((P, H, A)), W=0.05 * rs.standard_normal((ref.d_obs + 1, A)), rollout=None, closed=None,
               oracle_fails=ref.newton_stats()["fails"])
    _REF[key] = out
    return out


def _oracle_rollout(R, case, act):
    """The oracle's open-loop rollout from the shared start (RK4: the composed step on the actions the engine applied)."""
    if R["rollout"] is None:
        q, v = R["start"]
        if case.integrator:
            import rk4_ref
            got = [rk4_ref.rollout(R["ref"], R["raw"], q, v, R["tgt"], act[p])[:2] for p in range(P)]
            R["rollout"] = (np.array([g[0] for g in got]), np.array([g[1] for g in got]))
        else:
            o = R["ref"].rollout(q, v, R["tgt"], R["mean"], R["eps"])
            R["rollout"] = (o[1], o[4])
        assert np.isfinite(R["rollout"][1]).all()
        R["oracle_fails"] = R["ref"].newton_stats()["fails"]
    return R["rollout"]


def _one_step_worst(eng, R, dtype="f64"):
    errs = []
    for (q, v, u), (q1, v1, r1, o1) in zip(R["states"], R["steps"]):
        eng.set_env_state(dict(qp=q, qv=v, target_pos=R["tgt"]))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        assert np.isfinite(nobs[0, 0]).all()
        e = np.abs(nobs[0, 0] - o1).max() / max(1.0, np.abs(o1).max())
        errs.append(e if dtype == "f32" else max(e, abs(rew[0, 0] - r1) / max(1.0, abs(r1))))
    return errs


def _rollout_worst(eng, R, case):
    from test_random_models_gpu import _assert_rollouts_close
    q, v = R["start"]
    eng.set_env_state(dict(qp=q, qv=v, target_pos=R["tgt"]))
    obs, rew, act, done, info, nobs = eng.rollout(P, H, R["mean"], R["eps"], "open_loop")
    o_rew, o_nobs = _oracle_rollout(R, case, act)
    scale = np.maximum(1.0, np.abs(o_nobs).reshape(P, -1).max(axis=1))
    worst = float((np.abs(nobs - o_nobs).reshape(P, -1).max(axis=1) / scale).max())
    return worst, lambda: (_assert_rollouts_close(nobs, o_nobs), np.testing.assert_allclose(rew, o_rew, rtol=1e-7, atol=1e-7))


def _check_f64(case, tag=""):
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from test_random_models_gpu import _assert_rollouts_close
    R = _reference(case)
    eng = TreeRolloutEngine(R["raw"], dtype="f64")
    try:
        m = eng.model
        assert (m.nv, m.max_path) == (case.nv, case.max_path) and tsc.model_instantiation(m, bool(tag)) == case.inst
        step = max(_one_step_worst(eng, R))
        roll, assert_rollout = _rollout_worst(eng, R, case)
        closed = None
        if case.nv == 32 and not case.integrator:       # closed-loop linear, 8 x 4: the observation at its largest width
            q, v = R["start"]
            if R["closed"] is None:
                R["closed"] = R["ref"].rollout(q, v, R["tgt"], R["W"], R["eps"][:8], mode="closed_loop_linear")
                assert np.isfinite(R["closed"][4]).all()
            eng.set_env_state(dict(qp=q, qv=v, target_pos=R["tgt"]))
            obs, rew, act, done, info, nobs = eng.rollout(8, H, R["W"], R["eps"][:8], "closed_loop_linear")
            o_act, o_nobs = R["closed"][2], R["closed"][4]
            scale = np.maximum(1.0, np.abs(o_nobs).reshape(8, -1).max(axis=1))
            closed = float((np.abs(nobs - o_nobs).reshape(8, -1).max(axis=1) / scale).max())
        fails = eng.solver_failures()
        _record(case=case.name + tag, inst=str(case.inst), fill=case.fill, nv=case.nv, path=case.max_path, one_step=float(step),
                rollout=roll, closed_loop=closed, solver_failures=int(fails), oracle_failures=int(R["oracle_fails"]))
        assert step < 1e-9, step
        assert_rollout()
        if closed is not None:
            _assert_rollouts_close(act, o_act, o_nobs)
            _assert_rollouts_close(nobs, o_nobs)
        if R["oracle_fails"] == 0:
            assert fails == 0
    finally:
        eng.close()


@pytest.mark.parametrize("case", EULER, ids=_ids(EULER))
def test_case_matches_oracle_f64(case):
    """One env step from the two designed and six random states at 1e-9, a 19 x 4 open-loop rollout at 1e-7 of the particle's
    largest observation, the 32-dof models also closed-loop linear (8 x 4); no solver failure where the oracle's Newton
    iteration converges."""
    _check_f64(case)


@pytest.mark.parametrize("case", RK4, ids=_ids(RK4))
def test_rk4_case_matches_the_composed_step_f64(case):
    """The twelve RK4 shapes at their fill, and one dof / one link over, against MuJoCo's RK4 composed from the oracle's forward
    evaluations (tests/rk4_ref.py): 1e-9 per env step, 1e-7 over the 19 x 4 rollout."""
    _check_f64(case)


@pytest.mark.parametrize("case", tsc.SWITCHED, ids=_ids(tsc.SWITCHED))
def test_sparse_switch_shapes_match_oracle(case, monkeypatch):
    """MJMPC_TREE_SPARSE (read at every launch) keeps the tree-sparse factorisation on paths beyond 8 links: the two gen-0
    shapes nothing else reaches (DP = 16, DP = 32) and the general DP = 16 shape on a path of 16, at the same bounds."""
    monkeypatch.setenv("MJMPC_TREE_SPARSE", "1")
    _check_f64(case, tag=" (switch)")


@pytest.mark.parametrize("case", tsc.FILLS, ids=_ids(tsc.FILLS))
def test_fill_f32_stays_close(case):
    """The exact-fill cases in single precision, by the statistic and bound of test_random_model_f32_stays_close: the median
    relative error of the next observation below 1e-4, nothing non-finite.  That test's second bound - the 95th percentile of
    16 random states below 1e-2, "contacts amplify it in a few states" - does not carry over: here two of the eight states are
    in contact by design.  Measured (profiles/r24_tree_shapes.txt): medians 3e-7 ... 6e-6; the worst single state 2.3e-2, a
    designed state of the 32-link chain with the cylinder's four records and the tip sphere on the floor."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    R = _reference(case)
    eng = TreeRolloutEngine(R["raw"], dtype="f32")
    try:
        errs = np.sort(_one_step_worst(eng, R, "f32"))
    finally:
        eng.close()
    _record(case=case.name + " f32", inst=str(case.inst), median=float(np.median(errs)), worst=float(errs[-1]))
    assert np.median(errs) < 1e-4, errs


def test_rk4_refuses_17_dofs_and_elliptic_cones():
    """mjmpc_tree_create_ex with MJMPC_INTEGRATOR_RK4: MJMPC_E_BADMODEL (-2) for a 17-dof model and for elliptic cones (the
    compiler refuses both first; here the blocks are compiled for Euler and handed over as RK4)."""
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.compile_tree import compile_tree
    for name in ("g0_1+16", "g3_16"):
        raw = tsc.build(tsc.BY_NAME[name])
        with pytest.raises(ValueError, match="RK4"):
            compile_tree(dataclasses.replace(raw, integrator="RK4"))
        tm = compile_tree(raw)
        tm.integrator = "RK4"
        with pytest.raises(_lib.MjmpcError, match=r"\(-2\).*RK4 runs models of up to 16 dofs without elliptic"):
            TreeRolloutEngine(tm, dtype="f64")


BATCH = ["lean_32", "g0_8+8+8+8", "g0_16", "g0_32", "g1_16+16", "g3_16", "rk4g1_16"]
# (lean, tree-sparse, dense over 16 lanes, dense over 32, general, cone, RK4: the EB = 1 twin of one exact fill per family)


@pytest.mark.parametrize("name", BATCH)
def test_fill_in_an_episode_batch(name):
    """Three episodes through the episode-batch build (EB = 1), 64 x 8 over four steps, each equal - bit for bit - to its own
    single-engine run (tests/batched_cases.py)."""
    import batched_cases as bc
    from test_random_models_gpu import random_state
    case = tsc.BY_NAME[name]
    raw = _reference(case)["raw"]
    rs = np.random.RandomState(55 + case.nv)
    tgt = np.asarray(raw.target_pos, float)
    states = []
    for e in range(3):
        q, v = random_state(raw, rs)
        states.append(dict(qp=q, qv=0.3 * v, target_pos=tgt + 0.05 * e))
    mppi = bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype), guards=False)
    out = bc.check_against_singles(mppi, raw, states, [31, 32, 33], 64, 8, 4, (0.5, 1.0, 0.3), "f64")
    assert not np.array_equal(out["nobs"][:, 0], out["nobs"][:, 1])
