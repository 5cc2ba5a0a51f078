"""GPU parity of the tree engine's row parameters (tree_row_params: every constraint row's D and aref) with solver sets across
their ranges, against the FP64 C oracle - which clamps, mixes and evaluates them on its own, with ``pow``
(tests/solver_set_cases.py has the generator and the designed models; tests/test_solver_sets_cpu.py pins the host side).

* the random models of tests/test_random_models_gpu.py with every set redrawn: one env step at 1e-9 (SURVEY 8d's gate), short
  rollouts under the scaled 1e-7, f32 under the random suite's own bounds;
* one row kind at a time at the corners of the impedance curve, for every designed set, f64 at 1e-9 and f32 at 1e-3;
* a model that fills all eight solver classes; a varied model through the RK4 and the episode-batch builds of the same text.
MJMPC_SOLSET_SEEDS=a:b runs another range of seeds (a soak, not part of the suite); MJMPC_SOLSET_STATS=file appends one JSON
line per test."""
import json
import os

import numpy as np
import pytest

import solver_set_cases as sc

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(x) for x in os.environ["MJMPC_SOLSET_SEEDS"].split(":")]) if os.environ.get("MJMPC_SOLSET_SEEDS") else range(48)


def _stats(**kw):
    if os.environ.get("MJMPC_SOLSET_STATS"):
        with open(os.environ["MJMPC_SOLSET_STATS"], "a") as f:
            f.write(json.dumps(kw) + "\n")


def _varied(seed, dtype, integrator=None, fits=lambda raw: True):
    """The seed's varied model, its engine and its oracle; models engine or oracle refuse are drawn again, counted and bounded."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    from test_random_models_gpu import MAX_REDRAWS, random_model
    tries, refusals = 0, []
    while True:
        raw = sc.vary_solver_sets(random_model(1000 * tries + seed), 1000 * tries + seed)
        if integrator is not None:
            raw.integrator = integrator
        try:
            if not fits(raw):
                raise NotImplementedError("does not fit this build")
            return raw, TreeRolloutEngine(raw, dtype=dtype), RefArm(raw.to_flat()), tries, refusals
        except (ValueError, NotImplementedError, AssertionError) as e:
            refusals.append("%s: %s" % (type(e).__name__, str(e)[:80]))
            tries += 1
            assert tries <= MAX_REDRAWS, "seed %d: %d models in a row refused: %s" % (seed, tries, refusals)


@pytest.mark.parametrize("seed", _SEEDS)
def test_varied_sets_match_oracle(seed):
    """tests/test_random_models_gpu.py's test_random_model_matches_oracle on the varied models, bound for bound."""
    from test_random_models_gpu import _assert_rollouts_close, _beyond_one_step_tolerance, random_state
    raw, eng, ref, tries, refusals = _varied(seed, "f64")
    rs = np.random.RandomState(seed + 77)
    tgt = np.asarray(raw.target_pos, float)
    A = eng.d_action
    worst = 0.0
    for k in range(12):
        q, v = random_state(raw, rs)
        v *= (0.0 if k % 4 == 0 else 1.0)
        u = rs.uniform(-1.5, 1.5, A)
        eng.set_env_state(dict(qp=q, qv=v, target_pos=tgt))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        q1, v1, r1, o1 = ref.env_step(q, v, u, tgt)
        assert np.isfinite(o1).all() and np.isfinite(r1), "seed %d state %d: the oracle left a non-finite step" % (seed, k)
        worst = max(worst, np.abs(nobs[0, 0] - o1).max() / max(1.0, np.abs(o1).max()), abs(rew[0, 0] - r1) / max(1.0, abs(r1)))
    print("seed %d (%d re-draws): nv %d, general %s: worst relative error %.2e" % (seed, tries, eng.model.nv, eng.model.general, worst))
    hits = 0
    try:
        assert worst < 1e-9, worst
        P, H = 32, 6
        q, v = random_state(raw, rs)
        eps = 0.5 * rs.standard_normal((P, H, A))
        eng.set_env_state(dict(qp=q, qv=0.3 * v, target_pos=tgt))
        obs, rew, act, done, info, nobs = eng.rollout(P, H, np.zeros((H, A)), eps, "open_loop")
        o_obs, o_rew, _, _, o_nobs = ref.rollout(q, 0.3 * v, tgt, np.zeros((H, A)), eps)
        assert np.isfinite(o_nobs).all(), "seed %d: oracle rollouts turned non-finite" % seed
        hits += _beyond_one_step_tolerance(nobs, o_nobs)
        _assert_rollouts_close(nobs, o_nobs)
        np.testing.assert_allclose(rew, o_rew, rtol=1e-7, atol=1e-7)
        W = 0.05 * rs.standard_normal((eng.d_obs + 1, A))
        obs, rew, act, done, info, nobs = eng.rollout(8, 4, W, eps[:8, :4], "closed_loop_linear")
        o_obs, o_rew, o_act, _, o_nobs = ref.rollout(q, 0.3 * v, tgt, W, eps[:8, :4], mode="closed_loop_linear")
        assert np.isfinite(o_nobs).all(), "seed %d: closed-loop oracle rollouts turned non-finite" % seed
        hits += _beyond_one_step_tolerance(nobs, o_nobs)
        _assert_rollouts_close(act, o_act, o_nobs)
        _assert_rollouts_close(nobs, o_nobs)
        assert eng.solver_failures() == 0
    finally:
        # (the oracle's Newton iteration reaching its cap of 100 is recorded, not judged: the comparisons above are the gate)
        _stats(test="varied", seed=seed, redraws=tries, refusals=refusals, worst=worst, scaled_tolerance_hits=hits,
               oracle_newton_cap=ref.newton_stats()["fails"])
        eng.close()


@pytest.mark.parametrize("seed", range(0, 48, 4))
def test_varied_sets_f32(seed):
    """test_random_model_f32_stays_close on the varied models, with its bounds: median 1e-4, 95th percentile 1e-2, finite
    wherever the oracle is."""
    from test_random_models_gpu import random_state
    raw, eng, ref, _, _ = _varied(seed, "f32")
    rs = np.random.RandomState(seed + 99)
    tgt = np.asarray(raw.target_pos, float)
    errs = []
    for k in range(16):
        q, v = random_state(raw, rs)
        u = rs.uniform(-1.0, 1.0, eng.d_action)
        eng.set_env_state(dict(qp=q, qv=v, target_pos=tgt))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        q1, v1, r1, o1 = ref.env_step(q, v, u, tgt)
        if np.isfinite(o1).all():
            assert np.isfinite(nobs[0, 0]).all()
            errs.append(np.abs(nobs[0, 0] - o1).max() / max(1.0, np.abs(o1).max()))
    errs = np.sort(errs)
    print("seed %d f32: median %.2e, 95th percentile %.2e" % (seed, np.median(errs), errs[int(0.95 * (len(errs) - 1))]))
    _stats(test="f32", seed=seed, median=float(np.median(errs)), p95=float(errs[int(0.95 * (len(errs) - 1))]))
    eng.close()
    assert np.median(errs) < 1e-4 and errs[int(0.95 * (len(errs) - 1))] < 1e-2, errs


def _step_errors(raw, eng, ref, states):
    tgt = np.asarray(raw.target_pos, float)
    u = np.full(eng.d_action, 0.3)
    out = []
    for x, q, v in states:
        eng.set_env_state(dict(qp=q, qv=v, target_pos=tgt))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        q1, v1, r1, o1 = ref.env_step(q, v, u, tgt)
        assert np.isfinite(o1).all() and np.isfinite(r1)
        with np.errstate(invalid="ignore"):
            out.append(max(np.abs(nobs[0, 0] - o1).max() / max(1.0, np.abs(o1).max()), abs(rew[0, 0] - r1) / max(1.0, abs(r1))))
    return np.array(out)


@pytest.mark.parametrize("name", list(sc.DESIGNED_SETS))
@pytest.mark.parametrize("kind", sc.KINDS)
def test_designed_rows(kind, name):
    """One row kind, one set: one env step from every designed state, f64 at 1e-9.  The f32 engine runs the same states
    (not the sets it refuses, nor power 64): finite, and within 1e-3 of the oracle - a gross-error bound (f32 loses 1.6e-5 of D
    to cancellation near imp = 0.9995; measured worst per kind 2e-6 ... 3e-5, profiles/r23_solver_sets.txt)."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    sol = sc.DESIGNED_SETS[name]
    raw = sc.designed_model(kind, sol)
    states = sc.designed_states(kind, sol)
    ref = RefArm(raw.to_flat())
    eng = TreeRolloutEngine(raw, dtype="f64")
    err = _step_errors(raw, eng, ref, states)
    fails = eng.solver_failures()
    eng.close()
    print("%s / %s: f64 worst %.2e over %d states" % (kind, name, np.nanmax(err), len(states)))
    err32 = None
    try:
        assert np.isfinite(err).all() and err.max() < 1e-9, [(s[0], e) for s, e in zip(states, err) if not e < 1e-9]
        assert fails == 0 and ref.newton_stats()["fails"] == 0
        if name in sc.F32_REFUSED:
            with pytest.raises(NotImplementedError, match="single precision"):
                TreeRolloutEngine(raw, dtype="f32")
        elif name not in sc.F32_LEFT_OUT:
            eng = TreeRolloutEngine(raw, dtype="f32")
            err32 = _step_errors(raw, eng, ref, states)
            eng.close()
            assert np.isfinite(err32).all(), [(s[0], e) for s, e in zip(states, err32) if not np.isfinite(e)]
            assert err32.max() < 1e-3, [(s[0], e) for s, e in zip(states, err32) if not e < 1e-3]
    finally:
        _stats(test="designed", kind=kind, set=name, f64=float(np.nanmax(err)), f32=None if err32 is None else float(np.nanmax(err32)))


def test_last_class_model():
    """All eight classes in use, the last two read from both halves of dofcls: 16 random states at 1e-9."""
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from oracle.physics_ref import RefArm
    raw, _, pick = sc.last_class_model()
    eng, ref = TreeRolloutEngine(raw, dtype="f64"), RefArm(raw.to_flat())
    assert [(int(c) & 7, int(c) >> 3) for c in eng.model.field("dofcls")[:5]] == pick
    rs = np.random.RandomState(3)
    states = [(0.0, rs.uniform(-0.5, 0.5, 5), rs.standard_normal(5) * rs.choice([0.0, 1e-3, 1.0])) for _ in range(16)]
    live = sum(int(ref.step(q, v, np.zeros(5))[3][0] > 0) for _, q, v in states)
    assert live == 16
    err = _step_errors(raw, eng, ref, states)
    print("last-class model: worst %.2e" % err.max())
    _stats(test="last_class", f64=float(err.max()))
    assert err.max() < 1e-9 and eng.solver_failures() == 0


_OTHER_HOSTS = (0, 5, 7)


@pytest.mark.parametrize("seed", _OTHER_HOSTS)
def test_varied_model_on_the_rk4_build(seed):
    """The varied model through tree_rollout_rk4.hip against the RK4 step composed from the oracle's forward evaluations
    (tests/rk4_ref.py), as tests/test_rk4_gpu.py does with the plain random models: redrawn until it has at most 16 dofs and
    pyramidal cones, which is what those kernels hold."""
    import rk4_ref
    from test_random_models_gpu import random_state
    raw, eng, ref, tries, _ = _varied(seed, "f64", integrator="RK4", fits=lambda raw: raw.nv <= 16 and raw.cone == "pyramidal")
    rs = np.random.RandomState(seed + 77)
    tgt = np.asarray(raw.target_pos, float)
    worst = 0.0
    for k in range(6):
        q, v = random_state(raw, rs)
        u = rs.uniform(-1.5, 1.5, eng.d_action)
        eng.set_env_state(dict(qp=q, qv=v, target_pos=tgt))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        q1, v1, r1, o1, _ = rk4_ref.env_step(ref, raw, q, v, u, tgt)
        worst = max(worst, np.abs(nobs[0, 0] - o1).max() / max(1.0, np.abs(o1).max()), abs(rew[0, 0] - r1) / max(1.0, abs(r1)))
    print("seed %d (%d re-draws) RK4: nv %d, worst %.2e" % (seed, tries, raw.nv, worst))
    _stats(test="rk4", seed=seed, redraws=tries, worst=worst)
    assert worst < 1e-9 and eng.solver_failures() == 0
    eng.close()


@pytest.mark.parametrize("seed", _OTHER_HOSTS)
def test_varied_model_in_an_episode_batch(seed):
    """Three episodes of the varied model through the episode-batch build, each equal - bit for bit - to its own single-engine
    run (tests/batched_cases.py): no episode's rows read another's parameters or state."""
    import batched_cases as bc
    from test_random_models_gpu import random_state
    raw, eng, _, _, _ = _varied(seed, "f64")
    eng.close()
    rs = np.random.RandomState(seed + 55)
    tgt = np.asarray(raw.target_pos, float)
    states = []
    for e in range(3):
        q, v = random_state(raw, rs)
        states.append(dict(qp=q, qv=0.3 * v, target_pos=tgt + 0.05 * e))
    mppi = bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype), guards=False)
    out = bc.check_against_singles(mppi, raw, states, [31 + seed, 32 + seed, 33 + seed], 64, 8, 4, (0.5, 1.0, 0.3), "f64")
    assert not np.array_equal(out["nobs"][:, 0], out["nobs"][:, 1])
