"""CPU: the random hinge chains of tests/arm_chain_cases.py are what tests/test_arm_chains_gpu.py needs them to be.

Every chain of the suite compiles with ``compile_arm`` onto the PLAIN build of the arm kernels (no slide joint, no dry friction),
and its start states are live: shown by the oracle alone against twin models - the same chain with every joint unlimited, the
same chain without the floor.  A state has an active limit (contact) when the oracle's observation after one env step differs
from the twin's by more than 1e-9.  Last: ``compile_arm`` refuses solver sets it would ignore (a colliding geom's own
solref / solimp, a limited joint's own solreflimit / solimplimit), so ``make_engine`` sends such models to the tree engine."""
import numpy as np
import pytest

import arm_chain_cases as ac


@pytest.fixture(scope="module")
def chains(tmp_path_factory):
    from oracle.physics_ref import RefArm
    folder = tmp_path_factory.mktemp("chains")
    out = {}
    for seed in ac.SEEDS:
        raw = ac.load_chain(seed, folder)
        out[seed] = (raw, RefArm(raw.to_flat()))
    return out


def test_every_chain_lands_on_the_plain_build(chains):
    from mjmpc_amd.models.compile import compile_arm
    for seed, (raw, _) in chains.items():
        xml, nv, nu = ac.hinge_chain_xml(seed)
        m = compile_arm(raw)
        assert (m.nv, m.nu) == (nv, nu) == (raw.nv, len(raw.actuators)), seed
        # make_engine's rule: compile_arm accepts the model -> the arm engine; jtype / frictionloss all zero -> its plain build
        assert not m.field("jtype").any() and not m.field("frictionloss").any(), seed
        assert int(m.field("n_sphere")[0]) == (1 if raw.plane is not None else 0), seed
        assert all(1e-4 < x < 0.9999 for x in raw.solimp[:2]) and raw.solimp[0] < raw.solimp[1], seed
        assert tuple(raw.solref_limit) == tuple(raw.solref) and tuple(raw.solimp_limit) == tuple(raw.solimp), seed
        lo, hi = np.array([a.ctrlrange for a in raw.actuators]).T
        assert (lo < 0).all() and (hi > 0).all() and not np.array_equal(-lo, hi), seed


def test_the_chains_vary_what_they_are_meant_to_vary(chains):
    raws = [raw for raw, _ in chains.values()]
    assert {raw.nv for raw in raws} == set(range(1, 8))
    assert {int(raw.solimp[4]) for raw in raws} == {1, 2, 3, 4}
    assert {ac.gravity_kind(raw) for raw in raws} == {"down", "none", "tilted"}
    assert any(len(raw.actuators) < raw.nv for raw in raws)
    assert any(raw.solref[0] < 2 * raw.timestep for raw in raws) and any(raw.solref[0] > 2 * raw.timestep for raw in raws)
    assert any(raw.plane is None for raw in raws) and any(raw.plane is not None for raw in raws)
    # an unlimited joint beside a limited one, a body frame rotated against its parent, a link offset along no axis
    assert any(0 < sum(j.limited for j in raw.joints) < raw.nv for raw in raws)
    assert any(abs(b.quat[0]) < 0.999 for raw in raws for b in raw.bodies)
    assert any(np.count_nonzero(np.abs(np.asarray(b.pos, float)) > 1e-3) == 3 for raw in raws for b in raw.bodies)


def test_the_seeds_picked_by_the_gpu_tests_have_the_properties_they_are_picked_for(chains):
    def nv(s):
        return chains[s][0].nv

    def nu(s):
        return len(chains[s][0].actuators)
    assert {nv(s) for s in ac.SIZE_SEEDS} >= {1, 4, 7} and len(ac.SIZE_SEEDS) == 4
    assert any(chains[s][0].plane is not None for s in ac.SIZE_SEEDS) and any(nu(s) < nv(s) for s in ac.SIZE_SEEDS)
    assert len(ac.CL_SEEDS) == 3 and all(nu(s) < nv(s) or nv(s) < 7 for s in ac.CL_SEEDS)
    assert len(ac.MONO_SEEDS) == 3 and all(nu(s) in (1, 3, 5, 6) for s in ac.MONO_SEEDS) and len({nu(s) for s in ac.MONO_SEEDS}) == 3
    assert len(ac.BATCH_SEEDS) == 2 and any(nv(s) < 7 and nu(s) < nv(s) for s in ac.BATCH_SEEDS)


def test_the_states_are_live(chains):
    """Per chain: at least 3 of the 24 states with an active limit (where a joint is limited), at least 6 in contact (where
    there is a floor); no state makes the oracle reset, fail to solve or leave the finite numbers."""
    from oracle.physics_ref import RefArm
    for seed, (raw, ref) in chains.items():
        tgt = np.asarray(raw.target_pos, float)
        sts = ac.states(raw, ref, seed)
        assert len(sts) == ac.N_STATES
        limited, floor = any(j.limited for j in raw.joints), raw.plane is not None
        free = RefArm(ac.without_limits(raw).to_flat()) if limited else None
        clear = RefArm(ac.without_floor(raw).to_flat()) if floor else None
        n_limit = n_contact = n_clamped = 0
        for q, v, u in sts:
            o = ref.env_step(q, v, u, tgt)[3]
            assert np.isfinite(o).all(), seed
            if limited:
                n_limit += bool(np.abs(free.env_step(q, v, u, tgt)[3] - o).max() > 1e-9)
            if floor:
                n_contact += bool(np.abs(clear.env_step(q, v, u, tgt)[3] - o).max() > 1e-9)
            n_clamped += bool(any(not a.ctrlrange[0] <= x <= a.ctrlrange[1] for a, x in zip(raw.actuators, u)))
        print("chain %2d: nv %d nu %d, %d limited joints, %s: active limits in %2d, contact in %2d, clamped control in %2d of %d states"
              % (seed, raw.nv, len(raw.actuators), sum(j.limited for j in raw.joints), "floor" if floor else "no floor",
                 n_limit, n_contact, n_clamped, len(sts)))
        assert not limited or n_limit >= 3, (seed, n_limit)
        assert not floor or n_contact >= 6, (seed, n_contact)
        assert n_clamped >= 3, (seed, n_clamped)
        assert ref.newton_stats()["fails"] == 0 and ref.resets() == 0, seed
        # the same call gives the same states (the GPU file's parent and the oracle fixture rely on it)
        again = ac.states(raw, ref, seed)
        assert all(np.array_equal(a, b) for s, t in zip(sts, again) for a, b in zip(s, t))


def test_the_short_rollouts_stay_finite_on_the_oracle(chains):
    for seed, (raw, ref) in chains.items():
        q, v, mean, noise = ac.rollout_case(raw, seed)
        _, rew, _, _, nobs = ref.rollout(q, v, np.asarray(raw.target_pos, float), mean, noise)
        assert np.isfinite(rew).all() and np.isfinite(nobs).all(), seed
        assert ref.newton_stats()["fails"] == 0 and ref.resets() == 0, seed


# ------------------------------------------------------------------ compile_arm refuses solver sets it would ignore
def _load(xml, folder, name):
    from mjmpc_amd.models.mjcf import load_mjcf
    path = folder / name
    path.write_text(xml)
    return load_mjcf(str(path), frame_skip=2)


def test_compile_arm_refuses_per_element_solver_sets(chains, tmp_path):
    from mjmpc_amd.models.compile import compile_arm
    raw, _ = chains[ac.OWN_SET_SEED]
    assert raw.plane is not None and any(j.limited for j in raw.joints)
    base = compile_arm(raw)
    for what, xml in ac.own_solver_set_xmls(ac.OWN_SET_SEED).items():
        edited = _load(xml, tmp_path, what + ".xml")
        assert edited.solref == raw.solref and edited.solimp == raw.solimp, what        # the model-wide set did not move
        with pytest.raises(ValueError, match="tree engine"):
            compile_arm(edited)
        # ... and the oracle honours the element's set: what the arm engine would have simulated is another model
        assert not np.array_equal(edited.to_flat(), raw.to_flat()), what
    # a set EQUAL to the model's is fine, written on the element or not
    same = ac.hinge_chain_xml(ac.OWN_SET_SEED)[0].replace('<geom name="tip"', '<geom name="tip" solref="%g %g" solimp="%s"' % (
        raw.solref[0], raw.solref[1], " ".join("%g" % x for x in raw.solimp)))
    np.testing.assert_array_equal(compile_arm(_load(same, tmp_path, "same.xml")).blob, base.blob)


def test_compile_arm_refuses_raw_models_with_their_own_sets(chains):
    """The same on RawModel fields (models built in code): geom, plane and joint; a set on a geom that does not collide or on an
    unlimited joint reaches no constraint row and is accepted."""
    import copy
    from mjmpc_amd.models.compile import compile_arm
    raw, _ = chains[ac.OWN_SET_SEED]
    other_ref, other_imp = (0.05, 0.5), (0.8, 0.9, 0.002, 0.5, 2.0)

    def edit(fn):
        twin = copy.deepcopy(raw)
        fn(twin)
        return twin
    tip = lambda r: next(g for b in r.bodies for g in b.geoms if g.collide)                      # noqa: E731
    lim = lambda r: next(j for j in r.joints if j.limited)                                       # noqa: E731
    for fn in (lambda r: setattr(tip(r), "solref", other_ref), lambda r: setattr(tip(r), "solimp", other_imp),
               lambda r: setattr(r.plane, "solref", other_ref), lambda r: setattr(r.plane, "solimp", other_imp),
               lambda r: setattr(lim(r), "solref_limit", other_ref), lambda r: setattr(lim(r), "solimp_limit", other_imp)):
        with pytest.raises(ValueError, match="tree engine"):
            compile_arm(edit(fn))
    blob = compile_arm(raw).blob
    for fn in (lambda r: setattr(tip(r), "solref", tuple(r.solref)), lambda r: setattr(r.plane, "solimp", tuple(r.solimp)),
               lambda r: setattr(lim(r), "solref_limit", tuple(r.solref_limit)),
               lambda r: setattr(next(g for b in r.bodies for g in b.geoms if not g.collide), "solref", other_ref)):
        np.testing.assert_array_equal(compile_arm(edit(fn)).blob, blob)
    if any(not j.limited for j in raw.joints):
        np.testing.assert_array_equal(
            compile_arm(edit(lambda r: setattr(next(j for j in r.joints if not j.limited), "solref_limit", other_ref))).blob, blob)


def test_the_models_of_the_suite_still_compile(tmp_path):
    """reacher7dof, the cart-pole, the gantry and every serial chain of tests/test_arm_xj_random_gpu.py."""
    from mjmpc_amd.models.compile import compile_arm
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    from test_arm_xj_gpu import GANTRY
    from test_arm_xj_random_gpu import chain_xml
    compile_arm(reacher7dof_raw())
    compile_arm(synthetic_raw("cartpole"))
    compile_arm(_load(GANTRY, tmp_path, "gantry.xml"))
    for seed in range(32):
        compile_arm(_load(chain_xml(seed)[0], tmp_path, "xj%d.xml" % seed))
