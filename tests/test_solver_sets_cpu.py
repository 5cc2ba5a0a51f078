"""Solver-parameter sets on the host (no GPU): what compile_tree puts into ``soltab`` - clamped, mixed, refsafe'd - evaluated
the way the kernel's tree_row_params evaluates it, against a plain-numpy transcription of MuJoCo's getimpedance /
mj_referenceConstraint / mj_contactParam written with ``**``; the random generator of tests/solver_set_cases.py is live and
reaches what it is meant to reach; the designed states put x = |r| / width where they claim."""
import collections

import numpy as np
import pytest

from solver_set_cases import (DESIGNED_SETS, KINDS, MARGIN, TIMESTEP, WIDTH, clamped_mid, designed_model, designed_states,
                              draw_set, last_class_model, model_sets, row_violation, vary_solver_sets, x_grid)


def kernel_row(sol, r, diag, jv, dtype=np.float64):
    """tree_row_params (csrc/tree_rollout.hip) operation by operation, from one row of ``soltab``."""
    T = dtype
    K, B, dmin, dmax, width, mid = (T(s) for s in sol[:6])
    n = int(sol[6])
    r, diag, jv = T(r), T(diag), T(jv)
    x = abs(r) * (T(1) / width)
    x = T(1) if x > T(1) else x
    lo = x <= mid
    xa, ma = (x, mid) if lo else (T(1) - x, T(1) - mid)
    num, den = xa, T(1)
    for _ in range(1, n):
        num, den = num * xa, den * ma
    with np.errstate(all="ignore"):
        qq = num * (T(1) / den)
    y = x if n == 1 else (qq if lo else T(1) - qq)
    imp = dmin + y * (dmax - dmin)
    R = max((T(1) - imp) * (T(1) / imp) * diag, T(1e-15))
    return T(1) / R, -B * jv - K * imp * r


def mujoco_row(solref, solimp, timestep, r, diag, jv):
    """MuJoCo's getsolparam clamps, getimpedance and mj_referenceConstraint for one scalar row [EXT]."""
    dmin, dmax = (min(max(float(d), 1e-4), 0.9999) for d in solimp[:2])
    width, mid, power = max(float(solimp[2]), 0.0), min(max(float(solimp[3]), 1e-4), 0.9999), max(float(solimp[4]), 1.0)
    if dmin == dmax or width <= 1e-15:
        imp = 0.5 * (dmin + dmax)
    else:
        x = abs(r) / width
        if x >= 1:
            imp = dmax
        elif x <= 0:
            imp = dmin
        else:
            if power == 1:
                y = x
            elif x <= mid:
                y = x ** power / mid ** (power - 1)
            else:
                y = 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
            imp = dmin + y * (dmax - dmin)
    R = max((1 - imp) / imp * diag, 1e-15)
    tc, dr = solref
    if tc > 0:
        tc = max(tc, 2 * timestep)
        k, b = 1 / (dmax * dmax * tc * tc * dr * dr), 2 / (dmax * tc)
    else:
        k, b = -tc / (dmax * dmax), -dr / dmax
    return 1 / R, -b * jv - k * imp * r


def mj_contact_param(a, b):
    """mj_contactParam [EXT] for the solver set, each side (solref, solimp, solmix, priority); transcribed on its own."""
    if a[3] != b[3]:
        top = a if a[3] > b[3] else b
        return tuple(top[0]), tuple(top[1])
    if a[2] >= 1e-15 and b[2] >= 1e-15:
        mix = a[2] / (a[2] + b[2])
    elif a[2] < 1e-15 and b[2] < 1e-15:
        mix = 0.5
    elif a[2] < 1e-15:
        mix = 0.0
    else:
        mix = 1.0
    if a[0][0] > 0 and b[0][0] > 0:
        ref = tuple(mix * p + (1 - mix) * q for p, q in zip(a[0], b[0]))
    else:
        ref = tuple(min(p, q) for p, q in zip(a[0], b[0]))
    return ref, tuple(mix * p + (1 - mix) * q for p, q in zip(a[1], b[1]))


def _r_values(sol):
    width = sol[1][2] if sol[1][2] > 1e-15 else WIDTH
    return [-x * width for x in [0.0] + x_grid("limit", sol)]


def _worst(row, solref, solimp):
    """Largest relative difference of (D, aref) between the kernel's arithmetic on a soltab row and MuJoCo's formulas, over
    the x grid; jv has the sign of r, so that aref's two terms add and its relative error means something."""
    worst = 0.0
    for r in _r_values((solref, solimp)):
        for diag, jv in ((0.37, -0.3), (12.0, 0.0)):
            D, aref = kernel_row(row, r, diag, jv)
            D0, aref0 = mujoco_row(solref, solimp, TIMESTEP, r, diag, jv)
            worst = max(worst, abs(D - D0) / D0, abs(aref - aref0) / max(abs(aref0), 1e-300))
    return worst


def _limit_row(sol):
    from mjmpc_amd.models.compile_tree import compile_tree
    m = compile_tree(designed_model("limit", sol))
    lc = int(m.field("dofcls")[0]) & 7
    assert lc == 1
    return m.field("soltab")[7 * lc:7 * lc + 7]


def test_soltab_evaluates_to_mujocos_rows():
    """Measured 9e-15 (repeated multiplication against ``**``, up to power 64); the bound is 1e-12."""
    rs = np.random.RandomState(11)
    sets = [draw_set(rs, TIMESTEP) for _ in range(300)] + [draw_set(rs, TIMESTEP, p) for p in (1, 2, 3, 4, 5, 6) for _ in range(10)]
    sets += list(DESIGNED_SETS.values())
    worst = max(_worst(_limit_row(sol), *sol) for sol in sets)
    print("worst relative difference over %d sets: %.2e" % (len(sets), worst))
    assert worst < 1e-12, worst


def _contact_model(geom, plane, pair=None):
    """The condim-1 sphere over the floor (or, with ``pair``, over the slab under a <pair> override) with sets of their own:
    geom, plane = (solref, solimp, solmix, priority)."""
    raw = designed_model("pair" if pair is not None else "contact_condim1", ((0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2.0)))
    tip = raw.bodies[1].geoms[0]
    tip.solref, tip.solimp, tip.solmix, tip.priority = geom
    other = raw.world_geoms[0] if pair is not None else raw.plane
    other.solref, other.solimp, other.solmix, other.priority = plane
    if pair is not None:
        raw.pair_params[("tip", "slab")].update(pair)
    return raw


A_SET = ((0.011, 0.7), (0.6, 0.93, 0.004, 0.3, 3.0))
B_SET = ((0.003, 1.4), (0.97, 0.45, 0.02, 0.8, 3.0))
DIRECT = ((-3000.0, -90.0), (0.8, 0.9, 0.01, 0.6, 3.0))
MIXES = {
    "both_zero": (A_SET + (0.0, 0), B_SET + (0.0, 0), None),
    "geom_zero": (A_SET + (0.0, 0), B_SET + (2.0, 0), None),
    "plane_zero": (A_SET + (0.5, 0), B_SET + (0.0, 0), None),
    "weights": (A_SET + (0.5, 0), B_SET + (3.0, 0), None),
    "priority": (A_SET + (3.0, 0), B_SET + (0.0, 1), None),
    "direct_and_standard": (DIRECT + (1.0, 0), B_SET + (3.0, 0), None),
    "two_direct": (DIRECT + (1.0, 0), ((-900.0, -200.0), B_SET[1], 1.0, 0), None),
    "pair_override": (A_SET + (1.0, 0), B_SET + (1.0, 1), dict(solref=(0.009, 0.5), solimp=(0.5, 0.99, 0.03, 0.2, 4.0))),
}


@pytest.mark.parametrize("name", sorted(MIXES))
def test_contact_sets_mix_as_mj_contactparam(name):
    """The contact record's class holds mj_contactParam's mix (or the <pair>'s own set), and the oracle's compiler - which mixes
    on its own, in C - steps the model to the same next state whichever way the set is given: mixed here, or by the geoms."""
    from mjmpc_amd.models.compile_tree import compile_tree
    from oracle.physics_ref import RefArm
    geom, plane, pair = MIXES[name]
    raw = _contact_model(geom, plane, pair)
    m = compile_tree(raw)
    rec = m.field("spheres")[:24]
    cls = int(rec[21])
    want = (pair["solref"], pair["solimp"]) if pair is not None else mj_contact_param(geom, plane)
    assert _worst(m.field("soltab")[7 * cls:7 * cls + 7], *want) < 1e-12
    # the oracle: the geoms' sets as they are, against a model that is handed the mix as its model-wide set
    plain = designed_model("pair" if pair is not None else "contact_condim1", want)
    a, b = RefArm(raw.to_flat()), RefArm(plain.to_flat())
    tgt = np.asarray(raw.target_pos, float)
    for x, q, v in designed_states("contact_condim1", want):
        oa, ob = a.env_step(q, v, np.zeros(1), tgt)[3], b.env_step(q, v, np.zeros(1), tgt)[3]
        np.testing.assert_allclose(oa, ob, rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
SEEDS = range(48)
_N_STATES = 12


@pytest.fixture(scope="module")
def varied():
    """Every suite seed's varied model through compile_tree and the oracle: redraws, live states, oracle health, features."""
    from mjmpc_amd.models.compile_tree import compile_tree
    from oracle.physics_ref import RefArm
    from test_random_models_gpu import MAX_REDRAWS, random_model, random_state
    out = []
    for seed in SEEDS:
        tries, reasons, ref = 0, [], None
        while ref is None:
            raw = vary_solver_sets(random_model(1000 * tries + seed), 1000 * tries + seed)
            try:
                m = compile_tree(raw)
                ref = RefArm(raw.to_flat())
            except (ValueError, NotImplementedError, AssertionError) as e:
                reasons.append(str(e)[:60])
                ref, tries = None, tries + 1
                assert tries <= MAX_REDRAWS, "seed %d: %s" % (seed, reasons)
        rs = np.random.RandomState(seed + 77)
        tgt = np.asarray(raw.target_pos, float)
        live, finite = 0, True
        for k in range(_N_STATES):
            q, v = random_state(raw, rs)
            v *= (0.0 if k % 4 == 0 else 1.0)
            u = rs.uniform(-1.5, 1.5, m.nu)
            live += int(ref.step(q, v, np.clip(u, -1, 1))[3][0] > 0)
            finite &= bool(np.isfinite(ref.env_step(q, v, u, tgt)[3]).all())
        q, v = random_state(raw, rs)
        eps = 0.5 * rs.standard_normal((32, 6, m.nu))
        finite &= bool(np.isfinite(ref.rollout(q, 0.3 * v, tgt, np.zeros((6, m.nu)), eps)[4]).all())
        sets, mixes = model_sets(raw)
        out.append(dict(seed=seed, redraws=tries, reasons=reasons, live=live, finite=finite, fails=ref.newton_stats()["fails"],
                        resets=ref.resets(), sets=sets, mixes=mixes))
    return out


def test_generator_redraws_stay_bounded(varied):
    counts = collections.Counter(r for m in varied for r in m["reasons"])
    print("redraws per seed: max %d, total %d; by reason: %s" % (max(m["redraws"] for m in varied), sum(m["redraws"] for m in varied), dict(counts)))
    # (the fixture already asserts at most MAX_REDRAWS per seed)


def test_generator_states_have_active_rows(varied):
    """At least 9 of the 12 states of every model step with constraint rows in the oracle (measured minimum: see the print)."""
    print("live states per model: min %d" % min(m["live"] for m in varied))
    assert all(m["live"] >= 9 for m in varied), [(m["seed"], m["live"]) for m in varied if m["live"] < 9]


def test_generator_keeps_the_oracle_healthy(varied):
    assert all(m["finite"] for m in varied), [m["seed"] for m in varied if not m["finite"]]
    assert all(m["fails"] == 0 for m in varied), [(m["seed"], m["fails"]) for m in varied if m["fails"]]


def test_generator_reaches_every_feature(varied):
    """Over the 48 models: every contact power 1..4 and joint power 1..6; a flat width, a falling impedance, a clamped mid, a
    direct solref and a time constant under the refsafe clamp; a contact mixed with a zero solmix and one won by priority."""
    cp = {int(s[1][4]) for m in varied for s in m["sets"]["contact"]}
    jp = {int(s[1][4]) for m in varied for s in m["sets"]["joint"]}
    assert cp >= {1, 2, 3, 4} and jp >= {1, 2, 3, 4, 5, 6}, (cp, jp)
    every = [s for m in varied for kind in ("contact", "joint") for s in m["sets"][kind]]
    assert any(s[1][2] == 0.0 for s in every)
    assert any(s[1][0] > s[1][1] for s in every)
    assert any(s[1][3] == 0.0 for s in every) and any(s[1][3] == 1.0 for s in every)
    assert any(s[0][0] < 0 for s in every)
    assert any(0 < s[0][0] < 2 * TIMESTEP for s in every)
    mixes = sum((m["mixes"] for m in varied), collections.Counter())
    print("contact mixes:", dict(mixes))
    assert mixes["zero_solmix"] > 0 and mixes["priority"] > 0 and mixes["pair_override"] > 0


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["limit", "contact_condim1", "joint_equality", "tendon_limit"])
def test_designed_states_land_where_they_claim(kind):
    for name, sol in DESIGNED_SETS.items():
        mid = clamped_mid(sol)
        xs, signs = [], set()
        for x, q, v in designed_states(kind, sol):
            r = row_violation(kind, q)
            got = abs(r) / WIDTH
            assert abs(got - x) < 1e-12, (name, x, got)
            if kind != "joint_equality":
                assert r < 0 or x == 0      # the row is active
                signs.add(np.sign(r + MARGIN))
            else:
                signs.add(np.sign(r))
            xs.append(got)
        xs = np.array(xs)
        # both sides of mid - the two states a millionth of mid away from it included - and x >= 1
        assert ((xs < mid) & (xs > mid * (1 - 2e-6))).any() and ((xs > mid) & (xs < mid * (1 + 2e-6))).any(), (name, xs)
        assert (xs >= 1).any() and ((xs < 1) & (xs > 1 - 2e-6)).any()
        assert {-1.0, 1.0} <= signs, (name, signs)     # limit, contact, tendon: both signs of dist inside the margin


def test_every_designed_model_compiles_and_has_its_row():
    """Every kind x set compiles for the kernel and for the oracle, and the oracle steps every designed state with rows."""
    from mjmpc_amd.models.compile_tree import compile_tree
    from oracle.physics_ref import RefArm
    for kind in KINDS:
        for name, sol in DESIGNED_SETS.items():
            raw = designed_model(kind, sol)
            m = compile_tree(raw)
            assert m.nv <= 4
            ref = RefArm(raw.to_flat())
            for x, q, v in designed_states(kind, sol):
                diag = ref.step(q, v, np.zeros(m.nu))[3]
                assert diag[0] > 0, (kind, name, x)
            assert ref.newton_stats()["fails"] == 0


def test_last_class_model_fills_the_table():
    from mjmpc_amd.models.compile_tree import compile_tree
    raw, S, pick = last_class_model()
    m = compile_tree(raw)
    cls = m.field("dofcls")[:5].astype(int)
    assert [(c & 7, c >> 3) for c in cls] == pick
    for k in range(8):
        assert _worst(m.field("soltab")[7 * k:7 * k + 7], *S[k]) < 1e-12
