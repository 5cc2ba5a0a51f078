"""The designed models of tests/tree_shape_cases.py without a GPU: the Python restatement of the tree kernel's dispatch against
the instantiations the source compiles (the drift guard), what every case compiles to, the coverage of every instantiation by an
exact-fill case, the instantiation each named model of the suite takes, and - with the oracle alone - that the states the GPU
tests use load the last link (its limit row, its contact record, its motor) and that the oracle is well conditioned there."""
import dataclasses

import numpy as np
import pytest

import tree_shape_cases as tsc
from mjmpc_amd.models.compile_tree import PT_PLANE, PT_PLANE_CYL, SPH_STRIDE, compile_tree
from oracle.physics_ref import RefArm

ALL = tsc.CASES + tsc.SWITCHED


def test_restatement_names_what_the_source_instantiates():
    """The drift guard: every MJMPC_TREE_LAUNCH* call in the launch functions of tree_rollout.hip is an instantiation the
    restatement can return, and the other way round; two of them only with MJMPC_TREE_SPARSE in the environment."""
    plain, switched = tsc.all_restated()
    source = tsc.source_instantiations()
    assert source == plain | switched, sorted(source ^ (plain | switched), key=str)
    assert switched == {("sparse", 16, 0), ("sparse", 32, 0)}
    assert len(source) == 52


def test_cases_cover_every_instantiation_at_its_fill():
    """Every instantiation of the source is named by an exact-fill case: nv == DN on a path of DP links - or, for the 32-lane
    shapes without a dense factor, 32 dofs on the longest path the class admits - the plain launches by ``FILLS``, the two
    behind the sparse switch by ``SWITCHED``."""
    plain, switched = tsc.all_restated()
    by_inst = {}
    for c in tsc.FILLS:
        by_inst.setdefault(c.inst, []).append(c)
    assert set(by_inst) == plain, sorted(plain ^ set(by_inst), key=str)
    assert switched <= {c.inst for c in tsc.SWITCHED}
    for inst, cs in sorted(by_inst.items(), key=str):
        c = cs[0]
        print("%-26s %-16s nv %2d path %2d" % (inst, c.name, c.nv, c.max_path))
        if inst[0] == "dense":
            assert (c.max_path, c.nv) == (inst[1], inst[3])
        elif inst[0] == "rk4":
            assert (c.max_path, c.nv) == (inst[1], inst[2])
        elif inst[0] == "cone" and inst[3]:
            assert (c.max_path, c.nv) == (inst[1], inst[3])
        elif inst == ("sparse", 16, 1):
            assert (c.max_path, c.nv) == (8, 32)        # (paths of 9 .. 16 go to the dense shape unless the switch is set)
        else:
            assert (c.max_path, c.nv) == (inst[-1] if inst[0] == "lean" else inst[1], 32)
    print("%d instantiations, each with an exact-fill case; %d cases in all" % (len(plain | switched), len(ALL)))
    # the edge models the issue names
    shapes = {(c.family, c.nv, c.max_path, c.records) for c in ALL}
    for want in [("g0", 32, 32, 1), ("lean", 32, 32, 1), ("g0", 32, 16, 1), ("g1", 32, 16, 1), ("g2", 32, 16, 1), ("g3", 32, 16, 1),
                 ("g0", 32, 8, 1), ("g0", 31, 31, 1), ("g0", 17, 9, 1), ("g0", 17, 8, 1), ("g0", 16, 16, 1), ("g1", 16, 16, 1),
                 ("g2", 16, 16, 1), ("g3", 16, 16, 1), ("g0", 32, 17, 1), ("g0", 32, 31, 1), ("g0", 32, 16, 16)]:
        assert want in shapes, want
    assert tsc.BY_NAME["g0_8+9"].inst == ("dense", 16, 32, 32, 0) and tsc.BY_NAME["g0_1+8+8"].inst == ("sparse", 8, 0)
    assert tsc.BY_NAME["rk4g0_16"].inst == ("rk4", 16, 16, 0)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_compiles_to_what_it_declares(case):
    raw = tsc.build(case)
    m = compile_tree(raw)
    assert (m.nv, m.max_path, int(m.field("gen")[0]), tsc.is_full(m)) == (case.nv, case.max_path, case.gen, case.full)
    assert tsc.model_instantiation(m, sparse_switch=case in tsc.SWITCHED) == case.inst and case.inst is not None
    # the tracked site on the last link, motors on the first and the last hinge / slide dof, the last plane record on the last link
    single = [raw.dof_of_joint(b.joint.name) for b in raw.bodies if b.joint.ndof == 1]
    assert int(m.field("site_link")[0]) == m.nv - 1
    assert sorted(d for d in range(m.nv) if m.field("act")[d] >= 0) == sorted({single[0], single[-1]})
    recs = m.field("spheres").reshape(-1, SPH_STRIDE)[:int(m.field("n_sphere")[0])]
    plane = [r for r in recs if int(r[12]) in (PT_PLANE, PT_PLANE_CYL)]
    assert len(plane) == case.records + (4 if case.family == "g2" else 0)
    assert int(plane[-1][0]) == m.nv - 1 and int(plane[-1][12]) == PT_PLANE and int(plane[-1][11]) == case.max_path - 1


def test_edge_models_sit_where_the_issue_puts_them():
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE
    raw = tsc.build(tsc.BY_NAME["ball_32"])
    lanes = {raw.dof_of_joint(b.joint.name): b.joint.type for b in raw.bodies if b.joint.type in (JOINT_BALL, JOINT_FREE)}
    assert lanes == {0: JOINT_FREE, 13: JOINT_BALL, 16: JOINT_BALL, 29: JOINT_BALL}
    raw = tsc.build(tsc.BY_NAME["ball_16+16"])
    assert {raw.dof_of_joint(b.joint.name) for b in raw.bodies if b.joint.type in (JOINT_BALL, JOINT_FREE)} == {0, 13, 16, 29}
    raw = tsc.build(tsc.BY_NAME["nq40_16+16"])
    assert (raw.nq, raw.nv) == (40, 32) and compile_tree(raw).d_obs == 40 + 32 + 6
    for name in ("rec16_16+16", "rec16_32"):
        m = compile_tree(tsc.build(tsc.BY_NAME[name]))
        recs = m.field("spheres").reshape(-1, SPH_STRIDE)
        assert int(m.field("n_sphere")[0]) == 16 and int(recs[15][0]) == 31
    raw41 = tsc.build(tsc.NQ41, plane_z=-1.0)
    assert (raw41.nq, raw41.nv) == (41, 32)
    with pytest.raises(ValueError, match="too many qpos entries"):
        compile_tree(raw41)


def _named_models(tmp_path):
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    from mjmpc_amd.models.hand24 import hand24_raw
    from mjmpc_amd.models.pen_hand import pen_hand_raw
    from mjmpc_amd.models.swimmer import swimmer_raw
    from mjmpc_amd.models.synthetic import synthetic_raw
    from test_general_models_cpu import WELDED, WELDS, _model
    fr = hand24_raw()               # (test_hand_with_friction_runs_the_full_kernel_at_32_lanes' edits)
    for b in fr.bodies:
        if b.joint is not None and b.name.endswith("_mid"):
            b.joint.stiffness, b.joint.springref = 0.05, 0.3
        for g in b.geoms:
            if g.collide:
                g.friction, g.condim = 0.8, 3
    fr.plane = dataclasses.replace(fr.plane, friction=0.5, condim=3)
    out = [("hand", hand24_raw()), ("hand with friction", fr), ("pen_hand", pen_hand_raw()), ("cheetah", half_cheetah_raw()),
           ("cheetah RK4", dataclasses.replace(half_cheetah_raw(), integrator="RK4")), ("swimmer", swimmer_raw()),
           ("swimmer RK4", dataclasses.replace(swimmer_raw(), integrator="RK4"))]
    out += [(n, synthetic_raw(n)) for n in ("cartpole", "door", "tray", "gripper")]
    out.append(("welded bodies", _model(tmp_path, WELDED, extra=WELDS, timestep="0.001")[0]))
    return out


def test_named_models_table(tmp_path):
    """Which instantiation each named model of the suite takes (printed; DESIGN 4.6 holds the table)."""
    rows = []
    for name, raw in _named_models(tmp_path):
        m = compile_tree(raw)
        rows.append((name, m.nv, m.max_path, int(m.field("gen")[0]), tsc.is_full(m), tsc.model_instantiation(m)))
    # test_deep_chains_use_the_wider_row_instantiations asserts nv == n_links + 2 on a path of n_links, lean and full (gen 0)
    for n in (12, 20):
        for full in (False, True):
            rows.append(("deep chain %d %s" % (n, "full" if full else "lean"), n + 2, n, 0, full, tsc.instantiation(n + 2, n, full, 0)))
    source = tsc.source_instantiations()
    for name, nv, path, gen, full, inst in rows:
        print("%-22s nv %2d path %2d gen %d %-4s -> %s" % (name, nv, path, gen, "full" if full else "lean", inst))
        assert inst in source
    got = dict((r[0], r[5]) for r in rows)
    assert got["hand"] == ("lean", 8) and got["hand with friction"] == ("sparse", 8, 0) and got["cheetah"] == ("dense", 8, 16, 9, 0)
    assert got["swimmer"] == ("dense", 7, 16, 7, 0) and got["cartpole"] == ("dense", 2, 16, 2, 1)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_states_load_the_last_link_and_the_oracle_is_well_conditioned(case):
    """Of the states the GPU tests step from: one at least has the last joint beyond its limit, one at least has the last plane
    record's sphere inside the contact margin, every one drives the last dof's motor - and the oracle's own env step moves by
    less than 1e-10 (relative) when the state moves by 1e-15: the 1e-9 gate measures the kernel, not the model's conditioning."""
    raw = tsc.build(case)
    ref = RefArm(raw.to_flat())
    sts = tsc.states(case, np.random.RandomState(7), raw)
    tgt = np.asarray(raw.target_pos, float)
    limit = [tsc.last_limit_violation(raw, q) > 0 for q, v, u in sts]
    dist = [ref.site(q)[2] - tsc.TIP_RADIUS - raw.plane.pos[2] for q, v, u in sts]
    assert any(limit) and limit[0] and limit[1]
    assert -0.002 < dist[0] < 0 and dist[1] == dist[0]          # (penetrating by a millimetre: a force, not only a row)
    last_act = raw.actuators[-1]
    assert raw.dof_of_joint(last_act.joint) == max(raw.dof_of_joint(b.joint.name) for b in raw.bodies if b.joint.ndof == 1)
    worst = 0.0
    for k, (q, v, u) in enumerate(sts):
        assert abs(last_act.gear * np.clip(u[-1], *last_act.ctrlrange)) >= 0.1
        q1, v1, r1, o1 = ref.env_step(q, v, u, tgt)
        assert np.isfinite(o1).all() and np.isfinite(r1)
        q2, v2, r2, o2 = ref.env_step(q * (1 + 1e-15), v * (1 + 1e-15), u, tgt)
        worst = max(worst, np.abs(o2 - o1).max() / max(1.0, np.abs(o1).max()), abs(r2 - r1) / max(1.0, abs(r1)))
    print("%s: the oracle moves by %.1e under a 1e-15 perturbation" % (case.name, worst))
    assert worst < 1e-10, worst
    assert ref.newton_stats()["fails"] == 0
