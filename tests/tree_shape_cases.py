"""Designed models that fill every instantiation of the tree rollout kernel to its last lane, shared by
tests/test_tree_shapes_cpu.py and tests/test_tree_shapes_gpu.py.  Not a test file.

``instantiation(nv, max_path, full, gen, integrator, sparse_switch)`` restates, in Python, the choice the four launch functions at
the end of mjmpc_amd/csrc/tree_rollout.hip make (launch_tree_rows, launch_tree_rollout_dense, _cone, _rk4); ``is_full(model)``
restates capi.hip's tree_blob_is_full.  ``source_instantiations()`` reads the launch functions as text: the CPU test holds the
restatement to the set of instantiations the source compiles, so a shape added to the kernel without a case fails there.

``CASES``: bushes of hinge chains hanging from the world, every chain along -z under gravity, oblique joint axes, every joint
limited, motors on the first and the last dof, the tracked site and a contact sphere at the tip of the LAST chain - the
longest, whose last link sits on the model's last lane.  The family adds only what selects the kernel: ``lean`` nothing
(frictionless sphere); ``g0`` a slide joint, springs and a friction cone; ``g1`` friction loss on top; ``g2`` a cylinder on the
last link (its four plane records are what compile_tree's gen = 2 stands for - a joint margin alone stays gen 1); ``g3`` an
elliptic cone.  The floor's height is set from the designed state, so that there the tip sphere penetrates by a millimetre
while the last joint stands beyond its limit.
"""
import collections
import dataclasses
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_SOURCE = os.path.join(ROOT, "mjmpc_amd", "csrc", "tree_rollout.hip")


# ------------------------------------------------------------------------------------------- the dispatch, restated
def _dense(max_path, nv, gen):
    """launch_tree_rollout_dense -> ("dense", DP, PL, DN, GEN)"""
    if nv > 16:
        if gen >= 2:
            return ("dense", 16, 32, 32, 2)
        if gen:
            return ("dense", 16, 32, 32, 1)
        return ("dense", 16 if max_path <= 16 else 32, 32, 32, 0)
    if gen >= 2:
        sizes = [(4, 4), (8, 8), (8, 12), (8, 16)]
    elif gen:
        sizes = [(2, 2), (4, 4), (8, 8), (8, 12), (8, 16), (10, 10), (12, 12)]
    else:
        sizes = [(7, 7), (8, 8), (8, 9), (8, 10), (8, 12), (8, 16)]
    for dp, dn in sizes:
        if max_path <= dp and nv <= dn:
            return ("dense", dp, 16, dn, min(gen, 2))
    return ("dense", 16, 16, 16, min(gen, 2))


def _cone(max_path, nv):
    """launch_tree_rollout_cone -> ("cone", DP, PL, DN); DN = 0: the tree-sparse factorisation"""
    if nv > 16:
        return ("cone", 16, 32, 32) if max_path <= 16 else ("cone", 32, 32, 0)
    for dp, dn in [(4, 4), (8, 8), (8, 12), (8, 16)]:
        if max_path <= dp and nv <= dn:
            return ("cone", dp, 16, dn)
    return ("cone", 16, 16, 16)


def _rk4(max_path, nv, gen):
    """launch_tree_rollout_rk4 -> ("rk4", DP, DN, GEN), None where the launch is refused"""
    if nv > 16 or gen >= 3:
        return None
    for dp, dn in [(4, 4), (8, 8), (8, 12)]:
        if max_path <= dp and nv <= dn:
            return ("rk4", dp, dn, gen)
    return ("rk4", 16, 16, gen)


def instantiation(nv, max_path, full, gen, integrator=0, sparse_switch=False):
    """The instantiation launch_tree_rows runs for a model: ("lean", DP), ("sparse", DP, GEN), ("dense", DP, PL, DN, GEN),
    ("cone", DP, PL, DN) or ("rk4", DP, DN, GEN); None where the launch returns an error.  ``integrator``: 0 Euler, 1 RK4;
    ``sparse_switch``: MJMPC_TREE_SPARSE is in the environment."""
    if gen and not full:
        return None
    if integrator == 1:
        return _rk4(max_path, nv, gen)
    if integrator != 0:
        return None
    if gen >= 3:
        return _cone(max_path, nv)
    if not full:
        return ("lean", 8 if max_path <= 8 else (16 if max_path <= 16 else 32))
    if nv <= 16:
        return _dense(max_path, nv, gen)
    if (max_path <= 16) if gen >= 2 else (max_path > 8 and not (gen and max_path > 16) and not sparse_switch):
        return _dense(max_path, nv, gen)
    if gen >= 2:
        return ("sparse", 32, 2)
    if gen:
        return ("sparse", 16 if max_path <= 16 else 32, 1)
    return ("sparse", 8 if max_path <= 8 else (16 if max_path <= 16 else 32), 0)


def all_restated():
    """Every instantiation the restatement can return: (plain launches, those only the sparse switch reaches)."""
    plain, switched = set(), set()
    for nv in range(1, 33):
        for max_path in range(1, nv + 1):
            for gen in range(4):
                for full in (False, True):
                    for integrator in (0, 1):
                        plain.add(instantiation(nv, max_path, full, gen, integrator))
                        switched.add(instantiation(nv, max_path, full, gen, integrator, True))
    plain.discard(None)
    switched.discard(None)
    return plain, switched - plain


def is_full(model):
    """capi.hip's tree_blob_is_full on a compiled TreeModel."""
    nv = model.nv
    return bool(model.field("any_friction")[0] != 0.0 or int(model.field("n_sphere")[0]) > 8 or model.field("density")[0] > 0.0 or
                model.field("viscosity")[0] > 0.0 or model.field("gen")[0] != 0.0 or
                np.any(model.field("jtype")[:nv].astype(int) == 2) or np.any(model.field("stiffness")[:nv] != 0.0))


def model_instantiation(model, sparse_switch=False):
    return instantiation(model.nv, model.max_path, is_full(model), int(model.field("gen")[0]),
                         1 if model.integrator == "RK4" else 0, sparse_switch)


def _name(dp, ns, fric, pl, dn, gen):
    if gen == 3:
        return ("cone", dp, pl, dn)
    if not fric:
        return ("lean", dp)
    return ("dense", dp, pl, dn, gen) if dn else ("sparse", dp, gen)


def source_instantiations(path=TREE_SOURCE):
    """The argument tuples of every MJMPC_TREE_LAUNCH / _G / _D / _RK4 call inside the launch functions of the kernel source,
    under the names ``instantiation`` gives them."""
    text = open(path).read()
    text = text[text.index("hipError_t launch_tree_rollout_dense(int max_path, int nv, int gen, const T* model, const T* noise, T* cost, "
                           "T* act, T* obs, T* nobs,\n                                     const TreeLaunchArgs& a) {"):]
    out = set()
    for line in text.splitlines():
        code = line.split("//")[0]
        if code.lstrip().startswith("#define"):
            continue
        for macro, args in re.findall(r"\bMJMPC_TREE_LAUNCH(_RK4|_G|_D|)\(([^()]*)\)", code):
            a = [x.strip() for x in args.split(",")]
            if any(x.endswith("_") for x in a):
                # MJMPC_TREE_LAUNCH_RK4_SIZES' body: the four sizes, once per GEN_ it is expanded with (counted below)
                assert macro == "_RK4" and a[2] == "GEN_", line
                out.add(("rk4_sizes", int(a[0]), int(a[1])))
                continue
            b = {"true": True, "false": False}
            if macro == "_RK4":
                out.add(("rk4", int(a[0]), int(a[1]), int(a[2])))
            elif macro == "_D":
                out.add(_name(int(a[0]), int(a[1]), b[a[2]], int(a[3]), int(a[4]), int(a[5])))
            elif macro == "_G":
                out.add(_name(int(a[0]), int(a[1]), b[a[2]], int(a[3]), 0, int(a[4])))
            else:
                out.add(_name(int(a[0]), int(a[1]), b[a[2]], int(a[3]), 0, 0))
    gens = [int(g) for g in re.findall(r"\bMJMPC_TREE_LAUNCH_RK4_SIZES\((\d+)\)", text)]
    sizes = [s for s in out if s[0] == "rk4_sizes"]
    assert gens and sizes
    out -= set(sizes)
    out |= {("rk4", dp, dn, g) for _, dp, dn in sizes for g in gens}
    return out


# ------------------------------------------------------------------------------------------------------ the models
LINK = 0.04             # link length: a 32-link chain is 1.3 m long
TIP_RADIUS = 0.015
MARGIN = 0.002
HINGE_RANGE = (-1.0, 1.0)
BALL_RANGE = (0.0, 0.8)
AXES = [(1.0, 0.3, 0.2), (-0.3, 1.0, 0.25), (0.7, 0.7, -0.2)]
FAMILIES = ("lean", "g0", "g1", "g2", "g3")
GEN_OF = dict(lean=0, g0=0, g1=1, g2=2, g3=3)

Case = collections.namedtuple("Case", "name chains family integrator nv max_path gen full inst fill records")
# chains: per chain the joints root to tip, "H" hinge, "S" slide, "B" ball, "F" free; the chains are listed shortest first
# fill: the case stands for its instantiation at nv == DN and max_path == DP (or the most the class admits)
# records: colliding tip spheres on the last `records` bodies (1: the tip of the last chain only)


def _unit(a):
    a = np.asarray(a, float)
    return tuple(a / np.linalg.norm(a))


def build(case, plane_z=None):
    """RawModel of a case.  The floor's height comes from the designed state (the oracle's site position there) unless given."""
    from mjmpc_amd.models.raw import (GEOM_CAPSULE, GEOM_CYLINDER, GEOM_SPHERE, JOINT_BALL, JOINT_FREE, JOINT_HINGE, JOINT_SLIDE,
                                      RawActuator, RawBody, RawGeom, RawJoint, RawModel, RawPlane)
    fam = case.family
    full, gen = fam != "lean", GEN_OF[fam]
    bodies, k = [], 0
    for c, chain in enumerate(case.chains):
        for d, kind in enumerate(chain):
            i = len(bodies)
            pos = (0.3 * c, 0.1 * (c % 2), 0.0) if d == 0 else (0.0, 0.0, -LINK)
            if kind == "F":
                jt = RawJoint((0.0, 0.0, 1.0), (0.0, 0.0), False, 0.0, 0.0, "j%d" % i, type=JOINT_FREE)
            elif kind == "B":
                jt = RawJoint((0.0, 0.0, 1.0), BALL_RANGE, True, 0.1, 0.005, "j%d" % i, type=JOINT_BALL)
            elif kind == "S":
                jt = RawJoint(_unit(AXES[k % 3]), (-0.1, 0.1), True, 0.1, 0.005, "j%d" % i, type=JOINT_SLIDE)
            else:
                jt = RawJoint(_unit(AXES[k % 3]), HINGE_RANGE, True, 0.1, 0.005, "j%d" % i, type=JOINT_HINGE)
            if kind in "HS":
                if full and k % 4 == 1:
                    jt.stiffness, jt.springref = 1.0, 0.1
                if gen >= 1 and k % 5 == 2:
                    jt.frictionloss = 0.05
            k += {"H": 1, "S": 1, "B": 3, "F": 6}[kind]
            bodies.append(RawBody("b%d" % i, -1 if d == 0 else i - 1, pos, joint=jt,
                                  geoms=[RawGeom(GEOM_CAPSULE, 0.012, (0.0, 0.0, 0.0), (0.0, 0.0, -LINK), margin=MARGIN, name="c%d" % i)]))
    last = bodies[-1]
    if last.joint.type == JOINT_HINGE and full:
        last.joint.stiffness, last.joint.springref = 1.0, 0.1
        if gen >= 1:
            last.joint.frictionloss = 0.05
    if fam == "g2":         # a cylinder lying across the tip, its lowest line half a millimetre above the sphere's lowest point
        last.geoms.append(RawGeom(GEOM_CYLINDER, TIP_RADIUS - 0.0005, (-0.01, 0.0, -LINK), (0.01, 0.0, -LINK), margin=MARGIN,
                                  name="cyl", friction=0.6, condim=3, collide=True))
    for b in bodies[len(bodies) - case.records:]:
        b.geoms.append(RawGeom(GEOM_SPHERE, TIP_RADIUS, (0.0, 0.0, -LINK), margin=MARGIN, name="s" + b.name, friction=0.6,
                               condim=3 if full else 1, collide=True))
    single = [b.joint.name for b in bodies if b.joint.type in (JOINT_HINGE, JOINT_SLIDE)]
    acts = [RawActuator(n, 0.5, (-1.0, 1.0)) for n in dict.fromkeys([single[0], single[-1]])]
    raw = RawModel(bodies=bodies, actuators=acts, site_body=len(bodies) - 1, site_pos=(0.0, 0.0, -LINK), target_pos=(0.2, 0.1, -0.3),
                   plane=RawPlane((0.0, 0.0, -10.0), (0.0, 0.0, 1.0), MARGIN, friction=0.5, condim=3 if full else 1),
                   timestep=0.002, frame_skip=2, gravity=(0.0, 0.0, -9.81), cone="elliptic" if fam == "g3" else "pyramidal",
                   impratio=3.0 if fam == "g3" else 1.0, integrator="RK4" if case.integrator else "Euler")
    if plane_z is None:
        plane_z = _PLANE_Z.get(case.name)
    if plane_z is None:
        from oracle.physics_ref import RefArm
        q = designed_q(raw)
        plane_z = _PLANE_Z[case.name] = float(np.asarray(RefArm(raw.to_flat()).site(q))[2]) - TIP_RADIUS + 0.001
    raw.plane = dataclasses.replace(raw.plane, pos=(0.0, 0.0, plane_z))
    return raw


_PLANE_Z = {}


def _quat(w):
    w = np.asarray(w, float)
    a = np.linalg.norm(w)
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * w / max(a, 1e-12)])


def designed_q(raw, beyond=0.03):
    """Every chain nearly straight down; the last joint ``beyond`` past its upper limit."""
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE, JOINT_SLIDE
    q, adr = raw.qpos0.copy(), 0
    for i, b in enumerate(raw.bodies):
        jt = b.joint
        lastj = i == len(raw.bodies) - 1
        if jt.type == JOINT_FREE:
            q[adr + 3:adr + 7] = _quat(0.1 * np.array([np.sin(i + 1.0), np.cos(i + 1.0), 0.3]))
        elif jt.type == JOINT_BALL:
            q[adr:adr + 4] = _quat((max(jt.range) + beyond if lastj else 0.15) * np.array(_unit([np.sin(1.7 * i), np.cos(1.7 * i), 0.4])))
        elif lastj:
            q[adr] = jt.range[1] + beyond
        else:
            q[adr] = (0.03 if jt.type == JOINT_SLIDE else 0.15) * np.sin(1.7 * i + 0.5)
        adr += jt.nq
    return q


def states(case, rs, raw=None, n_random=6):
    """[(q, v, u)]: two designed states (at rest and moving: the last link beyond its limit, its sphere on the floor), then
    random ones as tests/test_random_models_gpu.py's ``random_state`` draws them (every fourth at rest).  The last dof's
    actuator always gets a control of at least 0.2."""
    from test_random_models_gpu import random_state
    raw = build(case) if raw is None else raw
    A = len(raw.actuators)
    out = []
    for k in range(2 + n_random):
        if k < 2:
            q, v = designed_q(raw), (0.0 if k == 0 else 0.3) * rs.standard_normal(raw.nv)
        else:
            q, v = random_state(raw, rs)
            v = v * (0.0 if k % 4 == 2 else 1.0)
        u = rs.uniform(-1.5, 1.5, A)
        if abs(u[-1]) < 0.2:
            u[-1] = 0.2 if u[-1] >= 0 else -0.2
        out.append((q, v, u))
    return out


def last_limit_violation(raw, q):
    """How far the last joint stands beyond its range in ``q`` (positive: its limit row is active)."""
    from mjmpc_amd.models.raw import JOINT_BALL
    jt = raw.bodies[-1].joint
    if jt.type == JOINT_BALL:
        w = np.clip(abs(q[-4]), 0.0, 1.0)
        return 2.0 * np.arccos(w) - max(jt.range)
    return max(jt.range[0] - q[-1], q[-1] - jt.range[1])


def _chains(lengths, slide):
    """Hinge chains of the given lengths, shortest first; ``slide``: the second joint of the last chain is a slide (chains of
    three links and more)."""
    out = ["H" * n for n in sorted(lengths)]
    if slide and len(out[-1]) >= 3:
        out[-1] = "HS" + out[-1][2:]
    return tuple(out)


def _case(name, lengths, family, integrator=0, fill=False, chains=None, records=1, switch=False):
    chains = _chains(lengths, family != "lean") if chains is None else tuple(chains)
    nd = dict(H=1, S=1, B=3, F=6)
    nv = sum(nd[j] for c in chains for j in c)
    max_path = max(sum(nd[j] for j in c) for c in chains)
    gen, full = GEN_OF[family], family != "lean"
    if any(j in "BF" for c in chains for j in c):
        gen = max(gen, 1)
    return Case(name, chains, family, integrator, nv, max_path, gen, full,
                instantiation(nv, max_path, full, gen, integrator, switch), fill, records)


def _fills():
    """One exact-fill case per instantiation: the declared (DP, DN) written out by hand, the chains chosen to meet them."""
    out = []

    def add(inst, lengths, family, integrator=0, switch=False):
        c = _case("%s_%s%s" % (("rk4" if integrator else "") + family, "+".join(str(n) for n in sorted(lengths)), "_sw" if switch else ""),
                  lengths, family, integrator, fill=True, switch=switch)
        assert c.inst == inst, (c.name, c.inst, inst)
        out.append(c)
    # lean and tree-sparse: 32 lanes, no dense factor - the most dofs and the longest path the class admits
    add(("lean", 8), [8, 8, 8, 8], "lean")
    add(("lean", 16), [16, 16], "lean")
    add(("lean", 32), [32], "lean")
    add(("sparse", 8, 0), [8, 8, 8, 8], "g0")
    add(("sparse", 16, 1), [8, 8, 8, 8], "g1")             # (plain launches: paths of up to 8; 16 + 16 under the switch below)
    add(("sparse", 32, 1), [32], "g1")
    add(("sparse", 32, 2), [32], "g2")
    add(("cone", 32, 32, 0), [32], "g3")
    # dense over 32 lanes
    add(("dense", 16, 32, 32, 0), [16, 16], "g0")
    add(("dense", 32, 32, 32, 0), [32], "g0")
    add(("dense", 16, 32, 32, 1), [16, 16], "g1")
    add(("dense", 16, 32, 32, 2), [16, 16], "g2")
    add(("cone", 16, 32, 32), [16, 16], "g3")
    # dense over 16 lanes: nv == DN on a path of DP links
    for dp, dn in [(7, 7), (8, 8), (8, 9), (8, 10), (8, 12), (8, 16), (16, 16)]:
        add(("dense", dp, 16, dn, 0), [dp] + ([dn - dp] if dn > dp else []), "g0")
    for dp, dn in [(2, 2), (4, 4), (8, 8), (8, 12), (8, 16), (10, 10), (12, 12), (16, 16)]:
        add(("dense", dp, 16, dn, 1), [dp] + ([dn - dp] if dn > dp else []), "g1")
    for dp, dn in [(4, 4), (8, 8), (8, 12), (8, 16), (16, 16)]:
        add(("dense", dp, 16, dn, 2), [dp] + ([dn - dp] if dn > dp else []), "g2")
        add(("cone", dp, 16, dn), [dp] + ([dn - dp] if dn > dp else []), "g3")
    for gen in (0, 1, 2):
        for dp, dn in [(4, 4), (8, 8), (8, 12), (16, 16)]:
            add(("rk4", dp, dn, gen), [dp] + ([dn - dp] if dn > dp else []), "g%d" % gen, integrator=1)
    return out


def _overs(fills):
    """For every exact fill, the model one dof over (one more one-link chain) and the model one link over (the longest chain
    one link longer, the shortest other chain one shorter where the dofs are at the fill already): each lands in another class."""
    out, seen = [], {(c.chains, c.family, c.integrator) for c in fills}
    for c in fills:
        lengths = [len(ch) for ch in c.chains]
        grown = []
        if c.nv < 32 and not (c.integrator and c.nv == 16):
            grown.append(("dof", [1] + lengths))
        longer = sorted(lengths[:-1]) + [lengths[-1] + 1]
        if c.nv == 32 or (c.integrator and c.nv == 16) or len(lengths) > 1:
            if len(longer) > 1:
                longer[0] -= 1
                longer = [n for n in longer if n > 0]
            else:
                longer = None
        if longer is not None:
            grown.append(("link", longer))
        for what, ls in grown:
            o = _case("%s_%s" % (("rk4" if c.integrator else "") + c.family, "+".join(str(n) for n in sorted(ls))), ls, c.family,
                      c.integrator)
            key = (o.chains, o.family, o.integrator)
            if key in seen or o.inst is None:
                continue
            seen.add(key)
            assert o.inst != c.inst, (c.name, what, o.name, o.inst)
            out.append(o)
    return out


def _edges():
    """The edge models the fills do not already hold."""
    H = "H"
    out = [
        # (32 dofs as one chain / as 16 + 16 / as four chains of 8 are fills above; under the sparse switch they are SWITCHED)
        _case("g0_31", [31], "g0"),                                     # 31 dofs as one chain
        _case("g0_8+9", [8, 9], "g0"),                                  # the smallest model on the dense 32-lane shape
        _case("g0_1+8+8", [1, 8, 8], "g0"),                             # the smallest on the tree-sparse shape
        _case("g0_17+15", [15, 17], "g0"),
        _case("g0_31+1", [1, 31], "g0"),
        _case("lean_31+1", [1, 31], "lean"),
        # a free joint on lanes 0..5, ball joints on lanes 13..15, 16..18 and 29..31: one chain of 32 links, and as 16 + 16
        _case("ball_32", None, "g1", chains=["F" + H * 7 + "BB" + H * 10 + "B"]),
        _case("ball_16+16", None, "g1", chains=["F" + H * 7 + "B", "B" + H * 10 + "B"]),
        _case("ballcone_16+16", None, "g3", chains=["F" + H * 7 + "B", "B" + H * 10 + "B"]),
        # nq == 40: eight ball joints and eight hinges
        _case("nq40_16+16", None, "g1", chains=["BBBB" + H * 4, H * 4 + "BBBB"]),
        # 16 contact records on 32 dofs, the last one anchored on link 31
        _case("rec16_16+16", [16, 16], "g0", records=16),
        _case("rec16_32", [32], "g1", records=16),
    ]
    return out


FILLS = _fills()
SWITCHED = [_case("g0_16+16_sw", [16, 16], "g0", fill=True, switch=True), _case("g0_32_sw", [32], "g0", fill=True, switch=True),
            _case("g1_16+16_sw", [16, 16], "g1", fill=True, switch=True)]     # run with MJMPC_TREE_SPARSE set
OVERS = _overs(FILLS)
_have = {(c.chains, c.family, c.integrator, c.records) for c in FILLS + OVERS}
EDGES = [c for c in _edges() if (c.chains, c.family, c.integrator, c.records) not in _have]     # (some are an over-model already)
CASES = FILLS + OVERS + EDGES
NQ41 = _case("nq41_16+16", None, "g1", chains=["BBBBB" + "H", "HHHH" + "BBBB"])        # compile_tree refuses it
BY_NAME = {c.name: c for c in CASES + SWITCHED}
assert len(BY_NAME) == len(CASES) + len(SWITCHED)
