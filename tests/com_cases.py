"""Shared by tests/test_com_cpu.py and tests/test_com_gpu.py: a numpy interpreter of the tree program, written
from the row format documented in include/mjmpc_amd.h (rotation matrices, a plain loop over the rows, every state of a batch at
once - not from ``cost_terms.tree_program`` and not from the kernel), the oracle for a centre of mass (the C oracle's own
kinematics with the tracked site moved to every body's inertial position, weighted by the C oracle's own masses; its velocity as
``motion_cases``' fourth-order central difference of that), and the cases: models, their centres of mass, an ordinary point and
its velocity, and differences."""
import dataclasses
import functools

import numpy as np

import motion_cases as mc
import points_cases as pc
import points_tile_cases as ptc

POINT, HINGE, SLIDE, BALL, FREE, DIFFERENCE, AXIS, VELOCITY, ANGULAR = 0, 1, 2, 3, 4, 5, 6, 7, 8
MASS, SAVE, RESTORE, COM, COM_VELOCITY = 9, 10, 11, 12, 13
CLOSING = (POINT, AXIS, VELOCITY, ANGULAR, COM, COM_VELOCITY)
WRONG = ("restore", "ipos", "lever", "shares")
MAX_LEVELS = 4


# ---------------------------------------------------------------------------------------------------------- the interpreter
def interpret(program, n_rows, dofadr, n_out, n_levels, q, qd, wrong=None, dtype=float, guards=False):
    """The augmented entries of ``(qpos, qvel)`` - one state, or ``[N][nq]`` and ``[N][nv]`` and then ``[N][.]`` -: three per
    output slot, then three per difference, as ``mjmpc_points_tree`` is documented to form them.  ``wrong``: one of the
    deliberately wrong variants the oracle comparison must catch - 'restore' (a RESTORE does nothing), 'ipos' (a MASS row's centre
    ignored: the group's mass at its frame's origin), 'lever' (the ``w x (R c)`` term of a MASS row dropped) and 'shares' (every
    share taken as 1: the sum not normalised).  ``dtype``: the type every array and intermediate is held in.  ``guards``: the
    kernel's documented ones - qpos and dof indices held inside, a closing row with a slot outside ``0 .. n_out - 1`` writes
    nothing, a difference's indices are held inside, a SAVE with a level outside ``0 .. n_levels - 1`` writes nothing and a
    RESTORE with one gives the world frame at rest; a level never saved holds the world frame at rest either way."""
    program, q, qd = np.asarray(program, dtype), np.asarray(q, dtype), np.asarray(qd, dtype)
    if q.ndim == 1:
        return interpret(program, n_rows, dofadr, n_out, n_levels, q[None], qd[None], wrong, dtype, guards)[0]
    N = len(q)

    def rot(R, x):
        return np.einsum("nij,nj->ni", R, np.broadcast_to(x, (N, 3)))

    def rest():
        return (np.zeros((N, 3), dtype), np.broadcast_to(np.eye(3, dtype=dtype), (N, 3, 3)).copy(), np.zeros((N, 3), dtype),
                np.zeros((N, 3), dtype))

    def take(x, adr, n):
        if guards:
            return x[:, np.clip(np.arange(adr, adr + n), 0, x.shape[1] - 1)]
        return x[:, adr:adr + n].copy()

    out = np.zeros((N, n_out, 3), dtype)
    p, R, v, w = rest()
    S, Sv = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
    levels = [rest() for _ in range(n_levels)]
    for k, row in enumerate(program[:n_rows]):
        kind = int(row[0])
        if kind == MASS:
            c = np.zeros(3, dtype) if wrong == "ipos" else row[3:6]
            share = 1.0 if wrong == "shares" else row[6]
            x = rot(R, c)
            S = S + share * (p + x)
            Sv = Sv + share * (v + (0.0 if wrong == "lever" else np.cross(w, x)))
            continue
        if kind in (SAVE, RESTORE):
            level = int(row[1])
            held = 0 <= level < n_levels
            assert guards or held or (kind == RESTORE and level == -1), (kind, level)
            if kind == SAVE:
                if held:
                    levels[level] = (p.copy(), R.copy(), v.copy(), w.copy())
            elif wrong != "restore":
                p, R, v, w = [x.copy() for x in levels[level]] if held else rest()
            continue
        if kind in CLOSING:
            slot = int(row[2])
            if not guards or 0 <= slot < n_out:
                if kind == COM:
                    out[:, slot] = S
                elif kind == COM_VELOCITY:
                    out[:, slot] = Sv
                else:
                    x = rot(R, row[3:6])
                    out[:, slot] = {POINT: p + x, AXIS: x, VELOCITY: v + np.cross(w, x), ANGULAR: w}[kind]
            if row[1] == 0:
                p, R, v, w = rest()
                S, Sv = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
            continue
        adr, dof = int(row[1]), int(dofadr[k])
        if kind == FREE:
            p, R = take(q, adr, 3), mc._mats(take(q, adr + 3, 4), dtype)
            v, w = take(qd, dof, 3), rot(R, take(qd, dof + 3, 3))
            continue
        t = rot(R, row[3:6])
        p, v = p + t, v + np.cross(w, t)
        R = R @ mc._mats(row[None, 6:10], dtype)
        d = take(q, adr, 1)[:, 0] - row[2]
        if kind == SLIDE:
            a = rot(R, row[10:13])
            v = v + np.cross(w, a * d[:, None]) + a * take(qd, dof, 1)
            p = p + a * d[:, None]
            continue
        assert kind in (HINGE, BALL), kind
        r = rot(R, row[13:16])
        anchor, v_anchor = p + r, v + np.cross(w, r)
        if kind == HINGE:
            R = R @ mc._turns(row[10:13], d, dtype)
            w = w + rot(R, row[10:13]) * take(qd, dof, 1)
        else:
            R = R @ mc._mats(take(q, adr, 4), dtype)
            w = w + rot(R, take(qd, dof, 3))
        r = rot(R, row[13:16])
        p, v = anchor - r, v_anchor - np.cross(w, r)
    blocks = [out[:, i] for i in range(n_out)]
    for row in program[n_rows:]:
        assert int(row[0]) == DIFFERENCE
        a, b = int(row[1]), int(row[2])
        if guards:
            a, b = min(max(a, 0), n_out - 1), min(max(b, 0), n_out - 1)
        blocks.append(out[:, a] - out[:, b])
    return np.concatenate(blocks, axis=1)


# ---------------------------------------------------------------------------------------------------------- the oracle
def subtree(raw, body):
    """The bodies of ``body``'s subtree (``None``: all)."""
    inside = []
    for i, b in enumerate(raw.bodies):
        if body is None or i == body or b.parent in inside:
            inside.append(i)
    return inside


class Oracle:
    """Centres of mass from the C oracle: ``sum m_b x_b / sum m_b`` with ``x_b`` ``RefArm.site`` moved to body ``b``'s inertial
    position and ``m_b``, ``ipos`` from ``RefArm.inertial()`` (entry 0 there is the world body)."""

    def __init__(self, raw):
        from oracle.physics_ref import RefArm
        self.raw = raw
        mass, ipos, _ = RefArm(raw.to_flat()).inertial()
        self.mass, self.ipos = mass[1:].copy(), ipos[1:].copy()
        assert len(self.mass) == len(raw.bodies)
        self._refs = {}

    def _site(self, b, q):
        from oracle.physics_ref import RefArm
        if b not in self._refs:
            self._refs[b] = RefArm(dataclasses.replace(self.raw, site_body=int(b),
                                                       site_pos=tuple(float(x) for x in self.ipos[b])).to_flat())
        return self._refs[b].site(np.asarray(q, float))

    def com(self, body, q):
        bodies = [b for b in subtree(self.raw, body) if self.mass[b] > 0.0]
        return sum(self.mass[b] * self._site(b, q) for b in bodies) / sum(self.mass[b] for b in bodies)

    def com_velocity(self, body, q, qd):
        """The fourth-order central difference of ``com`` along ``qpos`` integrated by ``qvel`` (``motion_cases``' scheme)."""
        at = {s: self.com(body, mc.integrate(self.raw, q, qd, s * mc.FD_H)) for s in (-2, -1, 1, 2)}
        return (8.0 * (at[1] - at[-1]) - (at[2] - at[-2])) / (12.0 * mc.FD_H)


# ---------------------------------------------------------------------------------------------------------- the cases
def comb(n, name="comb"):
    """A planar tree built by hand: a spine of ``n + 1`` hinged capsules on a sliding root, every spine body but the last with
    its next spine body as its FIRST child and a hinged leaf as its second - so the walk has saved ``n`` frames when it reaches
    the spine's end (nesting ``n``) - and a massless welded marker at the tip."""
    from mjmpc_amd.models.raw import (GEOM_CAPSULE, JOINT_HINGE, JOINT_SLIDE, RawActuator, RawBody, RawGeom, RawJoint, RawModel)

    def geom(k, length, gname):
        return RawGeom(GEOM_CAPSULE, 0.03 + 0.002 * k, (length, 0.0, 0.0), (0.0, 0.0, 0.0), density=1000.0, condim=3, name=gname)

    bodies = [RawBody("base", -1, (0.0, 0.0, 0.5), joint=RawJoint((1, 0, 0), name="base", type=JOINT_SLIDE,
                                                                   range=(-1.0, 1.0), limited=False), geoms=[geom(0, 0.1, "g_base")])]
    for i in range(n + 1):          # depth-first, as the model compiler wants the bodies: the spine, then the leaves from the tip back
        bodies.append(RawBody("s%d" % i, i, (0.1 if i == 0 else 0.2, 0.0, 0.0),
                              joint=RawJoint((0, 1, 0), range=(-1.5, 1.5), limited=True, name="js%d" % i, type=JOINT_HINGE),
                              geoms=[geom(i, 0.2, "g_s%d" % i)]))
    spine = len(bodies) - 1
    bodies.append(RawBody("marker", spine, (0.2, 0.0, 0.0)))
    for i in range(n - 1, -1, -1):  # the leaf of spine body i, listed behind that body's spine child and all below it
        bodies.append(RawBody("l%d" % i, 1 + i, (0.1, 0.0, 0.02), quat=(0.9238795325112867, 0.0, 0.3826834323650898, 0.0),
                              joint=RawJoint((0, 0, 1), range=(-1.5, 1.5), limited=True, name="jl%d" % i, type=JOINT_HINGE,
                                             pos=(0.01, 0.0, 0.0)),
                              geoms=[geom(i, 0.12, "g_l%d" % i)]))
    actuators = [RawActuator(b.joint.name, 5.0, (-1.0, 1.0)) for b in bodies[1:] if b.joint is not None]
    return RawModel(bodies=bodies, actuators=actuators, site_body=spine, site_pos=(0.2, 0.0, 0.0), target_pos=(0.3, 0.0, 0.6),
                    plane=None, timestep=0.005, frame_skip=2, gravity=(0.0, 0.0, -9.81))


def case_names():
    return ["cheetah", "swimmer", "hand24", "pen_hand", "gripper", "tray", "reacher", "comb2"] + \
        ["random%d" % s for s in pc.RANDOM_SEEDS]


_RAW = {}


def raw_model(name):
    if name not in _RAW:
        if name == "cheetah":           # (the observation opens with all of qpos: a forward task's obs_skip is refused)
            from mjmpc_amd.models.half_cheetah import half_cheetah_raw
            _RAW[name] = dataclasses.replace(half_cheetah_raw(), obs_skip=0)
        elif name == "swimmer":
            from mjmpc_amd.models.swimmer import swimmer_raw
            _RAW[name] = dataclasses.replace(swimmer_raw(), obs_skip=0)
        elif name == "hand24":
            from mjmpc_amd.models.hand24 import hand24_raw
            _RAW[name] = hand24_raw()
        elif name == "pen_hand":
            from mjmpc_amd.models.pen_hand import pen_hand_raw
            _RAW[name] = pen_hand_raw()
        elif name.startswith("comb"):
            _RAW[name] = comb(int(name[4:]), name)
        else:
            _RAW[name] = pc.case(name)[0]
    return _RAW[name]


def part_body(raw):
    """The root of a proper subtree below a branch point: among the bodies that are not a root and whose parent has several
    children, the one with the most descendants (the last of them); on a chain, its middle body."""
    kids = [sum(1 for b in raw.bodies if b.parent == i) for i in range(len(raw.bodies))]
    below = [i for i, b in enumerate(raw.bodies) if b.parent >= 0 and kids[b.parent] > 1]
    if not below:
        return len(raw.bodies) // 2
    return max(below, key=lambda i: (len(subtree(raw, i)), i))


def outputs_for(raw):
    """-> (outputs [(builder, name, kwargs)], differences [(name, a, b)]) for any model: a whole-model centre of mass, one of a
    proper subtree, their velocities, an ordinary point and its velocity among them (so that the slots are out of program order), a
    difference centre of mass - point and one of two centre-of-mass velocities."""
    tip = raw.bodies[pc.deepest(raw)].name
    outputs = [("com", "whole", dict()), ("point", "tip", dict(body=tip, pos=(0.03, -0.02, 0.05))),
               ("com", "part", dict(body=raw.bodies[part_body(raw)].name)), ("com_velocity", "whole_vel", dict(com="whole")),
               ("velocity", "tip_vel", dict(point="tip")), ("com_velocity", "part_vel", dict(com="part"))]
    differences = [("whole_from_tip", "whole", "tip"), ("part_from_whole_vel", "part_vel", "whole_vel")]
    return outputs, differences


def case(name):
    """-> (raw, engine kind, outputs, differences) of a case: ``outputs_for`` its model."""
    raw = raw_model(name)
    return (raw, "arm" if name == "reacher" else "tree") + outputs_for(raw)


def add_outputs(terms, outputs, differences):
    return mc.add_outputs(terms, outputs, differences)


def host_engine(name):
    raw, kind, _, _ = case(name)
    return pc.host_engine(raw, kind)


def random_state(raw, rs):
    return pc.random_qpos(raw, rs), mc.random_qvel(raw, rs)


# ---------------------------------------------------------------------------------------------------------- synthetic programs
@dataclasses.dataclass
class TreeCase(ptc.Case):
    n_levels: int = 0


def tree_lds_bytes(dtype, d_obs, n_out, n_levels, rows):
    """The launcher's rule (include/mjmpc_amd.h): the tile, a row's parked outputs and 104 n_levels bytes of saved frames."""
    return ptc.lds_bytes(dtype, d_obs, n_out, rows) + rows * 104 * n_levels


def tree_tile_rows(dtype, d_obs, n_out, n_levels):
    rows = 256
    while tree_lds_bytes(dtype, d_obs, n_out, n_levels, rows) > ptc.LDS_BYTES:
        rows >>= 1
    return rows


SYNTH_KINDS = (ptc.FREE, ptc.HINGE, ptc.BALL, ptc.SLIDE, ptc.HINGE, ptc.HINGE, ptc.BALL, ptc.HINGE, ptc.SLIDE, ptc.HINGE, ptc.HINGE)
SYNTH_OUT = 6


def synthetic_program(rs, joints, n_levels, wild):
    """Two centre-of-mass walks and a point's in the header's row format, from a seed and no model.  The first saves ``n_levels``
    frames on its way down a chain and restores them on its way back, a MASS row at every node, one of them with share 0; the
    second starts over (its sums must not hold the first's), restores to the world frame once and - ``wild`` - names levels
    outside ``0 .. n_levels - 1`` on SAVEs and RESTOREs;
    the third is a point and its velocity.  Slots are out of program order.  -> (program, dofadr, n_rows, longest walk's nodes)."""
    rows, dofadr = [], []

    def node(j):
        rows.append(ptc.node_row(rs, joints[j]))
        dofadr.append(joints[j][2])

    def plain(*head):
        rows.append(np.array(list(head) + [0.0] * (16 - len(head)), float))
        dofadr.append(0)

    def mass(share=None):
        c = ptc._offset(rs)
        plain(MASS, 0, 0, c[0], c[1], c[2], rs.uniform(0.05, 0.3) if share is None else share)

    node(0), mass()
    for level in range(n_levels):
        plain(SAVE, level), node(1 + level), mass()
    for level in reversed(range(n_levels)):
        plain(RESTORE, level), node(6 + level), mass(0.0 if level == 0 else None)
    plain(COM, 1, 2), plain(COM_VELOCITY, 0, 0)
    longest = 1 + 2 * n_levels
    node(1), mass()                                 # (a walk that does not begin at the free joint: from the world frame)
    if wild:
        plain(SAVE, n_levels), plain(SAVE, -1), plain(SAVE, 1 << 20)        # written nowhere
        plain(RESTORE, n_levels + 5)                                        # outside: the world frame at rest
    node(2), mass()
    plain(RESTORE, -1), node(3), mass()
    if wild:
        plain(RESTORE, -7), node(4), mass()
    plain(COM, 1, 1), plain(COM_VELOCITY, 0, 3)
    node(0), node(1), node(2)
    c = ptc._offset(rs)
    plain(POINT, 1, 5, c[0], c[1], c[2]), plain(VELOCITY, 0, 4, c[0], c[1], c[2])
    n_rows = len(rows)
    rows.append(np.array([DIFFERENCE, 2, 5] + [0.0] * 13))
    rows.append(np.array([DIFFERENCE, 0, 3] + [0.0] * 13))
    return np.array(rows), np.array(dofadr, np.int32), n_rows, max(longest, 4)


def make_synthetic(name, seed, dtype, n_levels, d_obs, n, wild=False, never_saved=False):
    rs = np.random.RandomState(seed)
    joints, nq, nv = ptc.skeleton(rs, SYNTH_KINDS)
    program, dofadr, n_rows, nodes = synthetic_program(rs, joints, n_levels, wild)
    if never_saved:                                 # the first walk's deepest SAVE is dropped: its RESTORE reads a level never saved
        k = [i for i in range(n_rows) if program[i, 0] == SAVE and program[i, 1] == n_levels - 1][0]
        program, dofadr, n_rows = np.delete(program, k, axis=0), np.delete(dofadr, k), n_rows - 1
    d_obs = max(d_obs, nq + nv + ptc.PAD)
    tile = tree_tile_rows(dtype, d_obs, SYNTH_OUT, n_levels)
    N = n(tile) if callable(n) else n
    obs = ptc.observations(rs, dtype, N, d_obs, joints, nq, nv, "motion")
    return TreeCase(name=name, entry="motion", dtype=dtype, tile=tile, N=N, d_obs=d_obs, nq=nq, nv=nv, program=program,
                    dofadr=dofadr, n_rows=n_rows, n_out=SYNTH_OUT, n_diff=2, nodes=nodes, obs=obs,
                    tags=frozenset(t for t, on in (("wild", wild), ("never saved", never_saved)) if on), n_levels=n_levels)


@functools.lru_cache(maxsize=None)
def synthetic_cases():
    """Per dtype: ``n_levels`` 0 .. 4 at the narrowest observation and at two wider ones (the tiles the sizing rule then gives),
    three workgroups with the last ragged; N = 1, rows and rows + 1; the guards; a RESTORE of a level never saved."""
    out, seed = [], 2900
    for dtype in ("f64", "f32"):
        for n_levels in range(MAX_LEVELS + 1):
            for d_obs in (0, 66, 301):
                seed += 1
                out.append(make_synthetic("tree-%s-l%d-d%d" % (dtype, n_levels, d_obs), seed, dtype, n_levels, d_obs, ptc._ragged))
        for tag, n in (("N1", 1), ("Nrows", lambda r: r), ("Nrows+1", lambda r: r + 1)):
            seed += 1
            out.append(make_synthetic("tree-%s-%s" % (dtype, tag), seed, dtype, 2, 67, n))
        for n_levels in (0, 1, 3):
            seed += 1
            out.append(make_synthetic("tree-%s-wild-l%d" % (dtype, n_levels), seed, dtype, n_levels, 0, ptc._ragged, wild=True))
        seed += 1
        out.append(make_synthetic("tree-%s-never-saved" % dtype, seed, dtype, 3, 0, ptc._ragged, never_saved=True))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def synthetic_names():
    return [c.name for c in synthetic_cases()]


def synthetic_case(name):
    return {c.name: c for c in synthetic_cases()}[name]


def synthetic_interpret(c, dtype, wrong=None):
    obs = c.obs[:, :c.base].astype(dtype)
    return interpret(c.program, c.n_rows, c.dofadr, c.n_out, c.n_levels, obs[:, :c.nq], obs[:, c.nq:c.nq + c.nv], wrong=wrong,
                     dtype=dtype, guards=True)


@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    """-> (want80, interp64, bound) with ``points_tile_cases``' criteria: made once, read only."""
    c = synthetic_case(name)
    want80, interp64 = synthetic_interpret(c, np.longdouble), synthetic_interpret(c, np.float64)
    assert want80.dtype == np.longdouble and np.all(np.isfinite(want80))
    b = ptc.bound(c, want80, interp64)
    for a in (want80, interp64):
        a.setflags(write=False)
    return want80, interp64, b

