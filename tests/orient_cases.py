"""Shared by tests/test_orient_cpu.py and tests/test_orient_gpu.py: a numpy interpreter of the program of
``mjmpc_points_orient``, the oracle for an orientation error, the cases and the synthetic programs of the C entry.

The interpreter extends tests/com_cases.py's by import.  Every old row kind is that interpreter's: the program is handed to it
with each HOLD row restated as ``RESTORE -1`` (the world frame at rest, the sums left alone - what the header says a HOLD does to
the frame) and each ORIENTATION row as an ANGULAR closing row on a spare slot with the same ``keep`` (what a closing row does to
the frame and the sums).  The two new kinds are read here, from the row format of include/mjmpc_amd.h: a walk over the same rows
that carries only the frame's orientation as a quaternion - the sign of ``e`` matters to the log map, and a rotation matrix has
none -, the held quaternion ``h``, and the log map statement by statement.  Neither ``cost_terms.tree_program`` nor the kernel is
read.

The oracle gives no body orientation: the body's rotation matrix comes from four world points on it (its origin and the three unit
offsets) through ``motion_cases.Oracle``, i.e. ``RefArm`` with its site moved; the goal-to-body rotation matrix ``E = A' B`` is
formed from those, and its rotation vector by a route that shares nothing with the log map above: the angle from
``atan2(|vee|, (trace - 1) / 2)``, the axis from the antisymmetric part."""
import dataclasses
import functools

import numpy as np

import com_cases as cc
import motion_cases as mc
import points_cases as pc
import points_tile_cases as ptc

POINT, HINGE, SLIDE, BALL, FREE, DIFFERENCE, AXIS, VELOCITY, ANGULAR = 0, 1, 2, 3, 4, 5, 6, 7, 8
MASS, SAVE, RESTORE, COM, COM_VELOCITY, HOLD, ORIENTATION = 9, 10, 11, 12, 13, 14, 15
CLOSING = cc.CLOSING + (ORIENTATION,)
WRONG = ("conj", "offset", "hold", "flip")
BAND = 0.05                     # draws and rows with an angle above pi - BAND are left out: the sign of r flips at pi
SMALL = 2.0 ** -26
ORIENT_BOUND = 7.55e-14          # |entry - oracle|: ten times the worst measured on the CPU (tests/test_orient_cpu.py); the cap is 1e-9


# ---------------------------------------------------------------------------------------------------------- the interpreter
def qmul(a, b):
    """``a * b`` of quaternions ``[..., 4]`` (w, x, y, z)."""
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def conj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0], a.dtype)


def log_map(e, flip=True):
    """The header's log map over ``e`` ``[N][4]``: the half with ``w >= 0`` (``flip``), ``s = |(x, y, z)|``, ``k = 2 / w`` below
    ``s = 2^-26`` and ``2 atan2(s, w) / s`` from there, ``r = k (x, y, z)``."""
    e = np.where((e[:, :1] < 0) & flip, -e, e)
    w, xyz = e[:, 0], e[:, 1:]
    s = np.sqrt((xyz * xyz).sum(-1))
    small = s < SMALL
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(small, 2 / w, 2 * np.arctan2(s, w) / np.where(small, 1, s))
    return k[:, None] * xyz


def orientation_walk(program, n_rows, n_levels, q, wrong=None, dtype=float, guards=False):
    """-> {row index: (r [N][3], w [N])} for every ORIENTATION row: its rotation vector and the ``w`` of its ``e`` before the
    flip.  Only the frame's orientation is carried: a node turns it by its fixed quaternion and its joint (a free joint replaces
    it), SAVE / RESTORE / closing rows treat it as they treat the frame, HOLD puts it by in ``h`` and starts over."""
    program, q = np.asarray(program, dtype), np.asarray(q, dtype)
    N = len(q)

    def one():
        out = np.zeros((N, 4), dtype)
        out[:, 0] = 1
        return out

    def take(adr, n):
        if guards:
            return q[:, np.clip(np.arange(adr, adr + n), 0, q.shape[1] - 1)]
        return q[:, adr:adr + n]

    def unit(x):
        return x / np.sqrt((x * x).sum(-1, keepdims=True))

    Q, h, levels, out = one(), one(), [one() for _ in range(n_levels)], {}
    for k, row in enumerate(program[:n_rows]):
        kind = int(row[0])
        if kind == MASS:
            continue
        if kind in (SAVE, RESTORE):
            level = int(row[1])
            held = 0 <= level < n_levels
            if kind == SAVE:
                if held:
                    levels[level] = Q.copy()
            else:
                Q = levels[level].copy() if held else one()
            continue
        if kind == HOLD:
            h = Q.copy()
            if wrong != "hold":
                Q = one()
            continue
        if kind in CLOSING:
            if kind == ORIENTATION:
                o = np.broadcast_to(row[3:7], (N, 4))
                b = Q if wrong == "offset" else qmul(Q, o)
                g = np.broadcast_to(row[7:11], (N, 4))
                a = qmul(h, g) if row[11] != 0 else g.copy()
                e = qmul(a, conj(b)) if wrong == "conj" else qmul(conj(a), b)
                out[k] = (log_map(e, flip=wrong != "flip"), e[:, 0].copy())
            if row[1] == 0:
                Q = one()
            continue
        adr = int(row[1])
        if kind == FREE:
            Q = unit(take(adr + 3, 4))
            continue
        Q = qmul(Q, np.broadcast_to(row[6:10], (N, 4)))
        if kind == HINGE:
            half = (take(adr, 1)[:, 0] - row[2]) / 2
            Q = qmul(Q, np.concatenate([np.cos(half)[:, None], np.sin(half)[:, None] * row[10:13]], -1))
        elif kind == BALL:
            Q = qmul(Q, unit(take(adr, 4)))
        else:
            assert kind == SLIDE, kind
    return out


def interpret(program, n_rows, dofadr, n_out, n_levels, q, qd, wrong=None, dtype=float, guards=False, with_w=False):
    """The augmented entries ``[N][3 n_out + 3 n_diff]`` of ``(qpos [N][nq], qvel [N][nv])`` as ``mjmpc_points_orient`` is
    documented to form them.  ``wrong``: 'conj' (``a * conj(b)``: the conjugate on the wrong side), 'offset' (the offset ``o``
    ignored), 'hold' (a HOLD that does not reset the frame) or 'flip' (no flip for ``w < 0``).  ``guards`` as in com_cases.
    ``with_w``: also the smallest ``|w|`` of a row's orientation errors ``[N]`` (inf without an orientation)."""
    program, q, qd = np.asarray(program, dtype), np.asarray(q, dtype), np.asarray(qd, dtype)
    old = program[:n_rows].copy()
    for k in range(n_rows):
        kind = int(old[k, 0])
        if kind == HOLD:
            old[k] = 0
            old[k, 0], old[k, 1] = RESTORE, -1
        elif kind == ORIENTATION:
            keep = old[k, 1]
            old[k] = 0
            old[k, 0], old[k, 1], old[k, 2] = ANGULAR, keep, n_out          # (a spare slot, dropped below)
    slots = cc.interpret(old, n_rows, dofadr, n_out + 1, n_levels, q, qd, dtype=dtype, guards=guards)
    slots = slots.reshape(len(q), n_out + 1, 3)[:, :n_out].copy()
    least = np.full(len(q), np.inf)
    for k, (r, w) in orientation_walk(program, n_rows, n_levels, q, wrong, dtype, guards).items():
        slot = int(program[k, 2])
        if 0 <= slot < n_out:
            slots[:, slot] = r
            least = np.minimum(least, np.abs(w).astype(float))
        else:
            assert guards, slot
    blocks = [slots[:, i] for i in range(n_out)]
    for row in program[n_rows:]:
        assert int(row[0]) == DIFFERENCE
        a, b = int(row[1]), int(row[2])
        if guards:
            a, b = min(max(a, 0), n_out - 1), min(max(b, 0), n_out - 1)
        blocks.append(slots[:, a] - slots[:, b])
    out = np.concatenate(blocks, axis=1)
    return (out, least) if with_w else out


# ---------------------------------------------------------------------------------------------------------- the oracle
def quat2mat(quat):
    return pc._quat2mat(np.asarray(quat, float))


def rotation_vector(E):
    """``theta u`` of the rotation matrix ``E``: the angle from ``atan2(|vee|, (trace - 1) / 2)``, the axis from the
    antisymmetric part ``vee = sin(theta) u``."""
    vee = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    s = np.linalg.norm(vee)
    theta = np.arctan2(s, 0.5 * (np.trace(E) - 1.0))
    return theta * vee / s if s > 0 else np.zeros(3)


class Oracle:
    """Orientation errors from the C oracle's ``site``: a body's rotation matrix is ``[x_1 - x_0, x_2 - x_0, x_3 - x_0]`` with
    ``x_0`` the world position of its origin and ``x_i`` those of its unit offsets."""

    def __init__(self, raw):
        self.raw, self._sites = raw, mc.Oracle(raw, [], [])

    def frame(self, body, q):
        return np.stack([self._sites.axis(body, e, q) for e in np.eye(3)], axis=1)

    def error(self, spec, q):
        """``spec``: ``(body, quat, goal quaternion, other body or -1)`` with unit quaternions, as ``resolved`` gives them."""
        body, o, g, other = spec
        B = self.frame(body, q) @ quat2mat(o)
        A = (self.frame(other, q) if other >= 0 else np.eye(3)) @ quat2mat(g)
        return rotation_vector(A.T @ B)


# ---------------------------------------------------------------------------------------------------------- the cases
def case_names():
    return ["reacher", "tray", "hand24", "pen_hand", "gripper", "cheetah"] + ["random%d" % s for s in pc.RANDOM_SEEDS]


def raw_model(name):
    return cc.raw_model(name)


def _turn(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def nominal_quat(raw, body):
    """The body's world orientation at ``qpos0``: the bodies' own quaternions down its path, a ball joint's and a free joint's
    ``qpos0`` entries behind theirs (hinges stand at their reference there)."""
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE
    adr, at = {}, 0
    for i, b in enumerate(raw.bodies):
        if b.joint is not None:
            adr[i], at = at, at + b.joint.nq
    Q = np.array([1.0, 0.0, 0.0, 0.0])
    for i in pc.path(raw, body):
        b = raw.bodies[i]
        Q = qmul(Q, np.asarray(b.quat, float) / np.linalg.norm(b.quat))
        if b.joint is not None and b.joint.type in (JOINT_BALL, JOINT_FREE):
            j = adr[i] + (3 if b.joint.type == JOINT_FREE else 0)
            quat = np.asarray(raw.qpos0[j:j + 4], float)
            Q = qmul(Q, quat / np.linalg.norm(quat))
    return Q


def other_branch(raw, a):
    """The deepest body that is neither on ``a``'s path nor below ``a``; None on a chain."""
    on_path = set(pc.path(raw, a))
    rest = [b for b in range(len(raw.bodies)) if b not in on_path and a not in pc.path(raw, b)]
    return max(rest, key=lambda b: (pc._depth(raw, b), b)) if rest else None


def outputs_for(raw, com=False):
    """-> (outputs [(builder, name, kwargs)], differences) for any model, the slots out of program order: a point on the deepest
    body; the deepest body's orientation relative to an ancestor (the body at half depth of its path, or on a root body the
    world's first body below it); the deepest body's absolute orientation with a ``quat`` and a ``target`` - it shares the point's
    walk -; the point's velocity on that walk too; an orientation between two bodies on different branches (on a chain: of the
    ancestor relative to the deepest body, a descendant); an angular velocity of the deepest body; ``com``: a centre of mass and
    its velocity beside them.  The goals are set about the orientations at ``qpos0``, so that the errors there are 0.9, 0.7 and
    0.8 rad; the absolute goal is given with ``w < 0`` (the log map's flip)."""
    a = pc.deepest(raw)
    chain = pc.path(raw, a)
    anc = chain[len(chain) // 2] if len(chain) > 1 and chain[len(chain) // 2] != a else chain[0]
    if anc == a:                                    # (a root body: any other body stands in)
        anc = next(b for b in range(len(raw.bodies)) if b != a)
    side = other_branch(raw, a)
    pair = (a, side) if side is not None else (anc, a)
    name = [b.name for b in raw.bodies]
    nom = {b: nominal_quat(raw, b) for b in {a, anc} | set(pair)}
    offset = _turn((1.0, 2.0, -1.0), 0.6)
    target = -qmul(qmul(nom[a], offset), _turn((0.3, -1.0, 0.5), 0.9))
    rel_anc = qmul(qmul(conj(nom[anc]), nom[a]), _turn((1.0, 0.2, 0.4), 0.7))
    rel_side = qmul(qmul(conj(nom[pair[1]]), nom[pair[0]]), _turn((-0.5, 1.0, 0.3), 0.8))
    outputs = [("point", "tip", dict(body=name[a], pos=(0.03, -0.02, 0.05))),
               ("orientation", "to_ancestor", dict(body=name[a], relative_to=name[anc], relative_quat=tuple(3.0 * rel_anc))),
               ("orientation", "absolute", dict(body=name[a], quat=tuple(offset), target=tuple(0.5 * target))),
               ("velocity", "tip_vel", dict(point="tip")),
               ("orientation", "across", dict(body=name[pair[0]], relative_to=name[pair[1]], relative_quat=tuple(rel_side))),
               ("angular_velocity", "spin", dict(body=name[a]))]
    if com:
        outputs += [("com", "whole", dict()), ("com_velocity", "whole_vel", dict(com="whole"))]
    return outputs, [("tip_from_whole", "tip", "whole")] if com else []


def case(name):
    """-> (raw, engine kind, outputs, differences)."""
    raw = raw_model(name)
    return (raw, "arm" if name == "reacher" else "tree") + outputs_for(raw, com=name == "cheetah")


def add_outputs(terms, outputs, differences):
    return mc.add_outputs(terms, outputs, differences)


def resolved(raw, outputs):
    """-> {name: (body, o, g, other)} of the orientations, by the names alone, the quaternions normalised."""
    names = [b.name for b in raw.bodies]

    def unit(x):
        x = np.asarray((1.0, 0.0, 0.0, 0.0) if x is None else x, float)
        return x / np.linalg.norm(x)

    out = {}
    for builder, name, kw in outputs:
        if builder == "orientation":
            rel = kw.get("relative_to")
            out[name] = (names.index(kw["body"]), unit(kw.get("quat")), unit(kw.get("relative_quat") if rel else kw.get("target")),
                         names.index(rel) if rel else -1)
    return out


def host_engine(name):
    raw, kind, _, _ = case(name)
    return pc.host_engine(raw, kind)


def draw_states(raw, oracle, specs, n, seed, band=BAND):
    """``n`` random states at which every orientation error of ``specs`` has an angle of at most ``pi - band``:
    -> (qpos [n][nq], qvel [n][nv], draws made)."""
    rs = np.random.RandomState(seed)
    q, qd, drawn = [], [], 0
    while len(q) < n:
        drawn += 1
        x, y = cc.random_state(raw, rs)
        if all(np.linalg.norm(oracle.error(s, x)) <= np.pi - band for s in specs.values()):
            q.append(x)
            qd.append(y)
    return np.array(q), np.array(qd), drawn


# ---------------------------------------------------------------------------------------------------------- synthetic programs
SYNTH_KINDS = cc.SYNTH_KINDS
SYNTH_OUT = 14
PI_MINUS = np.pi - 1e-6


def _plain(*head):
    return np.array(list(head) + [0.0] * (16 - len(head)), float)


def orientation_row(keep, slot, o=(1.0, 0.0, 0.0, 0.0), g=(1.0, 0.0, 0.0, 0.0), rel=0):
    return _plain(ORIENTATION, keep, slot, *o, *g, rel)


def synthetic_program(rs, joints, n_levels, n_out):
    """A program in the header's row format, from a seed and no model.  It opens with closing rows on the world frame, where
    ``e`` is the row's ``o`` exactly: the identity, ``s`` just under and just over 2^-26, ``theta = pi - 1e-6``, ``w`` exactly 0
    with ``o = (0, 1, 0, 0)``, ``w < 0``, and ``rel = 1`` with no HOLD before it.  Then a relative walk (two paths and a HOLD),
    an absolute orientation sharing a walk with a point and its velocity, a centre-of-mass walk over ``n_levels`` saved frames
    with a HOLD in its middle (the sums are left alone), a second relative walk whose ``h`` is its own HOLD's, and closing rows
    with slots outside ``0 .. n_out - 1``.  -> (program, dofadr, n_rows, longest walk's nodes, {tag: slot})."""
    rows, dofadr, at = [], [], {}

    def node(j):
        rows.append(ptc.node_row(rs, joints[j]))
        dofadr.append(joints[j][2])

    def plain(row):
        rows.append(row)
        dofadr.append(0)

    def mass():
        c = ptc._offset(rs)
        plain(_plain(MASS, 0, 0, c[0], c[1], c[2], rs.uniform(0.05, 0.3)))

    under, over = 0.75 * SMALL, 1.5 * SMALL
    exact = [("identity", (1.0, 0.0, 0.0, 0.0)), ("under", (1.0, under, 0.0, 0.0)), ("over", (1.0, 0.0, -over, 0.0)),
             ("near pi", (np.cos(PI_MINUS / 2), 0.0, 0.0, np.sin(PI_MINUS / 2))), ("w zero", (0.0, 1.0, 0.0, 0.0)),
             ("w negative", (-0.8, 0.0, 0.6, 0.0))]
    for slot, (tag, o) in zip((9, 3, 11, 0, 6, 12), exact):
        plain(orientation_row(0, slot, o=o))
        at[tag] = slot
    g = ptc._unit(rs, 4)
    plain(orientation_row(0, 1, o=ptc._unit(rs, 4), g=g, rel=1))           # h is the identity here: a = g
    at["no hold"] = 1
    # (the second path starts at the world frame, not at the free joint, which would replace whatever frame a HOLD left)
    node(0), node(1), node(2), plain(_plain(HOLD)), node(1), node(3)
    plain(orientation_row(0, 5, o=ptc._unit(rs, 4), g=ptc._unit(rs, 4), rel=1))
    at["relative"] = 5
    node(0), node(1), node(2), node(3)
    c = ptc._offset(rs)
    plain(_plain(POINT, 1, 8, c[0], c[1], c[2]))
    plain(orientation_row(1, 2, o=ptc._unit(rs, 4), g=-np.abs(ptc._unit(rs, 4))))
    plain(_plain(VELOCITY, 0, 4, c[0], c[1], c[2]))
    at["absolute"] = 2
    node(0), mass()
    for level in range(n_levels):
        plain(_plain(SAVE, level)), node(1 + level), mass()
    plain(_plain(HOLD))                                 # the frame starts over, S and Sv go on
    node(1), mass()
    for level in reversed(range(n_levels)):
        plain(_plain(RESTORE, level)), node(6 + level), mass()
    plain(_plain(COM, 1, 7)), plain(_plain(COM_VELOCITY, 1, 10))
    plain(orientation_row(0, 13, o=ptc._unit(rs, 4), g=ptc._unit(rs, 4), rel=1))      # (on the walk's last frame, h its HOLD's)
    at["after com"] = 13
    node(1), node(2), plain(_plain(HOLD)), node(0), node(4), node(5)
    plain(orientation_row(0, n_out, o=ptc._unit(rs, 4), rel=1))            # slots outside: nothing is written
    node(0)
    plain(orientation_row(1, -1, o=ptc._unit(rs, 4)))
    plain(orientation_row(0, 1 << 20, o=ptc._unit(rs, 4)))
    n_rows = len(rows)
    rows.append(_plain(DIFFERENCE, 8, 7))
    return np.array(rows), np.array(dofadr, np.int32), n_rows, max(5, 2 + 2 * n_levels), at


@dataclasses.dataclass
class OrientCase(cc.TreeCase):
    slots: dict = None


def make_synthetic(name, seed, dtype, n_levels, d_obs, n):
    rs = np.random.RandomState(seed)
    joints, nq, nv = ptc.skeleton(rs, SYNTH_KINDS)
    program, dofadr, n_rows, nodes, at = synthetic_program(rs, joints, n_levels, SYNTH_OUT)
    d_obs = max(d_obs, nq + nv + ptc.PAD)
    tile = cc.tree_tile_rows(dtype, d_obs, SYNTH_OUT, n_levels)
    N = n(tile) if callable(n) else n
    obs = ptc.observations(rs, dtype, N, d_obs, joints, nq, nv, "motion")
    return OrientCase(name=name, entry="motion", dtype=dtype, tile=tile, N=N, d_obs=d_obs, nq=nq, nv=nv, program=program,
                      dofadr=dofadr, n_rows=n_rows, n_out=SYNTH_OUT, n_diff=1, nodes=nodes, obs=obs, tags=frozenset(),
                      n_levels=n_levels, slots=at)


@functools.lru_cache(maxsize=None)
def synthetic_cases():
    """Per dtype: ``n_levels`` 0 and 2, three workgroups with the last ragged; N = 1, rows and rows + 1 at two tile widths."""
    out, seed = [], 3000
    for dtype in ("f64", "f32"):
        for n_levels in (0, 2):
            seed += 1
            out.append(make_synthetic("orient-%s-l%d" % (dtype, n_levels), seed, dtype, n_levels, 0, ptc._ragged))
        for d_obs in (67, 301):
            for tag, n in (("N1", 1), ("Nrows", lambda r: r), ("Nrows+1", lambda r: r + 1)):
                seed += 1
                out.append(make_synthetic("orient-%s-d%d-%s" % (dtype, d_obs, tag), seed, dtype, 2, d_obs, n))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def synthetic_names():
    return [c.name for c in synthetic_cases()]


def synthetic_case(name):
    return {c.name: c for c in synthetic_cases()}[name]


def synthetic_interpret(c, dtype, wrong=None):
    obs = c.obs[:, :c.base].astype(dtype)
    return interpret(c.program, c.n_rows, c.dofadr, c.n_out, c.n_levels, obs[:, :c.nq], obs[:, c.nq:c.nq + c.nv], wrong=wrong,
                     dtype=dtype, guards=True, with_w=True)


@functools.lru_cache(maxsize=None)
def synthetic_reference(name):
    """-> (want80, interp64, bound, settled) with ``points_tile_cases``' criteria, made once and read only.  ``settled [N]``: the
    rows on which no orientation error stands within 1e-6 of ``w = 0``, where 80-bit and 64-bit arithmetic may take different
    halves; the rows that open the program on the world frame are exact and always settled (their ``w`` is the row's own)."""
    c = synthetic_case(name)
    (want80, _), (interp64, _) = synthetic_interpret(c, np.longdouble), synthetic_interpret(c, np.float64)
    assert want80.dtype == np.longdouble and np.all(np.isfinite(want80))
    obs = c.obs[:, :c.base].astype(np.float64)
    walk = orientation_walk(c.program, c.n_rows, c.n_levels, obs[:, :c.nq], guards=True)
    moving = [w for k, (r, w) in walk.items() if k >= len(EXACT_TAGS)]
    settled = np.all([np.abs(w) >= 1e-6 for w in moving], axis=0)
    b = ptc.bound(c, want80[settled], interp64[settled])
    for a in (want80, interp64, settled):
        a.setflags(write=False)
    return want80, interp64, b, settled


EXACT_TAGS = ("identity", "under", "over", "near pi", "w zero", "w negative")
