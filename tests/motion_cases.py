"""Shared by tests/test_motion_cpu.py and tests/test_motion_gpu.py: a numpy interpreter of the motion program,
written from the row format documented in include/mjmpc_amd.h (rotation matrices, a plain loop over the rows, every state of
a batch at once - not from
``cost_terms.motion_program`` and not from the kernel), the oracle for every kind of output (the C oracle's own kinematics:
positions and axes directly, velocities as a fourth-order central difference of its positions along ``qpos`` integrated by
``qvel`` with MuJoCo's rule, which ``integrate`` restates), and the cases: ``points_cases``' models and points with axes,
velocities, angular velocities and differences of each kind on them."""
import dataclasses

import numpy as np

import points_cases as pc

POINT, HINGE, SLIDE, BALL, FREE, DIFFERENCE, AXIS, VELOCITY, ANGULAR = 0, 1, 2, 3, 4, 5, 6, 7, 8
CLOSING = (POINT, AXIS, VELOCITY, ANGULAR)
WRONG = ("ball_world", "free_world", "hinge_lever", "slide_carry")

# the step and stencil of the oracle's velocities: (8 (f(h) - f(-h)) - (f(2h) - f(-2h))) / 12h
FD_H = 2.5e-4


# ---------------------------------------------------------------------------------------------------------- the interpreter
def _mats(quats, dtype=float):
    """Rotation matrices [N][3][3] of quaternions [N][4] (w, x, y, z), each used as q / |q|."""
    w, x, y, z = (np.asarray(quats, dtype) / np.linalg.norm(quats, axis=-1, keepdims=True)).T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _turns(u, angles, dtype=float):
    """Rotation matrices [N][3][3] by ``angles`` [N] about the unit axis ``u`` (Rodrigues)."""
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]], dtype)
    a = np.asarray(angles, dtype)[:, None, None]
    return np.eye(3, dtype=dtype) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def interpret(program, n_rows, dofadr, n_out, q, qd, wrong=None, dtype=float, slots_in_order=False, guards=False):
    """The augmented entries of ``(qpos, qvel)`` - one state, or ``[N][nq]`` and ``[N][nv]`` and then ``[N][.]`` -: three per
    output slot, then three per difference.  ``wrong``: one of the deliberately wrong variants the oracle comparison must catch -
    'ball_world' (a ball joint's rates read in the world frame), 'free_world' (a free joint's angular rates read in the world
    frame), 'hinge_lever' (the hinge's anchor taken to move with the origin and the origin with the anchor: its lever arm
    dropped) and 'slide_carry' (the slide's ``w x (a d)`` dropped); points_cases' 'anchor' (the hinge turns about the body
    origin) is taken too.  ``dtype``: the type every array and intermediate is held in (``np.longdouble``: 80-bit on x86).
    ``slots_in_order``: the program as ``mjmpc_points`` reads it - a closing row's slot is the count of closing rows before it,
    every closing row ends its walk, ``dofadr`` and ``qd`` may be None.  ``guards``: the kernel's documented ones
    (include/mjmpc_amd.h) - every qpos index is held inside ``0 .. nq - 1`` and every dof index inside ``0 .. nv - 1``, each on
    its own; a closing row whose slot is outside ``0 .. n_out - 1`` writes nothing; a difference's indices are held inside
    ``0 .. n_out - 1`` (a slot no row names reads as 0 either way)."""
    program, q = np.asarray(program, dtype), np.asarray(q, dtype)
    qd = np.zeros(q.shape[:-1] + (6,), dtype) if qd is None else np.asarray(qd, dtype)       # (6: a free joint's dofs)
    if q.ndim == 1:
        return interpret(program, n_rows, dofadr, n_out, q[None], qd[None], wrong, dtype, slots_in_order, guards)[0]
    N = len(q)
    if dofadr is None:
        dofadr = np.zeros(n_rows, np.int32)

    def rot(R, x):                                  # R x for every state; x [3] or [N][3]
        return np.einsum("nij,nj->ni", R, np.broadcast_to(x, (N, 3)))

    def rest():
        return (np.zeros((N, 3), dtype), np.broadcast_to(np.eye(3, dtype=dtype), (N, 3, 3)).copy(), np.zeros((N, 3), dtype),
                np.zeros((N, 3), dtype))

    def take(x, adr, n):                            # entries adr .. adr + n of every state
        if guards:
            return x[:, np.clip(np.arange(adr, adr + n), 0, x.shape[1] - 1)]
        return x[:, adr:adr + n].copy()

    out = np.zeros((N, n_out, 3), dtype)
    p, R, v, w = rest()
    closed = 0
    for k, row in enumerate(program[:n_rows]):
        kind = int(row[0])
        if kind in CLOSING:
            x = rot(R, row[3:6])
            slot = closed if slots_in_order else int(row[2])
            closed += 1
            if not guards or 0 <= slot < n_out:
                out[:, slot] = {POINT: p + x, AXIS: x, VELOCITY: v + np.cross(w, x), ANGULAR: w}[kind]
            if slots_in_order or row[1] == 0:
                p, R, v, w = rest()
            continue
        adr, dof = int(row[1]), int(dofadr[k])
        if kind == FREE:
            p, R = take(q, adr, 3), _mats(take(q, adr + 3, 4), dtype)
            v = take(qd, dof, 3)
            w = take(qd, dof + 3, 3) if wrong == "free_world" else rot(R, take(qd, dof + 3, 3))
            continue
        t = rot(R, row[3:6])
        p, v = p + t, v + np.cross(w, t)
        R = R @ _mats(row[None, 6:10], dtype)
        d = take(q, adr, 1)[:, 0] - row[2]
        if kind == SLIDE:
            a = rot(R, row[10:13])
            v = v + (0.0 if wrong == "slide_carry" else np.cross(w, a * d[:, None])) + a * take(qd, dof, 1)
            p = p + a * d[:, None]
            continue
        assert kind in (HINGE, BALL), kind
        lever = not (wrong == "hinge_lever" and kind == HINGE)
        local = np.zeros(3, dtype) if (wrong == "anchor" and kind == HINGE) else row[13:16]
        r = rot(R, local)
        anchor, v_anchor = p + r, v + (np.cross(w, r) if lever else 0.0)
        if kind == HINGE:
            R = R @ _turns(row[10:13], d, dtype)
            w = w + rot(R, row[10:13]) * take(qd, dof, 1)
        else:
            R = R @ _mats(take(q, adr, 4), dtype)
            w = w + (take(qd, dof, 3) if wrong == "ball_world" else rot(R, take(qd, dof, 3)))
        r = rot(R, local)
        p, v = anchor - r, v_anchor - (np.cross(w, r) if lever else 0.0)
    blocks = [out[:, i] for i in range(n_out)]
    for row in program[n_rows:]:
        assert int(row[0]) == DIFFERENCE
        a, b = int(row[1]), int(row[2])
        if guards:
            a, b = min(max(a, 0), n_out - 1), min(max(b, 0), n_out - 1)
        blocks.append(out[:, a] - out[:, b])
    return np.concatenate(blocks, axis=1)


# ---------------------------------------------------------------------------------------------------------- the oracle
def integrate(raw, q, qd, h):
    """``qpos`` after ``h`` at the constant ``qvel``, MuJoCo's rule (mj_integratePos): hinge and slide ``q + h qd``; a ball
    joint's quaternion ``q * exp(h omega / 2)`` with ``omega`` in the local frame; a free joint's position ``+ h v`` in the
    world and its quaternion as the ball's."""
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE

    def turned(quat, omega):
        n = np.linalg.norm(omega)
        if n < 1e-300:
            return quat.copy()
        a = 0.5 * n * h
        r = np.concatenate([[np.cos(a)], np.sin(a) * omega / n])
        w0, x0, y0, z0 = quat
        w1, x1, y1, z1 = r
        t = np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                      w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1])
        return t / np.linalg.norm(t)

    out, qa, da = np.array(q, float), 0, 0
    for b in raw.bodies:
        jt = b.joint
        if jt is None:
            continue
        if jt.type == JOINT_FREE:
            out[qa:qa + 3] = q[qa:qa + 3] + h * qd[da:da + 3]
            out[qa + 3:qa + 7] = turned(q[qa + 3:qa + 7], qd[da + 3:da + 6])
        elif jt.type == JOINT_BALL:
            out[qa:qa + 4] = turned(q[qa:qa + 4], qd[da:da + 3])
        else:
            out[qa] = q[qa] + h * qd[da]
        qa, da = qa + jt.nq, da + jt.ndof
    return out


class Oracle:
    """Every kind of output from the C oracle's ``site``: ``RefArm`` of the model with its tracked site moved about."""

    def __init__(self, raw, outputs, differences):
        """``outputs``: ``[(kind, body index, vector)]``; ``differences``: ``[(a, b)]``."""
        self.raw, self.outputs, self.differences, self._refs = raw, outputs, differences, {}

    def _site(self, body, pos, q):
        from oracle.physics_ref import RefArm
        key = (int(body), tuple(float(x) for x in pos))
        if key not in self._refs:
            self._refs[key] = RefArm(dataclasses.replace(self.raw, site_body=key[0], site_pos=key[1]).to_flat())
        return self._refs[key].site(np.asarray(q, float))

    def _rate(self, f, q, qd):
        """d/dt f(qpos(t)) at 0: the fourth-order central difference along ``integrate``."""
        at = {s: f(integrate(self.raw, q, qd, s * FD_H)) for s in (-2, -1, 1, 2)}
        return (8.0 * (at[1] - at[-1]) - (at[2] - at[-2])) / (12.0 * FD_H)

    def position(self, body, pos, q):
        return self._site(body, pos, q)

    def axis(self, body, a, q):
        return self._site(body, a, q) - self._site(body, (0.0, 0.0, 0.0), q)

    def velocity(self, body, pos, q, qd):
        return self._rate(lambda x: self._site(body, pos, x), q, qd)

    def angular(self, body, q, qd):
        """``w`` from ``d/dt R = [w]x R``, ``R``'s columns the body's three axes."""
        def frame(x):
            return np.stack([self.axis(body, e, x) for e in np.eye(3)], axis=1)
        S = self._rate(frame, q, qd) @ frame(q).T
        return 0.5 * np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])

    def __call__(self, q, qd=None, kinds=CLOSING):
        """Three entries per output and per difference; those whose kind is not in ``kinds`` are NaN (without ``qd`` only
        positions and axes are formed)."""
        q = np.asarray(q, float)
        if qd is None:
            kinds = tuple(k for k in kinds if k in (POINT, AXIS))
        out = []
        for kind, body, vec in self.outputs:
            if kind not in kinds:
                out.append(np.full(3, np.nan))
            elif kind == POINT:
                out.append(self.position(body, vec, q))
            elif kind == AXIS:
                out.append(self.axis(body, vec, q))
            elif kind == VELOCITY:
                out.append(self.velocity(body, vec, q, qd))
            else:
                out.append(self.angular(body, q, qd))
        return np.concatenate(out + [out[a] - out[b] for a, b in self.differences])


# ---------------------------------------------------------------------------------------------------------- the cases
def case_names():
    return pc.case_names()


def case(name):
    """-> (raw, engine kind, outputs, differences): ``points_cases``' points, then - so that the slots are out of program order,
    every body carrying several outputs on one walk - a velocity of every point, an axis and an angular velocity on the first
    two points' bodies; ``points_cases``' differences, then one of two velocities, of two axes and of two angular velocities.
    ``outputs``: ``[(builder, name, kwargs)]``; ``differences``: ``[(name, a, b)]``."""
    raw, kind, points, differences = pc.case(name)
    bodies = [raw.bodies[b].name for b, _ in pc.resolved(raw, points, differences)[0]]
    outputs = [("point", n, kw) for n, kw in points]
    outputs += [("velocity", n + "_vel", dict(point=n)) for n, _ in points]
    outputs += [("axis", "up0", dict(body=bodies[0], axis=(0.2, -0.3, 0.9))), ("angular_velocity", "spin0", dict(body=bodies[0])),
                ("axis", "up1", dict(body=bodies[1], axis=(2.0, 0.0, 0.0))), ("angular_velocity", "spin1", dict(body=bodies[1]))]
    differences = list(differences) + [("slip", points[0][0] + "_vel", points[1][0] + "_vel"), ("tilt", "up0", "up1"),
                                       ("twist", "spin0", "spin1")]
    return raw, kind, outputs, differences


def add_outputs(terms, outputs, differences):
    for builder, name, kw in outputs:
        getattr(terms, builder)(name, **kw)
    for name, a, b in differences:
        terms.difference(name, a, b)
    return terms


def resolved(raw, outputs, differences):
    """-> ([(kind, body index, vector in the body frame)], [(a, b)]) by the names alone; axes are normalised."""
    names = [b.name for b in raw.bodies]
    out, at = [], {}
    for builder, name, kw in outputs:
        if builder == "point":
            body, vec = raw.sites[kw["site"]] if "site" in kw else (names.index(kw["body"]), kw.get("pos", (0.0, 0.0, 0.0)))
            out.append((POINT, int(body), np.asarray(vec, float)))
        elif builder == "velocity":
            _, body, vec = out[at[kw["point"]]]
            out.append((VELOCITY, body, vec))
        elif builder == "axis":
            a = np.asarray(kw["axis"], float)
            out.append((AXIS, names.index(kw["body"]), a / np.linalg.norm(a)))
        else:
            out.append((ANGULAR, names.index(kw["body"]), np.zeros(3)))
        at[name] = len(out) - 1
    return out, [(at[a], at[b]) for _, a, b in differences]


def kinds_of(outputs, differences):
    """The kind of every three-entry block, outputs then differences (a difference has its operands' kind)."""
    kind = {"point": POINT, "axis": AXIS, "velocity": VELOCITY, "angular_velocity": ANGULAR}
    by_name = {name: kind[builder] for builder, name, _ in outputs}
    return [by_name[n] for _, n, _ in outputs] + [by_name[a] for _, a, _ in differences]


def random_qvel(raw, rs):
    return 2.0 * rs.standard_normal(raw.nv)
