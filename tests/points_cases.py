"""Shared by tests/test_points_cpu.py and tests/test_points_gpu.py: a numpy interpreter of the points program,
written from the row format documented in include/mjmpc_amd.h (rotation matrices and plain loops - not from
``cost_terms.points_program``, which builds the table with quaternions, and not from the kernel), the oracle for a point
(the C oracle's own kinematics with the tracked site moved to the point), and the cases: models, their points and differences,
and random states."""
import dataclasses

import numpy as np

POINT, HINGE, SLIDE, BALL, FREE, DIFFERENCE = 0, 1, 2, 3, 4, 5


# ---------------------------------------------------------------------------------------------------------- the interpreter
def _quat2mat(q, dtype=float):
    w, x, y, z = np.asarray(q, dtype) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype)


def _axis_angle(u, a, dtype=float):
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]], dtype)
    return np.eye(3, dtype=dtype) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def interpret(program, n_rows, q, wrong=None, dtype=float, guards=False, n_points=None):
    """The augmented entries of one qpos ``q``: x, y, z of every point, then of every difference.  ``wrong``: 'anchor' (the
    hinge turns about the body origin, the anchor dropped) or 'qpos0' (qpos0 not subtracted) - the two deliberately wrong
    builds the oracle comparison must catch.  ``dtype``: the type every array and intermediate is held in (``np.longdouble``:
    80-bit on x86).  ``guards``: the kernel's documented ones (include/mjmpc_amd.h) - every qpos index is held inside
    ``0 .. nq - 1`` on its own, a point behind the ``n_points``-th is written nowhere and a difference's indices are held inside
    ``0 .. n_points - 1``."""
    program = np.asarray(program, dtype)
    q = np.asarray(q, dtype)

    def qpos(adr, n):
        return q[np.clip(np.arange(adr, adr + n), 0, len(q) - 1)] if guards else q[adr:adr + n]

    points, p, R = [], np.zeros(3, dtype), np.eye(3, dtype=dtype)
    for row in program[:n_rows]:
        kind, adr = int(row[0]), int(row[1])
        if kind == POINT:
            points.append(p + R @ row[3:6])
            p, R = np.zeros(3, dtype), np.eye(3, dtype=dtype)
            continue
        if kind == FREE:
            p, R = qpos(adr, 3).copy(), _quat2mat(qpos(adr + 3, 4), dtype)
            continue
        p = p + R @ row[3:6]
        R = R @ _quat2mat(row[6:10], dtype)
        d = qpos(adr, 1)[0] - (0.0 if wrong == "qpos0" else row[2])
        if kind == SLIDE:
            p = p + (R @ row[10:13]) * d
            continue
        assert kind in (HINGE, BALL), kind
        local = np.zeros(3, dtype) if (wrong == "anchor" and kind == HINGE) else row[13:16]
        anchor = p + R @ local
        R = R @ (_axis_angle(row[10:13], d, dtype) if kind == HINGE else _quat2mat(qpos(adr, 4), dtype))
        p = anchor - R @ local
    if guards:
        points = points[:len(points) if n_points is None else n_points]
    out = list(points)
    for row in program[n_rows:]:
        assert int(row[0]) == DIFFERENCE
        a, b = int(row[1]), int(row[2])
        if guards:
            a, b = min(max(a, 0), len(points) - 1), min(max(b, 0), len(points) - 1)
        out.append(points[a] - points[b])
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------- the oracle
class Oracle:
    """World positions from the C oracle: ``RefArm`` of the model with its tracked site moved to the point."""

    def __init__(self, raw, points, differences):
        from oracle.physics_ref import RefArm
        self.refs = [RefArm(dataclasses.replace(raw, site_body=int(b), site_pos=tuple(float(x) for x in p)).to_flat())
                     for b, p in points]
        self.differences = differences

    def __call__(self, q):
        pts = [r.site(np.asarray(q, float)) for r in self.refs]
        return np.concatenate(pts + [pts[a] - pts[b] for a, b in self.differences])


# ---------------------------------------------------------------------------------------------------------- the cases
def _depth(raw, b):
    d = 0
    while raw.bodies[b].parent >= 0:
        b, d = raw.bodies[b].parent, d + 1
    return d


def path(raw, b):
    """The bodies from the root to ``b``."""
    out = []
    while b >= 0:
        out.append(b)
        b = raw.bodies[b].parent
    return out[::-1]


def deepest(raw):
    return max(range(len(raw.bodies)), key=lambda b: (_depth(raw, b), b))


def _generic(raw):
    """A point on the deepest body, one on its ancestor at half depth (shared ancestors) and, where the first body of the
    model moves, one on it (a root body); the differences deep - mid and deep - root."""
    a = deepest(raw)
    chain = path(raw, a)
    mid = chain[len(chain) // 2] if len(chain) > 1 else a
    points = [("deep", dict(body=raw.bodies[a].name, pos=(0.03, -0.02, 0.05))),
              ("mid", dict(body=raw.bodies[mid].name, pos=(0.0, 0.01, 0.02)))]
    differences = [("deep_from_mid", "deep", "mid")]
    if raw.bodies[0].joint is not None and raw.bodies[0].parent < 0 and 0 not in (a, mid):
        points.append(("root", dict(body=raw.bodies[0].name, pos=(0.01, 0.0, 0.0))))
        differences.append(("deep_from_root", "deep", "root"))
    return points, differences


# random_model seeds both compilers take: paths of 18, 15 and 20 joints with ball joints, anchors and refs; 17 and 35 hang
# from a free root (tests/test_points_cpu.py asserts what the cases must cover)
RANDOM_SEEDS = (5, 17, 35)


def case_names():
    return ["reacher", "cartpole", "tray", "door", "gripper"] + ["random%d" % s for s in RANDOM_SEEDS]


_RAW = {}


def case(name):
    """-> (raw model, engine kind 'arm' / 'tree', points [(name, dict(body= / site=, pos=))], differences [(name, a, b)])."""
    if name not in _RAW:
        if name == "reacher":
            from mjmpc_amd.models.reacher7dof import reacher7dof_raw
            _RAW[name] = reacher7dof_raw()
        elif name.startswith("random"):
            from test_random_models_gpu import random_model
            _RAW[name] = random_model(int(name[6:]))
        else:
            from mjmpc_amd.models.synthetic import synthetic_raw
            _RAW[name] = synthetic_raw(name)
    raw = _RAW[name]
    kind = "arm" if name == "reacher" else "tree"
    if name == "tray":
        return raw, kind, [("glass", dict(site="finger")), ("tray", dict(body="wrist", pos=(0.0, 0.0, 0.02))),
                           ("fore", dict(body="elbow", pos=(0.1, 0.0, 0.0)))], \
            [("glass_from_tray", "glass", "tray"), ("tray_from_fore", "tray", "fore")]
    if name == "door":
        return raw, kind, [("grip", dict(site="finger")), ("bolt", dict(body="bolt", pos=(0.03, 0.0, 0.0))),
                           ("leaf", dict(body="leaf", pos=(0.2, 0.0, 0.5)))], [("grip_from_bolt", "grip", "bolt")]
    if name == "gripper":
        return raw, kind, [("pen", dict(body="pen")), ("left", dict(body="finger_l", pos=(0.0, 0.0, 0.05))),
                           ("right", dict(body="finger_r", pos=(0.0, 0.0, 0.05))), ("can", dict(body="can", pos=(0.0, 0.0, 0.05)))], \
            [("pen_from_left", "pen", "left"), ("left_from_right", "left", "right")]
    if name == "cartpole":
        return raw, kind, [("cart", dict(body=raw.bodies[0].name, pos=(0.0, 0.0, 0.05))),
                           ("tip", dict(body=raw.bodies[-1].name, pos=(0.0, 0.0, 0.6)))], [("tip_from_cart", "tip", "cart")]
    return (raw, kind) + _generic(raw)


def resolved(raw, points, differences):
    """-> ([(body index, pos)], [(a, b)]) of a case's points and differences, by the names alone."""
    names = [b.name for b in raw.bodies]
    pts = []
    for _, kw in points:
        if "site" in kw:
            pts.append((raw.sites[kw["site"]][0], np.asarray(raw.sites[kw["site"]][1], float)))
        else:
            pts.append((names.index(kw["body"]), np.asarray(kw.get("pos", (0.0, 0.0, 0.0)), float)))
    order = [n for n, _ in points]
    return pts, [(order.index(a), order.index(b)) for _, a, b in differences]


def add_points(terms, points, differences):
    for name, kw in points:
        terms.point(name, **kw)
    for name, a, b in differences:
        terms.difference(name, a, b)
    return terms


def random_qpos(raw, rs):
    """A random configuration: hinges and slides about their ``ref``, unit quaternions for ball and free joints."""
    from mjmpc_amd.models.raw import JOINT_BALL, JOINT_FREE, JOINT_SLIDE

    def quat(scale):
        w = scale * rs.standard_normal(3)
        a = np.linalg.norm(w)
        return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * w / max(a, 1e-12)])

    q, adr = raw.qpos0.copy(), 0
    for b in raw.bodies:
        jt = b.joint
        if jt is None:
            continue
        if jt.type == JOINT_FREE:
            q[adr:adr + 3] += 0.1 * rs.standard_normal(3)
            q[adr + 3:adr + 7] = quat(1.0)
        elif jt.type == JOINT_BALL:
            q[adr:adr + 4] = quat(0.8)
        else:
            q[adr] = jt.ref + rs.uniform(-1.2, 1.2) * (0.25 if jt.type == JOINT_SLIDE else 1.0)
        adr += jt.nq
    return q


def host_engine(raw, kind="tree"):
    """What ``CostTerms`` reads of an engine, without a device: ``raw``, ``model`` and ``obs_layout``."""
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    return (ArmRolloutEngine if kind == "arm" else TreeRolloutEngine).host_only(raw)
