"""User-defined cost terms: a table of terms over the next observation and the action of every (particle,
step), evaluated on the device by a second launch behind the rollout (``mjmpc_cost_terms``, csrc/cost_terms.hip) in place
of, or on top of, the cost the rollout kernel has built in.

    terms = CostTerms(engine)
    terms.norm(obs="site_minus_target", weight=5.0)
    terms.cos(obs="qpos", index=1)
    terms.square(obs="qvel", weight=0.01)
    terms.square(action=0, weight=0.001)
    terms.square(obs="qvel", weight=1.0, terminal=True)
    engine.set_cost_terms(terms)                    # before make_device_rollout_fn(engine)

A table row is eight float64: ``kind, source, index, weight, target, group, when, reserved``.  ``v`` is entry ``index`` of
the next observation (``source`` 0) or of the action (``source`` 1); ``r = v - target``:

* kind 0 ABS ``w |r|``, kind 1 SQUARE ``w r^2``, kind 3 COS ``w (1 - cos r)``;
* kind 2 NORM: consecutive rows with one ``group`` > 0 add ``w sqrt(sum r^2)`` once, ``w`` the first row's weight;
* ``when`` 1: the row counts only at a rollout's last step, never in a step of the controlled env.

``obs=`` names a block of ``engine.obs_layout()`` (``index=`` counts inside it; left out: every entry) or gives absolute
indices into the observation; ``action=`` gives action indices (``True`` or ``"all"``: the block, with ``index=``).
Everything is checked here, on the host: the kernel assumes a valid table.

A term may follow a reference trajectory instead of a constant target: ``reference=`` is ``[N]`` (one value for
all its indices) or ``[N][n_idx]``, row ``n`` the goal for env time ``n``; beyond the last row the goal is held, or with
``periodic=True`` the reference starts over.  Step ``t`` of a plan made at env time ``s`` compares its next observation with
row ``s + t + 1`` and its action with row ``s + t``.  All tracked terms of a table share ``N`` and ``periodic``.  A tracked
row's ``reserved`` column holds 1 + its column of ``reference_table()`` and its ``target`` column the first goal; the env time
is a counter on the device (``engine.set_track_step`` / ``track_step``; the controlled env's steps advance it).

    terms.square(obs="qpos", index=0, weight=0.5, reference=np.repeat([0.0, 0.4, 0.0, -0.4], 50), periodic=True)

Action rates and one-sided kinds.  ``action_rate=`` (what ``action=`` takes) makes rows of ``source`` 2:
``v = u_t - u_{t-1}``, the change of the action from the step before - at a plan's first step from the action last applied
to the controlled env, which the engine keeps on the device (``engine.set_prev_action`` / ``prev_action``; before the first
step the rate is 0).  The kinds 4 .. 7 are zero on one side of the bound ``target``: ABOVE ``w max(0, r)``, BELOW
``w max(0, -r)``, ABOVE_SQUARE and BELOW_SQUARE their squares.  A table with either is costed by ``mjmpc_cost_terms_rate``
(``needs_rate_entry``); every other table is what it was, byte for byte.

    terms.square(action_rate="all", weight=0.1)                         # smooth controls
    terms.outside(obs="qpos", index=0, low=-2.0, high=2.0, weight=10.0)  # the cart stays within +-2 m
    terms.above(obs="qvel", index=1, target=3.0)                        # joint speed below 3 rad/s, linear beyond it

Quadratic forms and signed linear rows.  ``quadratic`` adds one group of kind 8 QUAD rows over its indices:
``weight * sum_ij r_i Q_ij r_j`` with ``r_i = v_i - goal_i``, ``Q`` the ``matrix=`` (``[n][n]``, stored as ``(M + M') / 2``, or
``[n]`` for a diagonal; ``n <= 32``; it may be indefinite).  The matrices of a table live in a pool beside it (``quad_table()``,
float64, back to back in table order).  ``parts=`` concatenates rows of several sources into one vector, each part resolved like
a term of its own.  ``linear`` is kind 9, ``weight * r`` with its sign.  A table with either is costed by
``mjmpc_cost_terms_quad`` (``needs_quad_entry``); every other table is what it was.

    terms.quadratic(obs=[0, 1, 2, 3], matrix=Q, target=[0.0, np.pi, 0.0, 0.0])      # (x - x*)' Q (x - x*)
    terms.quadratic(obs=[0, 1, 2, 3], matrix=P_riccati, terminal=True)              # x' P x at a plan's last step
    terms.quadratic(parts=[dict(obs="qpos"), dict(obs="qvel"), dict(action="all")], matrix=QNR)
    terms.linear(obs="qvel", index=0, weight=-1.0)                                  # reward forward velocity

World positions of points.  ``point`` names a point on any body - ``body=`` with ``pos=`` in the body frame, or
``site=``, a body-attached site of the model (``RawModel.sites``) - and ``difference`` the vector from one point to another.
Each is a block of three entries (world x, y, z) behind the observation, in definition order, which every kind above takes like
any other block: the engine launches ``mjmpc_points`` (csrc/points.hip) in front of the cost entry, which copies each next
observation into an augmented row ``[d_obs + n_extra]`` and appends the positions, computed in double from the row's own
``qpos`` by the points program (``points_table()``; the row format: include/mjmpc_amd.h).  They are the positions AT that
``qpos``; the built-in ``site`` block lags one substep and is not expected to equal a point on the same body.

    terms.point("tray", body="wrist", pos=(0.0, 0.0, 0.02))
    terms.point("glass", body="glass")
    terms.difference("glass_from_tray", "glass", "tray")
    terms.norm(obs="glass_from_tray", index=[0, 1], weight=3.0)             # the glass over the tray's centre
    terms.below_square(obs="glass", index=2, target=0.45, weight=10.0)      # ... and not below 0.45 m

Axes and velocities.  ``axis`` gives the world direction of a body-fixed unit vector, ``velocity`` the world linear
velocity of a named point and ``angular_velocity`` the world angular velocity of a body, from the row's own ``qpos`` and ``qvel``
with MuJoCo's meaning of ``qvel`` (a ball joint's and a free joint's angular rates are in the body's frame).  They are blocks
like a point's - points, axes, velocities and angular velocities stand in definition order, at most 16 together, the
differences behind them - and ``difference`` takes two of one kind.  A table with any of them launches
``mjmpc_points_motion`` in place of ``mjmpc_points``; all outputs on one body share one walk of its path.

    terms.axis("glass_up", body="glass", axis=(0, 0, 1))
    terms.linear(obs="glass_up", index=2, weight=-2.0)                      # upright: reward the world z of the glass's z axis
    terms.velocity("glass_vel", "glass")
    terms.velocity("tray_vel", "tray")
    terms.difference("slip", "glass_vel", "tray_vel")
    terms.norm(obs="slip", weight=0.5)                                      # the glass at rest relative to the tray

Centres of mass.  ``com`` gives the world position of the centre of mass of a body and all its descendants
(``body=None``: of the whole model) and ``com_velocity`` its world velocity - the subtree's linear momentum over its mass -,
with the masses and inertial positions the engine's model compiler computes for the nominal model.  They are outputs like a
point and a velocity - in definition order, counted among the 16 - and ``difference`` takes a centre of mass with a centre of
mass or a point, its velocity with another or with a ``velocity``.  A table with either launches ``mjmpc_points_tree`` for its
whole program: one walk per centre of mass that visits every jointed body of the subtree once, saving the frame at a branch
point (at most 4 frames saved at a time).  Such a table cannot be combined with ``randomize_dynamics`` of ``body_mass``: every
shard would have a centre of mass of its own.

    terms.com("body_com")                                                   # the whole model
    terms.com_velocity("body_vel", "body_com")
    terms.linear(obs="body_vel", index=0, weight=-1.0)                      # forward progress of the centre of mass
    terms.outside(obs="body_com", index=2, low=-0.15, high=0.25, weight=5.0)

Orientations.  ``orientation`` gives the orientation error of a body as three entries: the rotation vector
``r = theta u`` of the rotation that takes a goal frame to the body's frame (times a body-fixed offset ``quat``), written in the
goal frame.  The goal is a constant world quaternion ``target`` or, with ``relative_to=``, the frame of another body (times
``relative_quat``), so the error is relative.  ``r = Log(conj(a) * q_body * o)`` with the log map of include/mjmpc_amd.h:
``theta`` in ``[0, pi]``, exactly 0 at the goal.  An output like a point - in definition order, counted among the 16 -, so
``norm`` is the geodesic angle, ``square`` its square, ``quadratic(parts=)`` couples it with an angular velocity and ``outside``
on a component is a band.  ``difference`` refuses it (subtracting rotation vectors is not a rotation: use ``relative_to``); a
``reference=`` on the block subtracts component by component.  A table with one launches ``mjmpc_points_orient`` for its whole
program; an absolute orientation shares its body's walk, a relative one walks both paths.

    terms.orientation("glass_on_tray", body="glass", relative_to="wrist")
    terms.norm(obs="glass_on_tray", weight=2.0)                            # level AND not spun on the tray: the angle
    terms.orientation("pen_err", body="pen", target=(0.707, 0.0, 0.707, 0.0))
    terms.square(obs="pen_err", weight=1.0, terminal=True)
"""
import numpy as np

from ..models.raw import JOINT_BALL, JOINT_FREE, JOINT_HINGE, JOINT_SLIDE, TASK_FORWARD, TASK_REACH

KIND_ABS, KIND_SQUARE, KIND_NORM, KIND_COS = 0, 1, 2, 3
KIND_ABOVE, KIND_BELOW, KIND_ABOVE_SQUARE, KIND_BELOW_SQUARE = 4, 5, 6, 7
KINDS = {"abs": KIND_ABS, "square": KIND_SQUARE, "norm": KIND_NORM, "cos": KIND_COS, "above": KIND_ABOVE, "below": KIND_BELOW,
         "above_square": KIND_ABOVE_SQUARE, "below_square": KIND_BELOW_SQUARE}
KIND_QUAD, KIND_LINEAR = 8, 9
KINDS.update(quadratic=KIND_QUAD, linear=KIND_LINEAR)
SOURCE_OBS, SOURCE_ACTION, SOURCE_ACTION_RATE = 0, 1, 2
MAX_TERMS = 128
MAX_QUAD = 32                   # rows of a quadratic group
ROW_LEN = 8
MAX_REFERENCE_ROWS = 1 << 20    # (the kernel's per-lane index arithmetic is 32-bit)


def _dims(engine):
    return int(engine.model.d_obs), int(engine.model.nu)


def _finite(x, what):
    x = np.asarray(x, np.float64)
    if not np.all(np.isfinite(x)):
        raise ValueError("cost term: %s must be finite, got %r" % (what, x.tolist()))
    return x


MAX_POINTS = 16
MAX_DIFFERENCES = 16
MAX_PATH_NODES = 33             # jointed bodies on a point's path (welded ones are folded into the pose behind them)
POINT_ROW_LEN = 16
POINT_ROW, DIFFERENCE_ROW = 0, 5
AXIS_ROW, VELOCITY_ROW, ANGULAR_ROW = 6, 7, 8      # the further closing rows of mjmpc_points_motion
MASS_ROW, SAVE_ROW, RESTORE_ROW, COM_ROW, COM_VELOCITY_ROW = 9, 10, 11, 12, 13     # mjmpc_points_tree's
HOLD_ROW, ORIENTATION_ROW = 14, 15                  # mjmpc_points_orient's
MAX_LEVELS = 4                  # frames a tree program may have saved at a time
MAX_PROGRAM_ROWS = 544
_POSITIONS, _VELOCITIES = (POINT_ROW, COM_ROW), (VELOCITY_ROW, COM_VELOCITY_ROW)  # what a difference may mix
_JOINT_KINDS = {JOINT_HINGE: 1, JOINT_SLIDE: 2, JOINT_BALL: 3, JOINT_FREE: 4}


def _quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _quat_rotate(q, v):
    t = 2.0 * np.cross(q[1:], v)
    return v + q[0] * t + np.cross(q[1:], t)


def _addresses(raw):
    """-> ({body: first qpos address of its joint}, {body: first qvel address})."""
    qadr, dadr, q, d = {}, {}, 0, 0
    for i, b in enumerate(raw.bodies):
        if b.joint is not None:
            qadr[i], dadr[i] = q, d
            q, d = q + b.joint.nq, d + b.joint.ndof
    return qadr, dadr


def _path(raw, body, qadr, dadr):
    """The node rows of the path from the root to ``body``, their dof addresses and the pose ``(at, turn)`` of the welded
    bodies behind the last node, which the closing row takes up."""
    chain = []
    while body >= 0:
        chain.append(body)
        body = raw.bodies[body].parent
    at, turn = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])       # the welded bodies' pose, waiting for the next node
    rows, dofs = [], []
    for i in reversed(chain):
        b = raw.bodies[i]
        quat = np.asarray(b.quat, float) / np.linalg.norm(b.quat)
        at, turn = at + _quat_rotate(turn, np.asarray(b.pos, float)), _quat_mul(turn, quat)
        if b.joint is None:
            continue
        j, row = b.joint, np.zeros(POINT_ROW_LEN)
        norm = np.linalg.norm(j.axis)
        row[0], row[1] = _JOINT_KINDS[j.type], qadr[i]
        row[2] = float(j.ref) if j.type in (JOINT_HINGE, JOINT_SLIDE) else 0.0
        row[3:6], row[6:10] = at, turn
        row[10:13] = np.asarray(j.axis, float) / norm if norm > 0 else 0.0
        row[13:16] = j.pos
        rows.append(row)
        dofs.append(dadr[i])
        at, turn = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    if len(rows) > MAX_PATH_NODES:
        raise ValueError("cost terms: a point's path holds %d jointed bodies, at most %d" % (len(rows), MAX_PATH_NODES))
    return rows, dofs, at, turn


def _program(raw, walks, differences):
    """The rows behind ``points_program`` and ``motion_program`` for ``walks`` - ``[(body index, [(kind, slot, vector)])]``:
    per walk the nodes of the body's path, then one closing row per output with its slot in column 2 and 1 in column 1 on all
    but the walk's last - and the ``differences`` rows behind them: float64 ``[n_rows + len(differences)][16]``, ``n_rows``
    and the node rows' first ``qvel`` addresses, int32 ``[n_rows]`` (0 on a closing row)."""
    qadr, dadr = _addresses(raw)
    rows, dofs = [], []
    for body, outputs, *tree in walks:
        # (a centre of mass, DESIGN 12.6, brings the rows of its walk; its closing rows take no vector)
        # (a relative orientation, DESIGN 12.7, brings both paths and the welded pose behind the second)
        nodes, node_dofs, at, turn = (tuple(tree[0]) + (None, None))[:4] if tree else _path(raw, body, qadr, dadr)
        rows.extend(nodes)
        dofs.extend(node_dofs)
        for k, (kind, slot, vec) in enumerate(outputs):
            row = np.zeros(POINT_ROW_LEN)
            row[0], row[1], row[2] = kind, float(k + 1 < len(outputs)), slot
            if kind in (POINT_ROW, VELOCITY_ROW):
                row[3:6] = at + _quat_rotate(turn, np.asarray(vec, float))
            elif kind == AXIS_ROW:
                row[3:6] = _quat_rotate(turn, np.asarray(vec, float))
            elif kind == ORIENTATION_ROW:       # (o behind the welded pose, the goal, rel)
                row[3:7], row[7:11], row[11] = _quat_mul(turn, vec[0:4]), vec[4:8], vec[8]
            rows.append(row)
            dofs.append(0)
    n_rows = len(rows)
    for a, b in differences:
        row = np.zeros(POINT_ROW_LEN)
        row[0], row[1], row[2] = DIFFERENCE_ROW, a, b
        rows.append(row)
    return np.ascontiguousarray(np.stack(rows), np.float64), n_rows, np.ascontiguousarray(dofs, np.int32)


def points_program(raw, points, differences=()):
    """The points program of ``mjmpc_points`` (row format: include/mjmpc_amd.h) for ``points`` - ``[(body index, position in
    the body frame)]`` - and ``differences`` - ``[(a, b)]``, indices into ``points`` - on ``raw``: float64
    ``[n_rows + len(differences)][16]`` and ``n_rows``.  A point's path holds one node per jointed body from the root to its
    body; a body without a joint is folded into the fixed pose of the node - or the point - behind it.  One walk per point, in
    definition order; columns 1 and 2 of its closing row are 0 (the kernel counts the points itself)."""
    return _program(raw, [(body, [(POINT_ROW, 0, pos)]) for body, pos in points], differences)[:2]


def motion_program(raw, outputs, differences=()):
    """The program of ``mjmpc_points_motion`` (row format: include/mjmpc_amd.h) for ``outputs`` -
    ``[(kind, body index, vector)]``, kind POINT_ROW / AXIS_ROW / VELOCITY_ROW / ANGULAR_ROW, the vector a position or an
    axis in the body frame - and ``differences`` - ``[(a, b)]``, indices into ``outputs``: float64
    ``[n_rows + len(differences)][16]``, ``n_rows`` and the node rows' first ``qvel`` addresses, int32 ``[n_rows]`` (0 on a
    closing row).  All outputs on one body share one walk, placed where the first of them was defined: the path's nodes, then
    one closing row per output with its slot - its index in ``outputs`` - in column 2 and 1 in column 1 on all but the last."""
    bodies = list(dict.fromkeys(body for _, body, _ in outputs))
    return _program(raw, [(body, [(kind, slot, vec) for slot, (kind, b, vec) in enumerate(outputs) if b == body])
                          for body in bodies], differences)


def inertials(engine):
    """``(mass [nb], ipos [nb][3])`` per raw body as the engine's own model compiler computes them for the nominal model:
    ``model.body_mass`` and ``model.body_ipos`` (models/compile.py) or ``body_inertials`` (models/compile_tree.py)."""
    ipos = getattr(engine.model, "body_ipos", None)
    if ipos is None:
        from ..models.compile_tree import body_inertials
        ipos = body_inertials(engine.raw)[3]
    return np.asarray(engine.model.body_mass, np.float64), np.asarray(ipos, np.float64).reshape(-1, 3)


def com_walk(raw, body, mass, ipos):
    """The rows of one centre-of-mass walk (row format: include/mjmpc_amd.h) without its closing rows, for the
    subtree of ``body`` (-1: every body) with the bodies' ``mass`` and ``ipos``: ``(rows, dofs, n_levels)``.  First the nodes of
    the path from the root to the subtree's root, then the subtree in depth-first order: a body without a joint is folded into
    the jointed body it is welded to, every such rigid group has its node row and, unless it is massless, its MASS row - its
    centre of mass in the node's frame and its share ``m / M`` of the subtree's mass -, a SAVE stands in front of the first
    child of a node with several children, a RESTORE in front of each further one, and a level is free again once its last
    child has begun.  Several root bodies restore to level -1, the world frame."""
    qadr, dadr = _addresses(raw)
    nb = len(raw.bodies)
    inside = [i == body or body < 0 for i in range(nb)]
    for i, b in enumerate(raw.bodies):              # (parents first)
        inside[i] = inside[i] or (b.parent >= 0 and inside[b.parent])
    total = float(sum(mass[i] for i in range(nb) if inside[i]))
    if not total > 0.0 or not np.isfinite(total):
        raise ValueError("cost terms: the bodies of this centre of mass weigh %r together" % total)

    def node_of(i):                                 # the jointed body whose frame carries body i; -1: the world
        while i >= 0 and raw.bodies[i].joint is None:
            i = raw.bodies[i].parent
        return i

    moment, weight, kids = {}, {}, {}               # per node: sum m c in its frame, sum m; its jointed children in the walk
    for i in range(nb):
        if not inside[i]:
            continue
        n = node_of(i)
        if raw.bodies[i].joint is not None:
            kids.setdefault(node_of(raw.bodies[i].parent), []).append(i)
            at, turn = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
        else:
            at, turn = _path(raw, i, qadr, dadr)[2:]
        moment[n] = moment.get(n, 0.0) + mass[i] * (at + _quat_rotate(turn, ipos[i]))
        weight[n] = weight.get(n, 0.0) + mass[i]

    rows, dofs, free, used = [], [], list(range(len(raw.bodies) + 1)), [0]

    def plain(kind, level):
        row = np.zeros(POINT_ROW_LEN)
        row[0], row[1] = kind, level
        rows.append(row)
        dofs.append(0)

    def mass_row(n):
        if weight.get(n, 0.0) > 0.0:
            row = np.zeros(POINT_ROW_LEN)
            row[0], row[3:6], row[6] = MASS_ROW, moment[n] / weight[n], weight[n] / total
            rows.append(row)
            dofs.append(0)

    def children(n, world):
        below = kids.get(n, [])
        level = -1
        if len(below) > 1 and not world:
            level = free.pop(0)
            used[0] = max(used[0], level + 1)
            plain(SAVE_ROW, level)
        for k, child in enumerate(below):
            if k > 0:
                plain(RESTORE_ROW, level)
            if k == len(below) - 1 and level >= 0:
                free.insert(0, level)
                free.sort()
            node_rows, node_dofs = _path(raw, child, qadr, dadr)[:2]
            rows.append(node_rows[-1])
            dofs.append(node_dofs[-1])
            mass_row(child)
            children(child, False)

    top = node_of(body) if body >= 0 else -1        # the frame the subtree hangs on: a node above it, its own root, or the world
    if body >= 0 and raw.bodies[body].joint is not None:
        top = node_of(raw.bodies[body].parent)
    if top >= 0:
        rows, dofs = [list(x) for x in _path(raw, top, qadr, dadr)[:2]]
    mass_row(top)                                   # (the subtree's bodies welded to that frame, if any)
    children(top, top < 0)
    if used[0] > MAX_LEVELS:
        raise ValueError("cost terms: this centre of mass needs %d saved frames at a time (nested branch points), the kernel "
                         "has %d" % (used[0], MAX_LEVELS))
    return rows, dofs, used[0]


def tree_program(raw, outputs, differences=(), mass=None, ipos=None):
    """The program of ``mjmpc_points_tree`` (row format: include/mjmpc_amd.h) for ``outputs`` - ``motion_program``'s
    ``[(kind, body index, vector)]`` and, for a centre of mass, ``(COM_ROW, body index or -1 for the whole model, None)`` and
    ``(COM_VELOCITY_ROW, index in outputs of its centre of mass, None)`` - with the bodies' ``mass`` and ``ipos``: the program,
    ``n_rows``, the dof addresses and ``n_levels``, the saved frames it uses.  The outputs on one body share one walk as in
    ``motion_program``; a centre of mass is a walk of its own (``com_walk``), closed by its COM row and, on the same walk, its
    COM_VELOCITY row; every walk stands where its first output was defined.

    The same builder makes the program of ``mjmpc_points_orient``: an orientation is ``(ORIENTATION_ROW, body
    index, (o[4], g[4], other))`` with the body-fixed offset ``o``, the goal ``g`` and ``other`` the index of the body the error
    is relative to, or -1.  An absolute one closes its body's walk like any output there; a relative one is a walk of its own:
    the path to ``other``, a HOLD row, the path to the body, then the closing row with ``rel`` 1 and, as its goal, ``g`` behind
    the pose of the bodies welded between ``other`` and its last node.  ``mass`` and ``ipos`` are read for a centre of mass
    only."""
    def relative(kind, vec):
        return kind == ORIENTATION_ROW and vec[8] >= 0

    keys = [("com", k) if kind == COM_ROW else ("com", int(b)) if kind == COM_VELOCITY_ROW
            else ("rel", k) if relative(kind, vec) else ("body", int(b)) for k, (kind, b, vec) in enumerate(outputs)]
    walks, n_levels = [], 0
    for key in dict.fromkeys(keys):
        closing = [(kind, slot, vec) for slot, (kind, _, vec) in enumerate(outputs) if keys[slot] == key]
        if key[0] == "com":
            rows, dofs, levels = com_walk(raw, int(outputs[key[1]][1]), mass, ipos)
            n_levels = max(n_levels, levels)
            walks.append((None, closing, (rows, dofs)))
        elif key[0] == "rel":
            (kind, slot, vec), body = closing[0], int(outputs[key[1]][1])
            adr = _addresses(raw)
            rows, dofs, _, other_turn = _path(raw, int(vec[8]), *adr)
            nodes, node_dofs, at, turn = _path(raw, body, *adr)
            hold = np.zeros(POINT_ROW_LEN)
            hold[0] = HOLD_ROW
            vec = np.concatenate([vec[0:4], _quat_mul(other_turn, vec[4:8]), [1.0]])
            walks.append((body, [(kind, slot, vec)], (rows + [hold] + nodes, dofs + [0] + node_dofs, at, turn)))
        else:
            closing = [(kind, slot, np.concatenate([vec[0:8], [0.0]]) if kind == ORIENTATION_ROW else vec)
                       for kind, slot, vec in closing]
            walks.append((key[1], closing))
    program, n_rows, dofadr = _program(raw, walks, differences)
    if n_rows > MAX_PROGRAM_ROWS:
        raise ValueError("cost terms: the points program has %d rows, at most %d" % (n_rows, MAX_PROGRAM_ROWS))
    return program, n_rows, dofadr, n_levels


def launch_points(lib, code, n, d_obs, nq, nv, obs, program, dofadr, n_rows, n_out, n_diff, out, stream, n_levels=None,
                  orient=False):
    """The one launch in front of a cost entry over ``n`` observation rows, the device arrays given as
    pointers: ``mjmpc_points`` without a dof-address table, ``mjmpc_points_motion`` - which reads the ``nv`` entries of ``qvel``
    behind ``qpos`` too - with one, ``mjmpc_points_tree`` with ``n_levels`` as well (a table that holds a centre of mass).
    ``orient``: a table that holds an orientation, whose whole program goes through ``mjmpc_points_orient``.
    -> the entry's return code."""
    if orient:
        return lib.mjmpc_points_orient(code, n, d_obs, nq, nv, obs, program, dofadr, n_rows, n_out, n_diff, n_levels or 0, out,
                                       stream)
    if n_levels is not None:
        return lib.mjmpc_points_tree(code, n, d_obs, nq, nv, obs, program, dofadr, n_rows, n_out, n_diff, n_levels, out, stream)
    if dofadr is None:
        return lib.mjmpc_points(code, n, d_obs, nq, obs, program, n_rows, n_out, n_diff, out, stream)
    return lib.mjmpc_points_motion(code, n, d_obs, nq, nv, obs, program, dofadr, n_rows, n_out, n_diff, out, stream)


def refuse_mass_randomization(terms, param_dict):
    """``ValueError`` if ``terms`` (a ``CostTerms``, a list of them or ``None``) hold a centre of mass while ``param_dict``
    (``randomize_dynamics``'s, or ``None``) randomizes ``body_mass``: every shard would have a centre of mass of its own and
    one program could not serve them.  The engines and the episode batches call it from ``set_cost_terms`` and
    from ``randomize_dynamics``, whichever comes second."""
    each = terms if isinstance(terms, (list, tuple)) else [terms]
    if param_dict and "body_mass" in param_dict and any(t is not None and t.needs_tree_entry for t in each):
        raise ValueError("cost terms with a centre of mass (com / com_velocity) cannot be combined with randomize_dynamics of "
                         "body_mass: every shard would have a centre of mass of its own, and the shards share one program")


class CostTerms:
    """A builder of the table.  With an ``engine`` every term is resolved and checked as it is added; without one the
    terms are kept as written and ``table(engine)`` / ``engine.set_cost_terms`` resolves them."""

    def __init__(self, engine=None, keep_builtin=False):
        self.engine = engine
        self.keep_builtin = bool(keep_builtin)
        # (kind, source block or None, indices or None, source 0 / 1 / 2 (non-zero: it indexes the action), weight, target,
        #  terminal, reference [N] / [N][n_idx] or None, quad: None, or for a part of a quadratic group its matrix [n][n] (the
        #  group's first part) or False (a later part))
        self._terms = []
        self._periodic = None       # the tracked terms' shared `periodic` (None: no tracked term yet)
        self._points = []           # the outputs (name, body index, position or axis in the body frame, closing kind): points
                                    # (DESIGN 12.4), axes, velocities and angular velocities, in definition order
        self._differences = []      # (name, output a, output b): indices into _points
        self._com_of = {}           # a COM velocity's index in _points -> its centre of mass's

    # ------------------------------------------------------------------ world positions of points and motion (12.5)
    def _raw_for_points(self, what):
        if self.engine is None:
            raise ValueError("cost terms: %s needs an engine - CostTerms(engine): a point is resolved against its model" % what)
        m = self.engine.model
        if getattr(m, "task", None) == TASK_FORWARD and getattr(m, "obs_skip", 0) > 0:
            raise ValueError("cost terms: this model's observation leaves out the first %d entries of qpos (a forward task "
                             "with obs_skip): world positions cannot be formed from it" % m.obs_skip)
        if getattr(self.engine, "raw", None) is None:
            raise ValueError("cost terms: %s needs an engine built from a RawModel (the bodies' poses are read from it)" % what)
        return self.engine.raw

    def _check_block_name(self, name):
        if not isinstance(name, str) or not name:
            raise ValueError("cost terms: a point or difference takes a name, got %r" % (name,))
        if name in self.engine.obs_layout():
            raise ValueError("cost terms: %r is a block of this engine's observation already" % name)
        if any(name == p[0] for p in self._points) or any(name == d[0] for d in self._differences):
            raise ValueError("cost terms: a point or difference named %r exists already" % name)

    def _body_index(self, raw, body):
        names = [b.name for b in raw.bodies]
        if body not in names:
            raise ValueError("cost terms: unknown body %r (this model has %s)" % (body, ", ".join(names)))
        return names.index(body)

    def _add_output(self, raw, name, index, vec, kind):
        if len(self._points) >= MAX_POINTS:
            raise ValueError("cost terms: a table holds at most %d points, axes, velocities and angular velocities" % MAX_POINTS)
        if self._differences:
            raise ValueError("cost terms: define the points before the differences (their blocks stand in that order)")
        if int(index) >= 0:
            _path(raw, int(index), *_addresses(raw))        # (a path too long is refused here)
        self._points.append((name, int(index), np.array(vec, np.float64), kind))
        return self

    def point(self, name, body=None, site=None, pos=None):
        """A block ``name`` of three entries behind the observation: the world position of the point ``pos`` (body frame,
        default its origin) of ``body``, or of the body-attached ``site`` (``RawModel.sites``), at the row's own ``qpos``.
        At most 16 points a table."""
        raw = self._raw_for_points("point")
        self._check_block_name(name)
        if (body is None) == (site is None):
            raise ValueError("cost terms: point takes body= or site=")
        if site is not None:
            if pos is not None:
                raise ValueError("cost terms: a site has its own position; drop pos=")
            if site not in raw.sites:
                raise ValueError("cost terms: unknown site %r (this model has %s)" % (site, ", ".join(sorted(raw.sites)) or "none"))
            index, pos = raw.sites[site]
        else:
            index = self._body_index(raw, body)
        pos = _finite((0.0, 0.0, 0.0) if pos is None else pos, "pos")
        if pos.shape != (3,):
            raise ValueError("cost terms: pos must be three numbers, got %r" % (pos.tolist(),))
        return self._add_output(raw, name, index, pos, POINT_ROW)

    def axis(self, name, body=None, axis=None):
        """A block ``name`` of three entries: the world direction of the body-fixed vector ``axis`` of ``body`` (normalised
        here), at the row's own ``qpos``.  Upright is then ``linear(obs=name, index=2, weight=-w)``."""
        raw = self._raw_for_points("axis")
        self._check_block_name(name)
        if body is None:
            raise ValueError("cost terms: axis takes body=")
        index = self._body_index(raw, body)
        if axis is None:
            raise ValueError("cost terms: axis takes axis=(x, y, z)")
        vec = _finite(axis, "axis")
        if vec.shape != (3,):
            raise ValueError("cost terms: axis must be three numbers, got %r" % (vec.tolist(),))
        norm = float(np.linalg.norm(vec))
        if not norm > 0.0 or not np.isfinite(norm):
            raise ValueError("cost terms: axis must not be zero, got %r" % (vec.tolist(),))
        return self._add_output(raw, name, index, vec / norm, AXIS_ROW)

    def velocity(self, name, point):
        """A block ``name`` of three entries: the world linear velocity of ``point``, a point named with ``point(...)``, from
        the row's own ``qpos`` and ``qvel`` with MuJoCo's meaning of ``qvel``.  It shares the point's walk."""
        raw = self._raw_for_points("velocity")
        self._check_block_name(name)
        known = [p for p in self._points if p[3] == POINT_ROW and p[0] == point]
        if not known:
            raise ValueError("cost terms: unknown point %r (defined: %s)"
                             % (point, ", ".join(p[0] for p in self._points if p[3] == POINT_ROW) or "none"))
        return self._add_output(raw, name, known[0][1], known[0][2], VELOCITY_ROW)

    def angular_velocity(self, name, body=None):
        """A block ``name`` of three entries: the world angular velocity of ``body``."""
        raw = self._raw_for_points("angular_velocity")
        self._check_block_name(name)
        if body is None:
            raise ValueError("cost terms: angular_velocity takes body=")
        return self._add_output(raw, name, self._body_index(raw, body), np.zeros(3), ANGULAR_ROW)

    def com(self, name, body=None):
        """A block ``name`` of three entries: the world position of the centre of mass of ``body`` and all its descendants
        (``None``: of every body of the model) at the row's own ``qpos``, with the nominal model's masses and
        inertial positions.  An output like a point; a subtree of mass 0 or one whose walk needs more than 4 saved frames at
        a time is refused."""
        raw = self._raw_for_points("com")
        self._check_block_name(name)
        index = -1 if body is None else self._body_index(raw, body)
        if len(self._points) < MAX_POINTS and not self._differences:
            com_walk(raw, index, *inertials(self.engine))       # (what the walk refuses is refused here)
        return self._add_output(raw, name, index, np.zeros(3), COM_ROW)

    def com_velocity(self, name, com):
        """A block ``name`` of three entries: the world velocity of ``com``, a centre of mass named with ``com(...)`` - the
        subtree's linear momentum over its mass, from the row's own ``qpos`` and ``qvel`` with MuJoCo's meaning of ``qvel``
        (DESIGN 12.5, 12.6).  It shares the walk of its centre of mass."""
        raw = self._raw_for_points("com_velocity")
        self._check_block_name(name)
        known = [k for k, p in enumerate(self._points) if p[3] == COM_ROW and p[0] == com]
        if not known:
            raise ValueError("cost terms: unknown centre of mass %r (defined: %s)"
                             % (com, ", ".join(p[0] for p in self._points if p[3] == COM_ROW) or "none"))
        self._add_output(raw, name, self._points[known[0]][1], np.zeros(3), COM_VELOCITY_ROW)
        self._com_of[len(self._points) - 1] = known[0]
        return self

    def orientation(self, name, body=None, quat=None, target=None, relative_to=None, relative_quat=None):
        """A block ``name`` of three entries: the rotation vector ``Log(conj(a) * q_body * o)`` that takes the goal frame ``a``
        to the frame of ``body`` times the body-fixed offset ``o = quat``, written in the goal frame, at the row's own ``qpos``
        (the log map: include/mjmpc_amd.h).  ``a`` is the constant world quaternion ``target`` or, with
        ``relative_to=`` another body, that body's frame times ``relative_quat``.  Quaternions are ``(w, x, y, z)``, normalised
        here, the identity by default.  An output like a point; ``norm(obs=name)`` is the geodesic angle in ``[0, pi]``."""
        raw = self._raw_for_points("orientation")
        self._check_block_name(name)
        if body is None:
            raise ValueError("cost terms: orientation takes body=")
        index = self._body_index(raw, body)
        if relative_to is not None and target is not None:
            raise ValueError("cost terms: an orientation takes target= or relative_to=, not both (relative_quat= is the offset "
                             "on the other body)")
        if relative_to is None and relative_quat is not None:
            raise ValueError("cost terms: relative_quat= goes with relative_to=")
        other = -1 if relative_to is None else self._body_index(raw, relative_to)

        def unit(q, what):
            q = _finite((1.0, 0.0, 0.0, 0.0) if q is None else q, what)
            if q.shape != (4,):
                raise ValueError("cost terms: %s must be four numbers (w, x, y, z), got %r" % (what, q.tolist()))
            norm = float(np.linalg.norm(q))
            if not norm > 0.0 or not np.isfinite(norm):
                raise ValueError("cost terms: %s must not be zero, got %r" % (what, q.tolist()))
            return q / norm

        vec = np.concatenate([unit(quat, "quat"), unit(relative_quat if relative_to is not None else target,
                                                       "relative_quat" if relative_to is not None else "target"), [other]])
        if other >= 0 and len(self._points) < MAX_POINTS and not self._differences:
            _path(raw, other, *_addresses(raw))             # (a path too long is refused here)
        return self._add_output(raw, name, index, vec, ORIENTATION_ROW)

    def difference(self, name, a, b):
        """A block ``name`` of three entries behind the outputs' blocks: ``a`` minus ``b`` (world frame), one double subtraction
        per component - two points, two axes, two velocities or two angular velocities; a centre of mass counts as a point
        and its velocity as a velocity.  At most 16 differences a table."""
        self._raw_for_points("difference")
        self._check_block_name(name)
        known = [p[0] for p in self._points]
        for x in (a, b):
            if x not in known:
                raise ValueError("cost terms: unknown point, axis or velocity %r (defined: %s)" % (x, ", ".join(known) or "none"))
        ia, ib = known.index(a), known.index(b)
        for x, i in ((a, ia), (b, ib)):
            if self._points[i][3] == ORIENTATION_ROW:
                raise ValueError("cost terms: %r is an orientation, and subtracting rotation vectors is not a rotation: define "
                                 "the error between two bodies with orientation(..., relative_to=)" % x)
        ka, kb = self._points[ia][3], self._points[ib][3]
        if ka != kb and not any(ka in both and kb in both for both in (_POSITIONS, _VELOCITIES)):
            raise ValueError("cost terms: a difference takes two points, two axes, two velocities or two angular velocities; "
                             "%r and %r are of different kinds" % (a, b))
        if len(self._differences) >= MAX_DIFFERENCES:
            raise ValueError("cost terms: a table holds at most %d differences" % MAX_DIFFERENCES)
        self._differences.append((name, ia, ib))
        return self

    @property
    def n_extra(self):
        """Entries the outputs and differences add behind the observation: three each."""
        return 3 * (len(self._points) + len(self._differences))

    @property
    def needs_motion_entry(self):
        """Whether an axis, a velocity or an angular velocity is defined: ``mjmpc_points_motion`` instead of ``mjmpc_points``."""
        return any(p[3] != POINT_ROW for p in self._points)

    @property
    def needs_tree_entry(self):
        """Whether a centre of mass is defined: ``mjmpc_points_tree`` for the whole program."""
        return any(p[3] in (COM_ROW, COM_VELOCITY_ROW) for p in self._points)

    @property
    def needs_orient_entry(self):
        """Whether an orientation is defined: ``mjmpc_points_orient`` for the whole program."""
        return any(p[3] == ORIENTATION_ROW for p in self._points)

    def points_layout(self, engine=None):
        """Named slices of the outputs' (points, axes, velocities, angular velocities) and differences' blocks in the augmented
        row, in definition order."""
        engine = engine if engine is not None else self.engine
        d, out = (_dims(engine)[0] if engine is not None else 0), {}
        for k, entry in enumerate(self._points + self._differences):
            out[entry[0]] = slice(d + 3 * k, d + 3 * k + 3)
        return out

    def points_table(self, engine=None):
        """``(program, n_rows, n_points, n_differences)`` - the points program of ``mjmpc_points``, float64
        ``[n_rows + n_differences][16]`` (``points_program``) -, or ``None`` for a table without points.  With an axis, a
        velocity or an angular velocity: ``(program, n_rows, n_outputs, n_differences, dofadr)``, the program and
        the node rows' ``qvel`` addresses (int32 ``[n_rows]``) of ``mjmpc_points_motion`` (``motion_program``).  With a centre of
        mass: ``(program, n_rows, n_outputs, n_differences, dofadr, n_levels)`` of ``mjmpc_points_tree``
        (``tree_program``).  With an orientation a seventh entry, ``True``, says that the six are
        ``mjmpc_points_orient``'s: the whole program goes through that entry, ``n_levels`` 0 without a centre of mass."""
        if not self._points:
            return None
        engine = engine if engine is not None else self.engine
        raw = getattr(engine, "raw", None)
        if raw is None:
            raise ValueError("cost terms: points need an engine built from a RawModel")
        differences = [(a, b) for _, a, b in self._differences]
        if self.needs_tree_entry or self.needs_orient_entry:
            outputs = [(k, self._com_of[i] if k == COM_VELOCITY_ROW else b, None if k in (COM_ROW, COM_VELOCITY_ROW) else p)
                       for i, (_, b, p, k) in enumerate(self._points)]
            program, n_rows, dofadr, n_levels = tree_program(raw, outputs, differences,
                                                             *(inertials(engine) if self.needs_tree_entry else (None, None)))
            return (program, n_rows, len(self._points), len(self._differences), dofadr, n_levels) + (
                (True,) if self.needs_orient_entry else ())
        if self.needs_motion_entry:
            program, n_rows, dofadr = motion_program(raw, [(k, b, p) for _, b, p, k in self._points], differences)
            return program, n_rows, len(self._points), len(self._differences), dofadr
        program, n_rows = points_program(raw, [(b, p) for _, b, p, _ in self._points], differences)
        return program, n_rows, len(self._points), len(self._differences)

    # ------------------------------------------------------------------ the kinds
    def abs(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
            periodic=False, action_rate=None):
        return self._add(KIND_ABS, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def square(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
               periodic=False, action_rate=None):
        return self._add(KIND_SQUARE, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def cos(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
            periodic=False, action_rate=None):
        return self._add(KIND_COS, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def norm(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
             periodic=False, action_rate=None):
        """``weight * sqrt(sum_i (v_i - target_i)^2)`` over the indices: one group of the table."""
        return self._add(KIND_NORM, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    # ------------------------------------------------------------------ one-sided kinds: `target` is the bound
    def above(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
              periodic=False, action_rate=None):
        """``weight * max(0, v - target)``: nothing up to the bound, linear above it."""
        return self._add(KIND_ABOVE, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def below(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
              periodic=False, action_rate=None):
        """``weight * max(0, target - v)``: nothing down to the bound, linear below it."""
        return self._add(KIND_BELOW, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def above_square(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
                     periodic=False, action_rate=None):
        """``weight * max(0, v - target)^2``."""
        return self._add(KIND_ABOVE_SQUARE, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def below_square(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
                     periodic=False, action_rate=None):
        """``weight * max(0, target - v)^2``."""
        return self._add(KIND_BELOW_SQUARE, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def outside(self, obs=None, action=None, index=None, low=None, high=None, weight=1.0, squared=True, terminal=False,
                action_rate=None):
        """A soft band: nothing inside ``[low, high]``, outside it ``weight`` times the distance to the band (``squared``: its
        square).  Adds the ``below`` row or rows at ``low`` and then the ``above`` row or rows at ``high``; either bound may
        be left out (``None``), each is a number or one number per index."""
        if low is None and high is None:
            raise ValueError("cost term: outside needs low=, high= or both")
        if low is not None and high is not None and np.any(_finite(low, "low") > _finite(high, "high")):
            raise ValueError("cost term: outside needs low <= high, got low %r, high %r" % (low, high))
        n = len(self._terms)
        try:
            if low is not None:
                self._add(KIND_BELOW_SQUARE if squared else KIND_BELOW, obs, action, index, weight, low, terminal, None, False,
                          action_rate)
            if high is not None:
                self._add(KIND_ABOVE_SQUARE if squared else KIND_ABOVE, obs, action, index, weight, high, terminal, None, False,
                          action_rate)
        except ValueError:
            del self._terms[n:]         # (both rows or neither)
            raise
        return self

    # ------------------------------------------------------------------ quadratic forms and signed linear rows
    def linear(self, obs=None, action=None, index=None, weight=1.0, target=0.0, terminal=False, reference=None,
               periodic=False, action_rate=None):
        """``weight * (v - target)``, signed: a reward where the weight is negative."""
        return self._add(KIND_LINEAR, obs, action, index, weight, target, terminal, reference, periodic, action_rate)

    def quadratic(self, obs=None, action=None, action_rate=None, index=None, matrix=None, weight=1.0, target=0.0,
                  terminal=False, reference=None, periodic=False, parts=None):
        """``weight * sum_ij r_i Q_ij r_j`` over the indices, ``r_i = v_i - target_i`` (or the tracked goal): one group of the
        table.  ``matrix``: ``[n][n]`` - kept as ``(M + M') / 2``, the same form - or ``[n]`` for a diagonal; finite, not
        necessarily positive semi-definite; ``n <= 32``.  ``parts=``: a list of ``dict(obs= / action= / action_rate=, index=,
        target=, reference=)`` whose rows are concatenated in order into the one vector the matrix applies to - a form over
        mixed sources such as ``[x; u]' [[Q, N], [N', R]] [x; u]``."""
        if matrix is None:
            raise ValueError("cost term: quadratic needs matrix=")
        try:
            Q = np.array(_finite(matrix, "matrix"), np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("cost term: matrix must be [n][n] or [n] finite numbers: %s" % (e,)) from e
        if Q.ndim == 1 and Q.size >= 1:
            Q = np.diag(Q)
        if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or Q.shape[0] < 1:
            raise ValueError("cost term: matrix must be square, [n][n], or [n] for a diagonal, got shape %s"
                             % (list(np.shape(matrix)),))
        if Q.shape[0] > MAX_QUAD:
            raise ValueError("cost term: a quadratic group holds at most %d rows, the matrix has %d" % (MAX_QUAD, Q.shape[0]))
        Q = 0.5 * (Q + Q.T)
        if parts is None:
            parts = [dict(obs=obs, action=action, action_rate=action_rate, index=index, target=target, reference=reference)]
        elif obs is not None or action is not None or action_rate is not None or index is not None or reference is not None \
                or np.ndim(target) != 0 or float(target) != 0.0:
            raise ValueError("cost term: with parts= the sources, indices, targets and references go into the parts")
        if not isinstance(parts, (list, tuple)) or not parts or not all(isinstance(p, dict) for p in parts):
            raise ValueError("cost term: parts= is a list of dict(obs= / action= / action_rate=, index=, target=, reference=)")
        if periodic and not any(p.get("reference") is not None for p in parts):
            raise ValueError("cost term: periodic= goes with a reference=")
        n0, periodic0 = len(self._terms), self._periodic
        try:
            for k, part in enumerate(parts):
                if set(part) - _PART_KEYS:
                    raise ValueError("cost term: a part takes %s, got %r" % (sorted(_PART_KEYS), part))
                self._add(KIND_QUAD, part.get("obs"), part.get("action"), part.get("index"), weight, part.get("target", 0.0),
                          terminal, part.get("reference"), periodic and part.get("reference") is not None,
                          part.get("action_rate"), quad=Q if k == 0 else False)
            if self.engine is not None or all(t[2] is not None for t in self._terms[n0:]):
                self._quad_groups(self.engine)              # (the matrix against the rows it applies to)
        except ValueError:
            del self._terms[n0:]            # (the whole group or nothing)
            self._periodic = periodic0
            raise
        return self

    def _quad_groups(self, engine):
        """-> [(matrix [n][n], rows)] of the quadratic groups in table order, each matrix checked against its rows."""
        groups = []
        for t in self._terms:
            if t[8] is None:
                continue
            n_idx = len(self._resolve(t, engine)[0])
            if t[8] is False:
                groups[-1][1] += n_idx
            else:
                groups.append([t[8], n_idx])
        for Q, n in groups:
            if Q.shape[0] != n:
                raise ValueError("cost term: the matrix is %d x %d, the group has %d rows" % (Q.shape[0], Q.shape[0], n))
        return groups

    def quad_table(self, engine=None):
        """The float64 pool of the quadratic groups' matrices - ``n x n`` row-major and symmetric, back to back in table order:
        a group's offset is the sum of ``n^2`` over the groups before it -, or ``None`` without a quadratic group."""
        groups = self._quad_groups(engine if engine is not None else self.engine)
        if not groups:
            return None
        return np.ascontiguousarray(np.concatenate([Q.reshape(-1) for Q, _ in groups]), np.float64)

    @property
    def needs_quad_entry(self):
        """Whether the table holds a quadratic group or a signed linear row: rows only ``mjmpc_cost_terms_quad`` and
        ``mjmpc_cost_terms_quad_batch`` serve."""
        return any(t[0] in (KIND_QUAD, KIND_LINEAR) for t in self._terms)

    @property
    def needs_rate_entry(self):
        """Whether the table holds an action-rate row or a one-sided kind: rows only ``mjmpc_cost_terms_rate`` and
        ``mjmpc_cost_terms_rate_batch`` serve - or, with ``needs_quad_entry``, the quad entries, which serve
        every row."""
        return any(t[3] == SOURCE_ACTION_RATE or KIND_ABOVE <= t[0] <= KIND_BELOW_SQUARE for t in self._terms)

    @property
    def reads_action_rate(self):
        """Whether a row reads an action rate: the engine then keeps the previous action."""
        return any(t[3] == SOURCE_ACTION_RATE for t in self._terms)

    # ------------------------------------------------------------------ tracked terms
    @property
    def tracked(self):
        """Whether a term takes a ``reference=``."""
        return any(t[7] is not None for t in self._terms)

    @property
    def periodic(self):
        """The tracked terms' ``periodic`` (False without one)."""
        return bool(self._periodic)

    def reference_table(self, engine=None):
        """The float64 ``[N][R]`` reference of the table's ``R`` tracked rows, in row order - column ``c`` belongs to the
        row whose ``reserved`` column holds ``1 + c`` -, or ``None`` without a tracked term."""
        engine = engine if engine is not None else self.engine
        cols = []
        for t in self._terms:
            if t[7] is not None:
                n_idx = len(self._resolve(t, engine)[0])
                cols.append(self._reference_columns(t[7], n_idx))
        return np.ascontiguousarray(np.concatenate(cols, axis=1), np.float64) if cols else None

    @staticmethod
    def _reference_columns(reference, n_idx):
        """A term's reference as ``[N][n_idx]``: ``[N]`` holds one value for all its indices."""
        if reference.ndim == 1:
            return np.repeat(reference[:, None], n_idx, axis=1)
        if reference.shape[1] != n_idx:
            raise ValueError("cost term: reference must be [N] or [N][%d] (one column per index), got %s"
                             % (n_idx, list(reference.shape)))
        return reference

    @classmethod
    def builtin_reach(cls, engine, keep_builtin=False):
        """The reach task's built-in cost ``|site - target|_1 + 5 |site - target|_2`` as terms: three ABS rows on
        ``site_minus_target`` and one NORM group of weight 5 over the same three entries.  Refused for forward and
        orient models (forward progress reads ``qpos[0]``, which the observation leaves out): add to their built-in cost
        with ``keep_builtin=True`` instead."""
        if getattr(engine.model, "task", TASK_REACH) != TASK_REACH:
            raise ValueError("builtin_reach restates the reach task's cost; this model's task is not reach - use "
                             "CostTerms(engine, keep_builtin=True) to add terms to its built-in cost")
        self = cls(engine, keep_builtin=keep_builtin)
        self.abs(obs="site_minus_target")
        self.norm(obs="site_minus_target", weight=5.0)
        return self

    # ------------------------------------------------------------------ the table
    def __len__(self):
        """Rows of the table (terms that name a block count its entries: needs the engine)."""
        return sum(len(self._resolve(t, self.engine)[0]) for t in self._terms)

    def table(self, engine=None):
        """The ``[K][8]`` float64 array for ``engine`` (default: the builder's own)."""
        engine = engine if engine is not None else self.engine
        rows, group, col = [], 0, 0
        for t in self._terms:
            (kind, _, _, _, weight, _, terminal, reference, quad), idx, source, targets = (t,) + self._resolve(t, engine)
            if kind == KIND_NORM or (kind == KIND_QUAD and quad is not False):
                group += 1              # a fresh id per norm and per quadratic: neighbouring groups never merge
            reserved = [0.0] * len(idx)
            if reference is not None:
                # a tracked row: 1 + its column of reference_table(); the target column holds the first goal
                targets = [float(x) for x in self._reference_columns(reference, len(idx))[0]]
                reserved = [1.0 + col + c for c in range(len(idx))]
                col += len(idx)
            for i, tg, rs in zip(idx, targets, reserved):
                rows.append([kind, source, i, weight, tg, group if kind in (KIND_NORM, KIND_QUAD) else 0,
                             1.0 if terminal else 0.0, rs])
        if not rows:
            raise ValueError("cost terms: an empty table (set_cost_terms(None) restores the built-in cost)")
        if len(rows) > MAX_TERMS:
            raise ValueError("cost terms: %d rows, the table holds at most %d" % (len(rows), MAX_TERMS))
        self._quad_groups(engine)       # (a matrix that does not fit its rows is refused here at the latest)
        return np.asarray(rows, np.float64).reshape(-1, ROW_LEN)

    # ------------------------------------------------------------------ internals
    def _add(self, kind, obs, action, index, weight, target, terminal, reference=None, periodic=False, action_rate=None,
             quad=None):
        if (obs is not None) + (action is not None) + (action_rate is not None) != 1:
            raise ValueError("cost term: give exactly one of obs=, action= and action_rate=")
        source = SOURCE_ACTION if action is not None else SOURCE_ACTION_RATE if action_rate is not None else SOURCE_OBS
        block = None
        if source:
            what = "action" if action is not None else "action_rate"
            action = action if action is not None else action_rate
            if isinstance(action, str) and action != "all":
                raise ValueError("unknown %s block %r (an index, a list of indices, True or 'all')" % (what, action))
            if not (action is True or isinstance(action, str)):
                if index is not None:
                    raise ValueError("cost term: %s= already gives the indices; drop index=" % what)
                index = action
        elif isinstance(obs, str):
            block = obs
        else:
            if index is not None:
                raise ValueError("cost term: obs= already gives the indices; drop index=")
            index = obs
        if index is not None:
            index = [int(i) for i in np.atleast_1d(np.asarray(index)).tolist()]
            if not index:
                raise ValueError("cost term: an empty index list")
        weight = float(_finite(weight, "weight"))
        target = _finite(target, "target")
        if target.ndim > 1 or (index is not None and target.ndim == 1 and target.size != len(index)):
            raise ValueError("cost term: target must be a number or one number per index")
        if reference is not None:
            if target.ndim != 0 or float(target) != 0.0:
                raise ValueError("cost term: give a constant target= or a reference=, not both")
            reference = np.array(_finite(reference, "reference"), np.float64)       # (a copy: the caller's array stays theirs)
            if reference.ndim not in (1, 2) or (reference.ndim == 2 and index is not None and reference.shape[1] != len(index)):
                raise ValueError("cost term: reference must be [N] or [N][n_idx] (one column per index), got shape %s"
                                 % (list(reference.shape),))
            if not 1 <= reference.shape[0] <= MAX_REFERENCE_ROWS:
                raise ValueError("cost term: a reference holds 1 .. 2^20 rows, got %d" % reference.shape[0])
            for other in self._terms:
                if other[7] is not None and other[7].shape[0] != reference.shape[0]:
                    raise ValueError("cost terms: the tracked terms of a table share one N; this reference has %d rows, an "
                                     "earlier one %d" % (reference.shape[0], other[7].shape[0]))
            if self._periodic is not None and self._periodic != bool(periodic):
                raise ValueError("cost terms: the tracked terms of a table share one periodic=")
        elif periodic:
            raise ValueError("cost term: periodic= goes with a reference=")
        term = (int(kind), block, index, source, weight, target, bool(terminal), reference, quad)
        if self.engine is not None:
            n_idx = len(self._resolve(term, self.engine)[0])    # refuse now what the engine would refuse later
            if reference is not None:
                self._reference_columns(reference, n_idx)
        self._terms.append(term)
        if self.engine is not None and len(self) > MAX_TERMS:
            self._terms.pop()
            raise ValueError("cost terms: the table holds at most %d rows" % MAX_TERMS)
        if reference is not None:
            self._periodic = bool(periodic)
        return self

    def _resolve(self, term, engine):
        """-> (absolute indices, source, one target per index) of a term, checked against the engine's dimensions (the
        observation's: with the points' and differences' blocks behind it)."""
        _, block, index, source, _, target = term[:6]
        extra = self.n_extra
        if engine is None:
            if block is not None or index is None:
                raise ValueError("cost terms that name a block or take every entry need an engine: CostTerms(engine) or "
                                 "table(engine)")
            lo, n, limit, what = 0, None, None, "action" if source else "observation"
        elif source:
            lo, n, limit, what = 0, _dims(engine)[1], _dims(engine)[1], "action"
        elif block is None:
            lo, n, limit, what = 0, _dims(engine)[0] + extra, _dims(engine)[0] + extra, "observation"
        else:
            layout = engine.obs_layout()
            if extra:
                layout = dict(layout, **self.points_layout(engine))
            if block not in layout:
                raise ValueError("unknown observation block %r (this engine has %s)" % (block, ", ".join(layout)))
            sl = layout[block]
            lo, n, limit, what = sl.start, sl.stop - sl.start, _dims(engine)[0] + extra, "block %r" % block
        idx = list(range(n)) if index is None else index
        for i in idx:
            if i < 0 or (n is not None and i >= n):
                raise ValueError("cost term: index %d outside the %s (%s entries)" % (i, what, n))
        idx = [lo + i for i in idx]
        assert limit is None or all(i < limit for i in idx)
        targets = np.broadcast_to(target, (len(idx),)) if target.ndim == 0 else target
        if len(targets) != len(idx):
            raise ValueError("cost term: target must be a number or one number per index")
        return idx, float(source), [float(x) for x in targets]


_TERM_KEYS = {"kind", "obs", "action", "action_rate", "index", "weight", "target", "terminal", "reference", "repeat",
              "periodic"}
_QUADRATIC_KEYS = _TERM_KEYS | {"matrix", "parts"}
_PART_KEYS = {"obs", "action", "action_rate", "index", "target", "reference"}
_OUTSIDE_KEYS = {"kind", "obs", "action", "action_rate", "index", "weight", "low", "high", "squared", "terminal"}


def _depth(value):
    """Nesting depth of a config list: 0 for a number."""
    d = 0
    while isinstance(value, (list, tuple)):
        if not value:
            raise ValueError("cost_terms: an empty list in a reference")
        value, d = value[0], d + 1
    return d


def _per_episode_reference(value, E):
    """A term's ``reference`` in a config -> its E references if it holds one per episode, else None.  A reference is a
    list of N numbers or of N lists (one number per index); a list of lists of lists is one reference per episode, and so -
    the list-valued ``weight`` / ``target`` rule - is a list of ``E`` lists of numbers in a batch of ``E`` episodes."""
    d = _depth(value)
    if d not in (1, 2, 3):
        raise ValueError("cost_terms: a reference is a list of N numbers or of N lists (or one such list per episode)")
    if d == 3 or (d == 2 and E is not None and len(value) == E):
        if E is None or len(value) != E:
            raise ValueError("cost_terms: a reference per episode holds one reference per episode%s, got %d"
                             % ("" if E is None else " (%d)" % E, len(value)))
        return list(value)
    return None


def _expanded(reference, repeat):
    """``repeat: k``: every entry of the reference holds for k env steps."""
    try:
        ref = np.asarray(reference, np.float64)
    except ValueError as e:
        raise ValueError("cost_terms: a ragged reference: %s" % (e,)) from e
    return np.repeat(ref, repeat, axis=0) if ref.ndim >= 1 else ref


def _per_episode_value(value, E):
    """A term's ``weight`` / ``target`` in a config for a batch of ``E`` episodes -> its E values if it is a list of E entries
    (one per episode: a number, or for ``target`` one number per index), else None (one value for every episode)."""
    return list(value) if E is not None and isinstance(value, (list, tuple)) and len(value) == E else None


def cost_terms_from_config(block, engine, num_episodes=None):
    """A config's ``cost_terms`` block -> ``CostTerms`` for ``engine``:

        cost_terms:
          keep_builtin: false
          terms:
            - {kind: norm, obs: site_minus_target, weight: 5.0}
            - {kind: square, action: 0, weight: 0.001}
            - {kind: square, obs: qvel, weight: 1.0, terminal: true}

    ``num_episodes`` (an episode batch's): a ``weight`` or ``target`` that is a list of ``num_episodes`` entries holds one
    value per episode (a target entry may itself be one number per index) and the result is a list of ``num_episodes``
    ``CostTerms``, one table per episode for ``_EpisodeBatch.set_cost_terms``; without such a list one ``CostTerms`` as ever.
    A ``weight`` list of another length is refused; a ``target`` list of another length is one number per index.

    A term may give ``reference:`` - a list of N numbers or of N lists (one number per index) - in place of ``target``,
    ``repeat: k`` (every entry holds for k env steps, expanded here) and ``periodic:``.  A ``reference`` that is a
    list of references - three levels, or a list of ``num_episodes`` lists of numbers - holds one per episode.

    DESIGN 12.2: ``action_rate:`` stands where ``action:`` may; the kinds ``above``, ``below``, ``above_square`` and
    ``below_square`` take the bound as ``target``; ``{kind: outside, obs: qpos, index: 0, low: -2.0, high: 2.0, weight: 10.0}``
    is ``CostTerms.outside`` (``squared:`` as there; ``weight``, ``low`` and ``high`` may hold one value per episode).

    DESIGN 12.3: ``{kind: quadratic, obs: [0, 1, 2, 3], matrix: [[..], ..], weight: 1.0}`` is ``CostTerms.quadratic``
    (``matrix:`` ``[n][n]`` or ``[n]``; ``parts:`` a list of mappings with ``obs`` / ``action`` / ``action_rate``, ``index``,
    ``target``, ``reference``, as there); ``kind: linear`` takes what ``square`` takes.  ``weight`` (and outside ``parts:``
    ``target`` and ``reference``) may hold one value per episode; the matrix is the batch's.

    DESIGN 12.4: beside ``terms:`` the block may hold ``points:`` - a list of ``{name: tray, body: wrist, pos: [0, 0, 0.02]}`` or
    ``{name: tip, site: finger}`` - and ``differences:`` - ``{name: glass_from_tray, a: glass, b: tray}`` -, defined in that
    order before the terms, which name them like any block; every episode of a batch gets the same ones.

    DESIGN 12.5: ``axes:`` - ``{name: glass_up, body: glass, axis: [0, 0, 1]}`` -, ``velocities:`` - ``{name: glass_vel, point:
    glass}`` - and ``angular_velocities:`` - ``{name: glass_spin, body: glass}`` - stand between ``points:`` and
    ``differences:``, and their blocks in that order: points, axes, velocities, angular velocities, differences.

    DESIGN 12.6: ``coms:`` - ``{name: body_com}`` for the whole model or ``{name: leg_com, body: bthigh}`` for a subtree - and
    ``com_velocities:`` - ``{name: body_vel, com: body_com}`` - stand between ``angular_velocities:`` and ``differences:``.

    DESIGN 12.7: ``orientations:`` - ``{name: pen_err, body: pen, target: [0.707, 0, 0.707, 0]}`` or ``{name: glass_on_tray, body:
    glass, relative_to: wrist}``, optionally ``quat:`` and ``relative_quat:`` - stand between ``com_velocities:`` and
    ``differences:``."""
    if not isinstance(block, dict) or set(block) - {"keep_builtin", "terms", "points", "differences", "axes", "velocities",
                                                     "angular_velocities", "coms", "com_velocities", "orientations"}:
        raise ValueError("cost_terms: expected a mapping with 'terms' and optionally 'keep_builtin', 'points', 'axes', "
                         "'velocities', 'angular_velocities', 'coms', 'com_velocities', 'orientations' and 'differences'")
    orientation_entries = block.get("orientations") or []
    for entry in orientation_entries:
        if not isinstance(entry, dict) or not {"name", "body"} <= set(entry) or set(entry) - {
                "name", "body", "quat", "target", "relative_to", "relative_quat"}:
            raise ValueError("cost_terms: an orientation takes name and body, optionally quat, target, relative_to and "
                             "relative_quat, got %r" % (entry,))
    com_entries, com_velocity_entries = block.get("coms") or [], block.get("com_velocities") or []
    for entry in com_entries:
        if not isinstance(entry, dict) or "name" not in entry or set(entry) - {"name", "body"}:
            raise ValueError("cost_terms: a com takes name and optionally body, got %r" % (entry,))
    for entry in com_velocity_entries:
        if not isinstance(entry, dict) or set(entry) != {"name", "com"}:
            raise ValueError("cost_terms: a com velocity takes name and com, got %r" % (entry,))
    point_entries, difference_entries = block.get("points") or [], block.get("differences") or []
    axis_entries, velocity_entries = block.get("axes") or [], block.get("velocities") or []
    angular_entries = block.get("angular_velocities") or []
    for entry in axis_entries:
        if not isinstance(entry, dict) or set(entry) != {"name", "body", "axis"}:
            raise ValueError("cost_terms: an axis takes name, body and axis, got %r" % (entry,))
    for entry in velocity_entries:
        if not isinstance(entry, dict) or set(entry) != {"name", "point"}:
            raise ValueError("cost_terms: a velocity takes name and point, got %r" % (entry,))
    for entry in angular_entries:
        if not isinstance(entry, dict) or set(entry) != {"name", "body"}:
            raise ValueError("cost_terms: an angular velocity takes name and body, got %r" % (entry,))
    for entry in point_entries:
        if not isinstance(entry, dict) or "name" not in entry or set(entry) - {"name", "body", "site", "pos"}:
            raise ValueError("cost_terms: a point takes name and body or site, optionally pos, got %r" % (entry,))
    for entry in difference_entries:
        if not isinstance(entry, dict) or set(entry) != {"name", "a", "b"}:
            raise ValueError("cost_terms: a difference takes name, a and b, got %r" % (entry,))
    E = None if num_episodes is None else int(num_episodes)
    entries = block.get("terms") or []
    per_episode = False
    for entry in entries:
        outside = isinstance(entry, dict) and entry.get("kind") == "outside"
        keys = _OUTSIDE_KEYS if outside else _QUADRATIC_KEYS if isinstance(entry, dict) and entry.get("kind") == "quadratic" \
            else _TERM_KEYS
        if not isinstance(entry, dict) or set(entry) - keys:
            raise ValueError("cost_terms: a term takes %s, got %r" % (sorted(keys), entry))
        if entry.get("kind") not in KINDS and not outside:
            raise ValueError("cost_terms: unknown kind %r (one of %s, outside)" % (entry.get("kind"), ", ".join(KINDS)))
        if isinstance(entry.get("weight"), (list, tuple)) and _per_episode_value(entry["weight"], E) is None:
            raise ValueError("cost_terms: a list-valued weight holds one weight per episode%s, got %d"
                             % ("" if E is None else " (%d)" % E, len(entry["weight"])))
        per_episode = per_episode or any(_per_episode_value(entry.get(k), E) is not None
                                          for k in ("weight", "target", "low", "high"))
        if "reference" in entry:
            per_episode = per_episode or _per_episode_reference(entry["reference"], E) is not None
            repeat = entry.get("repeat", 1)
            if isinstance(repeat, bool) or not isinstance(repeat, int) or repeat < 1:
                raise ValueError("cost_terms: repeat must be a whole number >= 1, got %r" % (repeat,))
        elif "periodic" in entry and "repeat" not in entry and any(isinstance(p, dict) and "reference" in p
                                                                   for p in entry.get("parts") or []):
            pass                    # (a quadratic whose parts carry the references)
        elif "repeat" in entry or "periodic" in entry:
            raise ValueError("cost_terms: repeat and periodic go with a reference, got %r" % (entry,))
    out = []
    for e in range(E if per_episode else 1):
        terms = CostTerms(engine, keep_builtin=bool(block.get("keep_builtin", False)))
        for entry in point_entries:         # (the same points and differences for every episode)
            terms.point(entry["name"], body=entry.get("body"), site=entry.get("site"), pos=entry.get("pos"))
        for entry in axis_entries:          # 
            terms.axis(entry["name"], body=entry["body"], axis=entry["axis"])
        for entry in velocity_entries:
            terms.velocity(entry["name"], entry["point"])
        for entry in angular_entries:
            terms.angular_velocity(entry["name"], body=entry["body"])
        for entry in com_entries:           # 
            terms.com(entry["name"], body=entry.get("body"))
        for entry in com_velocity_entries:
            terms.com_velocity(entry["name"], entry["com"])
        for entry in orientation_entries:   # 
            terms.orientation(entry["name"], body=entry["body"], quat=entry.get("quat"), target=entry.get("target"),
                              relative_to=entry.get("relative_to"), relative_quat=entry.get("relative_quat"))
        for entry in difference_entries:
            terms.difference(entry["name"], entry["a"], entry["b"])
        for entry in entries:
            kw = {k: entry[k] for k in ("obs", "action", "action_rate", "index", "weight", "target", "terminal", "low", "high",
                                        "squared", "matrix", "parts") if k in entry}
            for k in ("weight", "target", "low", "high"):
                each = _per_episode_value(kw.get(k), E)
                if each is not None:
                    kw[k] = each[e]
            if "reference" in entry:
                each = _per_episode_reference(entry["reference"], E)
                kw["reference"] = _expanded(entry["reference"] if each is None else each[e], entry.get("repeat", 1))
                kw["periodic"] = bool(entry.get("periodic", False))
            elif "periodic" in entry:
                kw["periodic"] = bool(entry["periodic"])
            getattr(terms, entry["kind"])(**kw)
        terms.table()               # (an empty block is refused here)
        out.append(terms)
    return out if per_episode else out[0]
