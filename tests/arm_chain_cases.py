"""Random hinge chains for the PLAIN build of the arm kernels (csrc/arm_rollout.hip without MJMPC_ARM_XJ), shared by
tests/test_arm_chains_cpu.py and tests/test_arm_chains_gpu.py.  Not a test file.

``hinge_chain_xml(seed)`` draws a serial chain of 1..7 hinges - no slide joint and no dry friction, so ``compile_arm`` leaves
``jtype`` and ``frictionloss`` all zero and the engine takes the plain build - and varies what the suite's two models on that
build (sawyer.xml, the two-link arm) hold fixed: nv, nu <= nv, unlimited joints beside limited ones, gravity in any direction,
body frames rotated against their parents, link offsets along no axis, inertia that is not symmetric about the link, with and
without the contact sphere, solimp powers 1..4, solref time constants on both sides of the refsafe clamp 2 * timestep.
``states`` draws start states for one-step checks, a share of them steered (on the CPU, with the oracle's kinematics and the
model's own numbers) past a joint limit or into the floor's contact margin."""
import copy
import functools

import numpy as np

SEEDS = range(24)               # the suite's chains
N_STATES = 24
TIP_RADIUS = 0.04
# what the GPU file runs on a few chains only (tests/test_arm_chains_cpu.py checks that they are what they are picked for)
SIZE_SEEDS = (2, 5, 7, 9)       # launch shapes chosen by size, f32, the real-env step: nv 1, 4, 5, 7; floors; nu < nv
CL_SEEDS = (0, 7, 10)           # closed-loop-linear mode: nu < nv or nv < 7
MONO_SEEDS = (0, 5, 9)          # the fused MPPI iteration: A = nu = 1, 3, 5
BATCH_SEEDS = (5, 9)            # episode batches: nv 4 with nu 3, and nv 7
OWN_SET_SEED = 5                # a floor and limited joints: the model that gets per-element solver sets


def _unit(rs, n=3):
    x = rs.standard_normal(n)
    return x / np.linalg.norm(x)


def _rot(axis, a):
    x, y, z = axis
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def _quat2mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _descend(height, q, lo, hi, stop):
    """Coordinate steps downhill on ``height`` inside [lo, hi], halving from 0.5 rad to 1 mrad; ends early below ``stop``."""
    low, h_low, step = q.copy(), height(q), 0.5
    while step > 1e-3 and h_low > stop:
        moved = False
        for j in range(q.size):
            for sgn in (1.0, -1.0):
                trial = low.copy()
                trial[j] = min(max(trial[j] + sgn * step, lo[j]), hi[j])
                h = height(trial)
                if h < h_low:
                    low, h_low, moved = trial, h, True
        if not moved:
            step *= 0.5
    return low, h_low


def _can_reach(rs, links, tip, z):
    """Whether the tip of the drawn links (body position, quaternion, joint axis, range each) gets below height ``z`` with every
    joint inside its range: descents from the drawn pose and from five random ones."""
    fixed = [(pos, _quat2mat(quat)) for pos, quat, _, _ in links]
    lo, hi = np.array([r[0] for _, _, _, r in links]), np.array([r[1] for _, _, _, r in links])

    def height(q):
        R, p = np.eye(3), np.zeros(3)
        for (pos, Rq), (_, _, ax, _), a in zip(fixed, links, q):
            p = p + R @ pos
            R = R @ Rq @ _rot(ax, a)
        return (p + R @ tip)[2]
    starts = [np.zeros(len(links))] + [rs.uniform(lo, hi) for _ in range(5)]
    return any(_descend(height, q0, lo, hi, z)[1] < z for q0 in starts)


@functools.lru_cache(maxsize=None)
def hinge_chain_xml(seed):
    """(xml, nv, nu) of chain ``seed``; everything is drawn from ``RandomState(seed)``: nv in 1..7, motors on the first nu <= nv
    joints (gear 2..20, asymmetric ctrlrange), hinges about random axes (40 % a coordinate axis; 60 % limited), bodies with a
    random quaternion (30 % identity) placed at the previous link's tip, one capsule per link and - 40 % - a lump beside it,
    gravity down / none / 9.81 in a random direction, timestep 0.002 / 0.005 / 0.01, one model-wide solver set (timeconst
    0.004..0.05, solimp inside MuJoCo's clamp, power 1..4), a tip sphere that - 50 % - collides with a floor at
    -0.5 * reach - 0.05.  With a floor, the links are drawn until the tip can reach it (``_can_reach``)."""
    rs = np.random.RandomState(seed)
    nv = int(rs.randint(1, 8))
    nu = int(rs.randint(1, nv + 1))
    gkind = int(rs.randint(3))
    gdir = _unit(rs)
    grav = ((0.0, 0.0, -9.81), (0.0, 0.0, 0.0), tuple(9.81 * gdir))[gkind]
    floor = rs.rand() < 0.5
    floor_margin = rs.uniform(0.0, 0.004)
    dt = float(rs.choice([0.002, 0.005, 0.01]))
    solref = "%.5f %.4f" % (rs.uniform(0.004, 0.05), rs.uniform(0.7, 1.5))
    solimp = "%.4f %.4f %.5f %.4f %d" % (rs.uniform(0.7, 0.92), rs.uniform(0.93, 0.99), rs.uniform(0.0005, 0.01),
                                         rs.uniform(0.3, 0.7), int(rs.choice([1, 2, 2, 3, 4])))
    while True:
        body, close, links = "", "", []
        tip, reach = np.zeros(3), 0.0
        for k in range(nv):
            ax = _unit(rs)
            coord = np.eye(3)[rs.randint(3)]
            if rs.rand() < 0.4:
                ax = coord
            quat = _unit(rs, 4)
            if rs.rand() < 0.3:
                quat = np.array([1.0, 0.0, 0.0, 0.0])
            length = rs.uniform(0.12, 0.35)
            pos, tip = tip, _unit(rs) * length
            reach += length
            lim = rs.rand() < 0.6
            rng = (rs.uniform(-2.0, -0.2), rs.uniform(0.2, 2.0))
            links.append((pos, quat, ax, rng if lim else (-np.pi, np.pi)))
            body += ('<body name="b%d" pos="%.6f %.6f %.6f" quat="%.8f %.8f %.8f %.8f">'
                     '<joint name="j%d" type="hinge" axis="%.8f %.8f %.8f" damping="%.4f" armature="%.5f"%s/>'
                     '<geom type="capsule" fromto="0 0 0 %.6f %.6f %.6f" size="%.4f" density="%.1f"/>'
                     % (k, pos[0], pos[1], pos[2], quat[0], quat[1], quat[2], quat[3], k, ax[0], ax[1], ax[2],
                        rs.uniform(0.02, 0.5), rs.uniform(0.0, 0.02),
                        (' limited="true" range="%.4f %.4f"' % rng) if lim else ' limited="false"',
                        tip[0], tip[1], tip[2], rs.uniform(0.02, 0.05), rs.uniform(300, 1500)))
            lump, lump_pos, lump_r, lump_rho = rs.rand() < 0.4, 0.06 * _unit(rs) + 0.5 * tip, rs.uniform(0.02, 0.04), rs.uniform(500, 3000)
            if lump:        # off the link's line: the link's inertia is not symmetric about it
                body += '<geom type="sphere" pos="%.6f %.6f %.6f" size="%.4f" density="%.1f"/>' % (
                    lump_pos[0], lump_pos[1], lump_pos[2], lump_r, lump_rho)
            close += "</body>"
        # a floor that the chain cannot touch inside its joints' ranges would leave the contact row dead in every state: with
        # a floor, the links are drawn again (same stream) until the tip sphere can sink 3 cm into it
        if not floor or _can_reach(rs, links, tip, -0.5 * reach - 0.05 + TIP_RADIUS - 0.03):
            break
    body += ('<geom name="tip" type="sphere" pos="%.6f %.6f %.6f" size="%g" %s/><site name="finger" pos="%.6f %.6f %.6f"/>'
             % (tip[0], tip[1], tip[2], TIP_RADIUS, 'contype="1" conaffinity="1"' if floor else "", tip[0], tip[1], tip[2]))
    acts = "".join('<motor joint="j%d" gear="%.3f" ctrlrange="%.4f %.4f" ctrllimited="true"/>'
                   % (k, rs.uniform(2, 20), -rs.uniform(0.5, 1.0), rs.uniform(0.5, 1.0)) for k in range(nu))
    target = _unit(rs) * rs.uniform(0.2, 0.8) * reach
    plane = ('<geom name="floor" type="plane" pos="0 0 %.5f" size="3 3 0.1" margin="%.5f" contype="1" conaffinity="1" condim="1"/>'
             % (-0.5 * reach - 0.05, floor_margin)) if floor else ""
    xml = ('<mujoco><compiler angle="radian" coordinate="local" inertiafromgeom="true"/>'
           '<option timestep="%g" gravity="%.6f %.6f %.6f" integrator="Euler"/>'
           '<default><joint solreflimit="%s" solimplimit="%s"/>'
           '<geom contype="0" conaffinity="0" condim="1" solref="%s" solimp="%s"/></default>'
           '<worldbody><site name="target" pos="%.5f %.5f %.5f"/>%s%s%s</worldbody><actuator>%s</actuator></mujoco>'
           % (dt, grav[0], grav[1], grav[2], solref, solimp, solref, solimp, target[0], target[1], target[2], plane, body, close, acts))
    return xml, nv, nu


def own_solver_set_xmls(seed):
    """Chain ``seed`` with a solver set of its own on the colliding sphere / on its first limited joint: what ``compile_arm``
    must refuse (the arm kernels carry the model-wide set only)."""
    xml = hinge_chain_xml(seed)[0]
    geom = xml.replace('<geom name="tip"', '<geom name="tip" solref="0.05 0.5"')
    k = xml.index(' limited="true"')
    joint = xml[:k] + ' solreflimit="0.05 0.5"' + xml[k:]
    assert geom != xml and joint != xml
    return dict(geom=geom, joint=joint)


def load_chain(seed, folder):
    """The chain's RawModel (``folder``: where its XML may be written)."""
    import os
    from mjmpc_amd.models.mjcf import load_mjcf
    path = os.path.join(str(folder), "chain%d.xml" % seed)
    with open(path, "w") as f:
        f.write(hinge_chain_xml(seed)[0])
    return load_mjcf(path, frame_skip=2)


def gravity_kind(raw):
    g = np.asarray(raw.gravity, float)
    return "none" if not g.any() else ("down" if not g[:2].any() else "tilted")


def without_limits(raw):
    """Twin model: every joint unlimited."""
    twin = copy.deepcopy(raw)
    for j in twin.joints:
        j.limited = False
    return twin


def without_floor(raw):
    """Twin model: no plane, so nothing collides."""
    twin = copy.deepcopy(raw)
    twin.plane = None
    return twin


def floor_gap(raw, ref, q):
    """(distance of the tip sphere from the floor, the margin below which the pair is a contact)."""
    g, = [g for b in raw.bodies for g in b.geoms if g.collide]
    n = np.asarray(raw.plane.normal, float)
    d = float(n @ (ref.site(q) - np.asarray(raw.plane.pos, float))) / float(np.linalg.norm(n)) - g.radius
    return d, max(raw.plane.margin, g.margin) - max(raw.plane.gap, g.gap)


def _into_the_floor_band(raw, ref, rs, q):
    """A pose whose tip sphere lies at a distance drawn from [-0.02, margin) of the floor.  Plain rejection on
    qpos0 + 1.5 U(-1, 1) almost never accepts for the long chains (a 2 cm slab of a reach of a metre and more), so each draw
    is followed downhill - coordinate steps on the tip's height, halving - and the pose is taken on the segment from the draw
    to the low point, by bisection on the distance.  Every pose on the way stays inside the joints' ranges (beyond them the
    limit rows push the arm off the floor harder than the contact would, and the contact row carries no force).  Draws already
    below the band, or whose descent ends above it, are rejected; after 64 of them (a floor the chain cannot reach) the first
    draw stands."""
    first = q
    lo = np.array([j.range[0] if j.limited else -np.pi for j in raw.joints])
    hi = np.array([j.range[1] if j.limited else np.pi for j in raw.joints])

    def height(x):
        return floor_gap(raw, ref, x)[0]
    margin = floor_gap(raw, ref, q)[1]
    for _ in range(64):
        q = np.clip(q, lo, hi)
        want = rs.uniform(-0.02, margin)
        if height(q) > want:
            low, d_low = _descend(height, q, lo, hi, -0.03)
            if d_low < want:
                a, b = 0.0, 1.0             # distance(a) > want > distance(b)
                for _ in range(60):
                    m = 0.5 * (a + b)
                    a, b = (m, b) if height(q + m * (low - q)) > want else (a, m)
                out = q + b * (low - q)
                if -0.02 <= height(out) < margin:
                    return out
        q = raw.qpos0 + 1.5 * rs.uniform(-1, 1, q.size)
    return first


def states(raw, ref, seed, n=N_STATES):
    """``n`` (q, v, u) triples for one-step checks of chain ``seed`` (``ref``: its RefArm, used for the tip's position only).
    q = qpos0 + 1.5 U(-1, 1); v at rest / creeping / moving by k % 4; u beyond the control range, so the clamp acts.  Steered:
    with a floor, every third state is redrawn until the tip sphere lies within [-0.02, margin) of the plane
    (``_into_the_floor_band``) and its velocity is turned towards the floor; with a limited joint, states 1, 7, 13, 19 put one limited joint up to 0.1 rad past one of its
    bounds."""
    rs = np.random.RandomState(5000 + seed)
    nv, nu = raw.nv, len(raw.actuators)
    limited = [k for k, j in enumerate(raw.joints) if j.limited]
    floor = raw.plane is not None and any(g.collide for b in raw.bodies for g in b.geoms)
    out = []
    for k in range(n):
        q = raw.qpos0 + 1.5 * rs.uniform(-1, 1, nv)
        v = rs.standard_normal(nv) * (0.0 if k % 4 == 0 else (0.03 if k % 4 == 1 else 2.0))
        u = rs.uniform(-1.3, 1.3, nu)
        if floor and k % 3 == 0:
            q = _into_the_floor_band(raw, ref, rs, q)
            if floor_gap(raw, ref, q + 1e-6 * v)[0] > floor_gap(raw, ref, q)[0]:
                v = -v                  # towards the floor: a tip that leaves fast enough gets no force from the contact row
        elif limited and k % 6 == 1:
            j = limited[rs.randint(len(limited))]
            lo, hi = raw.joints[j].range
            q[j] = hi + rs.uniform(0.0, 0.1) if rs.rand() < 0.5 else lo - rs.uniform(0.0, 0.1)
        out.append((q, v, u))
    return out


def filtered_noise(rs, P, H, nu, scale=0.4):
    eps = scale * rs.standard_normal((P, H, nu))
    for t in range(2, H):
        eps[:, t] = 0.25 * eps[:, t] + 0.8 * eps[:, t - 1]
    return eps


def rollout_case(raw, seed, P=40, H=4):
    """(q, v, mean, noise) of the short rollouts: one start state, a random mean, filtered noise scaled 0.4."""
    rs = np.random.RandomState(7000 + seed)
    nv, nu = raw.nv, len(raw.actuators)
    q = raw.qpos0 + 0.6 * rs.uniform(-1, 1, nv)
    v = 0.5 * rs.standard_normal(nv)
    mean = 0.3 * rs.standard_normal((H, nu))
    return q, v, mean, filtered_noise(rs, P, H, nu)
