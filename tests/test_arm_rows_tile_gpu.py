"""GPU: the arm kernels' joint-limit rows and mass-matrix tile in every launch shape, against the FP64 C oracle.

The tile holds the upper triangle of the mass matrix only (one run of stores per link, every reader mirrors the index), and
in the two-wave shape the SOLVE wave evaluates the limit rows itself before the first rendezvous.  Both are exercised where
they can go wrong: one particle group, a partial group and three groups (P = 8, 13, 24), f64 and f32, from three start
states chosen on the CPU from the model's own numbers -
  free      every joint inside its range, the wrist ball clear of the table;
  limit     one joint past its range, moving further into the limit;
  contact   two joints past their ranges AND the wrist ball inside the contact margin of the table
- in each of the four launch shapes (one wave per particle group, two waves with barriers, two and four waves with flags;
a fresh process per shape: the switch is read once per process).  Tolerances: those of tests/test_arm_rollout_gpu.py
(f64: costs 1e-9 relative, observations 1e-9 absolute; f32: costs 2e-3, observations 2e-2 absolute).
Last: one fused two-launch MPPI step (64 x 4) from the contact state against the multi-launch iteration."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 3
SIZES = (8, 13, 24)
SHAPES = {"one_wave": {"MJMPC_ARM_DUO": "0"}, "two_waves": {"MJMPC_ARM_DUO": "1"},
          "flags_two_waves": {"MJMPC_ARM_FLAGS": "2"}, "flags_four_waves": {"MJMPC_ARM_FLAGS": "4"}}


def _rot(axis, a):
    x, y, z = axis
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def _chain(raw, q):
    """World frames of the raw model's bodies (a serial chain, body frames aligned with their parents')."""
    R, p, k, out = np.eye(3), np.zeros(3), 0, []
    for b in raw.bodies:
        p = p + R @ np.asarray(b.pos, float)
        if b.joint is not None:
            R = R @ _rot(b.joint.axis, q[k])
            k += 1
        out.append((R, p))
    return out


def _ball_distance(raw, q):
    """Signed distance of the colliding sphere from the plane (mjc_PlaneSphere), and the margin inside which MuJoCo makes the
    pair a contact (the larger of the two geoms' margins, less the larger gap)."""
    frames = _chain(raw, q)
    (bi, geom), = [(i, g) for i, b in enumerate(raw.bodies) for g in b.geoms if g.collide]
    R, p = frames[bi]
    n = np.asarray(raw.plane.normal, float)
    c = p + R @ np.asarray(geom.a, float)
    return float(n @ (c - np.asarray(raw.plane.pos, float))) - geom.radius, max(raw.plane.margin, geom.margin) - max(raw.plane.gap, geom.gap)


def _ranges(raw):
    r = np.array([b.joint.range for b in raw.bodies if b.joint is not None])
    return r[:, 0], r[:, 1]


@pytest.fixture(scope="module")
def cases(raw_arm, ref_arm):
    """Start states, inputs and the oracle's results - computed once, shared by the four shapes."""
    lo, hi = _ranges(raw_arm)
    tgt = np.array([0.2, -0.1, -0.25])
    free = dict(qp=np.array([0.3, 0.5, -0.2, -1.0, 0.4, -0.6, 0.2]), qv=np.array([0.5, -1.0, 0.3, 2.0, -0.5, 1.0, 0.1]))
    # joint 2 (upper-arm roll) 0.03 rad beyond its upper bound, turning further into it
    limit = dict(qp=free["qp"].copy(), qv=free["qv"].copy())
    limit["qp"][2] = hi[2] + 0.03
    limit["qv"][2] = 2.0
    # elbow and wrist flex just beyond their upper bounds (an almost straight arm), the shoulder lifted down until the
    # wrist ball is half a millimetre INTO the table: bisection on the lift angle
    qc = np.array([0.2, 0.0, 0.1, hi[3] + 0.02, -0.1, hi[5] + 0.015, 0.3])

    def dist(a):
        q = qc.copy()
        q[1] = a
        return _ball_distance(raw_arm, q)[0]
    a, b = 0.0, hi[1] - 0.05
    assert dist(a) > 0.0 > dist(b)
    for _ in range(60):
        m = 0.5 * (a + b)
        a, b = (m, b) if dist(m) > -5e-4 else (a, m)
    qc[1] = a
    contact = dict(qp=qc, qv=np.array([0.0, 0.4, 0.0, 1.0, 0.0, 0.5, 0.0]))
    states = [free, limit, contact]
    # the hand-written kinematics above agree with the oracle's (the site sits at the origin of the ball's body)
    for st in states:
        np.testing.assert_allclose(_chain(raw_arm, st["qp"])[raw_arm.site_body][1] + 0.0, ref_arm.site(st["qp"]), atol=1e-12)
    # ... and the states are what they are meant to be
    out_lo = [st["qp"] < lo for st in states]
    out_hi = [st["qp"] > hi for st in states]
    d = [_ball_distance(raw_arm, st["qp"]) for st in states]
    assert not out_lo[0].any() and not out_hi[0].any() and d[0][0] > d[0][1] + 0.01
    assert not out_lo[1].any() and list(np.flatnonzero(out_hi[1])) == [2] and limit["qv"][2] > 0 and d[1][0] > d[1][1] + 0.01
    assert not out_lo[2].any() and list(np.flatnonzero(out_hi[2])) == [3, 5] and d[2][0] < d[2][1] and d[2][0] < 0.0
    rs = np.random.RandomState(41)
    data = {"target": tgt}
    for dt in ("f64", "f32"):
        mean = 0.3 * rs.standard_normal((H, 7))
        noise = rs.standard_normal((max(SIZES), H, 7))
        if dt == "f32":         # identical inputs to both sides
            mean, noise = mean.astype(np.float32).astype(np.float64), noise.astype(np.float32).astype(np.float64)
        data["mean_" + dt], data["noise_" + dt] = mean, noise
    ref = {}
    for si, st in enumerate(states):
        data["qp%d" % si], data["qv%d" % si] = st["qp"], st["qv"]
        for dt in ("f64", "f32"):
            for P in SIZES:
                o_obs, o_rew, o_act, _, o_nobs = ref_arm.rollout(st["qp"], st["qv"], tgt, data["mean_" + dt], data["noise_" + dt][:P])
                ref[si, dt, P] = (o_rew, o_act, o_obs, o_nobs)
    assert ref_arm.newton_stats()["calls"] > 0          # rows really were active on the oracle's side
    return data, ref


CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
from mjmpc_amd.models.reacher7dof import reacher7dof_raw
d = np.load(sys.argv[1])
out = {}
for dt in ("f64", "f32"):
    eng = ArmRolloutEngine(reacher7dof_raw(), dtype=dt)
    for si in range(3):
        eng.set_env_state(dict(qp=d["qp%%d" %% si], qv=d["qv%%d" %% si], qa=np.zeros(7), target_pos=d["target"], timestep=0))
        for P in %r:
            obs, rew, act, done, info, nobs = eng.rollout(P, %d, d["mean_" + dt], d["noise_" + dt][:P], "open_loop")
            k = "%%d_%%s_%%d_" %% (si, dt, P)
            out[k + "rew"], out[k + "act"], out[k + "obs"], out[k + "nobs"] = rew, act, obs, nobs
    out["failures_" + dt] = np.array(eng.solver_failures())
np.savez(sys.argv[2], **out)
""" % (ROOT, SIZES, H)


_RUNS = {}       # shape -> what its child process computed (each shape runs once per session)


def _run(shape, data, tmp_path_factory):
    if shape not in _RUNS:
        tmp = tmp_path_factory.mktemp("rows_tile_" + shape)
        script, inp, outp = tmp / "run.py", str(tmp / "in.npz"), str(tmp / "out.npz")
        script.write_text(CHILD)
        np.savez(inp, **data)
        env = {k: v for k, v in os.environ.items() if k not in ("MJMPC_ARM_DUO", "MJMPC_ARM_FLAGS", "MJMPC_ARM_ONE")}
        subprocess.run([sys.executable, str(script), inp, outp], check=True, timeout=300, env=dict(env, **SHAPES[shape]))
        with np.load(outp) as f:
            _RUNS[shape] = {k: f[k] for k in f.files}
    return _RUNS[shape]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_rollouts_match_the_oracle_in_every_shape(cases, tmp_path_factory, shape):
    data, ref = cases
    got = _run(shape, data, tmp_path_factory)
    assert int(got["failures_f64"]) == 0 and int(got["failures_f32"]) == 0
    for (si, dt, P), (o_rew, o_act, o_obs, o_nobs) in ref.items():
        k = "%d_%s_%d_" % (si, dt, P)
        rew, act, obs, nobs = got[k + "rew"], got[k + "act"], got[k + "obs"], got[k + "nobs"]
        what = "state %d, %s, P = %d, %s" % (si, dt, P, shape)
        if dt == "f64":
            assert np.array_equal(act, o_act), what
            np.testing.assert_allclose(rew, o_rew, rtol=1e-9, atol=1e-9, err_msg=what)
            np.testing.assert_allclose(nobs, o_nobs, rtol=0, atol=1e-9, err_msg=what)
            np.testing.assert_allclose(obs, o_obs, rtol=0, atol=1e-9, err_msg=what)
        else:
            # (actions: mean + noise, both exact in f32, added in f32 - one rounding of the sum)
            assert np.abs(act - o_act).max() <= 2.0 ** -23 * np.abs(o_act).max(), what
            assert np.abs(rew - o_rew).max() < 2e-3, what
            assert np.abs(nobs - o_nobs).max() < 2e-2, what
            assert np.abs(obs - o_obs).max() < 2e-2, what


def test_the_switches_select_different_kernels(cases, tmp_path_factory):
    """The shapes are chosen through the environment alone: if a later change to the launch logic made them collapse onto one
    kernel, the test above would compare one program with the oracle four times.  The one-wave kernel (LDL^T solves on the
    solver lanes) and the multi-wave kernels (explicit inverses, one column per lane) are algebraically different programs:
    on rollouts with active rows their f64 costs agree to 1e-9 (above) but not in every bit.  (The multi-wave shapes form the
    same sums in the same order and cannot be told apart this way.)"""
    data, _ = cases
    one = _run("one_wave", data, tmp_path_factory)
    keys = [k for k in one if k.endswith("_rew") and "_f64_" in k]
    assert keys
    for shape in ("two_waves", "flags_two_waves", "flags_four_waves"):
        other = _run(shape, data, tmp_path_factory)
        assert any(not np.array_equal(one[k], other[k]) for k in keys), shape


def test_fused_step_equals_the_multi_launch_step(cases):
    """One control step of MPPI 64 x 4 from the contact state: rollout launch + finish launch (whose workgroup 0 steps the
    real arm in the two-wave roles) against sampler, rollout, update and env-step launches."""
    import torch
    from mjmpc_amd.control import MPPI
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    data, _ = cases
    res = []
    for mono in (True, False):
        eng = ArmRolloutEngine(reacher7dof_raw(), dtype="f64")
        eng.set_env_state(dict(qp=data["qp2"], qv=data["qv2"], target_pos=data["target"]))
        c = MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=7, horizon=4, init_cov=0.6, base_action="null", lam=0.05,
                 num_particles=64, step_size=0.9, alpha=1, gamma=0.98, n_iters=1, action_lows=eng.action_lows,
                 action_highs=eng.action_highs, filter_coeffs=[0.25, 0.8, 0.0], seed=11, noise_mode="device", noise_dtype="f64")
        c.rollout_fn = make_device_rollout_fn(eng)
        c.set_sim_state_fn = lambda s: None
        c.enable_graph(post_step=eng.step_state, mono=mono)
        action = np.array(c.optimize({})[0])
        torch.cuda.synchronize()
        assert bool(c._mono) == mono and not getattr(c, "graph_fallback", False)
        _, nobs = eng.step_state(np.zeros(7))
        res.append((action, c.mean_action.copy(), nobs.cpu().numpy()))
        assert eng.solver_failures() == 0
    (a1, m1, o1), (a0, m0, o0) = res
    assert np.abs(a1).max() > 0
    np.testing.assert_allclose(a1, a0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(m1, m0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(o1, o0, rtol=0, atol=1e-8)
