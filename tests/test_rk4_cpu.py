"""CPU: MuJoCo's RK4 integrator (<option integrator="RK4">) through the model layer - the loader reads it, the exporter
writes it, the arm compiler refuses it (so that make_engine sends RK4 models to the tree engine), the tree compiler carries
it and refuses what its RK4 kernels do not run - and the composed reference of tests/rk4_ref.py is RK4: exact on a linear
model, fifth-order local error on a nonlinear one."""
import numpy as np
import pytest

from mjmpc_amd.models.compile import compile_arm
from mjmpc_amd.models.compile_tree import compile_tree
from mjmpc_amd.models.export_mjcf import to_mjcf
from mjmpc_amd.models.mjcf import load_mjcf
from mjmpc_amd.models.synthetic import synthetic_raw

_PENDULUM = """<mujoco model="rk4_pendulum">
  <compiler angle="radian" coordinate="local" inertiafromgeom="true"/>
  <option timestep="%s" gravity="0 0 %s" integrator="%s"/>
  <default><geom contype="0" conaffinity="0" density="1000"/></default>
  <worldbody>
    <site name="target" pos="0 0 1"/>
    <body name="bob" pos="0 0 0">
      <joint name="j" type="%s" axis="%s" stiffness="%s" damping="%s" armature="%s"/>
      <geom name="g" type="capsule" fromto="0 0 0 0 0 0.5" size="0.05"/>
      <site name="finger" pos="0 0 0.5"/>
    </body>
  </worldbody>
  <actuator><motor joint="j" gear="1" ctrlrange="-1 1"/></actuator>
</mujoco>
"""


def _model(tmp_path, integrator="RK4", timestep=0.01, gravity=-9.81, jtype="hinge", axis="0 1 0", k=0.0, b=0.0, arm=0.0):
    p = tmp_path / ("m_%s_%s.xml" % (integrator, timestep))
    p.write_text(_PENDULUM % (timestep, gravity, integrator, jtype, axis, k, b, arm))
    return load_mjcf(str(p), frame_skip=1)


def test_loader_reads_rk4_and_refuses_the_rest(tmp_path):
    assert _model(tmp_path, "RK4").integrator == "RK4"
    assert _model(tmp_path, "Euler").integrator == "Euler"
    assert synthetic_raw("double_pendulum").integrator == "RK4"
    assert synthetic_raw("cartpole").integrator == "Euler"
    for bad in ("implicit", "implicitfast", "rk4", "Verlet"):
        with pytest.raises(ValueError, match="supported: Euler, RK4"):
            _model(tmp_path, bad)


def test_export_round_trips_the_integrator(tmp_path):
    for name in ("double_pendulum", "cartpole"):
        raw = synthetic_raw(name)
        p = tmp_path / (name + ".xml")
        p.write_text(to_mjcf(raw))
        back = load_mjcf(str(p), frame_skip=raw.frame_skip)
        assert back.integrator == raw.integrator
        np.testing.assert_array_equal(back.to_flat(), raw.to_flat())


def test_arm_compiler_refuses_rk4_and_tree_compiler_carries_it():
    raw = synthetic_raw("cartpole")
    compile_arm(raw)                                # (Euler: the arm kernels run the cart-pole)
    raw.integrator = "RK4"
    with pytest.raises(ValueError, match="RK4: the tree engine"):
        compile_arm(raw)
    tm = compile_tree(raw)
    assert tm.integrator == "RK4"
    euler = compile_tree(synthetic_raw("cartpole"))
    assert euler.integrator == "Euler"
    np.testing.assert_array_equal(tm.blob, euler.blob)     # (the integrator is not in the blob)
    assert compile_tree(synthetic_raw("double_pendulum")).integrator == "RK4"


def test_tree_compiler_refuses_rk4_beyond_its_kernels():
    from mjmpc_amd.models.hand24 import hand24_raw
    raw = synthetic_raw("gripper")                  # (elliptic cones: GEN = 3)
    assert raw.cone == "elliptic"
    compile_tree(raw)
    raw.integrator = "RK4"
    with pytest.raises(ValueError, match="elliptic"):
        compile_tree(raw)
    raw.cone = "pyramidal"
    assert compile_tree(raw).integrator == "RK4"
    hand = hand24_raw()
    assert hand.nv > 16
    hand.integrator = "RK4"
    with pytest.raises(ValueError, match="up to 16 dofs"):
        compile_tree(hand)


def test_composed_step_is_rk4_on_a_linear_model(tmp_path):
    """One slide dof with spring and damper, no gravity: one step = P(hA) [q; v], P(Z) = I + Z + Z^2/2 + Z^3/6 + Z^4/24."""
    from oracle.physics_ref import RefArm
    from rk4_ref import rk4_step
    k, b, arm, h = 30.0, 0.7, 0.05, 0.02
    raw = _model(tmp_path, timestep=h, gravity=0.0, jtype="slide", axis="1 0 0", k=k, b=b, arm=arm)
    ref = RefArm(raw.to_flat())
    m = ref.mass_matrix(np.zeros(1))[0, 0]          # (the body's mass plus the armature)
    assert m > arm
    A = np.array([[0.0, 1.0], [-k / m, -b / m]])
    Z = h * A
    P = np.eye(2) + Z + Z @ Z / 2 + Z @ Z @ Z / 6 + Z @ Z @ Z @ Z / 24
    for x0 in ([0.1, 0.0], [-0.03, 1.5], [0.2, -0.4]):
        q, v, _, _, _, n = rk4_step(ref, raw, [x0[0]], [x0[1]], [0.0])
        assert n == 0
        np.testing.assert_allclose([q[0], v[0]], P @ np.array(x0), rtol=0, atol=1e-12)


def test_composed_step_has_fifth_order_local_error(tmp_path):
    """A pendulum: the one-step error against a fine-step reference falls by about 2^5 when h halves (Euler's by 2^2)."""
    from oracle.physics_ref import RefArm
    from rk4_ref import rk4_step
    q0, v0 = np.array([1.0]), np.array([0.5])

    def rk4_run(h, n):
        raw = _model(tmp_path, timestep=h)
        ref = RefArm(raw.to_flat())
        q, v = q0, v0
        for _ in range(n):
            q, v, _, _, _, _ = rk4_step(ref, raw, q, v, [0.0])
        return np.r_[q, v]

    def euler_step(h):
        raw = _model(tmp_path, "Euler", timestep=h)
        q, v, _, _ = RefArm(raw.to_flat()).step(q0, v0, [0.0])
        return np.r_[q, v]

    hs = (0.04, 0.02, 0.01)
    exact = {h: rk4_run(h / 64, 64) for h in hs}
    e_rk4 = [np.abs(rk4_run(h, 1) - exact[h]).max() for h in hs]
    e_eul = [np.abs(euler_step(h) - exact[h]).max() for h in hs]
    for a, b in zip(e_rk4, e_rk4[1:]):
        assert 20.0 < a / b < 45.0, e_rk4
    for a, b in zip(e_eul, e_eul[1:]):
        assert a / b < 6.0, e_eul
    assert e_rk4[-1] < 1e-3 * e_eul[-1]
