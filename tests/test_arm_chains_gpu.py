"""GPU: random hinge chains (tests/arm_chain_cases.py) on the PLAIN build of the arm kernels, against oracle/reacher_ref.c in
every shape that build launches.

The plain build (csrc/arm_rollout.hip without MJMPC_ARM_XJ) is the headline kernel and met two models in the suite: sawyer.xml
and a two-link arm.  The chains vary what those hold fixed - nv 1..7, nu <= nv (so A != 7 in the fused iteration's action
tile), unlimited joints beside limited ones, gravity in any direction, rotated body frames, oblique link offsets, with and
without the contact sphere, solimp powers 1..4, solref time constants below 2 * timestep - and run through
  a. the four launch shapes a switch selects (one wave per particle group, two waves with barriers, two and four waves with
     flags; a fresh process per shape: the switches are read once per process): 24 one-step checks and 4-step rollouts at
     P = 8, 13, 40 per chain;
  b. the shapes the launch chooses by size (P = 2061, 4104, 8200);      c. f32, with its three-waves-per-SIMD instantiation;
  d. the real-env step (STEP twins);      e. closed-loop-linear mode (CL);      f. the fused two-launch MPPI iteration (MONO);
  g. episode batches (EB twins);      h. the tree engine on the same inputs;
and the default process once per chain (one-step checks and the 40 x 4 rollout), which MJMPC_CHAIN_SEEDS=a:b turns into a soak
over another seed range (not part of the suite).
Tolerances are the project's: one env step 1e-9 relative (tests/test_arm_xj_random_gpu.py), short rollouts rtol 1e-8 and atol
1e-8 * max(1, |obs|max) (same file), actions bit-equal, no solver failure; f32 as tests/test_arm_xj_gpu.py::test_f32_stays_close.
Last: a model with per-element solver sets goes to the tree engine (``compile_arm`` refuses it) and matches the oracle there."""
import os
import subprocess
import sys

import numpy as np
import pytest

import arm_chain_cases as ac

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 4
SIZES = (8, 13, 40)
SHAPES = {"one_wave": {"MJMPC_ARM_DUO": "0"}, "two_waves": {"MJMPC_ARM_DUO": "1"},
          "flags_two_waves": {"MJMPC_ARM_FLAGS": "2"}, "flags_four_waves": {"MJMPC_ARM_FLAGS": "4"}}
_SOAK = os.environ.get("MJMPC_CHAIN_SEEDS")
DEFAULT_PROCESS_SEEDS = range(*[int(x) for x in _SOAK.split(":")]) if _SOAK else ac.SEEDS


def _one_step_error(nobs, rew, o1, r1):
    return max(np.abs(nobs - o1).max() / max(1.0, np.abs(o1).max()), abs(rew - r1) / max(1.0, abs(r1)))


def _check_rollout(got, want, what):
    """(rew, act, nobs) of the kernel against the oracle's at the rollout tolerance -> worst error relative to the scale."""
    (rew, act, nobs), (o_rew, o_act, o_nobs) = got, want
    assert np.array_equal(act, o_act), what
    scale = max(1.0, np.abs(o_nobs).max())
    np.testing.assert_allclose(nobs, o_nobs, rtol=1e-8, atol=1e-8 * scale, err_msg=what)
    np.testing.assert_allclose(rew, o_rew, rtol=1e-8, atol=1e-8 * scale, err_msg=what)
    return max(np.abs(nobs - o_nobs).max(), np.abs(rew - o_rew).max()) / scale


class Chain:
    """One chain with everything the oracle says about it, computed once: the one-step results from ``states`` and the
    40 x 4 rollout (P = 8 and 13 are its first rows: a particle's result does not depend on the population)."""

    def __init__(self, seed, folder):
        from oracle.physics_ref import RefArm
        self.seed, self.raw = seed, ac.load_chain(seed, folder)
        self.ref = RefArm(self.raw.to_flat())
        self.nv, self.nu = self.raw.nv, len(self.raw.actuators)
        self.tgt = np.asarray(self.raw.target_pos, float)
        self.states = ac.states(self.raw, self.ref, seed)
        steps = [self.ref.env_step(q, v, u, self.tgt) for q, v, u in self.states]
        self.o1, self.r1 = np.array([s[3] for s in steps]), np.array([s[2] for s in steps])
        assert np.isfinite(self.o1).all()
        self.q, self.v, self.mean, self.noise = ac.rollout_case(self.raw, seed, max(SIZES), H)
        _, rew, act, _, nobs = self.ref.rollout(self.q, self.v, self.tgt, self.mean, self.noise)
        self.rollout = (rew, act, nobs)
        assert self.ref.newton_stats()["fails"] == 0 and self.ref.resets() == 0

    def state(self, k=None):
        q, v = (self.q, self.v) if k is None else self.states[k][:2]
        return dict(qp=q, qv=v, target_pos=self.tgt)

    def describe(self):
        return "chain %d (nv %d nu %d, %s gravity, %s, power %d)" % (
            self.seed, self.nv, self.nu, ac.gravity_kind(self.raw), "floor" if self.raw.plane is not None else "no floor",
            int(self.raw.solimp[4]))


_CHAINS = {}


@pytest.fixture(scope="session")
def chain(tmp_path_factory):
    folder = tmp_path_factory.mktemp("arm_chains")

    def get(seed):
        if seed not in _CHAINS:
            _CHAINS[seed] = Chain(seed, folder)
        return _CHAINS[seed]
    return get


# ------------------------------------------------------------------------------------------------ a. every launch shape
CHILD = """
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import arm_chain_cases as ac
from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
d = np.load(sys.argv[1])
out = {}
for seed in %r:
    raw = ac.load_chain(seed, sys.argv[3])
    eng = ArmRolloutEngine(raw, dtype="f64")
    assert not eng.model.field("jtype").any() and not eng.model.field("frictionloss").any()
    k = "s%%d_" %% seed
    tgt = d[k + "tgt"]
    o1, r1 = [], []
    for q, v, u in zip(d[k + "q"], d[k + "v"], d[k + "u"]):
        eng.set_env_state(dict(qp=q, qv=v, target_pos=tgt))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        o1.append(nobs[0, 0].copy())
        r1.append(rew[0, 0])
    out[k + "o1"], out[k + "r1"] = np.array(o1), np.array(r1)
    eng.set_env_state(dict(qp=d[k + "rq"], qv=d[k + "rv"], target_pos=tgt))
    for P in %r:
        _, rew, act, _, _, nobs = eng.rollout(P, %d, d[k + "mean"], d[k + "noise"][:P], "open_loop")
        out[k + "rew%%d" %% P], out[k + "act%%d" %% P], out[k + "nobs%%d" %% P] = rew.copy(), act.copy(), nobs.copy()
    out[k + "failures"] = np.array(eng.solver_failures())
    eng.close()
np.savez(sys.argv[2], **out)
""" % (ROOT, os.path.join(ROOT, "tests"), list(ac.SEEDS), SIZES, H)

_RUNS = {}       # shape -> what its child process computed (each shape runs once per session)


def _run(shape, chain, tmp_path_factory):
    if shape not in _RUNS:
        tmp = tmp_path_factory.mktemp("arm_chains_" + shape)
        script, inp, outp = tmp / "run.py", str(tmp / "in.npz"), str(tmp / "out.npz")
        script.write_text(CHILD)
        data = {}
        for seed in ac.SEEDS:
            c, k = chain(seed), "s%d_" % seed
            data[k + "q"], data[k + "v"], data[k + "u"] = (np.array([s[i] for s in c.states]) for i in range(3))
            data[k + "tgt"], data[k + "rq"], data[k + "rv"], data[k + "mean"], data[k + "noise"] = c.tgt, c.q, c.v, c.mean, c.noise
        np.savez(inp, **data)
        env = {k: v for k, v in os.environ.items() if k not in ("MJMPC_ARM_DUO", "MJMPC_ARM_FLAGS", "MJMPC_ARM_ONE")}
        subprocess.run([sys.executable, str(script), inp, outp, str(tmp)], check=True, timeout=300, env=dict(env, **SHAPES[shape]))
        with np.load(outp) as f:
            _RUNS[shape] = {k: f[k] for k in f.files}
    return _RUNS[shape]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_chain_matches_the_oracle_in_every_shape(chain, tmp_path_factory, shape):
    got = _run(shape, chain, tmp_path_factory)
    for seed in ac.SEEDS:
        c, k = chain(seed), "s%d_" % seed
        step = max(_one_step_error(got[k + "o1"][i], got[k + "r1"][i], c.o1[i], c.r1[i]) for i in range(len(c.states)))
        roll = 0.0
        for P in SIZES:
            roll = max(roll, _check_rollout((got[k + "rew%d" % P], got[k + "act%d" % P], got[k + "nobs%d" % P]),
                                            tuple(x[:P] for x in c.rollout), "%s, P = %d, %s" % (c.describe(), P, shape)))
        print("%s, %s: worst relative error of one env step %.2e, of the %d-step rollouts %.2e" % (shape, c.describe(), step, H, roll))
        assert step < 1e-9, (c.describe(), shape, step)
        assert int(got[k + "failures"]) == 0, (c.describe(), shape)


def test_the_switches_select_different_kernels(chain, tmp_path_factory):
    """As in tests/test_arm_rows_tile_gpu.py: the one-wave kernel (LDL^T solves on the solver lanes) and the multi-wave kernels
    (explicit inverses) agree with the oracle above but not with each other in every bit - if the switches collapsed onto one
    kernel, the test above would compare one program four times."""
    one = _run("one_wave", chain, tmp_path_factory)
    keys = [k for k in one if "_rew" in k or k.endswith("_r1")]
    assert keys
    for shape in ("two_waves", "flags_two_waves", "flags_four_waves"):
        other = _run(shape, chain, tmp_path_factory)
        assert any(not np.array_equal(one[k], other[k]) for k in keys), shape


# --------------------------------------------------------- h / i. the default process, the tree engine, and the soak
@pytest.mark.parametrize("seed", DEFAULT_PROCESS_SEEDS)
def test_chain_in_the_default_process(chain, seed):
    """One-step checks and the 40 x 4 rollout with no switch set (the shape the launch picks for these sizes); every fourth
    chain also on the tree engine.  MJMPC_CHAIN_SEEDS=a:b: another seed range."""
    from mjmpc_amd.envs import make_engine
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    c = chain(seed)
    eng = make_engine(c.raw, dtype="f64")
    assert isinstance(eng, ArmRolloutEngine)
    assert not eng.model.field("jtype").any() and not eng.model.field("frictionloss").any()
    worst = 0.0
    for i, (q, v, u) in enumerate(c.states):
        eng.set_env_state(c.state(i))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        worst = max(worst, _one_step_error(nobs[0, 0], rew[0, 0], c.o1[i], c.r1[i]))
    eng.set_env_state(c.state())
    P = max(SIZES)
    _, rew, act, _, _, nobs = eng.rollout(P, H, c.mean, c.noise, "open_loop")
    roll = _check_rollout((rew, act, nobs), c.rollout, c.describe())
    print("%s: worst relative error of one env step %.2e, of the %d x %d rollout %.2e" % (c.describe(), worst, P, H, roll))
    assert worst < 1e-9, (c.describe(), worst)
    assert eng.solver_failures() == 0
    eng.close()
    if seed % 4 == 0:
        tree = TreeRolloutEngine(c.raw, dtype="f64")
        tree.set_env_state(c.state())
        _, t_rew, t_act, _, _, t_nobs = tree.rollout(P, H, c.mean, c.noise, "open_loop")
        _check_rollout((t_rew, t_act, t_nobs), c.rollout, "tree engine, " + c.describe())
        scale = max(1.0, np.abs(c.rollout[2]).max())
        np.testing.assert_allclose(rew, t_rew, rtol=1e-8, atol=1e-8 * scale)
        assert tree.solver_failures() == 0
        tree.close()


# ------------------------------------------------------------------------------------------ b. the shapes chosen by size
@pytest.mark.parametrize("P", [2061, 4104, 8200])
@pytest.mark.parametrize("seed", ac.SIZE_SEEDS)
def test_shapes_chosen_by_size(chain, seed, P):
    """2061 particles: a ragged last group on two waves per group; 4104: just past the two-wave shape's range, the one-wave
    kernel at one wave per SIMD; 8200: two waves per SIMD.  The oracle sees the first 40 and the last 21 particles."""
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    c, H3 = chain(seed), 3
    rs = np.random.RandomState(100 * P + seed)
    mean, noise = 0.3 * rs.standard_normal((H3, c.nu)), ac.filtered_noise(rs, P, H3, c.nu)
    eng = ArmRolloutEngine(c.raw, dtype="f64")
    eng.set_env_state(c.state())
    _, rew, act, _, _, nobs = eng.rollout(P, H3, mean, noise, "open_loop")
    pick = np.r_[0:40, P - 21:P]
    _, o_rew, o_act, _, o_nobs = c.ref.rollout(c.q, c.v, c.tgt, mean, noise[pick])
    err = _check_rollout((rew[pick], act[pick], nobs[pick]), (o_rew, o_act, o_nobs), "%s, P = %d" % (c.describe(), P))
    print("%s, P = %d: worst relative error %.2e" % (c.describe(), P, err))
    assert np.isfinite(rew).all() and np.isfinite(nobs).all()
    assert eng.solver_failures() == 0
    eng.close()


# ------------------------------------------------------------------------------------------------------------ c. f32
@pytest.mark.parametrize("seed", ac.SIZE_SEEDS)
def test_f32_stays_close(chain, seed):
    """Single precision held to the bounds of tests/test_arm_xj_gpu.py::test_f32_stays_close: one env step from the 24 states
    with a median relative error below 1e-4 and a 95th percentile below 1e-2, nothing non-finite; then 16392 x 3 (three waves
    per SIMD, an instantiation only f32 has) finite with at most 2 solver failures."""
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    c = chain(seed)
    eng = ArmRolloutEngine(c.raw, dtype="f32")
    errs = []
    for i, (q, v, u) in enumerate(c.states):
        eng.set_env_state(c.state(i))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        assert np.isfinite(nobs).all() and np.isfinite(rew).all()
        errs.append(np.abs(nobs[0, 0] - c.o1[i]).max() / max(1.0, np.abs(c.o1[i]).max()))
    errs = np.sort(errs)
    print("%s f32: median %.1e, 95th percentile %.1e, worst %.1e" % (c.describe(), errs[len(errs) // 2], errs[int(0.95 * len(errs))], errs[-1]))
    assert errs[len(errs) // 2] < 1e-4 and errs[int(0.95 * len(errs))] < 1e-2
    P, H3 = 16392, 3
    rs = np.random.RandomState(seed)
    eps = ac.filtered_noise(rs, P, H3, c.nu).astype(np.float32)
    eng.set_env_state(c.state())
    _, rew, _, _, _, nobs = eng.rollout(P, H3, np.zeros((H3, c.nu)), eps, "open_loop")
    assert np.isfinite(rew).all() and np.isfinite(nobs).all()
    assert eng.solver_failures() <= 2
    eng.close()


# -------------------------------------------------------------------------------------------------- d. the real-env step
@pytest.mark.parametrize("seed", ac.SIZE_SEEDS)
def test_real_env_step(chain, seed):
    """``step_state`` (the STEP twins) over 6 steps from a state of ``states``: every step against the oracle's env step from
    the state the device held before it (read back), observation and cost to 1e-9 relative; the state read back after the
    step is the observation's qpos | qvel."""
    import torch
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    c = chain(seed)
    eng = ArmRolloutEngine(c.raw, dtype="f64")
    eng.set_env_state(c.state(3 if c.raw.plane is not None else 1))          # (a steered state: in the floor / past a limit)
    rs = np.random.RandomState(300 + seed)
    worst = 0.0
    for step in range(6):
        before = eng.get_state_device()
        a = rs.uniform(-1.3, 1.3, c.nu)
        cost, nobs = eng.step_state(a)
        torch.cuda.synchronize()
        cost, nobs = float(cost.cpu().numpy()[0]), nobs.cpu().numpy().astype(np.float64)
        q1, v1, r1, o1 = c.ref.env_step(before["qp"], before["qv"], a, c.tgt)
        worst = max(worst, _one_step_error(nobs, -cost, o1, r1))
        after = eng.get_state_device()
        assert np.array_equal(after["qp"], nobs[:c.nv]) and np.array_equal(after["qv"], nobs[c.nv:2 * c.nv])
        assert not np.array_equal(after["qp"], before["qp"])
    print("%s: worst relative error of a real-env step %.2e" % (c.describe(), worst))
    assert worst < 1e-9, worst
    assert eng.solver_failures() == 0 and eng.env_resets() == 0
    eng.close()


# ------------------------------------------------------------------------------------------- e. closed-loop-linear mode
@pytest.mark.parametrize("seed", ac.CL_SEEDS)
def test_closed_loop_linear_mode(chain, seed):
    """action = W^T [obs; 1] + noise with W of shape (2 nv + 7, nu), 64 x 6 (the CL instantiations)."""
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    c = chain(seed)
    P, H6 = 64, 6
    rs = np.random.RandomState(400 + seed)
    W = 0.3 * rs.standard_normal((2 * c.nv + 7, c.nu))
    noise = ac.filtered_noise(rs, P, H6, c.nu, 0.3)
    eng = ArmRolloutEngine(c.raw, dtype="f64")
    assert eng.d_obs == 2 * c.nv + 6
    eng.set_env_state(c.state())
    obs, rew, act, _, _, nobs = eng.rollout(P, H6, W, noise, "closed_loop_linear")
    o_obs, o_rew, o_act, _, o_nobs = c.ref.rollout(c.q, c.v, c.tgt, W, noise, mode="closed_loop_linear")
    scale = max(1.0, np.abs(o_nobs).max())
    for got, want in ((act, o_act), (rew, o_rew), (nobs, o_nobs), (obs, o_obs)):
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-8 * scale)
    # the first action is a function of the fresh observation only
    np.testing.assert_allclose(act[:, 0] - noise[:, 0], (W.T @ np.append(o_obs[0, 0], 1.0))[None].repeat(P, 0),
                               rtol=1e-12, atol=1e-12)
    assert eng.solver_failures() == 0
    eng.close()


# ------------------------------------------------------------------------------------- f. the fused two-launch iteration
@pytest.mark.parametrize("P", [64, 4096])
@pytest.mark.parametrize("seed", ac.MONO_SEEDS)
def test_fused_mppi_iteration(chain, seed, P):
    """``mjmpc_arm_mppi_step`` with A = nu = 1, 3, 5 (the MONO instantiations' action tile met A = 7 only), in the four-wave
    flag shape (P = 64) and the two-wave shape (P = 4096): 4 control steps = the oracle-driven loop on the same Philox samples,
    as tests/test_arm_xj_gpu.py does for the cart-pole on the extended-joint build."""
    from mjmpc_amd.control import MPPI
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine, make_device_rollout_fn
    from oracle import controllers_ref as cr
    c = chain(seed)
    eng = ArmRolloutEngine(c.raw, dtype="f64")
    eng.set_env_state(c.state())
    H8, lam, A, filt = 8, 0.05, c.nu, [0.25, 0.8, 0.0]
    assert A in (1, 3, 5, 6)
    m = MPPI(d_state=eng.d_state, d_obs=eng.d_obs, d_action=A, horizon=H8, init_cov=0.3, base_action="null", lam=lam,
             num_particles=P, step_size=1.0, alpha=1, gamma=1.0, n_iters=1, action_lows=eng.action_lows,
             action_highs=eng.action_highs, filter_coeffs=filt, seed=3, noise_mode="device")
    m.rollout_fn = make_device_rollout_fn(eng)
    m.set_sim_state_fn = lambda s: None
    m.enable_graph(post_step=eng.step_state)
    q, v, mean = c.q.copy(), c.v.copy(), np.zeros((H8, A))
    for step in range(4):
        a, _ = m.optimize({})
        assert m._mono, "the chain should take the fused two-launch iteration on the arm engine"
        noise = m.dev.sample_noise(P, 0.3 * np.eye(A), filt, 3, step, filtered=True).cpu().numpy()
        _, rew, act, _, _ = c.ref.rollout(q, v, c.tgt, mean, noise, want_obs=False)
        mean = cr.mppi_update(-rew, act, mean, 0.3 * np.eye(A), cr.gamma_seq(1.0, H8), lam, 1, 1.0)
        np.testing.assert_allclose(a, mean[0], rtol=0, atol=1e-9)
        q, v, _, _ = c.ref.env_step(q, v, a, c.tgt)
        mean = cr.shift_mean(mean, "null")
    st = eng.get_state_device()
    np.testing.assert_allclose(st["qp"], q, rtol=0, atol=1e-7)           # (four steps of 1e-9 actions and env steps later)
    assert eng.solver_failures() == 0
    eng.close()


# -------------------------------------------------------------------------------------------------- g. episode batches
@pytest.mark.parametrize("seed", ac.BATCH_SEEDS)
def test_episode_batch_on_the_arm_engine(chain, seed):
    """The EB twins with A = nu and nv < 7: E = 3 episodes of one chain from different start states with their own means - the
    batch rollout (``mjmpc_arm_rollout_fused_batch``) against the oracle per episode, as
    tests/test_batched_arm_gpu.py::test_batch_rollout_against_the_oracle does for the reacher, and the batched env step
    (``mjmpc_arm_step_shard_states``) against the oracle's env step."""
    import torch
    from batched_cases import _vp
    from mjmpc_amd import _lib
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    c = chain(seed)
    E, P, H4, A = 3, 16, 4, c.nu
    states = [c.state(k) for k in (3, 5, 10)]
    rs = np.random.RandomState(500 + seed)
    means = torch.from_numpy(rs.uniform(-0.3, 0.3, (E, H4, A))).cuda()
    noise = torch.from_numpy(0.4 * rs.standard_normal((E * P, H4, A))).cuda()
    eng = ArmRolloutEngine(c.raw, dtype="f64")
    eng.set_shard_states_raw([eng._unpack(s) for s in states])
    costs = torch.empty((E * P, H4), dtype=torch.float64, device="cuda")
    acts = torch.empty((E * P, H4, A), dtype=torch.float64, device="cuda")
    _lib.check(eng._lib.mjmpc_arm_rollout_fused_batch(eng._h, eng._code, E * P, H4, _vp(means), _vp(noise), None, None,
                                                      _vp(costs), _vp(acts), None, eng._stream()))
    torch.cuda.synchronize()
    costs, acts, means_h, noise_h = costs.cpu().numpy(), acts.cpu().numpy(), means.cpu().numpy(), noise.cpu().numpy()
    for e in range(E):
        rows = slice(e * P, (e + 1) * P)
        _, rew, act, _, nobs = c.ref.rollout(states[e]["qp"], states[e]["qv"], c.tgt, means_h[e], noise_h[rows])
        assert np.array_equal(acts[rows], act), e
        scale = max(1.0, np.abs(nobs).max())
        np.testing.assert_allclose(costs[rows], -rew, rtol=1e-8, atol=1e-8 * scale)
    assert not np.array_equal(costs[:P], costs[P:2 * P])
    # the batched env step: every episode's real env, one launch
    actions = rs.uniform(-1.3, 1.3, (E, A))
    cost, obs = torch.empty(E, dtype=torch.float64, device="cuda"), torch.empty((E, eng.d_obs), dtype=torch.float64, device="cuda")
    _lib.check(eng._lib.mjmpc_arm_step_shard_states(eng._h, eng._code, _vp(torch.from_numpy(actions).cuda()), _vp(cost), _vp(obs),
                                                    eng._stream()))
    torch.cuda.synchronize()
    qp, qv = eng.get_shard_states()
    cost, obs = cost.cpu().numpy(), obs.cpu().numpy()
    for e in range(E):
        q1, v1, r1, o1 = c.ref.env_step(states[e]["qp"], states[e]["qv"], actions[e], c.tgt)
        err = _one_step_error(obs[e], -cost[e], o1, r1)
        assert err < 1e-9, (e, err)
        assert np.array_equal(qp[e], obs[e, :c.nv]) and np.array_equal(qv[e], obs[e, c.nv:2 * c.nv])
    assert eng.solver_failures() == 0 and eng.env_resets() == 0
    eng.close()


# ----------------------------------------------------------------------- per-element solver sets run on the tree engine
@pytest.mark.parametrize("what", ["geom", "joint"])
def test_a_model_with_its_own_solver_sets_runs_on_the_tree_engine(chain, tmp_path, what):
    """The colliding sphere with its own solref / a limited joint with its own solreflimit: ``make_engine`` gives the tree engine
    (the arm kernels carry one solver set and ``compile_arm`` refuses the model), and one env step from 12 states matches the
    oracle, which honours the element's set - and differs from the unedited chain's."""
    from mjmpc_amd.envs import make_engine
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.mjcf import load_mjcf
    from oracle.physics_ref import RefArm
    c = chain(ac.OWN_SET_SEED)
    path = tmp_path / "edited.xml"
    path.write_text(ac.own_solver_set_xmls(ac.OWN_SET_SEED)[what])
    raw = load_mjcf(str(path), frame_skip=2)
    eng, ref = make_engine(raw, dtype="f64"), RefArm(raw.to_flat())
    assert isinstance(eng, TreeRolloutEngine)
    worst, moved = 0.0, 0
    # (12 states: the steered ones - in the floor, past a limit - among them)
    for i in (0, 1, 3, 6, 7, 9, 12, 13, 15, 18, 19, 21):
        q, v, u = c.states[i]
        eng.set_env_state(c.state(i))
        _, rew, _, _, _, nobs = eng.rollout(1, 1, u[None], None, "open_loop")
        _, _, r1, o1 = ref.env_step(q, v, u, c.tgt)
        worst = max(worst, _one_step_error(nobs[0, 0], rew[0, 0], o1, r1))
        moved += bool(np.abs(o1 - c.o1[i]).max() > 1e-6)
    print("%s with its own %s solver set on the tree engine: worst relative error of one env step %.2e; %d of 12 states differ "
          "from the unedited chain's" % (c.describe(), what, worst, moved))
    assert worst < 1e-9, worst
    assert moved >= 3
    assert eng.solver_failures() == 0
    eng.close()
