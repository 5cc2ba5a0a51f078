"""GPU: dynamics-randomized episode batches (``BatchedMPPI.randomize_dynamics``) and the real-env model switch
of the tree engine (``TreeRolloutEngine.set_real_env_model``).

Bit identity: episode e of a randomized batch computes the bits of the single-episode device path of
tests/test_batched_mppi_gpu.py (``_single`` there) on ``TreeRolloutEngine(raw, dtype, num_shards=K)`` after
``randomize_dynamics(cfg, base_seed)`` and ``set_real_env_model("nominal")`` - every comparison is ``np.array_equal``: the
actions, real-env costs and next observations of every step, the final mean and the final state.  Parity: the cost rows of
every (episode, shard) against the FP64 C oracle edited through its setters, independent of the single path.
"""
import ctypes
import functools

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import _torch
from batched_cases import synthetic_states as _synthetic_states

pytestmark = pytest.mark.gpu

# the configuration of test_dynamics_randomization_per_shard_on_the_tree_engine (tests/test_locomotion_gpu.py) minus sensor_noise
CHEETAH_CFG = {"body_mass": {"torso": [0.3, 0.1], "ffoot": [0.5, 0.0]}, "body_inertia": {"bthigh": [0.3, 0.0]},
               "dof_damping": {"bshin": [0.4, 0.2]}, "geom_size": {"ffoot": [0.2, 0.0], "bfoot": [0.1, 0.0]},
               "geom_friction": {"bfoot": [0.5, 0.5]}, "dof_frictionloss": {"fshin": [0.5, 0.0]}}


MPPI = bc.case("BatchedMPPI", "MPPI", ("lam", "step_size", "init_cov"), lambda dtype: dict(alpha=1, noise_dtype=dtype),
               guards=False)          # (tests/test_batched_mppi_gpu.py's)


def _make_batch(raw, states, seeds, P, H, lam, cov, dtype):
    return bc.make_batch(MPPI, raw, states, seeds, P, H, (lam, 1.0, cov), dtype)


def _check(raw, states, seeds, P, H, T, lam, cov, dtype, K, cfg, dyn_seed):
    """``dyn_seed``: one int (one shared set of blocks) or one per episode."""
    E = len(states)
    b = _make_batch(raw, states, seeds, P, H, lam, cov, dtype)
    per_episode = isinstance(dyn_seed, (list, tuple))
    defaults, rand = b.randomize_dynamics(cfg, dyn_seed, K)
    assert len(rand) == (E if per_episode else K) and b.shard_blobs.shape[:2] == ((E if per_episode else 1), K)
    out = bc.check_against_singles(MPPI, raw, states, seeds, P, H, T, (lam, 1.0, cov), dtype, out=bc.run_batch(MPPI, b, T),
                                   K=K, cfg=cfg, dyn_seed=dyn_seed)
    for e, one in enumerate(out["singles"]):
        # the model-block bytes the batch uploads are the single engine's
        assert np.array_equal(b.shard_blobs[e if per_episode else 0], one["blobs"]), "episode %d: model blocks differ" % e
    return out["acts"], b.shard_blobs


_cheetah_states = functools.partial(bc._cheetah_states, copy=True)      # (copies: the tests here may edit their start states)


@pytest.mark.parametrize("dyn_seed", [321, [321, 77, 4242]], ids=["shared_set", "set_per_episode"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_randomized_batch_equals_single_episodes(dtype, dyn_seed):
    """E = 3, K = 2, P = 48: 24 particles per row is no multiple of a workgroup's particles (the partial-row ``live`` path)."""
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    E = 3
    acts, blobs = _check(half_cheetah_raw(), _cheetah_states(E), [123 + i * 12345 for i in range(E)], 48, 8, 4, 0.2, 0.3,
                         dtype, 2, CHEETAH_CFG, dyn_seed)
    assert not np.array_equal(acts[:, 0], acts[:, 1])
    assert not np.array_equal(blobs[0, 0], blobs[0, 1])                 # (the shards' models differ ...)
    if isinstance(dyn_seed, list):
        assert not np.array_equal(blobs[0, 0], blobs[1, 0])             # (... and so do the episodes' sets)


def test_one_model_per_episode():
    """K = 1 with per-episode seeds: every episode rolls out its own single randomized model."""
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    E = 3
    _check(half_cheetah_raw(), _cheetah_states(E), [5, 6, 7], 32, 8, 4, 0.2, 0.3, "f64", 1, CHEETAH_CFG, [11, 12, 13])


def test_rk4_double_pendulum_randomized():
    """The RK4 twin unit; a slide and two hinges: the state round-trips exactly.  E = 2, K = 3, P = 48."""
    raw, states = _synthetic_states("double_pendulum", 2, seed=1)
    assert raw.integrator == "RK4"
    cfg = {"dof_damping": {"slider": [0.5, 0.0], "hinge1": [0.5, 0.0], "hinge2": [0.3, 0.1]}}
    _check(raw, states, [21, 22], 48, 8, 4, 0.2, 0.3, "f64", 3, cfg, [17, 18])


def test_gripper_randomized():
    """The elliptic-cone twin unit, one small case."""
    raw, states = _synthetic_states("gripper", 2, seed=2)
    _check(raw, states, [31, 32], 16, 4, 2, 0.5, 0.3, "f64", 2, {"body_mass": {"pen": [0.3, 0.0], "palm": [0.2, 0.1]}}, 9)


def test_hand24_randomized():
    """The 32-lane twin (tree_rollout.hip's own instantiations), one small case."""
    from mjmpc_amd.models.compile_tree import compile_tree
    from mjmpc_amd.models.hand24 import hand24_raw
    raw = hand24_raw()
    m = compile_tree(raw)
    rng = np.random.RandomState(3)
    states = [dict(qp=m.qpos0 + 0.05 * rng.randn(m.nq), qv=0.05 * rng.randn(m.nv), target_pos=m.target_default.copy())
              for _ in range(2)]
    _check(raw, states, [41, 42], 16, 4, 2, 0.5, 0.3, "f64", 2, {"body_mass": {"palm": [0.3, 0.0], "f0_mid": [0.5, 0.0]}},
           [5, 6])


def test_clear_dynamics_restores_the_unrandomized_batch():
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw, E = half_cheetah_raw(), 2
    states, seeds = _cheetah_states(E), [3, 4]
    plain = _make_batch(raw, states, seeds, 32, 8, 0.2, 0.3, "f64")
    want = plain.run(3) + (plain.mean_action,)
    plain.close()
    b = _make_batch(raw, states, seeds, 32, 8, 0.2, 0.3, "f64")
    b.randomize_dynamics(CHEETAH_CFG, 321, 2)
    rnd = b.run(1)
    b.clear_dynamics()
    assert b.shard_blobs is None
    b.set_states([dict(s) for s in states])
    b.reset()
    got = b.run(3) + (b.mean_action,)
    b.close()
    assert not np.array_equal(rnd[0][0], want[0][0])                    # (the randomized step was a different step)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_randomized_batch_rows_match_the_oracle():
    """E = 2 start states, K = 2, P = 16, H = 4 (f64), a set of blocks per episode: after one ``step()`` the P / K cost rows of
    every (e, k) equal the oracle's, edited through its setters as tests/test_locomotion_gpu.py does, started from state e
    and fed the actions the launch wrote (zero mean, the action tensor as noise)."""
    from mjmpc_amd.models.compile import principal_inertia
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    from oracle.physics_ref import RefArm
    raw, E, K, P, H = half_cheetah_raw(), 2, 2, 16, 4
    states = _cheetah_states(E)
    assert not np.array_equal(states[0]["qpos"], states[1]["qpos"])
    b = _make_batch(raw, states, [123, 456], P, H, 0.2, 0.3, "f64")
    _, rand = b.randomize_dynamics(CHEETAH_CFG, [321, 99], K)
    b.step()
    _torch().cuda.synchronize()
    costs = b._costs.cpu().numpy().reshape(E, K, P // K, H)
    acts = b._actions.cpu().numpy().reshape(E, K, P // K, H, -1)
    names = [bd.name for bd in raw.bodies]
    joints = [bd.joint.name for bd in raw.bodies if bd.joint is not None]
    geoms = [g for bd in raw.bodies for g in bd.geoms if g.collide]         # two contact points each, "to" end first
    blocks = {}
    for e in range(E):
        for k in range(K):
            ref, r = RefArm(raw.to_flat()), rand[e][k]
            for n, m in r["body_mass"].items():
                ref.set_body_mass(names.index(n) + 1, m)
            for n, mom in r["body_inertia"].items():
                _, V = principal_inertia(b.model.body_inertia[names.index(n)])
                ref.set_body_inertia(names.index(n) + 1, V @ np.diag(mom) @ V.T)
            for n, d in r["dof_damping"].items():
                ref.set_dof_damping(joints.index(n), d)
            for n, size in r["geom_size"].items():
                j = [g.name for g in geoms].index(n)
                p0, p1 = np.asarray(geoms[j].a, float), np.asarray(geoms[j].b, float)
                c, u = 0.5 * (p0 + p1), (p1 - p0) / np.linalg.norm(p1 - p0)
                for end, sgn in ((0, 1.0), (1, -1.0)):
                    ref.set_sphere_radius(2 * j + end, size[0])
                    ref.set_sphere_pos(2 * j + end, c + sgn * size[1] * u)
            for n, fr in r["geom_friction"].items():
                j = [g.name for g in geoms].index(n)
                for end in (0, 1):
                    ref.set_sphere_mu(2 * j + end, max(fr[0], raw.plane.friction))
            o = ref.rollout(states[e]["qpos"], states[e]["qvel"], np.zeros(3), np.zeros((H, acts.shape[-1])), acts[e, k])
            print("(e, k) = (%d, %d): max |cost - oracle| = %.3g" % (e, k, np.abs(-costs[e, k] - o[1]).max()))
            np.testing.assert_allclose(-costs[e, k], o[1], rtol=1e-9, atol=1e-9)
            blocks[e, k] = o[1]
    assert np.abs(blocks[0, 0] - blocks[0, 1]).max() > 1e-3             # the shards really differ
    assert b.engine.solver_failures() == 0
    b.close()


def test_real_env_model_switch():
    """K = 2 randomized shards with a nominal real env: ``step_state`` is a fresh unrandomized engine's to the bit, ``rollout``
    still runs the randomized blocks, and ``set_real_env_model(None)`` is an engine that never called it."""
    torch = _torch()
    from mjmpc_amd.envs.tree_engine import TreeRolloutEngine
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    raw = half_cheetah_raw()
    state = _cheetah_states(1)[0]
    rng = np.random.RandomState(0)
    actions = rng.uniform(-1, 1, (6, 6))
    P, H = 16, 4
    mean, noise = 0.3 * rng.standard_normal((H, 6)), 0.7 * rng.standard_normal((P, H, 6))

    def steps(eng):
        out = []
        for a in actions:
            cost, obs = eng.step_state(a)
            torch.cuda.synchronize()
            out.append(np.concatenate([cost.cpu().numpy(), obs.cpu().numpy()]))
        st = eng.get_state_device()
        return np.array(out), st["qpos"], st["qvel"]

    def same(x, y):
        return all(np.array_equal(p, q) for p, q in zip(x, y))

    fresh = TreeRolloutEngine(raw, dtype="f64")
    fresh.set_env_state(dict(state))
    nominal = steps(fresh)
    fresh.close()
    plain = TreeRolloutEngine(raw, dtype="f64", num_shards=2)            # randomized, never switched
    plain.randomize_dynamics(CHEETAH_CFG, 321)
    plain.set_env_state(dict(state))
    rew_plain = plain.rollout(P, H, mean, noise)[1].copy()
    shard0 = steps(plain)
    plain.close()
    eng = TreeRolloutEngine(raw, dtype="f64", num_shards=2)
    eng.randomize_dynamics(CHEETAH_CFG, 321)
    eng.set_real_env_model("nominal")
    eng.set_env_state(dict(state))
    assert np.array_equal(eng.rollout(P, H, mean, noise)[1], rew_plain)     # rollouts: the randomized blocks, as before
    assert same(steps(eng), nominal)
    assert not same(nominal, shard0)                                        # (shard 0's block is not the nominal one)
    eng.set_real_env_model(None)
    eng.set_env_state(dict(state))
    assert same(steps(eng), shard0)
    with pytest.raises(ValueError):
        eng.set_real_env_model("true")
    eng.close()


def test_entry_points_refuse_what_does_not_fit_the_engine():
    """With an engine of E = 3 state shards: a set count that is neither 1 nor E, blocks of another topology, particles that
    do not divide into E K rows - a code and a message, and the engine keeps running."""
    from mjmpc_amd import _lib
    from mjmpc_amd.models.compile_tree import compile_tree
    from mjmpc_amd.models.half_cheetah import half_cheetah_raw
    from mjmpc_amd.models.swimmer import swimmer_raw
    raw, E = half_cheetah_raw(), 3
    b = _make_batch(raw, _cheetah_states(E), [1, 2, 3], 32, 4, 0.2, 0.3, "f64")
    lib, h = b.lib, b.engine._h
    own = np.ascontiguousarray(np.stack([b.model.blob] * 4), np.float64)
    other = np.ascontiguousarray(np.stack([compile_tree(swimmer_raw()).blob] * 2), np.float64)
    for blobs, n_sets, K in ((own, 2, 2), (own, 4, 1), (other, 1, 2), (own, 1, 0), (own, -1, 2), (None, 1, 2)):
        rc = lib.mjmpc_tree_set_batch_models(h, None if blobs is None else blobs.ctypes.data_as(_lib._dp), n_sets, K)
        assert rc != 0 and len(lib.mjmpc_last_error()) > 0, (n_sets, K)
    assert lib.mjmpc_tree_set_env_model(h, other.ctypes.data_as(_lib._dp)) != 0 and len(lib.mjmpc_last_error()) > 0
    b.randomize_dynamics(CHEETAH_CFG, 1, 2)
    b.num_particles = 31            # (31 particles per episode do not divide into two shards: the launch is refused)
    with pytest.raises(_lib.MjmpcError, match="divide"):
        lib_call = lib.mjmpc_tree_rollout_fused_batch
        vp = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
        _lib.check(lib_call(h, b._code, E * 31, 4, vp(b._means), vp(b._noise), vp(b._coeffs), vp(b._gseq), vp(b._costs),
                            vp(b._actions), vp(b._q0), b._stream()))
    b.num_particles = 32
    acts, _, _ = b.run(2)
    assert np.all(np.isfinite(acts))
    b.close()
