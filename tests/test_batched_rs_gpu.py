"""GPU: a random-shooting episode batch (``BatchedRandomShooting``) reproduces E separate single-episode runs to
the bit.

The single-episode reference is the device path of a fresh ``TreeRolloutEngine`` per episode: ``RandomShooting(...,
noise_mode='device', noise_dtype=dtype, seed=seed_e)``, ``make_device_rollout_fn(engine)``,
``enable_graph(post_step=engine.step_state)``, whose iteration runs the Philox draw, ``mjmpc_tree_rollout_fused`` (filter +
rollout + q0), ``mjmpc_rs_best`` + ``mjmpc_rs_combine`` and ``mjmpc_step_tail`` and steps the engine's device-resident real env;
``_single`` asserts that it took that q0-from-rollout branch.  Every comparison is ``np.array_equal``: the actions, real-env
costs and next observations of every step, the final mean and the final state.  No real env may reset on either side and
every action and cost is finite, so that two all-``inf`` runs cannot pass for equal.  A single run is computed once per
setting and shared, read-only, by the tests that compare against it.
"""
import ctypes
import os

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import FILT, ROOT, _cheetah_states, _torch, _vp
from batched_cases import cheetah as _cheetah

pytestmark = pytest.mark.gpu


def _takes_q0_from_the_rollout(c):
    # the branch of the device iteration that takes q0 from the rollout launch (draw, fused rollout, rs_best + rs_combine, tail)
    assert c._wants_q0() and c.noise_mode == "device" and hasattr(c._rollout_fn, "fused")
    assert not c.dev.gamma_zero and not c.use_zero_control_seq


RS = bc.case("BatchedRandomShooting", "RandomShooting", ("step_size", "init_cov"), lambda dtype: dict(noise_dtype=dtype),
             before=_takes_q0_from_the_rollout)


def _check_against_singles(raw, states, seeds, P, H, T, step_size, init_cov, dtype, **kw):
    out = bc.check_against_singles(RS, raw, states, seeds, P, H, T, (step_size, init_cov), dtype, **kw)
    return out["acts"], out["costs"]


def _cheetah_keys(E):
    return [("half_cheetah", i) for i in range(E)]


SEEDS = [123 + i * 12345 for i in range(3)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_half_cheetah_batch_equals_single_episodes(dtype):
    """E = 3, P = 64, H = 8, T = 6; step_size 0.7: the blend is a blend and not a copy of the best sequence."""
    E = 3
    acts, _ = _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS, 64, 8, 6, 0.7, 0.3, dtype, keys=_cheetah_keys(E))
    assert not np.array_equal(acts[:, 0], acts[:, 1])           # (the episodes are different episodes)


def test_per_episode_hyperparameters():
    """A step size of 1 (the copy), two below it; three covariances."""
    E = 3
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS, 64, 8, 6, np.array([1.0, 0.7, 0.4]), np.array([0.2, 0.3, 0.5]),
                           "f64", keys=_cheetah_keys(E))


def test_base_action_repeat():
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 64, 8, 6, 0.7, 0.3, "f64", base_action="repeat",
                           keys=_cheetah_keys(E))


def test_particles_not_a_multiple_of_the_block_or_a_wave():
    """P = 50: the scan's last stride is partial, and row e + 1's cost-to-go lies right behind row e's."""
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 50, 8, 6, 0.7, 0.3, "f64", keys=_cheetah_keys(E))


def test_one_episode():
    _check_against_singles(_cheetah(), _cheetah_states(1), SEEDS[:1], 64, 8, 6, 0.7, 0.3, "f64", keys=_cheetah_keys(1))


def test_permuting_the_episodes_permutes_the_results():
    step, cov = np.array([1.0, 0.7, 0.4]), np.array([0.2, 0.3, 0.5])
    bc.check_permutation(RS, _cheetah(), _cheetah_states(3), SEEDS, 64, 8, 6, (step, cov), "f64", [2, 0, 1])


def test_free_joint_model():
    """A general instantiation of the rollout kernel: the tray, whose glass has a free joint."""
    from mjmpc_amd.models.compile_tree import compile_tree
    raw, states = bc.synthetic_states("tray", 2)
    m = compile_tree(raw)
    assert m.nq > m.nv
    _check_against_singles(raw, states, [11, 12], 32, 4, 3, 0.7, 0.3, "f64")


@pytest.mark.parametrize("dyn_seed", [5, [3, 4]], ids=["shared_seed", "per_episode_seeds"])
def test_randomized_dynamics_two_shards(dyn_seed):
    """K = 2 shards of 32 particles roll out their own model blocks (the parameters of
    examples/configs/half_cheetah_gpu_dyn_randomize.yml); the real envs stay nominal."""
    import yaml
    with open(os.path.join(ROOT, "examples", "configs", "half_cheetah_gpu_dyn_randomize.yml")) as f:
        cfg = yaml.safe_load(f)
    assert set(cfg) == {"body_mass", "dof_damping", "geom_friction"}
    E = 2
    _check_against_singles(_cheetah(), _cheetah_states(E), SEEDS[:E], 64, 8, 6, 0.7, 0.3, "f64", K=2, cfg=cfg, dyn_seed=dyn_seed)


def test_best_particle_is_the_argmin_of_the_cost_to_go():
    from mjmpc_amd.control import BatchedRandomShooting
    E, P = 3, 64
    b = BatchedRandomShooting(_cheetah(), E, 8, P, 0.7, 0.3, 1.0, FILT, "null", SEEDS)
    b.set_states([dict(s) for s in _cheetah_states(E)])
    b.step()
    best = b.best_particle
    q0 = b._q0.cpu().numpy().reshape(E, P)
    b.close()
    assert best.shape == (E,) and best.dtype == np.int64
    assert np.all(np.isfinite(q0.min(axis=1)))
    assert np.array_equal(best, np.argmin(q0, axis=1))
    assert len(set(best.tolist())) > 1                          # (not one index for every episode)


# ---------------------------------------------------------------------------------------------------------- the C ABI alone
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("shift_mode", [0, 1])
def test_update_launch_on_hand_made_rows(shift_mode, dtype):
    """E = 4 rows of P = 300 (two strides of the block, the second partial), H = 3, A = 2: the minimum in the last entry; three
    tied minima, two in the two strides of one thread and one in another wavefront (the lowest index wins); a row of +inf
    (particle 0, never index P); a row of equal values.  Means and actions against a numpy evaluation to 1e-15 relative: means, actions and step sizes are
    positive, so neither the blend nor its fused-multiply-add form cancels and both are within two roundings (1.1e-16
    relative each) of the exact value of their common operands, at most 4.4e-16 apart - bitwise equality is not asserted, the
    contraction is not numpy's."""
    torch = _torch()
    from mjmpc_amd import _lib
    lib = _lib.require_gpu()
    E, P, H, A = 4, 300, 3, 2
    code = _lib.F32 if dtype == "f32" else _lib.F64
    npt = np.float32 if dtype == "f32" else np.float64
    rng = np.random.RandomState(4)
    q0 = rng.uniform(1.0, 2.0, (E, P))
    q0[0, 299] = 0.5
    q0[1, [7, 64, 263]] = 0.25
    q0[2, :] = np.inf
    q0[3, :] = 1.5
    expect = np.array([299, 7, 0, 0])
    assert np.array_equal(np.argmin(q0, axis=1), expect)
    actions = rng.uniform(0.1, 1.0, (E, P, H, A)).astype(npt)
    means0 = rng.uniform(0.1, 1.0, (E, H, A))
    step = np.array([0.7, 1.0, 0.4, 0.25])
    # -- numpy: blend, read the action out, shift
    blended = np.stack([(1.0 - step[e]) * means0[e] + step[e] * actions[e, expect[e]].astype(np.float64) for e in range(E)])
    ref_out = blended[:, 0].copy()
    ref_means = np.concatenate([blended[:, 1:], blended[:, -1:] if shift_mode == 1 else np.zeros((E, 1, A))], axis=1)

    dev = "cuda"
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_q0, d_act, d_step = d(q0), d(actions), d(step)
    step0 = 3
    for with_outputs in (True, False):
        d_means = d(means0)
        d_out = torch.zeros((E, A), dtype=torch.float64, device=dev) if with_outputs else None
        d_counter = torch.full((1,), step0, dtype=torch.int64, device=dev) if with_outputs else None
        d_best = torch.full((E,), -1, dtype=torch.int64, device=dev) if with_outputs else None
        _lib.check(lib.mjmpc_rs_update_batch(code, E, P, H, A, _vp(d_q0), _vp(d_act), _vp(d_step), shift_mode, _vp(d_means),
                                             _vp(d_out), _vp(d_counter), _vp(d_best), s))
        torch.cuda.synchronize()
        np.testing.assert_allclose(d_means.cpu().numpy(), ref_means, rtol=1e-15, atol=0)
        if with_outputs:
            assert np.array_equal(d_best.cpu().numpy(), expect)
            np.testing.assert_allclose(d_out.cpu().numpy(), ref_out, rtol=1e-15, atol=0)
            assert int(d_counter.item()) == step0 + 1           # advanced once, by row 0
    assert np.array_equal(d_q0.cpu().numpy(), q0) and np.array_equal(d_act.cpu().numpy(), actions)      # inputs untouched
