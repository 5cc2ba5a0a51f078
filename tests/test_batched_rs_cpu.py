"""CPU: ``BatchedRandomShooting`` refuses what it does not run before any engine or device memory exists,
broadcasts its per-episode settings as ``BatchedMPPI`` does, and its entry points are declared, bound, built and reject bad
arguments."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw
from mjmpc_amd.models.hand24 import hand24_raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mjmpc_rs_batch_supported", "mjmpc_rs_update_batch"]
E_BADARG = -1               # (MJMPC_E_BADARG of include/mjmpc_amd.h)


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, step_size=0.7, init_cov=0.3, gamma=1.0,
              filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.fixture
def no_engine(monkeypatch):
    """Making an engine fails the test: every refusal must come first."""
    from mjmpc_amd.envs import tree_engine

    def refuse(*a, **k):
        raise AssertionError("an engine was created before the settings were checked")
    monkeypatch.setattr(tree_engine.TreeRolloutEngine, "__init__", refuse)


@pytest.mark.parametrize("over", [
    dict(n_iters=2), dict(sample_mode="sample"), dict(use_zero_control_seq=True), dict(gamma=0.0),
    dict(base_action="random"), dict(base_action="zeros"), dict(dtype="f16"), dict(num_episodes=0), dict(num_episodes=65536),
    dict(horizon=0), dict(num_particles=0), dict(filter_coeffs=[1.0, 0.0]),
    # per-episode arrays of the wrong length / shape, and values random shooting cannot take
    dict(init_cov=[0.1] * 3), dict(step_size=np.ones(5)), dict(step_size=np.zeros((4, 2))), dict(init_mean=np.zeros((8, 5))),
    dict(init_mean=np.zeros((3, 8, 6))), dict(seeds=[1, 2, 3]), dict(seeds=7), dict(seeds=[1, 2, 3, -4]),
    dict(init_cov=[0.3, 0.3, -1.0, 0.3]), dict(init_cov=0.0), dict(step_size=-0.1), dict(step_size=[1.0, 0.7, -0.4, 0.2]),
    dict(init_cov=float("nan")), dict(step_size=float("nan")),
    # a model the tree engine refuses: RK4 beyond 16 dofs
    dict(raw_model=dataclasses.replace(hand24_raw(), integrator="RK4")),
], ids=lambda d: ",".join("%s=%s" % (k, type(v).__name__ if k in ("raw_model", "init_mean") else v) for k, v in d.items()))
def test_unsupported_settings_raise_before_any_engine(no_engine, over):
    from mjmpc_amd.control import BatchedRandomShooting
    with pytest.raises(ValueError):
        BatchedRandomShooting(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedRandomShooting
    for over in (dict(), dict(step_size=0.0), dict(step_size=1.0), dict(num_particles=50), dict(num_episodes=1, seeds=[9]),
                 dict(init_cov=[0.1, 0.2, 0.3, 0.4], step_size=[1.0, 0.9, 0.8, 0.7], base_action="repeat", dtype="f32",
                      seeds=np.arange(4), init_mean=np.zeros((4, 8, 6))),
                 dict(init_mean=np.full((8, 6), 0.1))):
        with pytest.raises(AssertionError, match="engine was created"):
            BatchedRandomShooting(**_kw(**over))


def test_per_episode_broadcasting(monkeypatch):
    """One value for every episode or one per episode, as they reach the batch's set-up."""
    from mjmpc_amd.control import BatchedRandomShooting, batched
    seen = {}

    def stop(self, raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean):
        seen.update(E=E, H=H, P=P, init_mean=init_mean)
        raise RuntimeError("far enough")
    monkeypatch.setattr(batched._EpisodeBatch, "_setup", stop)
    for P in (64, 50, 1000):
        with pytest.raises(RuntimeError, match="far enough"):
            BatchedRandomShooting(**_kw(num_particles=P))
        assert (seen["E"], seen["H"], seen["P"]) == (4, 8, P)
        assert seen["init_mean"].shape == (4, 8, 6) and not seen["init_mean"].any()
    one = np.random.RandomState(0).uniform(-1, 1, (8, 6))
    with pytest.raises(RuntimeError, match="far enough"):
        BatchedRandomShooting(**_kw(init_mean=one))
    assert all(np.array_equal(seen["init_mean"][e], one) for e in range(4))
    each = np.random.RandomState(1).uniform(-1, 1, (4, 8, 6))
    with pytest.raises(RuntimeError, match="far enough"):
        BatchedRandomShooting(**_kw(init_mean=each))
    assert np.array_equal(seen["init_mean"], each)
    a = batched._per_episode("step_size", 0.7, 4)
    assert a.shape == (4,) and np.all(a == 0.7)
    a = batched._per_episode("step_size", [1.0, 0.7, 0.4, 0.0], 4)
    assert a.tolist() == [1.0, 0.7, 0.4, 0.0]


def test_batched_random_shooting_is_exported():
    import mjmpc_amd.control as control
    from mjmpc_amd.control import BatchedRandomShooting
    from mjmpc_amd.control.batched import _EpisodeBatch
    assert "BatchedRandomShooting" in control.__all__
    assert issubclass(BatchedRandomShooting, _EpisodeBatch)
    for name in ("set_states", "get_states", "mean_action", "reset", "step", "run", "close", "on_env_reset",
                 "randomize_dynamics", "clear_dynamics", "best_particle"):
        assert hasattr(BatchedRandomShooting, name), name
    # the base class's, unchanged
    for name in ("run", "set_states", "get_states", "mean_action", "reset", "randomize_dynamics", "clear_dynamics", "close"):
        assert getattr(BatchedRandomShooting, name) is getattr(_EpisodeBatch, name), name


def test_new_entry_points_are_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "mjmpc_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name


def test_supported_shapes():
    ok = _lib.load().mjmpc_rs_batch_supported
    for good in ((1, 1, 1, 1), (3, 64, 8, 6), (2, 50, 8, 6), (65535, 256, 32, 6), (4, 2 ** 33, 32, 6), (4, 300, 3, 2),
                 (1, 64, 1, 24), (1, 64, 400, 256)):
        assert ok(*good) == 1, good
    for bad in ((0, 64, 8, 6), (65536, 64, 8, 6), (-1, 64, 8, 6), (3, 0, 8, 6), (3, -5, 8, 6), (3, 64, 0, 6), (3, 64, 8, 0),
                (3, 64, 8, 257)):
        assert ok(*bad) == 0, bad


def test_update_entry_point_rejects_bad_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
    F = _lib.F64
    upd = lib.mjmpc_rs_update_batch
    bad = [
        lambda: upd(F, 3, 64, 8, 6, None, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 6, fake, None, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 6, fake, fake, None, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 6, fake, fake, fake, 0, None, None, None, None, None),
        lambda: upd(F, 0, 64, 8, 6, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 65536, 64, 8, 6, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 0, 8, 6, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 0, 6, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 0, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 257, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(7, 3, 64, 8, 6, fake, fake, fake, 0, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 6, fake, fake, fake, 2, fake, None, None, None, None),
        lambda: upd(F, 3, 64, 8, 6, fake, fake, fake, -1, fake, None, None, None, None),
        lambda: upd(_lib.F32, 3, 64, 8, 6, fake, fake, fake, 3, fake, fake, fake, fake, None),
    ]
    for i, call in enumerate(bad):
        assert call() == E_BADARG, i
        assert len(lib.mjmpc_last_error()) > 0, i
