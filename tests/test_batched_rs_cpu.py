"""CPU: ``BatchedRandomShooting`` refuses what it does not run before any engine or device memory exists,
broadcasts its per-episode settings as ``BatchedMPPI`` does, and its entry points are declared, bound, built and reject bad
arguments."""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw

NEW_SYMBOLS = ["mjmpc_rs_batch_supported", "mjmpc_rs_update_batch"]
E_BADARG = -1               # (MJMPC_E_BADARG of include/mjmpc_amd.h)


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, step_size=0.7, init_cov=0.3, gamma=1.0,
              filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    dict(use_zero_control_seq=True),
    # per-episode arrays of the wrong length / shape, and values random shooting cannot take
    dict(init_cov=[0.1] * 3), dict(step_size=np.ones(5)), dict(step_size=np.zeros((4, 2))), dict(init_mean=np.zeros((8, 5))),
    dict(init_mean=np.zeros((3, 8, 6))),
    dict(init_cov=[0.3, 0.3, -1.0, 0.3]), dict(init_cov=0.0), dict(step_size=-0.1), dict(step_size=[1.0, 0.7, -0.4, 0.2]),
    dict(init_cov=float("nan")), dict(step_size=float("nan")),
    dict(raw_model=bc.rk4_hand()),
], ids=bc.refused_id(("raw_model", "init_mean")))
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedRandomShooting
    with pytest.raises(ValueError):
        BatchedRandomShooting(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedRandomShooting
    bc.check_reaches_the_engine(BatchedRandomShooting, [
        _kw(), _kw(step_size=0.0), _kw(step_size=1.0), _kw(num_particles=50), _kw(num_episodes=1, seeds=[9]),
        _kw(init_cov=[0.1, 0.2, 0.3, 0.4], step_size=[1.0, 0.9, 0.8, 0.7], base_action="repeat", dtype="f32",
            seeds=np.arange(4), init_mean=np.zeros((4, 8, 6))),
        _kw(init_mean=np.full((8, 6), 0.1))])


def test_per_episode_broadcasting(monkeypatch):
    """One value for every episode or one per episode, as they reach the batch's set-up."""
    from mjmpc_amd.control import BatchedRandomShooting
    seen = bc.stop_at_setup(monkeypatch)
    for P in (64, 50, 1000):
        bc.check_stops_at_setup(BatchedRandomShooting, _kw(num_particles=P), seen, 4, 8, P)
        assert seen["init_mean"].shape == (4, 8, 6) and not seen["init_mean"].any()
    one = np.random.RandomState(0).uniform(-1, 1, (8, 6))
    bc.check_stops_at_setup(BatchedRandomShooting, _kw(init_mean=one), seen, 4, 8, 64)
    assert all(np.array_equal(seen["init_mean"][e], one) for e in range(4))
    each = np.random.RandomState(1).uniform(-1, 1, (4, 8, 6))
    bc.check_stops_at_setup(BatchedRandomShooting, _kw(init_mean=each), seen, 4, 8, 64)
    assert np.array_equal(seen["init_mean"], each)
    bc.check_per_episode("step_size", 0.7, [1.0, 0.7, 0.4, 0.0])


def test_batched_random_shooting_is_exported():
    bc.check_exported("BatchedRandomShooting",
                      ("set_states", "get_states", "mean_action", "reset", "step", "run", "close", "on_env_reset",
                       "randomize_dynamics", "clear_dynamics", "best_particle"),
                      # the base class's, unchanged
                      ("run", "set_states", "get_states", "mean_action", "reset", "randomize_dynamics", "clear_dynamics", "close"))


def test_new_entry_points_are_declared_bound_and_built():
    bc.check_entry_points(NEW_SYMBOLS)


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
