"""CPU: ``BatchedCEM`` refuses what it does not run before any engine or device memory exists, broadcasts its
per-episode settings as ``BatchedMPPI`` does, and its entry points are declared, bound, built and reject bad arguments."""
import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw

NEW_SYMBOLS = ["mjmpc_cem_batch_supported", "mjmpc_cem_batch_workspace_bytes", "mjmpc_cem_select_moments_batch",
               "mjmpc_cem_finish_batch"]


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, init_cov=0.3, elite_frac=0.1,
              step_size=1.0, beta=0.45, gamma=1.0, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    dict(use_zero_control_seq=True), dict(cov_type="full_AxA"), dict(cov_type="sigma_I"),
    # an episode without an elite particle (int(64 * 0.01) = 0), or with more elites than particles
    dict(elite_frac=0.01), dict(elite_frac=[0.1, 0.1, 0.001, 0.1]), dict(elite_frac=1.5),
    # shapes outside the batched fused CEM step: P > 32768, A = 6 > H + 1
    dict(num_particles=32769), dict(horizon=4),
    # per-episode arrays of the wrong length / shape, and values CEM cannot take
    dict(init_cov=[0.1] * 3), dict(elite_frac=[0.1, 0.2]), dict(step_size=np.ones(5)), dict(beta=np.zeros((4, 2))),
    dict(init_cov=[0.3, 0.3, -1.0, 0.3]),
    dict(raw_model=bc.rk4_hand()),
], ids=bc.refused_id())
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedCEM
    with pytest.raises(ValueError):
        BatchedCEM(**_kw(**over))


def test_the_shape_refusal_states_the_limits(no_engine):                    # noqa: F811
    from mjmpc_amd.control import BatchedCEM
    with pytest.raises(ValueError) as ei:
        BatchedCEM(**_kw(num_particles=32769))
    for limit in ("A <= 8", "A <= H + 1", "P <= 32768"):
        assert limit in str(ei.value)


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedCEM
    bc.check_reaches_the_engine(BatchedCEM, [_kw(), _kw(cov_type="diagonal"), _kw(
        init_cov=[0.1, 0.2, 0.3, 0.4], elite_frac=[1 / 64, 0.1, 0.5, 1.0], step_size=[1.0, 0.9, 0.8, 0.7],
        beta=[0.0, 0.45, 0.2, 1.0], base_action="repeat", dtype="f32", seeds=np.arange(4))])


def test_per_episode_broadcasting_and_num_elite(monkeypatch):
    """One value for every episode or one per episode; num_elite_e = int(num_particles * elite_frac_e) as cem.py computes it."""
    from mjmpc_amd.control import BatchedCEM
    seen = bc.stop_at_setup(monkeypatch)
    fracs = [0.1, 0.3, 1 / 3, 0.999]
    for P in (64, 50, 1000):
        bc.check_stops_at_setup(BatchedCEM, _kw(num_particles=P, elite_frac=fracs), seen, 4, 8, P)
    assert [int(1000 * f) for f in fracs] == [100, 300, 333, 999]          # (what the check below compares against)
    bc.check_per_episode("beta", 0.45, [0.1, 0.2, 0.3, 0.4])
    # the elite counts the constructor derives (it raises when one of them is 0)
    with pytest.raises(ValueError, match=r"\[6, 0, 6, 6\]"):
        BatchedCEM(**_kw(elite_frac=[0.1, 0.015, 0.1, 0.1]))
    with pytest.raises(ValueError, match=r"\[100, 300, 333, 1001\]"):
        BatchedCEM(**_kw(num_particles=1000, elite_frac=[0.1, 0.3, 1 / 3, 1.0015]))


def test_batched_cem_is_exported():
    bc.check_exported("BatchedCEM", ("set_states", "get_states", "mean_action", "reset", "step", "run", "close", "on_env_reset",
                                     "randomize_dynamics", "clear_dynamics", "cov"), ())
    bc.check_exported("BatchedMPPI", (), ())


def test_new_entry_points_are_declared_bound_and_built():
    bc.check_entry_points(NEW_SYMBOLS)


def test_supported_shapes_and_workspace():
    lib = _lib.load()
    ok = lib.mjmpc_cem_batch_supported
    assert ok(3, 64, 6, 8, 6) == 1 and ok(1, 256, 25, 32, 6) == 1 and ok(65535, 64, 64, 8, 6) == 1
    assert ok(16, 32768, 3276, 32, 8) == 1
    for bad in ((0, 64, 6, 8, 6), (65536, 64, 6, 8, 6), (3, 64, 0, 8, 6), (3, 64, 65, 8, 6), (3, 32769, 6, 8, 6),
                (3, 64, 6, 8, 9), (3, 64, 6, 4, 6), (3, 0, 1, 8, 6), (3, 64, 6, 0, 6)):
        assert ok(*bad) == 0, bad
        assert lib.mjmpc_cem_batch_workspace_bytes(*bad) < 0, bad
        assert len(lib.mjmpc_last_error()) > 0
    # every row is what mjmpc_cem_fused_supported takes
    for P, k, H, A in ((64, 6, 8, 6), (50, 25, 8, 6), (256, 25, 32, 6), (1024, 102, 32, 7)):
        assert lib.mjmpc_cem_fused_supported(P, P, k, H, A) == 1 and ok(2, P, k, H, A) == 1
    # one block per episode: the size is linear in E and does not depend on k_max (the launches see k on the device only)
    one = lib.mjmpc_cem_batch_workspace_bytes(1, 64, 6, 8, 6)
    assert one > 8 * (64 // 2 + 8 * 6 + 6 * 6) and one % 8 == 0
    assert lib.mjmpc_cem_batch_workspace_bytes(5, 64, 6, 8, 6) == 5 * one
    assert lib.mjmpc_cem_batch_workspace_bytes(1, 64, 64, 8, 6) == one


def test_batch_entry_points_reject_bad_arguments():
    import ctypes
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
    F = _lib.F64
    sel = lib.mjmpc_cem_select_moments_batch
    fin = lib.mjmpc_cem_finish_batch
    bad = [
        lambda: sel(F, 3, 64, 8, 6, None, fake, fake, fake, fake, None, fake, None),
        lambda: sel(F, 3, 64, 8, 6, fake, None, fake, fake, fake, None, fake, None),
        lambda: sel(F, 3, 64, 8, 6, fake, fake, None, fake, fake, None, fake, None),
        lambda: sel(F, 3, 64, 8, 6, fake, fake, fake, None, fake, None, fake, None),
        lambda: sel(F, 3, 64, 8, 6, fake, fake, fake, fake, None, None, fake, None),
        lambda: sel(F, 3, 64, 8, 6, fake, fake, fake, fake, fake, None, None, None),
        lambda: sel(F, 0, 64, 8, 6, fake, fake, fake, fake, fake, None, fake, None),
        lambda: sel(F, 65536, 64, 8, 6, fake, fake, fake, fake, fake, None, fake, None),
        lambda: sel(F, 3, 32769, 8, 6, fake, fake, fake, fake, fake, None, fake, None),
        lambda: sel(F, 3, 64, 8, 9, fake, fake, fake, fake, fake, None, fake, None),
        lambda: sel(7, 3, 64, 8, 6, fake, fake, fake, fake, fake, None, fake, None),
        lambda: fin(F, 3, 64, 8, 6, None, 1, fake, 0, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, None, 0, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, fake, 0, None, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, fake, 0, fake, None, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, fake, 0, fake, fake, None, None, None, None, None, None, None, None, 0, None, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, fake, 2, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 8, 6, fake, 1, fake, 0, fake, fake, None, None, None, None, None, None, fake, None, 0, fake, None),
        lambda: fin(F, 0, 64, 8, 6, fake, 1, fake, 0, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(F, 3, 64, 4, 6, fake, 1, fake, 0, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
        lambda: fin(9, 3, 64, 8, 6, fake, 1, fake, 0, fake, fake, None, None, None, None, None, None, None, None, 0, fake, None),
    ]
    for i, call in enumerate(bad):
        assert call() != 0, i
        assert len(lib.mjmpc_last_error()) > 0, i
