"""CPU: ``BatchedDMDMPC`` refuses what it does not run before any engine or device memory exists, broadcasts its
per-episode settings as the other batches do, and its entry points are declared, bound, built and reject bad arguments."""
import ctypes
import types

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw

NEW_SYMBOLS = ["mjmpc_cholesky_lower_batch", "mjmpc_sample_noise_cov_batch", "mjmpc_dmd_batch_workspace_bytes",
               "mjmpc_dmd_update_batch"]


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, lam=0.2, step_size=1.0,
              init_cov=0.3, beta=0.05, gamma=1.0, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    dict(use_zero_control_seq=True),
    # values DMD-MPC cannot take, for every episode or for one of them
    dict(lam=0.0), dict(lam=[0.2, 0.2, -0.1, 0.2]), dict(init_cov=0.0), dict(init_cov=[0.3, 0.3, -1.0, 0.3]),
    dict(beta=-0.1), dict(beta=[0.0, 0.1, -1e-9, 0.1]),
    # covariance types the batch does not run
    dict(cov_type="full_AxA"), dict(cov_type="sigma_I"),
    # the arithmetic of BatchedMPPI
    dict(update_cov=False),
    # per-episode arrays of the wrong length / shape
    dict(lam=[0.1] * 3), dict(step_size=np.ones(5)), dict(beta=np.zeros((4, 2))), dict(init_cov=[0.3, 0.3]),
    dict(init_mean=np.zeros((8, 5))),
    dict(raw_model=bc.rk4_hand()),
], ids=bc.refused_id(("raw_model", "init_mean")))
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedDMDMPC
    with pytest.raises(ValueError):
        BatchedDMDMPC(**_kw(**over))


def test_update_cov_false_names_batched_mppi(no_engine):                    # noqa: F811
    from mjmpc_amd.control import BatchedDMDMPC
    with pytest.raises(ValueError, match="BatchedMPPI"):
        BatchedDMDMPC(**_kw(update_cov=False))


def test_more_than_64_action_channels_are_refused(no_engine, monkeypatch):  # noqa: F811
    """A > 64 is the limit of the Cholesky kernel: refused on the compiled model's nu, before the engine."""
    from mjmpc_amd.control import BatchedDMDMPC, batched
    for nu, ok in ((64, True), (65, False)):
        monkeypatch.setattr(batched._EpisodeBatch, "_compile", staticmethod(lambda raw, nu=nu: types.SimpleNamespace(nu=nu)))
        with pytest.raises(AssertionError if ok else ValueError, match="engine was created" if ok else "64"):
            BatchedDMDMPC(**_kw())


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedDMDMPC
    bc.check_reaches_the_engine(BatchedDMDMPC, [
        _kw(), _kw(cov_type="diagonal"), _kw(cov_type="full", update_cov=True), _kw(beta=0.0),
        _kw(init_mean=np.full((8, 6), 0.1)), _kw(init_mean=np.zeros((4, 8, 6))),
        _kw(lam=[0.1, 0.2, 0.3, 0.4], step_size=[1.0, 0.7, 0.5, 0.0], init_cov=[0.1, 0.2, 0.3, 0.4],
            beta=[0.0, 0.05, 0.2, 1.0], base_action="repeat", dtype="f32", seeds=np.arange(4), filter_coeffs=[1.0, 0.0, 0.0])])


def test_per_episode_broadcasting(monkeypatch):
    """One value for every episode or one per episode reaches the batch as float64 [E] (``_per_episode``)."""
    from mjmpc_amd.control import BatchedDMDMPC, batched
    seen = bc.stop_at_setup(monkeypatch)
    for P in (64, 50, 1043):
        bc.check_stops_at_setup(BatchedDMDMPC, _kw(num_particles=P, lam=[0.1, 0.2, 0.3, 0.4]), seen, 4, 8, P)
        assert seen["init_mean"].shape == (4, 8, 6) and not seen["init_mean"].any()
    bc.check_stops_at_setup(BatchedDMDMPC, _kw(init_mean=np.full((8, 6), 0.25)), seen, 4, 8, 64)
    assert seen["init_mean"].shape == (4, 8, 6) and np.all(seen["init_mean"] == 0.25)
    bc.check_per_episode("beta", 0.05, [0.1, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match="beta"):
        batched._per_episode("beta", [0.1, 0.2], 4)


def test_batched_dmdmpc_is_exported():
    bc.check_exported("BatchedDMDMPC", ("set_states", "get_states", "mean_action", "reset", "step", "run", "close",
                                        "on_env_reset", "randomize_dynamics", "clear_dynamics", "cov"),
                      ("randomize_dynamics", "set_states", "get_states", "run"))         # (from the base class, unchanged)


def test_new_entry_points_are_declared_bound_and_built():
    bc.check_entry_points(NEW_SYMBOLS, abi=4)


def test_workspace_is_positive_and_grows_with_E():
    lib = _lib.load()
    size = lib.mjmpc_dmd_batch_workspace_bytes
    for P, H, A in ((64, 8, 6), (50, 8, 6), (1043, 7, 9), (256, 32, 6), (16, 1, 1), (64, 8, 64)):
        one = size(1, P, H, A)
        nb, rec = (P + 15) // 16, 1 + H * A + A * A
        # per episode: a weight per particle, ceil(P / 16) partials and one record
        assert one >= 8 * (P + nb * rec + 2 + H * A + A * A) and one % 8 == 0, (P, H, A)
        assert size(2, P, H, A) == 2 * one and size(65535, P, H, A) == 65535 * one, (P, H, A)
    for bad in ((0, 64, 8, 6), (65536, 64, 8, 6), (-1, 64, 8, 6), (3, 0, 8, 6), (3, 64, 0, 6), (3, 64, 8, 0), (3, 64, 8, 65)):
        assert size(*bad) == -1, bad          # (MJMPC_E_BADARG)
        assert len(lib.mjmpc_last_error()) > 0


def test_batch_entry_points_reject_bad_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
    F, BADARG = _lib.F64, -1
    chol, draw, upd = lib.mjmpc_cholesky_lower_batch, lib.mjmpc_sample_noise_cov_batch, lib.mjmpc_dmd_update_batch

    def update(dtype=F, E=3, P=64, H=8, A=6, costs=fake, actions=fake, gseq=fake, lam=fake, step=fake, cov_mode=2, beta=fake,
               shift=0, means=fake, covs=fake, ws=fake):
        return upd(dtype, E, P, H, A, costs, actions, gseq, lam, step, cov_mode, beta, shift, means, covs, None, None, ws, None)

    bad = [
        lambda: chol(3, None, 6, fake, None, None),
        lambda: chol(3, fake, 6, None, None, None),
        lambda: chol(0, fake, 6, fake, None, None),
        lambda: chol(65536, fake, 6, fake, None, None),
        lambda: chol(3, fake, 65, fake, None, None),
        lambda: chol(3, fake, 0, fake, None, None),
        lambda: draw(F, 3, None, 64, 8, 6, fake, None, fake, 0, None, 0, None),
        lambda: draw(F, 3, fake, 64, 8, 6, None, None, fake, 0, None, 0, None),
        lambda: draw(F, 3, fake, 64, 8, 6, fake, None, None, 0, None, 0, None),
        lambda: draw(F, 0, fake, 64, 8, 6, fake, None, fake, 0, None, 0, None),
        lambda: draw(F, 65536, fake, 64, 8, 6, fake, None, fake, 0, None, 0, None),
        lambda: draw(F, 3, fake, 64, 8, 65, fake, None, fake, 0, None, 0, None),
        lambda: draw(F, 3, fake, 0, 8, 6, fake, None, fake, 0, None, 0, None),
        lambda: draw(7, 3, fake, 64, 8, 6, fake, None, fake, 0, None, 0, None),
        lambda: update(costs=None), lambda: update(actions=None), lambda: update(gseq=None), lambda: update(lam=None),
        lambda: update(step=None), lambda: update(beta=None), lambda: update(means=None), lambda: update(covs=None),
        lambda: update(ws=None),
        lambda: update(E=0), lambda: update(E=65536), lambda: update(A=65), lambda: update(A=0), lambda: update(P=0),
        lambda: update(H=0), lambda: update(cov_mode=0), lambda: update(cov_mode=3), lambda: update(shift=2),
        lambda: update(shift=-1), lambda: update(dtype=9),
    ]
    for i, call in enumerate(bad):
        assert call() == BADARG, i
        assert len(lib.mjmpc_last_error()) > 0, i
