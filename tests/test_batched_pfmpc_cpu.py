"""CPU: ``BatchedPFMPC`` refuses what it does not run before any engine or device memory exists, broadcasts its
per-episode settings as the other batches do, and its entry points are declared, bound, built and reject bad arguments."""
import ctypes

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw

NEW_SYMBOLS = ["mjmpc_pf_batch_workspace_bytes", "mjmpc_pf_delta_batch", "mjmpc_pf_weights_batch", "mjmpc_pf_resample_batch",
               "mjmpc_pf_gather_shift_batch", "mjmpc_pf_finish_batch"]


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, cov_shift=0.02, cov_resample=0.3,
              lam=1.0, gamma=0.99, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    # (n_iters > 1 of the single path is not batched)
    dict(n_iters=0), dict(base_action="repeat", horizon=1), dict(seeds=[1, 2, 3, 4, 5]),
    # the controller's own values
    dict(lam=0.0), dict(lam=-1.0), dict(lam=[1.0, 1.0, 0.0, 1.0]), dict(cov_shift=-0.1), dict(cov_shift=[0.1, 0.0, -1e-9, 0.1]),
    dict(cov_resample=0.0), dict(cov_resample=-0.3), dict(cov_resample=[0.3, 0.3, 0.0, 0.3]),
    # per-episode arrays of the wrong length / shape
    dict(lam=[1.0] * 3), dict(cov_shift=np.zeros(5)), dict(cov_resample=np.ones((4, 2))),
    dict(raw_model=bc.rk4_hand()),
], ids=bc.refused_id())
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedPFMPC
    with pytest.raises(ValueError):
        BatchedPFMPC(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine); a zero cov_shift is one."""
    from mjmpc_amd.control import BatchedPFMPC
    bc.check_reaches_the_engine(BatchedPFMPC, [
        _kw(), _kw(cov_shift=0.0), _kw(keep_stages=True), _kw(filter_coeffs=[1.0, 0.0, 0.0]),
        _kw(lam=[0.5, 1.0, 2.0, 4.0], cov_shift=[0.0, 0.01, 0.02, 0.03], cov_resample=[0.1, 0.2, 0.3, 0.4],
            base_action="repeat", dtype="f32", seeds=np.arange(4))])


def test_per_episode_broadcasting(monkeypatch):
    """``lam``, ``cov_shift`` and ``cov_resample``: one value for every episode or one per episode, through ``_per_episode``."""
    from mjmpc_amd.control import BatchedPFMPC, batched
    seen = bc.stop_at_setup(monkeypatch)
    bc.check_stops_at_setup(BatchedPFMPC, _kw(lam=[0.5, 1.0, 2.0, 4.0], cov_shift=0.0, cov_resample=np.array([0.1, 0.2, 0.3, 0.4])),
                            seen, 4, 8, 64)
    assert seen["init_mean"].shape == (4, 8, 6) and not seen["init_mean"].any()        # (the means start at zero)
    for name in ("lam", "cov_shift", "cov_resample"):
        bc.check_per_episode(name, 0.45, [0.1, 0.2, 0.3, 0.4])
        for bad in ([0.1, 0.2], np.zeros((4, 1)), np.zeros((2, 4))):
            with pytest.raises(ValueError, match=name):
                batched._per_episode(name, bad, 4)


def test_batched_pfmpc_is_exported():
    from mjmpc_amd.control import BatchedCEM, BatchedMPPI
    cls = bc.check_exported("BatchedPFMPC", ("set_states", "get_states", "mean_action", "action_samples", "last_step", "reset",
                                             "step", "run", "close", "on_env_reset", "randomize_dynamics", "clear_dynamics"),
                            # the base class's parts are inherited, not copied
                            ("set_states", "get_states", "run", "_env_step", "randomize_dynamics", "clear_dynamics", "close"))
    assert not issubclass(cls, (BatchedMPPI, BatchedCEM))


def test_new_entry_points_are_declared_bound_and_built():
    bc.check_entry_points(NEW_SYMBOLS, abi=4)


def test_batch_workspace_is_e_rows_of_the_single_layout():
    lib = _lib.load()
    one, many = lib.mjmpc_pf_workspace_bytes, lib.mjmpc_pf_batch_workspace_bytes
    assert many(3, 100, 7, 5) == 3 * one(100, 7, 5) > 0
    assert many(1, 4100, 3, 2) == one(4100, 3, 2) and many(65535, 37, 1, 2) == 65535 * one(37, 1, 2)
    for bad in ((0, 100, 7, 5), (-1, 100, 7, 5), (65536, 100, 7, 5), (3, 0, 7, 5), (3, 100, 0, 5), (3, 100, 7, 0)):
        assert many(*bad) <= 0, bad


def test_batch_entry_points_reject_bad_arguments():
    lib = _lib.load()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)      # never dereferenced: every call below is refused
    F = _lib.F64
    delta, wts, res = lib.mjmpc_pf_delta_batch, lib.mjmpc_pf_weights_batch, lib.mjmpc_pf_resample_batch
    gat, fin = lib.mjmpc_pf_gather_shift_batch, lib.mjmpc_pf_finish_batch

    def g(E=3, M=64, H=8, A=6, sets=fake, idx=fake, mode=0, chols=fake, coeffs=None, seeds=fake, out=other, gathered=None, ws=fake):
        return lambda: gat(E, M, H, A, sets, idx, mode, chols, coeffs, seeds, 1, None, out, gathered, ws, None)
    bad = [
        # null pointers
        lambda: delta(F, 3, 64, 8, 6, None, fake, fake, None), lambda: delta(F, 3, 64, 8, 6, fake, None, fake, None),
        lambda: delta(F, 3, 64, 8, 6, fake, fake, None, None),
        lambda: wts(3, 64, None, fake, fake, 0, None, fake, fake, None), lambda: wts(3, 64, fake, None, fake, 0, None, fake, fake, None),
        lambda: wts(3, 64, fake, fake, None, 0, None, fake, fake, None), lambda: wts(3, 64, fake, fake, fake, 0, None, None, fake, None),
        lambda: wts(3, 64, fake, fake, fake, 0, None, fake, None, None),
        lambda: res(3, 64, None, fake, fake, fake, None), lambda: res(3, 64, fake, None, fake, fake, None),
        lambda: res(3, 64, fake, fake, None, fake, None), lambda: res(3, 64, fake, fake, fake, None, None),
        g(sets=None), g(idx=None), g(seeds=None), g(out=None), g(ws=None), g(chols=None),
        lambda: fin(3, 64, 8, 6, None, fake, None, None, None), lambda: fin(3, 64, 8, 6, fake, None, None, None, None),
        # E = 0 and E = 65536
        lambda: delta(F, 0, 64, 8, 6, fake, fake, fake, None), lambda: delta(F, 65536, 64, 8, 6, fake, fake, fake, None),
        lambda: wts(0, 64, fake, fake, fake, 0, None, fake, fake, None), lambda: wts(65536, 64, fake, fake, fake, 0, None, fake, fake, None),
        lambda: res(0, 64, fake, fake, fake, fake, None), lambda: res(65536, 64, fake, fake, fake, fake, None),
        g(E=0), g(E=65536),
        lambda: fin(0, 64, 8, 6, fake, fake, None, None, None), lambda: fin(65536, 64, 8, 6, fake, fake, None, None, None),
        # the single entry points' refusals: a gather in place, shift_mode 2, 'repeat' with H = 1, M outside 1 .. 2^31 - 1,
        # bad shapes, a dtype that is none
        g(out=fake), g(mode=2), g(mode=1, H=1), g(M=0), g(M=2 ** 31), g(H=0), g(A=0),
        lambda: delta(7, 3, 64, 8, 6, fake, fake, fake, None), lambda: delta(F, 3, 0, 8, 6, fake, fake, fake, None),
        lambda: wts(3, 0, fake, fake, fake, 0, None, fake, fake, None), lambda: res(3, 2 ** 31, fake, fake, fake, fake, None),
        lambda: fin(3, 0, 8, 6, fake, fake, None, None, None), lambda: fin(3, 64, 0, 6, fake, fake, None, None, None),
    ]
    for i, call in enumerate(bad):
        assert call() != 0, i
        assert len(lib.mjmpc_last_error()) > 0, i
