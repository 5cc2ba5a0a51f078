"""CPU: ``BatchedPFMPC`` refuses what it does not run before any engine or device memory exists, broadcasts its
per-episode settings as the other batches do, and its entry points are declared, bound, built and reject bad arguments."""
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
NEW_SYMBOLS = ["mjmpc_pf_batch_workspace_bytes", "mjmpc_pf_delta_batch", "mjmpc_pf_weights_batch", "mjmpc_pf_resample_batch",
               "mjmpc_pf_gather_shift_batch", "mjmpc_pf_finish_batch"]


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, cov_shift=0.02, cov_resample=0.3,
              lam=1.0, gamma=0.99, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
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
    # what _check_common refuses (n_iters > 1 of the single path is not batched)
    dict(n_iters=2), dict(n_iters=0), dict(sample_mode="sample"), dict(gamma=0.0), dict(dtype="f16"), dict(num_episodes=0),
    dict(num_episodes=65536), dict(horizon=0), dict(num_particles=0), dict(filter_coeffs=[1.0, 0.0]),
    dict(base_action="random"), dict(base_action="zeros"), dict(base_action="repeat", horizon=1),
    # the controller's own values
    dict(lam=0.0), dict(lam=-1.0), dict(lam=[1.0, 1.0, 0.0, 1.0]), dict(cov_shift=-0.1), dict(cov_shift=[0.1, 0.0, -1e-9, 0.1]),
    dict(cov_resample=0.0), dict(cov_resample=-0.3), dict(cov_resample=[0.3, 0.3, 0.0, 0.3]),
    # per-episode arrays of the wrong length / shape
    dict(lam=[1.0] * 3), dict(cov_shift=np.zeros(5)), dict(cov_resample=np.ones((4, 2))),
    dict(seeds=[1, 2, 3]), dict(seeds=7), dict(seeds=[1, 2, 3, -4]), dict(seeds=[1, 2, 3, 4, 5]),
    # a model the tree engine refuses: RK4 beyond 16 dofs
    dict(raw_model=dataclasses.replace(hand24_raw(), integrator="RK4")),
], ids=lambda d: ",".join("%s=%s" % (k, type(v).__name__ if k == "raw_model" else v) for k, v in d.items()))
def test_unsupported_settings_raise_before_any_engine(no_engine, over):
    from mjmpc_amd.control import BatchedPFMPC
    with pytest.raises(ValueError):
        BatchedPFMPC(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):
    """The settings the batch runs pass the checks (and then get as far as making the engine); a zero cov_shift is one."""
    from mjmpc_amd.control import BatchedPFMPC
    for over in (dict(), dict(cov_shift=0.0), dict(keep_stages=True), dict(filter_coeffs=[1.0, 0.0, 0.0]),
                 dict(lam=[0.5, 1.0, 2.0, 4.0], cov_shift=[0.0, 0.01, 0.02, 0.03], cov_resample=[0.1, 0.2, 0.3, 0.4],
                      base_action="repeat", dtype="f32", seeds=np.arange(4))):
        with pytest.raises(AssertionError, match="engine was created"):
            BatchedPFMPC(**_kw(**over))


def test_per_episode_broadcasting(monkeypatch):
    """``lam``, ``cov_shift`` and ``cov_resample``: one value for every episode or one per episode, through ``_per_episode``."""
    from mjmpc_amd.control import BatchedPFMPC, batched
    seen = {}

    def stop(self, raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean):
        seen.update(E=E, H=H, P=P, mean=init_mean)
        raise RuntimeError("far enough")
    monkeypatch.setattr(batched._EpisodeBatch, "_setup", stop)
    with pytest.raises(RuntimeError, match="far enough"):
        BatchedPFMPC(**_kw(lam=[0.5, 1.0, 2.0, 4.0], cov_shift=0.0, cov_resample=np.array([0.1, 0.2, 0.3, 0.4])))
    assert (seen["E"], seen["H"], seen["P"]) == (4, 8, 64)
    assert seen["mean"].shape == (4, 8, 6) and not seen["mean"].any()        # (the means start at zero)
    for name in ("lam", "cov_shift", "cov_resample"):
        a = batched._per_episode(name, 0.45, 4)
        assert a.shape == (4,) and a.dtype == np.float64 and np.all(a == 0.45)
        a = batched._per_episode(name, [0.1, 0.2, 0.3, 0.4], 4)
        assert a.tolist() == [0.1, 0.2, 0.3, 0.4]
        for bad in ([0.1, 0.2], np.zeros((4, 1)), np.zeros((2, 4))):
            with pytest.raises(ValueError, match=name):
                batched._per_episode(name, bad, 4)


def test_batched_pfmpc_is_exported():
    import mjmpc_amd.control as control
    from mjmpc_amd.control import BatchedCEM, BatchedMPPI, BatchedPFMPC
    from mjmpc_amd.control.batched import _EpisodeBatch
    assert "BatchedPFMPC" in control.__all__
    assert issubclass(BatchedPFMPC, _EpisodeBatch) and not issubclass(BatchedPFMPC, (BatchedMPPI, BatchedCEM))
    for name in ("set_states", "get_states", "mean_action", "action_samples", "last_step", "reset", "step", "run", "close",
                 "on_env_reset", "randomize_dynamics", "clear_dynamics"):
        assert hasattr(BatchedPFMPC, name), name
    # the base class's parts are inherited, not copied
    for name in ("set_states", "get_states", "run", "_env_step", "randomize_dynamics", "clear_dynamics", "close"):
        assert getattr(BatchedPFMPC, name) is getattr(_EpisodeBatch, name), name


def test_new_entry_points_are_declared_bound_and_built():
    with open(os.path.join(ROOT, "include", "mjmpc_amd.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert re.search(r"#define\s+MJMPC_ABI_VERSION\s+4\b", header)          # additions do not move the version
    assert _lib.ABI_VERSION == 4 and lib.mjmpc_abi_version() == 4


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
