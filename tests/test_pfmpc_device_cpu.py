"""CPU: what ``PFMPC(noise_mode='device')`` decides without a device - its refusals, the new entry points in the header,
the binding and the built library - and the condition on the resampling tests' inputs: on every one of them
``systematic_resample_indices`` agrees with the serial walk of ``oracle.controllers_ref.pf_resample`` wherever the pointer
is positive (tests/test_pfmpc_device_gpu.py then holds the kernel to ``systematic_resample_indices``)."""
import os
import re

import numpy as np
import pytest

import pfmpc_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mjmpc_pf_workspace_bytes", "mjmpc_pf_weights", "mjmpc_pf_resample", "mjmpc_pf_gather_shift",
               "mjmpc_pf_finish", "mjmpc_pf_delta")


def _kw(**extra):
    kw = dict(d_state=5, d_obs=6, d_action=3, horizon=8, cov_shift=0.1, cov_resample=1.0, base_action="null", lam=0.5,
              num_particles=64, gamma=0.99, n_iters=1, action_lows=-np.ones(3), action_highs=np.ones(3), seed=1)
    kw.update(extra)
    return kw


class _NoDevice:
    """Stands where the device side would be made: reaching it means the constructor did not refuse first."""

    def __init__(self, *a, **k):
        raise AssertionError("device memory was about to be allocated")


@pytest.fixture
def no_device(monkeypatch):
    from mjmpc_amd.control import controller
    monkeypatch.setattr(controller, "DeviceUpdater", _NoDevice)


class _TwoRanks:
    rank, world_size = 0, 2


def test_device_mode_refuses_the_random_tail(no_device):
    from mjmpc_amd.control import PFMPC
    with pytest.raises(ValueError, match="base_action"):
        PFMPC(noise_mode="device", **_kw(base_action="random"))


def test_device_mode_refuses_sharded_runs(no_device):
    from mjmpc_amd.control import PFMPC
    with pytest.raises(ValueError, match="one GPU"):
        PFMPC(noise_mode="device", comm=_TwoRanks(), **_kw())


def test_device_mode_refuses_a_host_rollout_fn(no_device):
    from mjmpc_amd.control import PFMPC

    def host_rollout_fn(num_particles, horizon, mean, noise, mode):
        raise AssertionError("not called")

    with pytest.raises(ValueError, match="rollout_fn"):
        PFMPC(noise_mode="device", rollout_fn=host_rollout_fn, **_kw())


def test_unknown_noise_mode_raises(no_device):
    from mjmpc_amd.control import PFMPC
    with pytest.raises(ValueError, match="noise_mode"):
        PFMPC(noise_mode="device_mt19937", **_kw())


def test_new_entry_points_are_declared_bound_and_built():
    from mjmpc_amd import _lib
    with open(os.path.join(ROOT, "include", "mjmpc_amd.h")) as f:
        header = f.read()
    assert re.search(r"#define MJMPC_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4       # additions only
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    assert lib.mjmpc_pf_workspace_bytes(100, 7, 5) == 8 * (100 + 4 * 35)        # running sums | 4 chunks of 32 particles


@pytest.mark.parametrize("M", pc.SIZES)
@pytest.mark.parametrize("kind", pc.WEIGHT_KINDS)
def test_resampling_inputs_agree_with_the_serial_walk(kind, M):
    from mjmpc_amd.control.particle_filter_controller import systematic_resample_indices
    from oracle import controllers_ref as cr
    w = pc.weights(kind, M)
    assert w.shape == (M,) and (w >= 0).all() and abs(w.sum() - 1.0) < 1e-9
    for pk in pc.POINTER_KINDS:
        first = pc.pointer(pk, M)
        pointers = first + np.arange(M) * 1.0 / M * 1.0
        idx = systematic_resample_indices(w, first)
        walk = pc.serial_walk(cr, w, first)
        pos = pointers > 0.0
        assert np.array_equal(idx[pos], walk[pos]), (kind, M, pk)
        assert (idx[~pos] == -1).all() and (walk[~pos] == M - 1).all()          # index -1 IS the last particle
        if pk == "beyond_total":
            assert pointers[-1] > np.cumsum(w)[-1] and idx[-1] == M - 1
        if pk == "below_one_step":
            assert 0.0 < first < 1.0 / M


def test_first_pointer_restatement_is_a_uniform_below_one_step():
    for seed, k in ((0, 0), (123, 7), (2 ** 63 + 12345, 3), (2 ** 64 - 1, 2 ** 33 + 5)):
        for M in (8, 4096):
            f = pc.first_pointer_ref(seed, k, M)
            assert 0.0 < f <= 1.0 / M
    assert pc.first_pointer_ref(5, 1, 64) != pc.first_pointer_ref(5, 2, 64)
    assert pc.first_pointer_ref(5, 1, 64) != pc.first_pointer_ref(6, 1, 64)
