"""Inputs and numpy restatements shared by the device-mode PFMPC tests (tests/test_pfmpc_device_cpu.py checks the inputs on
the host, tests/test_pfmpc_device_gpu.py runs the kernels on them).  DESIGN 11 states the algorithm these restate."""
import numpy as np

import philox_ref as pr

SIZES = (8, 100, 4096, 65536)
WEIGHT_KINDS = ("softmax_lam0.01", "softmax_lam0.2", "softmax_lam5", "softmax_lam100", "exact_zeros", "one_hot", "equal")
POINTER_KINDS = ("zero", "half_step", "below_one_step", "beyond_total")


def weights(kind, M):
    rs = np.random.RandomState(M + len(kind))
    if kind.startswith("softmax_lam"):                  # peaked (lam 0.01) through flat (lam 100)
        x = -(20.0 * rs.rand(M)) / float(kind[len("softmax_lam"):])
        e = np.exp(x - x.max())
        return e / e.sum()
    if kind == "exact_zeros":
        w = rs.rand(M)
        w[rs.rand(M) < 0.3] = 0.0
        w[0] = 0.0                                      # (a zero in front: the first running sums are 0)
        w[-1] = 0.0                                     # (and a zero at the end: the total is reached before the last index)
        return w / w.sum()
    if kind == "one_hot":
        w = np.zeros(M)
        w[M // 3] = 1.0
        return w
    if kind == "equal":
        return np.full(M, 1.0 / M)
    raise KeyError(kind)


def pointer(kind, M):
    return {"zero": 0.0, "half_step": 1.0 / (2 * M), "below_one_step": float(np.nextafter(1.0 / M, 0.0)),
            "beyond_total": 1.5 / M}[kind]              # (the last pointer is (M + 0.5) / M: beyond any total of weights)


def serial_walk(cr, w, first):
    """``oracle.controllers_ref.pf_resample``'s serial walk (``cr``: that module) with ITS draw replaced by ``first``: the
    indices it selects, read off a set whose particle m holds the number m."""
    M = w.shape[0]
    real = cr.random.uniform
    cr.random.uniform = lambda lo, hi: first
    try:
        out, _ = cr.pf_resample(np.arange(M, dtype=np.float64).reshape(M, 1, 1), w, 0)
    finally:
        cr.random.uniform = real
    return out[:, 0, 0].astype(np.int64)


def first_pointer_ref(seed, k, M):
    """The device's first pointer: (1.0 / M) * double(u), u the first float32 uniform of the Philox block keyed
    (seed, offset k, chan 2^64 - 1, quad 0)."""
    u = pr.uniforms_and_angles(pr.normal_words(seed, k, 2 ** 64 - 1, 0))[0]
    assert u.dtype == np.float32
    return (1.0 / M) * np.float64(u)


def shift_ref(resampled, cov_shift, filter_coeffs, seed, k, base_action):
    """The reference's ``_shift`` (particle_filter_controller.py:127-150) on the resampled set with the device's Philox
    jitter of offset k + 1: (shifted set, per-element bound on what the device's transcendental units may add)."""
    M, H, A = resampled.shape
    fc = tuple(float(c) for c in filter_coeffs)
    coeffs = None if fc == (1.0, 0.0, 0.0) else fc
    jitter, scale = pr.sample_ref(M, H, A, np.sqrt(cov_shift) * np.eye(A), seed, k + 1, 0, True, coeffs, np.float64, True)
    bound = pr.error_bound(jitter, scale, coeffs)
    moved = resampled.copy()
    moved[:, :-1] = moved[:, 1:]
    moved = moved + jitter
    if base_action == "null":
        moved[:, -1] = 0.0
        bound[:, -1] = 0.0
    elif base_action == "repeat":                       # the JITTERED row H - 2
        moved[:, -1] = moved[:, -2]
        bound[:, -1] = bound[:, -2]
    else:
        raise KeyError(base_action)
    return moved, bound + 2.0 * np.spacing(np.abs(moved))          # (+ the rounding of the sum itself)
