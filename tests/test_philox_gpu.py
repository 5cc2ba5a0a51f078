"""GPU: every instantiation of the device Philox sampler (``csrc/noise_device.h``) against the numpy restatement of the
generator in tests/philox_ref.py, which tests/test_philox_ref_cpu.py holds to Philox4x32-10's published known-answer vectors.

Sites: ``noise_kernel`` (diagonal factor, or any factor with A > 8), ``noise_full_kernel`` (lower-triangular factor, A <= 8,
staged through LDS when H % 4 == 0, direct stores otherwise), ``noise_batch_kernel`` (episode batches), ``filter_kernel``, the
draw-ahead workgroups of ``mjmpc_mppi_fused_update_draw_next`` and ``mjmpc_cem_finish`` (csrc/update.hip) and the arm rollout's
in-kernel draw (csrc/arm_rollout_body.inc: ``mjmpc_arm_mppi_step``, ``mjmpc_arm_rollout_sampled``).

Every comparison has two parts, reported apart:

 1. WHICH VARIATE IS WHERE.  A wrong counter, key, round count, lane-to-element mapping or store address gives a value
    unrelated to the expected one (an error of order 1); this part asks for 1e-3 of the element's scale and so does not depend
    on the tolerance below.  Entries of the factor that are exactly zero are skipped by the kernels: exact 0.0 out.  Buffers
    carry a band of NaN in front and behind: idle lanes must write nothing.
 2. HOW WELL THE HARDWARE UNITS EVALUATE IT.  ``|z_gpu - z_ref| <= TOL * max(1, radius_ref)`` per normal, hence
    ``TOL * sum_b |L[a][b]| max(1, radius_b)`` per coloured sample, plus half a float32 ulp of every value a float32 buffer
    stores, carried through the filter with the coefficients' magnitudes (``philox_ref.error_bound``).  TOL is not read off
    the kernel: a correctly rounded float32 evaluation of the same transform (numpy float32 ``log2``, ``sqrt``, ``sin``,
    ``cos``) deviates from float64 by at most 4.30e-7 * max(1, radius) over 4.48 M variates (``philox_ref.F32_EVAL_ERROR``,
    re-measured by the CPU test), and the kernel is allowed 8 x that, TOL = 3.44e-6: v_log_f32, v_sqrt_f32, v_sin_f32 and
    v_cos_f32 are approximations of 1 - 2 ulp each, sine and cosine have an absolute, not a relative, error near their zeros,
    and the compiler may contract the multiply into the square root's argument.
    Measured on an MI355X (every test prints its worst ``|z_gpu - z_ref| / scale``): 2.36e-7 into float64 buffers (the
    headline shape's 917 504 variates; 2.35e-7 in the arm rollout's own draw), 2.64e-7 into float32 buffers, rounding of the
    stored value included - 0.55 x the CPU float32 figure, 0.07 x the tolerance.

The arm rollout filters on the fly with ``filter_kernel``'s recurrence and float64 carry, and its normals come from the same
hardware units, so against the reference the transcendental tolerance applies there too (plus the rounding of
``mean + eps`` in the engine's type); bit equality BETWEEN the GPU sites is what tests/test_mono_step_gpu.py,
tests/test_cem_fused_gpu.py and tests/test_controllers_gpu.py already assert."""
import ctypes

import numpy as np
import pytest

import philox_ref as pr

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements of NaN in front of and behind every buffer a kernel writes
COARSE = 1e-3 / pr.TOL          # part 1 asks for 1e-3 of the element's scale
DTYPES = ["f64", "f32"]
SEEDS_HI = [2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345, 2 ** 64 - 1]
OFFSETS_HI = [2 ** 32 - 1, 2 ** 32 + 7]


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _lib():
    from mjmpc_amd import _lib
    return _lib, _lib.require_gpu()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """n elements on the device between two bands of NaN."""

    def __init__(self, n, dtype):
        import torch
        self.n = n
        self.all = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32 if dtype == "f32" else torch.float64,
                              device="cuda")
        self.view = self.all[GUARD:GUARD + n]

    def read(self, shape):
        import torch
        torch.cuda.synchronize()
        host = self.all.cpu().numpy()
        assert np.isnan(host[:GUARD]).all() and np.isnan(host[GUARD + self.n:]).all(), "a store outside the buffer"
        return host[GUARD:GUARD + self.n].reshape(shape).copy()


def _dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype).reshape(-1).copy()).cuda()


def draw(P, H, A, chol, seed, offset, particle_offset=0, diag_only=False, coeffs=None, dtype="f64", d_step=None):
    """``mjmpc_sample_noise`` into a guarded buffer -> numpy [P][H][A]"""
    import torch
    L, lib = _lib()
    buf = Guarded(P * H * A, dtype)
    chol_d = _dev(chol)
    co_d = None if coeffs is None else _dev(coeffs)
    step_d = None if d_step is None else torch.tensor([d_step], dtype=torch.int64, device="cuda")
    L.check(lib.mjmpc_sample_noise(L.F32 if dtype == "f32" else L.F64, _vp(buf.view), P, H, A, _vp(chol_d), _vp(co_d), seed,
                                   offset, particle_offset, _vp(step_d), int(diag_only), _stream()))
    return buf.read((P, H, A))


def compare(got, ref, scale, coeffs, what, extra=None, f32=None):
    """The two-part comparison of the module docstring.  ``extra``: a further per-element allowance (roundings outside the
    sampler); ``f32``: the values went through a float32 buffer (default: ``got`` is one).  Returns and prints the worst
    deviation in units of the element's scale."""
    f32 = got.dtype == np.float32 if f32 is None else f32
    assert got.shape == ref.shape and np.isfinite(got).all(), "%s: shape or non-finite samples" % what
    bound = pr.error_bound(ref, scale.copy(), coeffs, f32)
    if extra is not None:
        bound = bound + extra
    err = np.abs(got.astype(np.float64) - ref)
    zero = scale == 0.0
    assert (got[zero] == 0.0).all(), "%s: a zero entry of the factor must give exact 0.0" % what
    live = ~zero
    wrong = err > COARSE * bound
    assert not wrong.any(), ("%s: WHICH VARIATE IS WHERE - %d of %d samples are unrelated to the reference (first at %s: %r, "
                             "expected %r)" % (what, wrong.sum(), wrong.size, np.argwhere(wrong)[0], got[wrong][0], ref[wrong][0]))
    worst = float((err[live] / bound[live]).max() * pr.TOL) if live.any() else 0.0
    print("%s [%s]: worst |gpu - ref| / scale = %.3e (tolerance %.2e = 8 x %.2e)"
          % (what, "f32" if f32 else "f64", worst, pr.TOL, pr.F32_EVAL_ERROR))
    over = err > bound
    assert not over.any(), ("%s: HARDWARE TRANSCENDENTALS - %d samples beyond the tolerance, worst scaled deviation %.3e against "
                            "%.2e" % (what, over.sum(), worst, pr.TOL))
    return worst


def check_draw(P, H, A, chol, seed, offset, particle_offset=0, diag_only=False, coeffs=None, dtype="f64", d_step=None,
               what="draw"):
    got = draw(P, H, A, chol, seed, offset, particle_offset, diag_only, coeffs, dtype, d_step)
    ref, scale = pr.sample_ref(P, H, A, chol, seed, offset + (d_step or 0), particle_offset, diag_only, coeffs, with_scale=True)
    compare(got, ref, scale, coeffs, "%s P=%d H=%d A=%d" % (what, P, H, A))
    return got


def diag_factor(A, rs, zero_at=None):
    """A factor whose diagonal is what a diagonal draw reads; everything else is junk that a diagonal draw must ignore."""
    L = rs.uniform(-2.0, 2.0, (A, A))
    L[np.arange(A), np.arange(A)] = rs.uniform(0.3, 1.7, A)
    if zero_at is not None:
        L[zero_at, zero_at] = 0.0
    return L


def lower_factor(A, rs):
    """Dense lower triangle with some exact zeros below the diagonal (and junk above it, which nothing may read)."""
    L = np.tril(rs.uniform(-1.0, 1.0, (A, A)))
    L[np.arange(A), np.arange(A)] = rs.uniform(0.3, 1.7, A)
    for a in range(2, A, 3):
        L[a, rs.randint(0, a)] = 0.0
    L += np.triu(rs.uniform(5.0, 9.0, (A, A)), 1)
    return L


# ---------------------------------------------------------------------------------------------------------------------------
# noise_kernel: one thread per (particle, channel, t-quad), workgroups of 256
DIAG_CASES = [(1, 1, 1), (63, 2, 7), (64, 3, 24), (65, 4, 64), (1000, 5, 7), (1000, 32, 1), (65, 33, 24), (1, 33, 64), (63, 32, 7),
              (64, 5, 1), (1000, 3, 64), (65, 1, 7), (1, 4, 24)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H,A", DIAG_CASES)
def test_diagonal_factor(P, H, A, dtype):
    """Partial last workgroup, H not a multiple of 4 (the ``t < H`` guard), a zero on the diagonal (exact 0.0 out); the
    off-diagonal entries of the factor are junk that ``diag_only`` must not read."""
    rs = np.random.RandomState(1000 * A + H)
    L = diag_factor(A, rs, zero_at=A // 2 if A > 1 else None)
    got = check_draw(P, H, A, L, 20231 + P, 3 + H, 0, True, None, dtype, what="noise_kernel diag")
    if A > 1:
        assert (got[:, :, A // 2] == 0.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_headline_shape(dtype):
    """The benchmark's draw (4096 x 32 x 7, diagonal factor, small seed and step): 917 504 variates - the largest sample
    this file takes of the hardware units' error."""
    L = np.diag(np.sqrt(np.full(7, 0.6)))
    for offset in (0, 1):
        check_draw(4096, 32, 7, L, 0, offset, 0, True, None, dtype, what="headline shape, step %d" % offset)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_zero_factor_gives_exact_zeros(dtype):
    got = draw(65, 5, 1, np.zeros((1, 1)), 5, 6, 0, True, None, dtype)
    assert (got == 0.0).all() and not np.signbit(got).any()
    got = draw(65, 5, 3, np.zeros((3, 3)), 5, 6, 0, False, None, dtype)
    assert (got == 0.0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A,H", [(9, 3), (9, 8), (24, 3), (24, 8)])
def test_full_factor_wide_action(A, H, dtype):
    """A > 8: the per-element kernel colours with the whole row of the factor."""
    L = lower_factor(A, np.random.RandomState(A * H))
    check_draw(37, H, A, L, 99, 12, 5, False, None, dtype, what="noise_kernel full")


# ---------------------------------------------------------------------------------------------------------------------------
# noise_full_kernel: one thread per (particle, t-quad), workgroups of one wavefront
FULL_CASES = [(1, 4, 7), (1, 1, 1), (37, 8, 8), (50, 4, 2), (129, 32, 7), (3, 4, 8), (200, 12, 1),      # staged through LDS
              (37, 5, 7), (21, 7, 2), (33, 30, 8), (1, 30, 1), (65, 1, 8), (1, 5, 7)]                      # direct stores


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H,A", FULL_CASES)
def test_full_factor_narrow_action(P, H, A, dtype):
    """P x ceil(H / 4) not a multiple of 64 and P = 1: the staged loop's ``first + i < total`` guard - idle lanes write
    nothing (the NaN bands around the buffer stay NaN)."""
    assert (P * ((H + 3) // 4)) % 64 != 0
    L = lower_factor(A, np.random.RandomState(100 * A + H))
    check_draw(P, H, A, L, 777 + H, 41, 9, False, None, dtype, what="noise_full_kernel %s" % ("staged" if H % 4 == 0 else "direct"))


# ---------------------------------------------------------------------------------------------------------------------------
# the high words of seed, offset and channel index
@pytest.mark.parametrize("diag_only,A", [(True, 7), (False, 7), (False, 24)])
@pytest.mark.parametrize("seed", SEEDS_HI)
def test_seed_high_word(seed, diag_only, A):
    L = diag_factor(A, np.random.RandomState(3)) if diag_only else lower_factor(A, np.random.RandomState(3))
    for offset in [5] + OFFSETS_HI:
        check_draw(8, 6, A, L, seed, offset, 0, diag_only, None, "f64", what="seed %#x offset %#x" % (seed, offset))


@pytest.mark.parametrize("diag_only,A", [(True, 7), (False, 7), (False, 24)])
def test_offset_high_word_is_not_the_seeds(diag_only, A):
    """The step offset's high word is XORed into the key: offset 2^32 + 7 is neither offset 7 nor seed ^ 2^32 at offset 7
    in the counter's own word (c3 = 7 in both) - the reference says which block each one is."""
    L = diag_factor(A, np.random.RandomState(4)) if diag_only else lower_factor(A, np.random.RandomState(4))
    a = check_draw(8, 6, A, L, 11, 2 ** 32 + 7, 0, diag_only, what="offset 2^32 + 7")
    b = check_draw(8, 6, A, L, 11, 7, 0, diag_only, what="offset 7")
    assert np.abs(a - b).max() > 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("diag_only,A", [(True, 7), (False, 7), (False, 24)])
def test_channel_index_crosses_2_to_32(diag_only, A, dtype):
    """(p + particle_offset) * A + b crosses 2^32 inside the draw: the counter's second word takes the carry."""
    po = 2 ** 32 // A - 3
    assert po * A < 2 ** 32 <= (po + 7) * A
    L = diag_factor(A, np.random.RandomState(5)) if diag_only else lower_factor(A, np.random.RandomState(5))
    check_draw(8, 6, A, L, 2 ** 63 + 12345, 2 ** 32 + 7, po, diag_only, None, dtype, what="channel index across 2^32")
    check_draw(8, 8, A, L, 31, 2, 2 ** 40 + 17, diag_only, None, dtype, what="particle_offset 2^40")


# ---------------------------------------------------------------------------------------------------------------------------
# the step counter on the device
@pytest.mark.parametrize("o,s", [(3, 4), (0, 1), (2 ** 32 - 5, 9), (7, 2 ** 32 + 1), (2 ** 32 + 7, 2 ** 33)])
@pytest.mark.parametrize("diag_only,A", [(True, 7), (False, 7), (False, 24)])
def test_device_step_counter(o, s, diag_only, A):
    """``d_step`` holding s with host offset o = host offset o + s without ``d_step`` (bit for bit) = the reference at o + s."""
    L = diag_factor(A, np.random.RandomState(6)) if diag_only else lower_factor(A, np.random.RandomState(6))
    a = check_draw(9, 6, A, L, 2 ** 32 + 77, o, 2, diag_only, d_step=s, what="d_step %#x + offset %#x" % (s, o))
    b = check_draw(9, 6, A, L, 2 ** 32 + 77, o + s, 2, diag_only, what="offset %#x" % (o + s))
    np.testing.assert_array_equal(a, b)


def test_device_updater_passes_64_bit_arguments_through():
    """``DeviceUpdater.sample_noise`` (what every other GPU test draws with): 64-bit seed, offset, particle_offset, d_step."""
    import torch
    from mjmpc_amd.control._device import DeviceUpdater
    P, H, A = 70, 6, 3
    dev = DeviceUpdater(H, A, np.ones(H))
    rs = np.random.RandomState(8)
    B = rs.randn(A, A)
    cov = B @ B.T + 0.3 * np.eye(A)
    co = [0.25, 0.8, 0.1]
    step = torch.tensor([2 ** 32 - 1], dtype=torch.int64, device="cuda")
    for dtype in DTYPES:
        got = dev.sample_noise(P, cov, co, 2 ** 64 - 1, 3, dtype=dtype, particle_offset=2 ** 33, d_step=step).cpu().numpy()
        chol = dev._rec["chol"].cpu().numpy().reshape(A, A)
        np.testing.assert_allclose(chol @ chol.T, cov, rtol=1e-13)
        ref, scale = pr.sample_ref(P, H, A, chol, 2 ** 64 - 1, 2 ** 32 + 2, 2 ** 33, False, co, with_scale=True)
        compare(got, ref, scale, co, "DeviceUpdater.sample_noise")
    # negative Python seeds are taken modulo 2^64
    got = dev.sample_noise(P, np.diag([0.5, 1.5, 0.8]), [1.0, 0.0, 0.0], -5, 0).cpu().numpy()
    chol = dev._rec["chol"].cpu().numpy().reshape(A, A)
    ref, scale = pr.sample_ref(P, H, A, chol, 2 ** 64 - 5, 0, 0, True, with_scale=True)
    compare(got, ref, scale, None, "seed -5")


# ---------------------------------------------------------------------------------------------------------------------------
# noise_batch_kernel
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [1, 3, 70])
def test_episode_batch(E, dtype):
    """Episode e's block is the single-episode draw with e's seed, the DIAGONAL of e's factor and particle_offset 0.  Two
    episodes given the SAME seed get the same normals (documented behaviour: the seed is the only thing that tells episodes
    apart), so their blocks differ only by their factors."""
    import torch
    L, lib = _lib()
    P, H, A, offset, s = 37, 6, 7, 2 ** 32 - 2, 5
    assert (P * A * ((H + 3) // 4)) % 256 != 0
    rs = np.random.RandomState(E)
    chols = np.stack([diag_factor(A, rs, zero_at=e % A if e % 5 == 4 else None) for e in range(E)])
    seeds = [int(rs.randint(0, 2 ** 62)) * 4 + e for e in range(E)]            # 64-bit, all different
    seeds[0] = 2 ** 64 - 1
    if E > 2:
        seeds[2] = seeds[1]                                  # the same seed twice
        chols[2] = chols[1]
    seeds_d = torch.from_numpy(np.array(seeds, np.uint64).view(np.int64)).cuda()
    buf = Guarded(E * P * H * A, dtype)
    step_d = torch.tensor([s], dtype=torch.int64, device="cuda")
    L.check(lib.mjmpc_sample_noise_batch(L.F32 if dtype == "f32" else L.F64, E, _vp(buf.view), P, H, A, _vp(_dev(chols)),
                                         _vp(seeds_d), offset, _vp(step_d), _stream()))
    got = buf.read((E, P, H, A))
    ref, scale = pr.sample_batch_ref(E, P, H, A, chols, seeds, offset + s, with_scale=True)
    compare(got.reshape(E * P, H, A), ref.reshape(E * P, H, A), scale.reshape(E * P, H, A), None, "noise_batch_kernel E=%d" % E)
    if E > 2:
        np.testing.assert_array_equal(got[2], got[1])
    # an episode's block is what the single-episode entry point draws for that seed, bit for bit
    e = E - 1
    np.testing.assert_array_equal(got[e], draw(P, H, A, chols[e], seeds[e], offset + s, 0, True, None, dtype))


# ---------------------------------------------------------------------------------------------------------------------------
# filter_kernel
COEFFS = [(0.25, 0.8, 0.0), (0.5, 0.3, 0.2), (1.0, 0.0, 0.0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [1, 2, 3, 12])
@pytest.mark.parametrize("coeffs", COEFFS)
def test_filter(coeffs, H, dtype):
    """The recursive three-tap filter behind the draw (``mjmpc_sample_noise`` with coefficients) and on an uploaded array
    (``mjmpc_filter_noise``).  The second is pure float64 arithmetic on given numbers: against the reference's filter it may
    differ by the contraction of the three-term sum into fused multiply-adds only, 3 x 2^-53 of the terms' magnitudes per step
    carried along the horizon (bounded here by 2^-49 of the largest entry over 12 steps), and for a float32 buffer by one
    float32 ulp where the two sums straddle a rounding boundary."""
    import torch
    L, lib = _lib()
    P, A = 70, 7
    chol = lower_factor(A, np.random.RandomState(H))
    raw = draw(P, H, A, chol, 17, 4, 0, False, None, dtype)
    got = check_draw(P, H, A, chol, 17, 4, 0, False, coeffs, dtype, what="draw + filter %s" % (coeffs,))
    if coeffs == (1.0, 0.0, 0.0) or H < 3:
        np.testing.assert_array_equal(got, raw)                 # the identity triple returns early; t < 2 is never touched
    # an uploaded array through mjmpc_filter_noise
    rs = np.random.RandomState(H + 50)
    x = rs.standard_normal((P, H, A)).astype(np.float32 if dtype == "f32" else np.float64)
    buf = Guarded(x.size, dtype)
    buf.view.copy_(torch.from_numpy(x.reshape(-1)).cuda())
    L.check(lib.mjmpc_filter_noise(L.F32 if dtype == "f32" else L.F64, _vp(buf.view), P, H, A, _vp(_dev(coeffs)), _stream()))
    out = buf.read((P, H, A))
    want = pr.filter_ref(x.copy(), coeffs)
    atol = 2.0 ** -49 * np.abs(want).max()
    if dtype == "f32":
        atol = atol + np.spacing(np.abs(want)).astype(np.float64)
    dev = np.abs(out.astype(np.float64) - want.astype(np.float64))
    print("mjmpc_filter_noise %s H=%d [%s]: worst deviation %.3e" % (coeffs, H, dtype, dev.max()))
    assert (dev <= atol).all()
    np.testing.assert_array_equal(out[:, :2], x[:, :2])
    # the draw's filter is the same kernel: the filtered draw is the reference's filter of the GPU's own raw draw
    want = pr.filter_ref(raw.copy(), coeffs)
    atol = 2.0 ** -49 * np.abs(want).max() + (np.spacing(np.abs(want)).astype(np.float64) if dtype == "f32" else 0.0)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= atol).all()


def test_f32_buffer_is_the_rounded_f64_draw():
    """The float32 instantiations round the same float64 sum: bit for bit the float64 draw cast to float32."""
    for P, H, A, diag_only in [(65, 5, 7, True), (65, 8, 7, False), (65, 7, 7, False), (37, 5, 24, False)]:
        L = lower_factor(A, np.random.RandomState(A))
        a = draw(P, H, A, L, 2 ** 40 + 3, 2 ** 32 + 1, 6, diag_only, None, "f64")
        b = draw(P, H, A, L, 2 ** 40 + 3, 2 ** 32 + 1, 6, diag_only, None, "f32")
        np.testing.assert_array_equal(a.astype(np.float32), b)


# ---------------------------------------------------------------------------------------------------------------------------
# the draw-ahead workgroups of the update launches (csrc/update.hip)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H", [(300, 6), (1000, 8), (5000, 5)])
def test_mppi_update_draws_the_next_steps_samples(P, H, dtype):
    """``mjmpc_mppi_fused_update_draw_next``: the extra workgroups of the update's second launch leave the raw samples of the
    NEXT control step, host offset + the step counter's value before this update advances it, diagonal factor."""
    import torch
    from mjmpc_amd.control._device import DeviceUpdater
    A, seed, s, po = 7, 2 ** 32 + 19, 2 ** 32 - 2, 4096
    rs = np.random.RandomState(P)
    dev = DeviceUpdater(H, A, 0.98 ** np.arange(H))
    cov = np.diag(rs.uniform(0.2, 1.5, A))
    dev.sample_noise(P, cov, [0.25, 0.8, 0.0], seed, 0, dtype=dtype, filtered=False)        # (buffer, factor, coefficients)
    assert dev._rec["chol_diag"] == 1
    buf = Guarded(P * H * A, dtype)
    dev._rec[("noise", dtype)] = buf.view.view(P, H, A)
    actions = torch.from_numpy(rs.standard_normal((P, H, A))).to(buf.view.dtype).cuda()
    q0 = torch.from_numpy(rs.uniform(0.0, 3.0, P)).cuda()
    step = torch.tensor([s], dtype=torch.int64, device="cuda")
    act = torch.zeros(A, dtype=torch.float64, device="cuda")
    dev.mppi_fused_update(q0, actions, 0.5, 0.9, 0, act, None, step,
                          draw_next=dict(seed=seed, offset=1, particle_offset=po, d_step=step))
    got = buf.read((P, H, A))
    assert int(step.item()) == s + 1
    chol = dev._rec["chol"].cpu().numpy().reshape(A, A)
    np.testing.assert_allclose(np.diag(chol) ** 2, np.diag(cov), rtol=1e-14)
    ref, scale = pr.sample_ref(P, H, A, chol, seed, 1 + s, po, True, None, with_scale=True)
    compare(got, ref, scale, None, "draw-ahead of the MPPI update P=%d H=%d" % (P, H))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,H,A", [(3000, 6, 5), (1000, 8, 7), (65, 8, 8)])
def test_cem_finish_draws_the_next_steps_samples(P, H, A, dtype):
    """``mjmpc_cem_finish``: the samples it leaves for the next step are the reference's at offset = step + 1, coloured by
    the whole lower triangle of the factor the same launch computed (read back from the device).  Set-up of
    tests/test_cem_fused_gpu.py::test_fused_step_degenerate_populations."""
    import torch
    from mjmpc_amd.control._device import DeviceUpdater
    k, seed, s, po = max(12, P // 80), 2 ** 63 + 3, 4, 2 ** 32
    rs = np.random.RandomState(P + H)
    dev = DeviceUpdater(H, A, np.ones(H))
    assert dev.cem_fused_supported(P, k)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    actions = torch.from_numpy(rs.standard_normal((P, H, A))).to(tdt).cuda()
    dev.set_mean(0.1 * rs.standard_normal((H, A)))
    dev.set_cov(np.diag(rs.uniform(0.5, 1.0, A)))
    ws = dev.workspace(P)
    dev._q0_view(ws, P).copy_(torch.from_numpy(rs.uniform(0.0, 5.0, P)).cuda())
    step = torch.full((1,), s, dtype=torch.int64, device="cuda")
    act = torch.zeros(A, dtype=torch.float64, device="cuda")
    pin = torch.full((A + 1,), -1.0, dtype=torch.float64).pin_memory()
    buf = Guarded(P * H * A, dtype)
    dev.cem_fused_step(actions, k, 0.7, True, 1, act, pin, step, (None, 0.25), buf.view, seed, po)
    got = buf.read((P, H, A))
    assert int(step.item()) == s + 1
    chol = dev._rec["chol"].cpu().numpy().reshape(A, A)
    np.testing.assert_allclose(np.tril(chol) @ np.tril(chol).T, dev.get_cov(), rtol=1e-10, atol=1e-13)
    assert np.count_nonzero(np.tril(chol, -1)) > 0                     # a full factor
    ref, scale = pr.sample_ref(P, H, A, chol, seed, s + 1, po, False, None, with_scale=True)
    compare(got, ref, scale, None, "draw-ahead of the CEM finish P=%d H=%d A=%d" % (P, H, A))


# ---------------------------------------------------------------------------------------------------------------------------
# the in-kernel draw of the arm rollout (csrc/arm_rollout_body.inc)
def _arm(dtype):
    from mjmpc_amd.envs.arm_engine import ArmRolloutEngine
    from mjmpc_amd.models.reacher7dof import reacher7dof_raw
    eng = ArmRolloutEngine(reacher7dof_raw(), dtype=dtype)
    eng.set_env_state(dict(qp=np.array([0.1, 0.3, -0.2, -0.5, 0.2, -0.3, 0.1]), qv=np.zeros(7),
                           target_pos=np.array([0.1, 0.1, 0.1])))
    return eng


def _mean_rounding(mean, ref, f32):
    """u = (T)mean + eps in the engine's type T, and the test subtracts the mean again in float64: half an ulp of the sum
    (and, float32, of the rounded mean), and half a float64 ulp for the subtraction."""
    u = np.abs(mean[None] + ref)
    if f32:
        return 0.5 * (np.spacing(u.astype(np.float32)).astype(np.float64) + np.spacing(np.abs(mean).astype(np.float32))[None]
                      + np.spacing(u))
    return np.spacing(u)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [96, 4096])
def test_arm_mppi_step_draws_the_reference_samples(P, dtype):
    """``mjmpc_arm_mppi_step``: the actions the launch records minus the mean are the FILTERED reference samples (diagonal
    factor; set-up of tests/test_mono_step_gpu.py::test_one_launch_iteration_against_the_oracle).  The kernel filters on the
    fly with the stand-alone filter's recurrence, on normals from the same hardware units: the transcendental tolerance
    applies (not bit equality), plus the rounding of mean + eps."""
    import torch
    eng = _arm(dtype)
    H, A, seed, o, s, po = 16, 7, 2 ** 32 + 11, 2 ** 32 - 3, 5, 8192
    rs = np.random.RandomState(4)
    mean0 = 0.1 * rs.standard_normal((H, A))
    co = [0.25, 0.8, 0.1]
    chol = np.diag(rs.uniform(0.4, 1.1, A))
    mean_d, mean_out = _dev(mean0).view(H, A), torch.zeros(H, A, dtype=torch.float64, device="cuda")
    gseq = _dev(0.98 ** np.arange(H))
    step_dev = torch.tensor([s], dtype=torch.int64, device="cuda")
    costs, acts, q0 = eng.mppi_step(P, H, mean_d, mean_out, gseq, _dev(co), _dev(chol), seed, o, po, step_dev, 1.0, 0.9, 0,
                                    want_trajectories=True)
    torch.cuda.synchronize()
    got = acts.cpu().numpy()
    assert got.dtype == (np.float32 if dtype == "f32" else np.float64)
    ref, scale = pr.sample_ref(P, H, A, chol, seed, o + s, po, True, co, with_scale=True)
    eps = got.astype(np.float64) - mean0[None]
    compare(eps, ref, scale, co, "mjmpc_arm_mppi_step P=%d" % P, extra=_mean_rounding(mean0, ref, dtype == "f32"),
            f32=dtype == "f32")
    assert eng.solver_failures() == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,coeffs", [(96, (0.5, 0.3, 0.2)), (1000, None), (4096, (0.25, 0.8, 0.0))])
def test_arm_rollout_sampled_full_factor(P, coeffs, dtype):
    """``mjmpc_arm_rollout_sampled`` with the whole lower triangle of the factor: the DPP-broadcast colouring inside a
    particle's 8 lanes sums in ``noise_full_kernel``'s order.  Tolerance as for the fused MPPI step."""
    import torch
    eng = _arm(dtype)
    H, A, seed, o, s, po = 12, 7, 2 ** 64 - 1, 3, 2 ** 32, 2 ** 32 // 7 - 3
    rs = np.random.RandomState(P)
    mean0 = 0.1 * rs.standard_normal((H, A))
    chol = lower_factor(A, rs) * 0.5          # (junk above the diagonal: nothing may read it)
    step_dev = torch.tensor([s], dtype=torch.int64, device="cuda")
    costs, acts, q0 = eng.rollout_sampled(P, H, _dev(mean0).view(H, A), _dev(0.98 ** np.arange(H)),
                                          None if coeffs is None else _dev(coeffs), _dev(chol), True, seed, o, po, step_dev)
    torch.cuda.synchronize()
    got = acts.cpu().numpy()
    ref, scale = pr.sample_ref(P, H, A, chol, seed, o + s, po, False, coeffs, with_scale=True)
    eps = got.astype(np.float64) - mean0[None]
    compare(eps, ref, scale, coeffs, "mjmpc_arm_rollout_sampled P=%d" % P, extra=_mean_rounding(mean0, ref, dtype == "f32"),
            f32=dtype == "f32")
    assert int(step_dev.item()) == s
