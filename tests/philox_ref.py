"""The device Philox sampler (``csrc/noise_device.h``, ``csrc/noise.hip``) restated in numpy from the header's comments and
the published algorithm: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11;
multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds, key bumped after each round).

Exact where the kernel is exact, float64 where the kernel approximates:

* the generator is integer arithmetic, reproduced bit for bit (``philox4x32_10``; tests/test_philox_ref_cpu.py holds it to
  Random123's published known-answer vectors);
* the counter / key layout of ``normal_quad`` (``normal_words``): counter = (chan low word, chan high word, t / 4, offset
  low word), key = (seed low word, seed high word XOR offset high word), chan = (particle + particle_offset) * A + channel;
* the uniforms ``(float(w) + 0.5f) * 2^-32`` and the angles ``float(w) * 2^-32`` are formed in float32 exactly as the header
  forms them (numpy float32 rounds the same way), then ``sqrt(-2 ln u)``, ``cos(2 pi a)``, ``sin(2 pi a)`` in float64
  (``normal_quad_ref``): words (c0, c1) give the pair (z0, z1) = r0 (cos, sin), words (c2, c3) the pair (z2, z3);
* colouring ``x[a] = sum_{b <= a} L[a][b] z[b]`` in ascending b with zero entries skipped, the quad-to-time mapping
  ``t = 4 quad + k``, the rounding to the buffer's type and the recursive three-tap filter with its float64 carry
  (``sample_ref``, ``filter_ref``).

``F32_EVAL_ERROR`` is what a correctly rounded float32 evaluation of the same transform costs (numpy float32 ``log2``,
``sqrt``, ``sin``, ``cos`` against this module's float64, worst ``|z32 - z64| / max(1, radius)``; the CPU test measures it
again and holds the constant to the measurement); the GPU tests allow the hardware units ``HW_FACTOR`` times that."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
TWO_M32 = np.float32(2.0 ** -32)

# worst |z32 - z64| / max(1, radius) of a correctly rounded float32 evaluation (numpy) over the 4.48 M variates of
# seed 123, offset 5, 20000 particles x 7 channels x 8 quads: measured 4.30e-7, unscaled 1.85e-6 at radius 5.4
# (test_philox_ref_cpu.py re-measures it on a quarter of those draws and holds the constant to what it finds)
F32_EVAL_ERROR = 4.3e-7
HW_FACTOR = 8.0          # allowance for the hardware's approximate units over a correctly rounded float32 evaluation
TOL = HW_FACTOR * F32_EVAL_ERROR


def _u64(x):
    """Python ints (up to 2^64 - 1) or integer arrays -> uint64 array, modulo 2^64."""
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & (2 ** 64 - 1), dtype=np.uint64)
    x = np.asarray(x)
    return x if x.dtype == np.uint64 else x.astype(np.uint64)


def philox4x32_10(ctr, key, rounds=10):
    """``ctr``: four, ``key``: two arrays (or ints) of 32-bit words, broadcast against each other.  Returns uint32 [..., 4]."""
    c0, c1, c2, c3 = (_u64(c) & _MASK for c in ctr)
    k0, k1 = (_u64(k) & _MASK for k in key)
    m0, m1, w0, w1 = np.uint64(M0), np.uint64(M1), np.uint64(W0), np.uint64(W1)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                           # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + w0) & _MASK, (k1 + w1) & _MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def normal_words(seed, offset, chan, quad):
    """The Philox block of (seed, step offset, global channel index, t / 4): uint32 [..., 4]."""
    seed, offset, chan, quad = _u64(seed), _u64(offset), _u64(chan), _u64(quad)
    ctr = (chan & _MASK, chan >> _S32, quad & _MASK, offset & _MASK)
    key = (seed & _MASK, (seed >> _S32) ^ (offset >> _S32))
    return philox4x32_10(ctr, key)


def uniforms_and_angles(words):
    """float32 front end of ``normal_quad``: (u0, a0, u1, a1) from the words (c0, c1, c2, c3), each float32."""
    w = np.asarray(words, np.uint32).astype(np.float32)     # (float)c: round to nearest even, as v_cvt_f32_u32
    half = np.float32(0.5)
    return (w[..., 0] + half) * TWO_M32, w[..., 1] * TWO_M32, (w[..., 2] + half) * TWO_M32, w[..., 3] * TWO_M32


def normals_from_words(words, with_radius=False):
    """Two Box-Muller pairs in float64 from float32 uniforms / angles.  float64 [..., 4] (and the radii [..., 4])."""
    u0, a0, u1, a1 = (x.astype(np.float64) for x in uniforms_and_angles(words))
    r0, r1 = np.sqrt(-2.0 * np.log(u0)) + 0.0, np.sqrt(-2.0 * np.log(u1)) + 0.0      # (+ 0.0: sqrt(-0.0) -> 0.0)
    t0, t1 = 2.0 * np.pi * a0, 2.0 * np.pi * a1
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)
    if with_radius:
        return z, np.stack([r0, r0, r1, r1], axis=-1)
    return z


def normals_from_words_f32(words):
    """The same transform evaluated in float32 by numpy (correctly rounded library functions): float32 [..., 4]."""
    u0, a0, u1, a1 = uniforms_and_angles(words)
    m2ln2, twopi = np.float32(-2.0 * np.log(2.0)), np.float32(2.0 * np.pi)
    r0, r1 = np.sqrt(m2ln2 * np.log2(u0)), np.sqrt(m2ln2 * np.log2(u1))
    t0, t1 = twopi * a0, twopi * a1
    z = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=-1)
    assert z.dtype == np.float32
    return z


def normal_quad_ref(seed, offset, chan, quad, with_radius=False):
    """``normal_quad``: four standard normals, float64 [..., 4]."""
    return normals_from_words(normal_words(seed, offset, chan, quad), with_radius)


def filter_ref(x, coeffs):
    """``filter_kernel`` on a [P][H][A] buffer of x's type, in place: eps[t] = b0 eps[t] + b1 eps[t-1] + b2 eps[t-2], t >= 2,
    t - 1 and t - 2 already filtered; the sum and its carry in float64, the stored value rounded to the buffer's type."""
    b0, b1, b2 = (float(c) for c in coeffs)
    if b0 == 1.0 and b1 == 0.0 and b2 == 0.0:
        return x
    H = x.shape[1]
    e2 = x[:, 0].astype(np.float64) if H > 0 else None
    e1 = x[:, 1].astype(np.float64) if H > 1 else None
    for t in range(2, H):
        v = b0 * x[:, t].astype(np.float64) + b1 * e1 + b2 * e2
        x[:, t] = v.astype(x.dtype)
        e2, e1 = e1, v
    return x


def sample_ref(P, H, A, chol, seed, offset, particle_offset=0, diag_only=False, coeffs=None, out_dtype=np.float64,
               with_scale=False):
    """``mjmpc_sample_noise``: [P][H][A] samples of ``out_dtype``.  ``with_scale``: also, per element, the factor that turns
    the transcendental tolerance into a bound on the RAW (unfiltered) element, ``sum_b |L[a][b]| max(1, radius_b)``; see
    ``error_bound``."""
    L = np.asarray(chol, np.float64).reshape(A, A)
    H4 = (H + 3) // 4
    p = _u64(np.arange(P, dtype=np.uint64)) + _u64(particle_offset)
    chan = p[:, None] * np.uint64(A) + np.arange(A, dtype=np.uint64)[None, :]          # modulo 2^64, as the kernel's
    quad = np.arange(H4, dtype=np.uint64)
    z, r = normal_quad_ref(seed, offset, chan[:, :, None], quad[None, None, :], with_radius=True)     # [P][A][H4][4]
    z = z.reshape(P, A, 4 * H4)[:, :, :H].transpose(0, 2, 1)        # [P][H][A]: t = 4 quad + k
    r = np.maximum(1.0, r.reshape(P, A, 4 * H4)[:, :, :H].transpose(0, 2, 1))
    x, s = np.zeros((P, H, A)), np.zeros((P, H, A))
    for a in range(A):
        for b in ([a] if diag_only else range(a + 1)):
            if L[a, b] == 0.0:
                continue
            x[:, :, a] += L[a, b] * z[:, :, b]
            s[:, :, a] += abs(L[a, b]) * r[:, :, b]
    x = x.astype(out_dtype)
    if coeffs is not None:
        filter_ref(x, coeffs)
    return (x, s) if with_scale else x


def error_bound(ref, scale, coeffs=None, f32=False, tol=TOL):
    """Per-element bound on |kernel - ref| for ``ref`` = ``sample_ref(..., out_dtype=float64)`` and its raw ``scale``:
    ``tol * scale`` for the hardware's transcendental units, half a float32 ulp of every value a float32 buffer stores, and
    both carried through the recursive filter with the coefficients' magnitudes (the filter re-reads what it stored)."""
    half_ulp = (lambda v: 0.5 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)) if f32 else (lambda v: 0.0 * v)
    if coeffs is None or tuple(float(c) for c in coeffs) == (1.0, 0.0, 0.0):
        return tol * scale + half_ulp(ref)
    # ref is filtered: the raw values behind it are not needed beyond their size, |raw| <= scale (|z| <= radius)
    b0, b1, b2 = (abs(float(c)) for c in coeffs)
    e = tol * scale + half_ulp(scale)
    for t in range(2, e.shape[1]):
        e[:, t] = b0 * e[:, t] + b1 * e[:, t - 1] + b2 * e[:, t - 2] + half_ulp(ref[:, t])
    return e


def sample_batch_ref(E, P, H, A, chols, seeds, offset, out_dtype=np.float64, with_scale=False):
    """``mjmpc_sample_noise_batch``: episode e's [P][H][A] block is ``sample_ref`` with seed e, the DIAGONAL of factor e and
    particle_offset 0."""
    chols = np.asarray(chols, np.float64).reshape(E, A, A)
    out = [sample_ref(P, H, A, chols[e], int(seeds[e]), offset, 0, True, None, out_dtype, with_scale) for e in range(E)]
    if with_scale:
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return np.stack(out)
