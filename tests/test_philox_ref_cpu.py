"""CPU: the numpy restatement of the device Philox sampler (tests/philox_ref.py) held to something outside this repository.

 (a) Philox4x32-10's published known-answer vectors (Random123 ``kat_vectors``), exactly: with them the published statistical
     record of that generator applies to the reference, and through tests/test_philox_gpu.py to the kernels;
 (b) the quality of the normals the reference forms from those words the way ``normal_quad`` forms them, once, on fixed seeds:
     Kolmogorov-Smirnov against the normal CDF (1 % critical value 1.63), and correlations - all (t, channel) column pairs,
     neighbouring particles, step ``offset`` against ``offset + 1``, seed ``s`` against ``s + 1``, two ``particle_offset``
     shards - against the Gaussian bound for a maximum over m correlations of n samples, ``sqrt(2 ln(2 m / 0.01) / n)``.
     These are conditions on the REFERENCE (the design), not on the kernel;
 (c) the edge words through the float32 front end, and the float32-evaluation figure the GPU tolerance is built on."""
import numpy as np

import philox_ref as pr

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
SEED, OFFSET, A, H = 123, 5, 7, 32
P_CORR = 5000


def corr_bound(m, n):
    return np.sqrt(2.0 * np.log(2.0 * m / 0.01) / n)


def columns(seed=SEED, offset=OFFSET, particle_offset=0, P=P_CORR):
    """[P][H * A] raw standard normals, one column per (t, channel)."""
    return pr.sample_ref(P, H, A, np.eye(A), seed, offset, particle_offset).reshape(P, H * A)


def column_corr(x, y):
    """correlation of every column of x with the same column of y"""
    xc, yc = x - x.mean(0), y - y.mean(0)
    return (xc * yc).sum(0) / np.sqrt((xc * xc).sum(0) * (yc * yc).sum(0))


def test_known_answer_vectors():
    for ctr, key, want in KAT:
        got = pr.philox4x32_10(ctr, key)
        assert got.dtype == np.uint32 and tuple(int(w) for w in got) == want
    # vectorised over arrays: the three at once
    ctr = [np.array([k[0][i] for k in KAT], np.uint64) for i in range(4)]
    key = [np.array([k[1][i] for k in KAT], np.uint64) for i in range(2)]
    np.testing.assert_array_equal(pr.philox4x32_10(ctr, key), np.array([k[2] for k in KAT], np.uint32))


def test_counter_and_key_layout():
    """``normal_words`` is Philox of (chan lo, chan hi, quad, offset lo) under (seed lo, seed hi ^ offset hi)."""
    seed, offset, chan, quad = 0xA409382212345678, 0x0000000713198A2E, 0x85A308D3243F6A88, 9
    want = pr.philox4x32_10((0x243F6A88, 0x85A308D3, 9, 0x13198A2E), (0x12345678, 0xA4093822 ^ 7))
    np.testing.assert_array_equal(pr.normal_words(seed, offset, chan, quad), want)
    # every field reaches the block: changing any one of them changes all four words
    base = pr.normal_words(seed, offset, chan, quad)
    for other in (pr.normal_words(seed + 1, offset, chan, quad), pr.normal_words(seed + 2 ** 32, offset, chan, quad),
                  pr.normal_words(seed, offset + 1, chan, quad), pr.normal_words(seed, offset + 2 ** 32, chan, quad),
                  pr.normal_words(seed, offset, chan + 1, quad), pr.normal_words(seed, offset, chan + 2 ** 32, quad),
                  pr.normal_words(seed, offset, chan, quad + 1)):
        assert (other != base).all()


def test_edge_words_through_the_float32_front_end():
    words = np.array([[0, 0, 0, 0], [2 ** 32 - 1] * 4, [1, 2 ** 31, 2 ** 32 - 129, 2 ** 30]], np.uint32)
    u0, a0, u1, a1 = pr.uniforms_and_angles(words)
    assert u0.dtype == np.float32 and a0.dtype == np.float32
    assert u0[0] == 2.0 ** -33 and a0[0] == 0.0              # word 0: the smallest uniform, (0 + 0.5) 2^-32
    assert u0[1] == 1.0 and a0[1] == 1.0 and u1[1] == 1.0   # word 2^32 - 1 rounds to 2^32 in float32: u = 1, angle = 1
    assert u0[2] == 1.5 * 2.0 ** -32 and a0[2] == 0.5 and a1[2] == 0.25
    z, r = pr.normals_from_words(words, with_radius=True)
    assert np.isfinite(z).all() and np.isfinite(r).all()
    np.testing.assert_allclose(r[0], np.sqrt(66.0 * np.log(2.0)), rtol=1e-15)      # 6.7638: the header's "|z| <= 6.8"
    assert 6.76 < r[0, 0] < 6.8 and (np.abs(z) <= 6.8).all()
    np.testing.assert_allclose(z[0], [r[0, 0], 0.0, r[0, 2], 0.0], atol=1e-15)      # angle 0: (cos, sin) = (1, 0)
    assert (r[1] == 0.0).all() and (z[1] == 0.0).all()                              # u = 1: radius 0
    np.testing.assert_allclose(z[2, :2], [-r[2, 0], 0.0], atol=1e-14)               # half a revolution
    np.testing.assert_allclose(z[2, 2:], [0.0, r[2, 2]], atol=1e-14)                # a quarter: words (c2, c3) -> (z2, z3)
    zf = pr.normals_from_words_f32(words)
    assert np.isfinite(zf).all()


def test_float32_evaluation_figure():
    """What a correctly rounded float32 evaluation of the transform costs against float64, scaled by max(1, radius): the
    figure the GPU tolerance is a multiple of.  ``F32_EVAL_ERROR`` must describe it (measured 4.30e-7 on the full draw;
    a quarter of it is drawn here)."""
    chan = np.arange(P_CORR * A, dtype=np.uint64)[:, None]
    w = pr.normal_words(SEED, OFFSET, chan, np.arange(8, dtype=np.uint64)[None, :])
    z64, r = pr.normals_from_words(w, with_radius=True)
    z32 = pr.normals_from_words_f32(w).astype(np.float64)
    worst = (np.abs(z32 - z64) / np.maximum(1.0, r)).max()
    print("float32 against float64 evaluation, worst |dz| / max(1, r): %.3e (F32_EVAL_ERROR %.2e, GPU tolerance %.2e)"
          % (worst, pr.F32_EVAL_ERROR, pr.TOL))
    assert 0.6 * pr.F32_EVAL_ERROR <= worst <= 1.25 * pr.F32_EVAL_ERROR
    assert pr.TOL == 8.0 * pr.F32_EVAL_ERROR


def test_normals_pass_kolmogorov_smirnov():
    from scipy.special import ndtr
    chan = np.arange(20000 * A, dtype=np.uint64)[:, None]
    z = np.sort(pr.normal_quad_ref(SEED, OFFSET, chan, np.arange(8, dtype=np.uint64)[None, :]).reshape(-1))
    n = z.size
    assert n == 4480000
    cdf = ndtr(z)
    d = max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(n) / n).max())
    print("KS: D sqrt(n) = %.3f, mean %.2e, std %.6f" % (d * np.sqrt(n), z.mean(), z.std()))
    assert d * np.sqrt(n) < 1.63
    assert abs(z.mean()) < 5.0 / np.sqrt(n) and abs(z.std() - 1.0) < 5.0 / np.sqrt(2.0 * n)


def test_columns_are_uncorrelated():
    x = columns()
    c = np.corrcoef(x, rowvar=False)
    m = H * A * (H * A - 1) // 2
    worst = np.abs(c - np.eye(H * A)).max()
    print("all-pairs |corr| max %.4f (bound %.4f, %d pairs, n = %d)" % (worst, corr_bound(m, P_CORR), m, P_CORR))
    assert worst < corr_bound(m, P_CORR)


def _independent(x, y, what):
    per_col = np.abs(column_corr(x, y)).max()
    pooled = abs(np.corrcoef(x.reshape(-1), y.reshape(-1))[0, 1])
    print("%s: per-column |corr| max %.4f (bound %.4f), pooled %.5f (bound %.5f)"
          % (what, per_col, corr_bound(x.shape[1], x.shape[0]), pooled, corr_bound(1, x.size)))
    assert per_col < corr_bound(x.shape[1], x.shape[0])
    assert pooled < corr_bound(1, x.size)
    assert np.abs(x - y).max() > 1.0


def test_neighbouring_particles_are_uncorrelated():
    x = columns()
    _independent(x[:-1], x[1:], "particle p against p + 1")


def test_consecutive_steps_are_uncorrelated():
    _independent(columns(), columns(offset=OFFSET + 1), "offset against offset + 1")
    _independent(columns(offset=2 ** 32 - 1), columns(offset=2 ** 32), "offset 2^32 - 1 against 2^32")


def test_consecutive_seeds_are_uncorrelated():
    """The episode batches key their episodes by the seed alone."""
    _independent(columns(), columns(seed=SEED + 1), "seed against seed + 1")
    _independent(columns(seed=2 ** 32 - 1), columns(seed=2 ** 32), "seed 2^32 - 1 against 2^32")


def test_particle_offset_shards():
    whole = columns(P=2 * P_CORR)
    shard = columns(particle_offset=P_CORR)
    np.testing.assert_array_equal(shard, whole[P_CORR:])        # a shard is its rows of the one stream
    _independent(whole[:P_CORR], shard, "shard 0 against shard 1")


def test_colouring_time_mapping_and_filter():
    """``sample_ref`` against a scalar loop written from ``noise_element`` and ``filter_kernel``."""
    P, Hs, As, seed, offset, po = 3, 7, 3, 2 ** 63 + 12345, 2 ** 32 + 7, 11
    L = np.array([[0.5, 0.0, 0.0], [0.0, 1.5, 0.0], [-0.3, 0.7, 0.9]])
    co = [0.5, 0.3, 0.2]
    for diag_only in (False, True):
        for dt in (np.float64, np.float32):
            got = pr.sample_ref(P, Hs, As, L, seed, offset, po, diag_only, co, dt)
            assert got.dtype == dt and got.shape == (P, Hs, As)
            want = np.zeros((P, Hs, As), dt)
            for p in range(P):
                for a in range(As):
                    for t in range(Hs):
                        x = 0.0
                        for b in ([a] if diag_only else range(a + 1)):
                            if L[a, b] != 0.0:
                                x += L[a, b] * pr.normal_quad_ref(seed, offset, (p + po) * As + b, t // 4)[t % 4]
                        want[p, t, a] = x
                    e2, e1 = float(want[p, 0, a]), float(want[p, 1, a])
                    for t in range(2, Hs):
                        v = co[0] * float(want[p, t, a]) + co[1] * e1 + co[2] * e2
                        want[p, t, a] = v
                        e2, e1 = e1, v
            np.testing.assert_array_equal(got, want)
    # the identity triple leaves the samples alone; a batch is its episodes' draws with the diagonal of each factor
    np.testing.assert_array_equal(pr.sample_ref(P, Hs, As, L, 1, 2, coeffs=[1.0, 0.0, 0.0]), pr.sample_ref(P, Hs, As, L, 1, 2))
    batch = pr.sample_batch_ref(2, P, Hs, As, np.stack([L, 2.0 * L]), [5, 2 ** 64 - 1], 3)
    np.testing.assert_array_equal(batch[1], pr.sample_ref(P, Hs, As, 2.0 * L, 2 ** 64 - 1, 3, diag_only=True))
    _, s = pr.sample_ref(P, Hs, As, L, 1, 2, with_scale=True)
    assert (s[:, :, 2] >= 0.3 + 0.7 + 0.9 - 1e-15).all() and (s[:, :, 0] >= 0.5).all()
