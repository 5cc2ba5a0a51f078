// Device side of the particle-filter controller's update (reference mjmpc/control/particle_filter_controller.py:92-174):
// softmax weights of the rollouts' cost-to-go, the first pointer of the systematic resampling, the resampling itself, the
// gather of the survivors fused with the noisy time shift, the mean of the survivors, and the deviations the next rollout
// takes.  The particle set, its mean and the weights are float64 whatever the engine's storage type.
//
// What is pinned here (the tests restate it in numpy):
//   weights   w[p] = exp(x[p] - max x) / sum_p exp(x[p] - max x),  x[p] = (-1 / lam) q0[p]       (:104-113)
//   pointer   u = (float(c0) + 0.5f) 2^-32 with c0 the first word of the Philox block keyed (seed, offset + *d_step,
//             chan = 2^64 - 1, quad 0) - no particle's channel index reaches that chan -; first = (1.0 / M) * double(u),
//             random.uniform(0, 1 / M)'s formula                                                  (:160)
//   indices   running sum of w strictly left to right (np.cumsum's bits: ONE lane adds, the others stage), pointers
//             first + m / M, idx[m] = first i with running[i] >= pointer, capped at M - 1; a pointer <= 0 gives -1, which
//             names the last particle as numpy's index -1 does                                    (:159-171)
//   gather    out[m] = set[idx[m]], mean = sum_m out[m] / M: per-workgroup partial sums over PF_CHUNK consecutive particles
//             in particle order, then lane l of a wavefront adds partials l, l + 64, ... and a fixed butterfly joins the
//             lanes - no atomics, the same tree at every launch shape                              (:96-97)
//   shift     rows move up by one (the last row stays), every row gets + jitter - Philox N(0, cov_shift) keyed by the
//             global particle index, through the recursive three-tap filter with its float64 carry -, then the last row
//             becomes 0 ('null') or the jittered row H - 2 ('repeat')                             (:127-150)
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mjmpc_amd.h"
#include "noise_device.h"

namespace mjmpc {
int set_error(int code, const char* what, const char* detail);      // capi.hip: the message mjmpc_last_error() returns

namespace {

constexpr int PF_WG = 1024;         // the one workgroup of the weights and the resampling launches
constexpr int PF_TILE = 4096;       // weights staged per pass of the running sum (32 KiB of LDS)
constexpr int PF_COARSE = 4096;     // entries of the search's coarse table (32 KiB of LDS)
constexpr int PF_CHUNK = 32;        // particles per workgroup of the gather: the unit of the mean's partial sums
constexpr int PF_BLK = 256;

// max / sum over the workgroup in a fixed tree: butterfly inside the wavefront, then the wavefronts in order
__device__ __forceinline__ double block_reduce(double v, double* sm, bool is_max) {
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(v, o);
        v = is_max ? fmax(v, other) : v + other;
    }
    __syncthreads();                // (sm may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = sm[0];
    for (int w = 1; w < PF_WG / 64; ++w) r = is_max ? fmax(r, sm[w]) : r + sm[w];
    return r;
}

// The bodies below are what a launch does for ONE particle set: the single kernels run them on their arguments, the
// episode batches' twins (pf_*_batch_kernel) on row e's slices - the same instructions, nothing is exchanged
// between rows, no workgroup straddles two rows.
__device__ __forceinline__ void pf_weights_body(const double* __restrict__ q0, long M, double lam, unsigned long long seed,
                                                unsigned long long offset, const long long* __restrict__ d_step,
                                                double* __restrict__ w, double* __restrict__ first) {
    __shared__ double sm[PF_WG / 64];
    const double neg_inv_lam = -1.0 / lam;
    // (a rollout that diverged carries a non-finite return: zero weight, as traj_cost_kernel has it)
    auto x_of = [&](long p) {
        const double q = q0[p];
        return fabs(q) < INFINITY ? neg_inv_lam * q : -INFINITY;
    };
    double m = -INFINITY;
    for (long p = threadIdx.x; p < M; p += PF_WG) m = fmax(m, x_of(p));
    m = block_reduce(m, sm, true);
    double s = 0.0;
    for (long p = threadIdx.x; p < M; p += PF_WG) s += exp(x_of(p) - m);
    s = block_reduce(s, sm, false);
    for (long p = threadIdx.x; p < M; p += PF_WG) w[p] = exp(x_of(p) - m) / s;
    if (first && threadIdx.x == 0) {
        if (d_step) offset += (unsigned long long)*d_step;
        unsigned c0 = 0xFFFFFFFFu, c1 = 0xFFFFFFFFu, c2 = 0u, c3 = (unsigned)offset;
        unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ (unsigned)(offset >> 32);
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            philox_round(c0, c1, c2, c3, k0, k1);
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const float u = ((float)c0 + 0.5f) * 2.3283064365386963e-10f;       // as normal_quad forms its uniforms
        *first = (1.0 / (double)M) * (double)u;
    }
}

__global__ __launch_bounds__(PF_WG) void pf_weights_kernel(const double* __restrict__ q0, long M, double lam,
                                                           unsigned long long seed, unsigned long long offset,
                                                           const long long* __restrict__ d_step, double* __restrict__ w,
                                                           double* __restrict__ first) {
    pf_weights_body(q0, M, lam, seed, offset, d_step, w, first);
}

// workgroup e = episode e: q0, w [E][M]; lams, seeds, first [E]
__global__ __launch_bounds__(PF_WG) void pf_weights_batch_kernel(const double* __restrict__ q0, long M,
                                                                 const double* __restrict__ lams,
                                                                 const unsigned long long* __restrict__ seeds,
                                                                 unsigned long long offset,
                                                                 const long long* __restrict__ d_step,
                                                                 double* __restrict__ w, double* __restrict__ first) {
    const long e = blockIdx.x;
    pf_weights_body(q0 + e * M, M, lams[e], seeds[e], offset, d_step, w + e * M, first + e);
}

// idx[m] of the systematic resampling.  The running sum is ONE chain of M dependent float64 additions (about M x the
// latency of v_add_f64: linear in M, and nothing may reassociate it without changing np.cumsum's bits); per tile the
// workgroup stages PF_TILE weights into LDS, lane 0 turns them into running sums in place, eight loads ahead of the chain,
// and the workgroup copies the tile out, keeping every `stride`-th running sum (and the last) in LDS.  The search is one
// binary search per pointer: over that coarse table in LDS, then over the one block of `stride` running sums it names.
// EB (episode batches): workgroup e = episode e - w, running, idx [E][M], first [E] -, and the E serial chains
// run side by side on different CUs.  A template switch and not a __device__ body as the other launches have it: the
// body cost pf_resample_kernel two scalar registers, the switch none.
template <bool EB>
__global__ __launch_bounds__(PF_WG) void pf_resample_kernel(const double* __restrict__ w, const double* __restrict__ first,
                                                            long M, long stride, double* __restrict__ running,
                                                            int* __restrict__ idx) {
    __shared__ double tile[PF_TILE];
    __shared__ double coarse[PF_COARSE];
    if (EB) {
        const long e = blockIdx.x;
        w += e * M;
        first += e;
        running += e * M;
        idx += e * M;
    }
    double c = 0.0;                             // (lane 0's: the running sum so far)
    for (long base = 0; base < M; base += PF_TILE) {
        const int n = (int)((M - base) < PF_TILE ? (M - base) : PF_TILE);
        for (int i = threadIdx.x; i < n; i += PF_WG) tile[i] = w[base + i];
        __syncthreads();
        if (threadIdx.x == 0) {
            int i = 0;
            for (; i + 8 <= n; i += 8) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = tile[i + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    c += v[k];
                    tile[i + k] = c;
                }
            }
            for (; i < n; ++i) {
                c += tile[i];
                tile[i] = c;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += PF_WG) {
            const long g = base + i;
            running[g] = tile[i];
            if ((g + 1) % stride == 0 || g == M - 1) coarse[g / stride] = tile[i];
        }
        __syncthreads();
    }
    // (`running`: the workgroup's own stores, read back by the same workgroup behind the barrier above)
    const int nc = (int)((M + stride - 1) / stride);
    const double f = *first, dM = (double)M;
    for (long m = threadIdx.x; m < M; m += PF_WG) {
        const double ptr = f + (double)m * 1.0 / dM * 1.0;
        int jl = 0, jh = nc;                    // first block whose last running sum reaches the pointer
        while (jl < jh) {
            const int mid = (jl + jh) >> 1;
            if (coarse[mid] < ptr) jl = mid + 1;
            else jh = mid;
        }
        long lo = M - 1;                        // no running sum reaches it: the last particle
        if (jl < nc) {                          // first i with running[i] >= ptr (np.searchsorted, side 'left')
            lo = (long)jl * stride;
            long hi = lo + stride < M ? lo + stride : M;
            hi -= 1;                            // (running[hi] >= ptr is known)
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if (running[mid] < ptr) lo = mid + 1;
                else hi = mid;
            }
        }
        idx[m] = ptr <= 0.0 ? -1 : (int)lo;
    }
}

// Workgroup b takes particles [b PF_CHUNK, (b + 1) PF_CHUNK): one thread per (particle, channel) walks the horizon - the
// filter's carry runs along it - and writes the shifted survivor into `dst` (shift_mode < 0: the survivor as it is); then
// lanes along the contiguous H A axis add the chunk's survivors in particle order into partial[b][H A].  `gathered` (may
// be null) receives the unshifted survivors.
__device__ __forceinline__ void pf_gather_shift_body(const double* __restrict__ src, const int* __restrict__ idx, long M,
                                                     int H, int A, int shift_mode, const double* __restrict__ chol,
                                                     const double* __restrict__ coeffs, unsigned long long seed,
                                                     unsigned long long offset, const long long* __restrict__ d_step,
                                                     double* __restrict__ dst, double* __restrict__ gathered) {
    const long p0 = (long)blockIdx.x * PF_CHUNK;
    const int n = (int)((M - p0) < PF_CHUNK ? (M - p0) : PF_CHUNK);
    const int HA = H * A;
    if (d_step) offset += (unsigned long long)*d_step;
    double b0 = 1.0, b1 = 0.0, b2 = 0.0;
    if (coeffs) { b0 = coeffs[0]; b1 = coeffs[1]; b2 = coeffs[2]; }
    const bool filtered = !(b0 == 1.0 && b1 == 0.0 && b2 == 0.0);
    const int H4 = (H + 3) / 4;
    for (int i = threadIdx.x; i < n * A; i += PF_BLK) {
        const long p = p0 + i / A;
        const int a = i % A;
        const int from = idx[p];
        const double* row = src + (from < 0 ? M + from : (long)from) * HA + a;
        double* out = dst + p * HA + a;
        if (gathered)
            for (int t = 0; t < H; ++t) gathered[p * HA + (long)t * A + a] = row[(long)t * A];
        if (shift_mode < 0) {
            for (int t = 0; t < H; ++t) out[(long)t * A] = row[(long)t * A];
            continue;
        }
        double e1 = 0.0, e2 = 0.0, before_last = 0.0;
        for (int t4 = 0; t4 < H4; ++t4) {
            double x[4];
            coloured_quad(chol, A, a, 1, seed, offset, p, t4, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = 4 * t4 + k;
                if (t >= H) break;
                double j = x[k];
                if (filtered && t >= 2) j = b0 * j + b1 * e1 + b2 * e2;
                e2 = e1;
                e1 = j;
                const double v = row[(long)(t + 1 < H ? t + 1 : t) * A] + j;
                if (t == H - 2) before_last = v;
                if (t < H - 1) out[(long)t * A] = v;
                else out[(long)t * A] = shift_mode == 1 ? before_last : 0.0;
            }
        }
    }
}

// (the second half of the launch: the chunk's survivors added in particle order)
__device__ __forceinline__ void pf_chunk_sum_body(const double* __restrict__ src, const int* __restrict__ idx, long M, int HA,
                                                  double* __restrict__ partial) {
    const long p0 = (long)blockIdx.x * PF_CHUNK;
    const int n = (int)((M - p0) < PF_CHUNK ? (M - p0) : PF_CHUNK);
    for (int j = threadIdx.x; j < HA; j += PF_BLK) {
        double s = 0.0;
        for (int q = 0; q < n; ++q) {
            const int from = idx[p0 + q];
            s += src[(from < 0 ? M + from : (long)from) * HA + j];
        }
        partial[(long)blockIdx.x * HA + j] = s;
    }
}

__global__ __launch_bounds__(PF_BLK) void pf_gather_shift_kernel(const double* __restrict__ src, const int* __restrict__ idx,
                                                                 long M, int H, int A, int shift_mode,
                                                                 const double* __restrict__ chol,
                                                                 const double* __restrict__ coeffs, unsigned long long seed,
                                                                 unsigned long long offset,
                                                                 const long long* __restrict__ d_step,
                                                                 double* __restrict__ dst, double* __restrict__ gathered,
                                                                 double* __restrict__ partial) {
    pf_gather_shift_body(src, idx, M, H, A, shift_mode, chol, coeffs, seed, offset, d_step, dst, gathered);
    pf_chunk_sum_body(src, idx, M, H * A, partial);
}

// grid (chunks of PF_CHUNK particles, E): src, dst, gathered [E][M][H A]; idx [E][M]; chols [E][A A]; seeds [E]; partial
// [E][nb][H A].  p of the body - the Philox key's particle index - is the index inside the episode.  `set_n` = M H A and
// `part_n` = nb H A come from the host (formed here they cost 2 SGPRs and 8 VGPRs).
__global__ __launch_bounds__(PF_BLK) void pf_gather_shift_batch_kernel(const double* __restrict__ src,
                                                                       const int* __restrict__ idx, long M, int H, int A,
                                                                       int shift_mode, const double* __restrict__ chols,
                                                                       const double* __restrict__ coeffs,
                                                                       const unsigned long long* __restrict__ seeds,
                                                                       unsigned long long offset,
                                                                       const long long* __restrict__ d_step,
                                                                       double* __restrict__ dst, double* __restrict__ gathered,
                                                                       double* __restrict__ partial, long set_n, long part_n) {
    const long e = blockIdx.y, set = e * set_n;
    // (the two halves are independent - the sums read src and idx only -: the cheap one first, so that its operands are
    // dead where the shift needs the scalar registers; in the single kernel's order this twin spills 4 to 6 SGPRs)
    pf_chunk_sum_body(src + set, idx + e * M, M, H * A, partial + e * part_n);
    pf_gather_shift_body(src + set, idx + e * M, M, H, A, shift_mode, chols ? chols + e * (A * A) : nullptr, coeffs, seeds[e],
                         offset, d_step, dst + set, gathered ? gathered + set : nullptr);
}

// mean[j] = (sum over the workgroups' partials) / M, one wavefront per entry; action = mean[0 .. A); the step counter moves
__device__ __forceinline__ void pf_finish_body(const double* __restrict__ partial, int nb, int HA, int A, long M,
                                               double* __restrict__ mean, double* __restrict__ action_out,
                                               long long* __restrict__ step_counter) {
    const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (j >= HA) return;
    const int l = threadIdx.x & 63;
    double s = 0.0;
    for (int b = l; b < nb; b += 64) s += partial[(long)b * HA + j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (l == 0) {
        const double v = s / (double)M;
        mean[j] = v;
        if (action_out && j < A) action_out[j] = v;
        if (step_counter && j == 0) *step_counter += 1;
    }
}

__global__ void pf_finish_kernel(const double* __restrict__ partial, int nb, int HA, int A, long M, double* __restrict__ mean,
                                 double* __restrict__ action_out, long long* __restrict__ step_counter) {
    pf_finish_body(partial, nb, HA, A, M, mean, action_out, step_counter);
}

// grid (entries of the mean / wavefronts per workgroup, E): partial [E][nb][H A]; mean [E][H A]; action_out [E][A].  The
// episodes advance together: row 0 alone moves the one step counter (as mjmpc_mppi_fused_update_batch has it).
__global__ void pf_finish_batch_kernel(const double* __restrict__ partial, int nb, int HA, int A, long M,
                                       double* __restrict__ mean, double* __restrict__ action_out,
                                       long long* __restrict__ step_counter) {
    const long e = blockIdx.y;
    pf_finish_body(partial + e * nb * HA, nb, HA, A, M, mean + e * HA, action_out ? action_out + e * A : nullptr,
                   e == 0 ? step_counter : nullptr);
}

template <typename T>
__device__ __forceinline__ void pf_delta_body(const double* __restrict__ set, const double* __restrict__ mean, long n, int HA,
                                              T* __restrict__ delta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) delta[i] = (T)(set[i] - mean[i % HA]);
}

template <typename T>
__global__ void pf_delta_kernel(const double* __restrict__ set, const double* __restrict__ mean, long n, int HA,
                                T* __restrict__ delta) {
    pf_delta_body(set, mean, n, HA, delta);
}

// grid (elements of one set / PF_BLK, E): sets, delta [E][n]; means [E][H A]
template <typename T>
__global__ void pf_delta_batch_kernel(const double* __restrict__ sets, const double* __restrict__ means, long n, int HA,
                                      T* __restrict__ delta) {
    const long e = blockIdx.y;
    pf_delta_body(sets + e * n, means + e * HA, n, HA, delta + e * n);
}

int bad(const char* what, const char* detail) { return set_error(MJMPC_E_BADARG, what, detail); }

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, what, hipGetErrorString(e));
}

}  // namespace
}  // namespace mjmpc

extern "C" {

int64_t mjmpc_pf_workspace_bytes(int64_t M, int H, int A) {
    if (M < 1 || H < 1 || A < 1) return 0;
    const int64_t nb = (M + mjmpc::PF_CHUNK - 1) / mjmpc::PF_CHUNK;
    return 8 * (M + nb * (int64_t)H * A);           // running sums [M] | partial sums [nb][H A]
}

int mjmpc_pf_weights(int64_t M, const double* d_q0, double lam, uint64_t seed, uint64_t offset, const int64_t* d_step,
                     double* d_weights, double* d_first, void* stream) {
    if (!d_q0 || !d_weights) return mjmpc::bad("mjmpc_pf_weights", "null argument");
    if (M < 1 || !(lam > 0.0)) return mjmpc::bad("mjmpc_pf_weights", "needs M >= 1 and lam > 0");
    hipLaunchKernelGGL(mjmpc::pf_weights_kernel, dim3(1), dim3(mjmpc::PF_WG), 0, (hipStream_t)stream, d_q0, (long)M, lam,
                       (unsigned long long)seed, (unsigned long long)offset, (const long long*)d_step, d_weights, d_first);
    return mjmpc::launched("mjmpc_pf_weights");
}

int mjmpc_pf_resample(int64_t M, const double* d_weights, const double* d_first, int32_t* d_idx, void* d_ws, void* stream) {
    if (!d_weights || !d_first || !d_idx || !d_ws) return mjmpc::bad("mjmpc_pf_resample", "null argument");
    if (M < 1 || M > INT32_MAX) return mjmpc::bad("mjmpc_pf_resample", "needs 1 <= M < 2^31");
    long stride = 16;                   // a power of two: M / stride entries fit the coarse table
    while ((M + stride - 1) / stride > mjmpc::PF_COARSE) stride *= 2;
    hipLaunchKernelGGL(mjmpc::pf_resample_kernel<false>, dim3(1), dim3(mjmpc::PF_WG), 0, (hipStream_t)stream, d_weights, d_first,
                       (long)M, stride, (double*)d_ws, (int*)d_idx);
    return mjmpc::launched("mjmpc_pf_resample");
}

int mjmpc_pf_gather_shift(int64_t M, int H, int A, const double* d_set, const int32_t* d_idx, int shift_mode,
                          const double* d_chol, const double* d_coeffs, uint64_t seed, uint64_t offset, const int64_t* d_step,
                          double* d_set_out, double* d_gathered, void* d_ws, void* stream) {
    if (!d_set || !d_idx || !d_set_out || !d_ws) return mjmpc::bad("mjmpc_pf_gather_shift", "null argument");
    if (d_set == d_set_out) return mjmpc::bad("mjmpc_pf_gather_shift", "the gather cannot be in place");
    if (M < 1 || M > INT32_MAX || H < 1 || A < 1) return mjmpc::bad("mjmpc_pf_gather_shift", "bad shape");
    if (shift_mode > 1) return mjmpc::bad("mjmpc_pf_gather_shift", "shift_mode must be 0 'null', 1 'repeat' or < 0 none");
    if (shift_mode >= 0 && !d_chol) return mjmpc::bad("mjmpc_pf_gather_shift", "the shift needs the jitter's factor");
    if (shift_mode == 1 && H < 2) return mjmpc::bad("mjmpc_pf_gather_shift", "'repeat' needs a horizon of at least 2");
    const int64_t nb = (M + mjmpc::PF_CHUNK - 1) / mjmpc::PF_CHUNK;
    hipLaunchKernelGGL(mjmpc::pf_gather_shift_kernel, dim3((unsigned)nb), dim3(mjmpc::PF_BLK), 0, (hipStream_t)stream, d_set,
                       (const int*)d_idx, (long)M, H, A, shift_mode, d_chol, d_coeffs, (unsigned long long)seed,
                       (unsigned long long)offset, (const long long*)d_step, d_set_out, d_gathered, (double*)d_ws + M);
    return mjmpc::launched("mjmpc_pf_gather_shift");
}

int mjmpc_pf_finish(int64_t M, int H, int A, const void* d_ws, double* d_mean, double* d_action_out, int64_t* d_step_counter,
                    void* stream) {
    if (!d_ws || !d_mean) return mjmpc::bad("mjmpc_pf_finish", "null argument");
    if (M < 1 || H < 1 || A < 1) return mjmpc::bad("mjmpc_pf_finish", "bad shape");
    const int64_t nb = (M + mjmpc::PF_CHUNK - 1) / mjmpc::PF_CHUNK;
    const int HA = H * A, per = mjmpc::PF_BLK / 64;
    hipLaunchKernelGGL(mjmpc::pf_finish_kernel, dim3((unsigned)((HA + per - 1) / per)), dim3(mjmpc::PF_BLK), 0,
                       (hipStream_t)stream, (const double*)d_ws + M, (int)nb, HA, A, (long)M, d_mean, d_action_out,
                       (long long*)d_step_counter);
    return mjmpc::launched("mjmpc_pf_finish");
}

int mjmpc_pf_delta(int dtype, int64_t M, int H, int A, const double* d_set, const double* d_mean, void* d_delta, void* stream) {
    if (!d_set || !d_mean || !d_delta) return mjmpc::bad("mjmpc_pf_delta", "null argument");
    if (M < 1 || H < 1 || A < 1) return mjmpc::bad("mjmpc_pf_delta", "bad shape");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return mjmpc::bad("mjmpc_pf_delta", "dtype must be MJMPC_F32 or MJMPC_F64");
    const long n = (long)M * H * A;
    const dim3 grid((unsigned)((n + mjmpc::PF_BLK - 1) / mjmpc::PF_BLK)), block(mjmpc::PF_BLK);
    if (dtype == MJMPC_F32)
        hipLaunchKernelGGL(mjmpc::pf_delta_kernel<float>, grid, block, 0, (hipStream_t)stream, d_set, d_mean, n, H * A,
                           (float*)d_delta);
    else
        hipLaunchKernelGGL(mjmpc::pf_delta_kernel<double>, grid, block, 0, (hipStream_t)stream, d_set, d_mean, n, H * A,
                           (double*)d_delta);
    return mjmpc::launched("mjmpc_pf_delta");
}

// ---- episode batches: row e of every launch is the single launch on episode e's slices.  d_ws holds the
// running sums [E][M], then the partial sums [E][nb][H A].
int64_t mjmpc_pf_batch_workspace_bytes(int E, int64_t M, int H, int A) {
    if (E < 1 || E > 65535) return 0;
    return (int64_t)E * mjmpc_pf_workspace_bytes(M, H, A);
}

int mjmpc_pf_delta_batch(int dtype, int E, int64_t M, int H, int A, const double* d_sets, const double* d_means, void* d_delta,
                         void* stream) {
    if (!d_sets || !d_means || !d_delta) return mjmpc::bad("mjmpc_pf_delta_batch", "null argument");
    if (E < 1 || E > 65535) return mjmpc::bad("mjmpc_pf_delta_batch", "needs 1 <= E <= 65535");
    if (M < 1 || M > INT32_MAX || H < 1 || A < 1) return mjmpc::bad("mjmpc_pf_delta_batch", "bad shape");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64)
        return mjmpc::bad("mjmpc_pf_delta_batch", "dtype must be MJMPC_F32 or MJMPC_F64");
    const long n = (long)M * H * A;
    const long blocks = (n + mjmpc::PF_BLK - 1) / mjmpc::PF_BLK;
    if (blocks > INT32_MAX) return mjmpc::bad("mjmpc_pf_delta_batch", "a set of more than 2^31 workgroups");
    const dim3 grid((unsigned)blocks, (unsigned)E), block(mjmpc::PF_BLK);
    if (dtype == MJMPC_F32)
        hipLaunchKernelGGL(mjmpc::pf_delta_batch_kernel<float>, grid, block, 0, (hipStream_t)stream, d_sets, d_means, n, H * A,
                           (float*)d_delta);
    else
        hipLaunchKernelGGL(mjmpc::pf_delta_batch_kernel<double>, grid, block, 0, (hipStream_t)stream, d_sets, d_means, n,
                           H * A, (double*)d_delta);
    return mjmpc::launched("mjmpc_pf_delta_batch");
}

int mjmpc_pf_weights_batch(int E, int64_t M, const double* d_q0, const double* d_lams, const uint64_t* d_seeds, uint64_t offset,
                           const int64_t* d_step, double* d_weights, double* d_first, void* stream) {
    if (!d_q0 || !d_lams || !d_seeds || !d_weights || !d_first) return mjmpc::bad("mjmpc_pf_weights_batch", "null argument");
    if (E < 1 || E > 65535) return mjmpc::bad("mjmpc_pf_weights_batch", "needs 1 <= E <= 65535");
    if (M < 1 || M > INT32_MAX) return mjmpc::bad("mjmpc_pf_weights_batch", "needs 1 <= M < 2^31");
    hipLaunchKernelGGL(mjmpc::pf_weights_batch_kernel, dim3((unsigned)E), dim3(mjmpc::PF_WG), 0, (hipStream_t)stream, d_q0,
                       (long)M, d_lams, (const unsigned long long*)d_seeds, (unsigned long long)offset,
                       (const long long*)d_step, d_weights, d_first);
    return mjmpc::launched("mjmpc_pf_weights_batch");
}

int mjmpc_pf_resample_batch(int E, int64_t M, const double* d_weights, const double* d_first, int32_t* d_idx, void* d_ws,
                            void* stream) {
    if (!d_weights || !d_first || !d_idx || !d_ws) return mjmpc::bad("mjmpc_pf_resample_batch", "null argument");
    if (E < 1 || E > 65535) return mjmpc::bad("mjmpc_pf_resample_batch", "needs 1 <= E <= 65535");
    if (M < 1 || M > INT32_MAX) return mjmpc::bad("mjmpc_pf_resample_batch", "needs 1 <= M < 2^31");
    long stride = 16;                   // (as mjmpc_pf_resample forms it: a row searches as the single launch does)
    while ((M + stride - 1) / stride > mjmpc::PF_COARSE) stride *= 2;
    hipLaunchKernelGGL(mjmpc::pf_resample_kernel<true>, dim3((unsigned)E), dim3(mjmpc::PF_WG), 0, (hipStream_t)stream,
                       d_weights, d_first, (long)M, stride, (double*)d_ws, (int*)d_idx);
    return mjmpc::launched("mjmpc_pf_resample_batch");
}

int mjmpc_pf_gather_shift_batch(int E, int64_t M, int H, int A, const double* d_sets, const int32_t* d_idx, int shift_mode,
                                const double* d_chols, const double* d_coeffs, const uint64_t* d_seeds, uint64_t offset,
                                const int64_t* d_step, double* d_sets_out, double* d_gathered, void* d_ws, void* stream) {
    const char* what = "mjmpc_pf_gather_shift_batch";
    if (!d_sets || !d_idx || !d_seeds || !d_sets_out || !d_ws) return mjmpc::bad(what, "null argument");
    if (d_sets == d_sets_out) return mjmpc::bad(what, "the gather cannot be in place");
    if (E < 1 || E > 65535) return mjmpc::bad(what, "needs 1 <= E <= 65535");
    if (M < 1 || M > INT32_MAX || H < 1 || A < 1) return mjmpc::bad(what, "bad shape");
    if (shift_mode > 1) return mjmpc::bad(what, "shift_mode must be 0 'null', 1 'repeat' or < 0 none");
    if (shift_mode >= 0 && !d_chols) return mjmpc::bad(what, "the shift needs the jitter's factors");
    if (shift_mode == 1 && H < 2) return mjmpc::bad(what, "'repeat' needs a horizon of at least 2");
    const int64_t nb = (M + mjmpc::PF_CHUNK - 1) / mjmpc::PF_CHUNK;
    hipLaunchKernelGGL(mjmpc::pf_gather_shift_batch_kernel, dim3((unsigned)nb, (unsigned)E), dim3(mjmpc::PF_BLK), 0,
                       (hipStream_t)stream, d_sets, (const int*)d_idx, (long)M, H, A, shift_mode, d_chols, d_coeffs,
                       (const unsigned long long*)d_seeds, (unsigned long long)offset, (const long long*)d_step, d_sets_out,
                       d_gathered, (double*)d_ws + (int64_t)E * M, (long)M * H * A, (long)nb * H * A);
    return mjmpc::launched(what);
}

int mjmpc_pf_finish_batch(int E, int64_t M, int H, int A, const void* d_ws, double* d_means, double* d_actions,
                          int64_t* d_step_counter, void* stream) {
    if (!d_ws || !d_means) return mjmpc::bad("mjmpc_pf_finish_batch", "null argument");
    if (E < 1 || E > 65535) return mjmpc::bad("mjmpc_pf_finish_batch", "needs 1 <= E <= 65535");
    if (M < 1 || M > INT32_MAX || H < 1 || A < 1) return mjmpc::bad("mjmpc_pf_finish_batch", "bad shape");
    const int64_t nb = (M + mjmpc::PF_CHUNK - 1) / mjmpc::PF_CHUNK;
    const int HA = H * A, per = mjmpc::PF_BLK / 64;
    hipLaunchKernelGGL(mjmpc::pf_finish_batch_kernel, dim3((unsigned)((HA + per - 1) / per), (unsigned)E),
                       dim3(mjmpc::PF_BLK), 0, (hipStream_t)stream, (const double*)d_ws + (int64_t)E * M, (int)nb, HA, A,
                       (long)M, d_means, d_actions, (long long*)d_step_counter);
    return mjmpc::launched("mjmpc_pf_finish_batch");
}

}  // extern "C"
