// User-defined cost terms: a second, bandwidth-bound launch behind a rollout that turns the next observations
// and the actions of every (particle, step) into a cost from a table of terms.  The rollout kernels keep their built-in
// costs and are not touched: the terms live neither in the model block (its length is part of the ABI) nor in the rollout
// translation units (an edit there moves the register allocation of every instantiation).
//
// A table row is eight doubles - kind, source, index, weight, target, group, when, reserved (include/mjmpc_amd.h):
//   v = next_obs[p][t][index] (source 0) or actions[p][t][index] (source 1), as double;  r = v - target
//   kind 0 ABS     w |r|
//   kind 1 SQUARE  w r^2
//   kind 2 NORM    consecutive rows of one group > 0: w_first sqrt(sum r^2), once, at the group's last row
//   kind 3 COS     w (1 - cos r), formed as 2 w sin^2(r / 2): no cancellation near r = 0
//   when = 1       the row counts only at t = H - 1 and only if the launch says `terminal`
// The cost of (p, t) is the sum over the rows in row order, in double whatever the storage type, behind the incoming cost
// when keep_builtin is set; an incoming cost that is not finite leaves as +inf either way (a particle that reset
// under set_reset_returns("inf"), or diverged, weighs nothing in the updates).
//
// Shape: the elements e = p H + t of a launch are independent and their observation rows lie back to back, so a workgroup
// takes `rows` (64, fewer for very wide rows) consecutive elements, copies their rows into LDS with unit-stride loads (lane i
// reads word i of the tile) and then lane j walks the table over row j of the tile.  Read straight from memory, lane j's gathers would be d_obs words
// apart: one 64-byte request per lane and per row of the table.  The LDS rows are padded to an odd number of words, which
// spreads the lanes' column reads over all banks.  The table is decoded once per workgroup into LDS; every lane reads the
// same entry at the same time (a broadcast).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mjmpc_amd.h"

namespace mjmpc {
int set_error(int code, const char* what, const char* detail);      // capi.hip: the message mjmpc_last_error() returns

namespace {

constexpr int CT_WG = 256;
constexpr int CT_ROWS = 64;                 // elements per workgroup: four wavefronts copy the tile, one walks the table.  Small
                                            // tiles put many workgroups in flight; measured against one-wavefront workgroups
                                            // and against a walk that fetches rows ahead (both slower): profiles/r16_cost_terms.txt
constexpr int CT_MAX_TERMS = 128;
constexpr int CT_LDS_BYTES = 60 * 1024;     // the tile's share of a workgroup's 64 KiB (the decoded table takes 3.5 KiB)
constexpr int CT_BATCH_LDS_BYTES = 56 * 1024;   // cost_terms_batch_kernel's tile: two sets of weights and targets and a chunk's
                                                // costs stand beside it (6 KiB)

// a decoded row's flags
constexpr int CT_ACTION = 1, CT_TERMINAL = 2, CT_GROUP_FIRST = 4, CT_GROUP_LAST = 8;
constexpr int CT_RATE = 16;                 // (only the extended decode, X, sets it: source 2)

// the odd row pitch in words of the tile
__host__ __device__ inline int ct_pitch(int n) { return n | 1; }

// copy `rows` rows of `width` words, back to back in memory from src, to LDS rows of `pitch` words; unit stride over the lanes
template <typename T>
__device__ __forceinline__ void ct_stage(const T* __restrict__ src, int rows, int width, int pitch, T* dst) {
    const int n = rows * width;
    int i = threadIdx.x, r = i / width, c = i - r * width;
    const int dr = CT_WG / width, dc = CT_WG - dr * width;
    for (; i < n; i += CT_WG) {
        dst[r * pitch + c] = src[i];
        r += dr;
        c += dc;
        if (c >= width) { c -= width; ++r; }
    }
}

// decode the structural columns of a table (kind, source, index, group, when) into LDS: `terms` is [n_terms][8].
// X (the kernels of DESIGN 12.2): a row of source 2 reads the action tile like one of source 1 and is marked CT_RATE.
template <bool X = false>
__device__ __forceinline__ void ct_decode(const double* __restrict__ terms, int n_terms, int* s_kind, int* s_col, int* s_flags) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        const double* row = terms + 8 * k;
        const int kind = (int)row[0];
        const double group = row[5];
        int f = (row[1] != 0.0 ? CT_ACTION : 0) | (row[6] != 0.0 ? CT_TERMINAL : 0);
        if (kind == 2) {
            if (k == 0 || (int)terms[8 * (k - 1)] != 2 || terms[8 * (k - 1) + 5] != group) f |= CT_GROUP_FIRST;
            if (k == n_terms - 1 || (int)terms[8 * (k + 1)] != 2 || terms[8 * (k + 1) + 5] != group) f |= CT_GROUP_LAST;
        }
        if constexpr (X) {
            if (row[1] == 2.0) f |= CT_RATE;
        }
        s_kind[k] = kind;
        s_col[k] = (int)row[2];
        s_flags[k] = f;
    }
}

// the weights and targets of a table into LDS
__device__ __forceinline__ void ct_decode_values(const double* __restrict__ terms, int n_terms, double* s_w, double* s_target) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        s_w[k] = terms[8 * k + 3];
        s_target[k] = terms[8 * k + 4];
    }
}

// where a walk takes row k's weight and target from: two arrays in LDS
struct CtArrays {
    const double *w, *target;
    __device__ __forceinline__ double weight(int k) const { return w[k]; }
    __device__ __forceinline__ double goal(int k) const { return target[k]; }
};

// one element's walk over the table: its observation row my_o and action row my_a (LDS), `acc` the first addend.
// X (the instantiations without it are the code they were): a CT_RATE row reads the action minus the action of
// the step before - the tile row in front of my_a, which its kernel staged, or at the first step of a plan entry `col` of
// `prev` (float64, through the cache; NaN or no `prev`: nothing has been applied yet and the rate is 0) - and the kinds
// 4 .. 7 are the one-sided ABOVE w max(0, r), BELOW w max(0, -r), ABOVE_SQUARE and BELOW_SQUARE.
template <bool X = false, typename T, typename V>
__device__ __forceinline__ double ct_walk(const int* s_kind, const int* s_col, const int* s_flags, int n_terms, const T* my_o,
                                          const T* my_a, bool last_step, double acc, const V values, int pa = 0,
                                          bool first_step = false, const double* prev = nullptr) {
    double sq = 0.0, w_group = 0.0;
    for (int k = 0; k < n_terms; ++k) {
        const int f = s_flags[k], kind = s_kind[k];
        if ((f & CT_TERMINAL) && !last_step) continue;
        double v = (double)((f & CT_ACTION) ? my_a[s_col[k]] : my_o[s_col[k]]);
        if constexpr (X) {
            if (f & CT_RATE) {
                const int c = s_col[k];
                if (first_step) {
                    const double before = prev ? prev[c] : (double)NAN;
                    v = before == before ? v - before : 0.0;
                } else {
                    v -= (double)my_a[c - pa];
                }
            }
        }
        const double r = v - values.goal(k);
        const double w = values.weight(k);
        if (kind == 0) {
            acc += w * fabs(r);
        } else if (kind == 1) {
            acc += w * (r * r);
        } else if (kind == 2) {
            if (f & CT_GROUP_FIRST) { sq = 0.0; w_group = w; }
            sq += r * r;
            if (f & CT_GROUP_LAST) acc += w_group * sqrt(sq);
        } else if (!X || kind == 3) {
            const double s = sin(0.5 * r);
            acc += w * (2.0 * s * s);
        } else {
            const double side = (kind & 1) ? -r : r;                // 5, 7: below the bound
            const double m = side > 0.0 ? side : 0.0;
            acc += w * (kind >= 6 ? m * m : m);
        }
    }
    return acc;
}

// grid: ceil(n / rows) workgroups of CT_WG; dynamic LDS: rows (pitch(d_obs) + pitch(A)) words of T
template <typename T>
__global__ __launch_bounds__(CT_WG) void cost_terms_kernel(const T* __restrict__ nobs, const T* __restrict__ act,
                                                           const double* __restrict__ terms, int n_terms, long n, int H,
                                                           int d_obs, int A, int rows, int keep_builtin, int terminal,
                                                           T* __restrict__ costs) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[CT_MAX_TERMS], s_target[CT_MAX_TERMS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS];
    const int po = ct_pitch(d_obs), pa = act ? ct_pitch(A) : 0;
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long e0 = (long)blockIdx.x * rows;
    const int mine = n - e0 < rows ? (int)(n - e0) : rows;

    ct_decode(terms, n_terms, s_kind, s_col, s_flags);
    ct_decode_values(terms, n_terms, s_w, s_target);
    ct_stage(nobs + e0 * d_obs, mine, d_obs, po, tile_o);
    if (act) ct_stage(act + e0 * A, mine, A, pa, tile_a);
    __syncthreads();

    const int j = threadIdx.x;
    if (j >= mine) return;
    const long e = e0 + j;
    const bool last_step = terminal && (int)(e % H) == H - 1;
    const T incoming = costs[e];
    const double acc = ct_walk(s_kind, s_col, s_flags, n_terms, tile_o + j * po, tile_a + j * pa, last_step,
                               keep_builtin ? (double)incoming : 0.0, CtArrays{s_w, s_target});
    costs[e] = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
}

// The episode batches' launch: the costs of E P particles, [E P][H], with one table for all or one per episode
// (the structural columns are episode 0's; weight and target the particle's own episode's), and in the same launch the
// discounted cost-to-go q0[p] = sum_t gseq[t] cost[p][t] of the costs as stored, forward, every product and sum rounded.
// A workgroup owns `ppw` whole particles - as many as fit the tile's `rows` elements, one if H is longer, and with a table per
// episode no more than an episode holds - and takes their ppw H elements in chunks of `rows`: stage, walk (lane j = element j
// of the chunk), store the cost and leave gseq[t] cost in LDS, then thread s < ppw carries particle s's sum on over the
// chunk's elements of that particle.  So a particle's costs meet in one thread whatever H is, the products are formed by all
// lanes and only the additions are serial, and the observations are read once.  ppw <= P consecutive particles cross at most
// one episode boundary: two sets of weights and targets are decoded into LDS and a lane picks its episode's.
// grid: ceil(E P / ppw) workgroups of CT_WG; dynamic LDS as cost_terms_kernel's
template <typename T>
__global__ __launch_bounds__(CT_WG) void cost_terms_batch_kernel(const T* __restrict__ nobs, const T* __restrict__ act,
                                                                 const double* __restrict__ terms, int n_terms, long np, long P,
                                                                 int H, int d_obs, int A, int rows, int ppw, int per_episode,
                                                                 int keep_builtin, int terminal, T* __restrict__ costs,
                                                                 const double* __restrict__ gseq, double* __restrict__ q0) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[2][CT_MAX_TERMS], s_target[2][CT_MAX_TERMS], s_gc[CT_ROWS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS];
    const int po = ct_pitch(d_obs), pa = act ? ct_pitch(A) : 0;
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long p0 = (long)blockIdx.x * ppw;                         // my first particle
    const int my_p = np - p0 < ppw ? (int)(np - p0) : ppw;          // my particles
    const long e0 = p0 * H;
    const int my_n = my_p * H;                                      // my elements (ppw > 1 only where ppw H <= rows)
    // my particles from `second` on belong to the episode after my first particle's
    int second = my_p;
    if (per_episode) {
        const long ep0 = p0 / P, next = (ep0 + 1) * P - p0;
        ct_decode_values(terms + ep0 * 8L * n_terms, n_terms, s_w[0], s_target[0]);
        if (next < my_p) {
            second = (int)next;
            ct_decode_values(terms + (ep0 + 1) * 8L * n_terms, n_terms, s_w[1], s_target[1]);
        }
    } else {
        ct_decode_values(terms, n_terms, s_w[0], s_target[0]);
    }
    ct_decode(terms, n_terms, s_kind, s_col, s_flags);
    double q = 0.0;                                                 // thread s < my_p: particle p0 + s's sum so far
    const int j = threadIdx.x;
    for (int c0 = 0; c0 < my_n; c0 += rows) {
        const int mine = my_n - c0 < rows ? my_n - c0 : rows;
        ct_stage(nobs + (e0 + c0) * d_obs, mine, d_obs, po, tile_o);
        if (act) ct_stage(act + (e0 + c0) * A, mine, A, pa, tile_a);
        __syncthreads();
        if (j < mine) {
            const int le = c0 + j, pl = le / H, t = le - pl * H;    // my element: particle pl of the workgroup's, step t
            const double g = gseq ? gseq[t] : 0.0;
            const T incoming = costs[e0 + le];
            const int slot = pl >= second;
            const double acc = ct_walk(s_kind, s_col, s_flags, n_terms, tile_o + j * po, tile_a + j * pa,
                                       terminal && t == H - 1, keep_builtin ? (double)incoming : 0.0,
                                       CtArrays{s_w[slot], s_target[slot]});
            const T out = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
            costs[e0 + le] = out;
            s_gc[j] = g * (double)out;
        }
        __syncthreads();
        if (q0 && j < my_p) {
            // my particle's elements are [j H, (j + 1) H) of the workgroup's; this chunk holds [c0, c0 + mine)
            const int lo = j * H > c0 ? j * H : c0;
            const int hi = (j + 1) * H < c0 + mine ? (j + 1) * H : c0 + mine;
#pragma unroll 4
            for (int i = lo; i < hi; ++i) q += s_gc[i - c0];
        }
    }
    if (q0 && j < my_p) q0[p0 + j] = fabs(q) < (double)INFINITY ? q : (double)INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Terms that track a reference trajectory.  A tracked row's `reserved` column holds 1 + c, c its column of the
// reference `ref` (float64 [n_ref][n_cols]; row n = the goal for env time n).  A launch's base time is b = *step + bias, a
// counter on the device: a captured graph or a launch tape freezes the pointer, not the value.  Element (p, t) compares its
// observation rows with reference row b + t + 1 and its action rows with row b + t, clamped to [0, n_ref - 1] or taken
// mod n_ref.  b is reduced once per workgroup (it is uniform) into a 32-bit base; a lane adds its t in 32 bits: n_ref <= 2^20.
constexpr int CT_MAX_REF_ROWS = 1 << 20;

struct CtClock {
    int base, n, periodic;      // periodic: base = b mod n in [0, n); else b clamped to [-2^31, n - 1]
};

__device__ __forceinline__ CtClock ct_clock(long b, int n, int periodic) {
    if (periodic) {
        long m = b % n;
        if (m < 0) m += n;
        return CtClock{(int)m, n, 1};
    }
    const long lo = -(1L << 31);        // lo + t < 0 for every t < 2^31: all of such a launch holds the first goal
    return CtClock{(int)(b < lo ? lo : b > n - 1 ? (long)(n - 1) : b), n, 0};
}

// the reference rows of step t >= 0: the observation's (time b + t + 1) and the action's (time b + t)
__device__ __forceinline__ void ct_ref_rows(const CtClock c, int t, int& n_obs, int& n_act) {
    if (c.periodic) {
        const unsigned a = ((unsigned)c.base + (unsigned)t) % (unsigned)c.n;        // base < 2^20, t < 2^31
        n_act = (int)a;
        n_obs = (int)a + 1 == c.n ? 0 : (int)a + 1;
    } else {
        const unsigned top = (unsigned)(c.n - 1);
        unsigned up = (unsigned)c.base + (unsigned)t;               // (used only where base >= 0: below 2^32)
        up = up < top ? up : top;
        const int s = c.base < 0 ? c.base + t : (int)up;            // min(b + t, n - 1) or, from a negative base, b + t < 2^31 - 1
        n_act = s < 0 ? 0 : s > c.n - 1 ? c.n - 1 : s;
        n_obs = s + 1 < 0 ? 0 : s + 1 > c.n - 1 ? c.n - 1 : s + 1;
    }
}

// a table's reference columns into LDS: -1 for a row with a constant target.  A column beyond the reference (the host
// builder never writes one) is held inside it: the walk must not read past `ref` whatever the table says.
__device__ __forceinline__ void ct_decode_ref_cols(const double* __restrict__ terms, int n_terms, int n_cols, int* s_rcol) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        const int c = (int)terms[8 * k + 7] - 1;
        s_rcol[k] = c < 0 ? -1 : c < n_cols ? c : n_cols - 1;
    }
}

// where a walk over a table with tracked rows takes row k's goal from: the element's two reference rows, read through the
// cache (a launch's window is (H + 1) n_cols doubles, the same few KB for every workgroup), or the constant target
struct CtTracked {
    const double *w, *target;
    const int *rcol, *flags;
    const double *ref_o, *ref_a;
    __device__ __forceinline__ double weight(int k) const { return w[k]; }
    __device__ __forceinline__ double goal(int k) const {
        const int c = rcol[k];
        return c < 0 ? target[k] : ((flags[k] & CT_ACTION) ? ref_a : ref_o)[c];
    }
};

// cost_terms_kernel with tracked rows.  advance (host: only for P = H = 1, one workgroup): every lane takes its copy of the
// counter before the barrier, the one walking lane stores counter + 1 behind its walk.
template <typename T>
__global__ __launch_bounds__(CT_WG) void cost_terms_track_kernel(const T* __restrict__ nobs, const T* __restrict__ act,
                                                                 const double* __restrict__ terms, int n_terms, long n, int H,
                                                                 int d_obs, int A, int rows, int keep_builtin, int terminal,
                                                                 const double* __restrict__ ref, int n_ref, int n_cols,
                                                                 int periodic, int64_t* step, int64_t bias, int advance,
                                                                 T* __restrict__ costs) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[CT_MAX_TERMS], s_target[CT_MAX_TERMS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[CT_MAX_TERMS];
    const int po = ct_pitch(d_obs), pa = act ? ct_pitch(A) : 0;
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long e0 = (long)blockIdx.x * rows;
    const int mine = n - e0 < rows ? (int)(n - e0) : rows;
    const int64_t now = *step;
    const CtClock clock = ct_clock((long)(now + bias), n_ref, periodic);

    ct_decode(terms, n_terms, s_kind, s_col, s_flags);
    ct_decode_values(terms, n_terms, s_w, s_target);
    ct_decode_ref_cols(terms, n_terms, n_cols, s_rcol);
    ct_stage(nobs + e0 * d_obs, mine, d_obs, po, tile_o);
    if (act) ct_stage(act + e0 * A, mine, A, pa, tile_a);
    __syncthreads();

    const int j = threadIdx.x;
    if (j >= mine) return;
    const long e = e0 + j;
    const int t = (int)(e % H);
    int n_obs, n_act;
    ct_ref_rows(clock, t, n_obs, n_act);
    const T incoming = costs[e];
    const double acc = ct_walk(s_kind, s_col, s_flags, n_terms, tile_o + j * po, tile_a + j * pa, terminal && t == H - 1,
                               keep_builtin ? (double)incoming : 0.0,
                               CtTracked{s_w, s_target, s_rcol, s_flags, ref + (long)n_obs * n_cols, ref + (long)n_act * n_cols});
    costs[e] = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
    if (advance) *step = now + 1;       // (n = 1: this lane is the launch's only one behind the barrier)
}

// cost_terms_batch_kernel with tracked rows: one reference for the batch or one per episode ([E][n_ref][n_cols], the
// particle's own episode's).  The counter is only read: the batch classes' update launches advance it.
template <typename T>
__global__ __launch_bounds__(CT_WG) void cost_terms_track_batch_kernel(
    const T* __restrict__ nobs, const T* __restrict__ act, const double* __restrict__ terms, int n_terms, long np, long P, int H,
    int d_obs, int A, int rows, int ppw, int per_episode, int keep_builtin, int terminal, const double* __restrict__ ref,
    int n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* __restrict__ step, int64_t bias,
    T* __restrict__ costs, const double* __restrict__ gseq, double* __restrict__ q0) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[2][CT_MAX_TERMS], s_target[2][CT_MAX_TERMS], s_gc[CT_ROWS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[CT_MAX_TERMS];
    const int po = ct_pitch(d_obs), pa = act ? ct_pitch(A) : 0;
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long p0 = (long)blockIdx.x * ppw;
    const int my_p = np - p0 < ppw ? (int)(np - p0) : ppw;
    const long e0 = p0 * H;
    const int my_n = my_p * H;
    const CtClock clock = ct_clock((long)(*step + bias), n_ref, periodic);
    // my particles from `second` on belong to the episode after my first particle's (the host keeps ppw <= P whenever
    // the tables or the references are per episode)
    int second = my_p;
    const long ep0 = p0 / P;
    if ((per_episode || ref_per_episode) && (ep0 + 1) * P - p0 < my_p) second = (int)((ep0 + 1) * P - p0);
    if (per_episode) {
        ct_decode_values(terms + ep0 * 8L * n_terms, n_terms, s_w[0], s_target[0]);
        if (second < my_p) ct_decode_values(terms + (ep0 + 1) * 8L * n_terms, n_terms, s_w[1], s_target[1]);
    } else {
        ct_decode_values(terms, n_terms, s_w[0], s_target[0]);
    }
    const long ref_len = (long)n_ref * n_cols;
    const double* const ref0 = ref + (ref_per_episode ? ep0 * ref_len : 0);
    ct_decode(terms, n_terms, s_kind, s_col, s_flags);
    ct_decode_ref_cols(terms, n_terms, n_cols, s_rcol);
    double q = 0.0;
    const int j = threadIdx.x;
    for (int c0 = 0; c0 < my_n; c0 += rows) {
        const int mine = my_n - c0 < rows ? my_n - c0 : rows;
        ct_stage(nobs + (e0 + c0) * d_obs, mine, d_obs, po, tile_o);
        if (act) ct_stage(act + (e0 + c0) * A, mine, A, pa, tile_a);
        __syncthreads();
        if (j < mine) {
            const int le = c0 + j, pl = le / H, t = le - pl * H;
            const double g = gseq ? gseq[t] : 0.0;
            const T incoming = costs[e0 + le];
            const int slot = pl >= second;
            const double* const my_ref = ref0 + (ref_per_episode && slot ? ref_len : 0);
            int n_obs, n_act;
            ct_ref_rows(clock, t, n_obs, n_act);
            const int ws = per_episode ? slot : 0;
            const double acc = ct_walk(s_kind, s_col, s_flags, n_terms, tile_o + j * po, tile_a + j * pa,
                                       terminal && t == H - 1, keep_builtin ? (double)incoming : 0.0,
                                       CtTracked{s_w[ws], s_target[ws], s_rcol, s_flags, my_ref + (long)n_obs * n_cols,
                                                 my_ref + (long)n_act * n_cols});
            const T out = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
            costs[e0 + le] = out;
            s_gc[j] = g * (double)out;
        }
        __syncthreads();
        if (q0 && j < my_p) {
            const int lo = j * H > c0 ? j * H : c0;
            const int hi = (j + 1) * H < c0 + mine ? (j + 1) * H : c0 + mine;
#pragma unroll 4
            for (int i = lo; i < hi; ++i) q += s_gc[i - c0];
        }
    }
    if (q0 && j < my_p) q0[p0 + j] = fabs(q) < (double)INFINITY ? q : (double)INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Action-rate rows and one-sided kinds.  A row of source 2 reads u_t - u_{t-1}: the action row of the element
// before, which may lie in another workgroup's tile.  So a tile (or a batch chunk) of these kernels holds one more action row
// in front - the row of element e0 - 1 where e0 > 0 - and lane j's action row is tile row j + 1, its previous one tile row j,
// whatever j is: no lane goes to memory for it.  Only the lanes at t = 0 leave the tile, for the launch's previous-action
// vector `prev` (float64 [A], through the cache).  TRACK: rows may be tracked as in the kernels above; without it the
// reference, the counter and their decode are compiled out (measured against the run-time test: profiles/r19_rate.txt).

// stage the action rows of elements [first, first + mine) behind tile row 0, and row first - 1 into it where there is one
template <typename T>
__device__ __forceinline__ void ct_stage_actions(const T* __restrict__ act, long first, int mine, int A, int pa, T* tile_a) {
    if (first > 0) ct_stage(act + (first - 1) * A, mine + 1, A, pa, tile_a);
    else ct_stage(act, mine, A, pa, tile_a + pa);
}

// grid: ceil(n / rows) workgroups of CT_WG; dynamic LDS: rows pitch(d_obs) + (rows + 1) pitch(A) words of T.
// advance (host: only for P = H = 1, one workgroup): the one walking lane stores counter + 1 (TRACK) and its action row
// into `prev` behind its walk - the lane that read them.
template <typename T, bool TRACK>
__global__ __launch_bounds__(CT_WG) void cost_terms_rate_kernel(const T* __restrict__ nobs, const T* __restrict__ act,
                                                                const double* __restrict__ terms, int n_terms, long n, int H,
                                                                int d_obs, int A, int rows, int keep_builtin, int terminal,
                                                                const double* __restrict__ ref, int n_ref, int n_cols,
                                                                int periodic, int64_t* step, int64_t bias, int advance,
                                                                double* prev, T* __restrict__ costs) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[CT_MAX_TERMS], s_target[CT_MAX_TERMS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[TRACK ? CT_MAX_TERMS : 1];
    const int po = ct_pitch(d_obs), pa = ct_pitch(A);
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long e0 = (long)blockIdx.x * rows;
    const int mine = n - e0 < rows ? (int)(n - e0) : rows;
    int64_t now = 0;
    CtClock clock{0, 1, 0};
    if constexpr (TRACK) {
        now = *step;
        clock = ct_clock((long)(now + bias), n_ref, periodic);
        ct_decode_ref_cols(terms, n_terms, n_cols, s_rcol);
    }
    ct_decode<true>(terms, n_terms, s_kind, s_col, s_flags);
    ct_decode_values(terms, n_terms, s_w, s_target);
    ct_stage(nobs + e0 * d_obs, mine, d_obs, po, tile_o);
    ct_stage_actions(act, e0, mine, A, pa, tile_a);
    __syncthreads();

    const int j = threadIdx.x;
    if (j >= mine) return;
    const long e = e0 + j;
    const int t = (int)(e % H);
    const T* const my_o = tile_o + j * po;
    const T* const my_a = tile_a + (j + 1) * pa;
    const T incoming = costs[e];
    const double first = keep_builtin ? (double)incoming : 0.0;
    double acc;
    if constexpr (TRACK) {
        int n_obs, n_act;
        ct_ref_rows(clock, t, n_obs, n_act);
        acc = ct_walk<true>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                            CtTracked{s_w, s_target, s_rcol, s_flags, ref + (long)n_obs * n_cols, ref + (long)n_act * n_cols},
                            pa, t == 0, prev);
    } else {
        acc = ct_walk<true>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                            CtArrays{s_w, s_target}, pa, t == 0, prev);
    }
    costs[e] = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
    if (advance) {                      // (n = 1: this lane is the launch's only one behind the barrier)
        if constexpr (TRACK) *step = now + 1;
        if (prev)
            for (int c = 0; c < A; ++c) prev[c] = (double)my_a[c];
    }
}

// The episode batches' launch with rate rows and one-sided kinds: cost_terms_track_batch_kernel's shape, every chunk with
// the action row in front of it (element e0 + c0 - 1).  `prev` is [E][A], the lane's own episode's row by the `slot` that
// picks its weights; advance_prev (host: only for P = H = 1, so a workgroup is one element): the element of episode e
// stores its action row into row e behind its walk.  The counter is only read.
// (waves_per_eu 5: left alone the tracked instantiations take 99 - 100 VGPRs, one allocation step past the five waves per
// SIMD of the kernels above; held to five they take 95, with no spill to scratch)
template <typename T, bool TRACK>
__global__ __launch_bounds__(CT_WG) __attribute__((amdgpu_waves_per_eu(5))) void cost_terms_rate_batch_kernel(
    const T* __restrict__ nobs, const T* __restrict__ act, const double* __restrict__ terms, int n_terms, long np, long P, int H,
    int d_obs, int A, int rows, int ppw, int per_episode, int keep_builtin, int terminal, const double* __restrict__ ref,
    int n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* __restrict__ step, int64_t bias, double* prev,
    int advance_prev, T* __restrict__ costs, const double* __restrict__ gseq, double* __restrict__ q0) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[2][CT_MAX_TERMS], s_target[2][CT_MAX_TERMS], s_gc[CT_ROWS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[TRACK ? CT_MAX_TERMS : 1];
    const int po = ct_pitch(d_obs), pa = ct_pitch(A);
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long p0 = (long)blockIdx.x * ppw;
    const int my_p = np - p0 < ppw ? (int)(np - p0) : ppw;
    const long e0 = p0 * H;
    const int my_n = my_p * H;
    CtClock clock{0, 1, 0};
    if constexpr (TRACK) {
        clock = ct_clock((long)(*step + bias), n_ref, periodic);
        ct_decode_ref_cols(terms, n_terms, n_cols, s_rcol);
    }
    // my particles from `second` on belong to the episode after my first particle's (the host keeps ppw <= P whenever the
    // tables, the references or the previous actions are per episode)
    int second = my_p;
    const long ep0 = p0 / P;
    if ((per_episode || ref_per_episode || prev) && (ep0 + 1) * P - p0 < my_p) second = (int)((ep0 + 1) * P - p0);
    if (per_episode) {
        ct_decode_values(terms + ep0 * 8L * n_terms, n_terms, s_w[0], s_target[0]);
        if (second < my_p) ct_decode_values(terms + (ep0 + 1) * 8L * n_terms, n_terms, s_w[1], s_target[1]);
    } else {
        ct_decode_values(terms, n_terms, s_w[0], s_target[0]);
    }
    const long ref_len = (long)n_ref * n_cols;
    const double* const ref0 = TRACK ? ref + (ref_per_episode ? ep0 * ref_len : 0) : nullptr;
    double* const prev0 = prev ? prev + ep0 * A : nullptr;
    ct_decode<true>(terms, n_terms, s_kind, s_col, s_flags);
    double q = 0.0;
    const int j = threadIdx.x;
    for (int c0 = 0; c0 < my_n; c0 += rows) {
        const int mine = my_n - c0 < rows ? my_n - c0 : rows;
        ct_stage(nobs + (e0 + c0) * d_obs, mine, d_obs, po, tile_o);
        ct_stage_actions(act, e0 + c0, mine, A, pa, tile_a);
        __syncthreads();
        if (j < mine) {
            const int le = c0 + j, pl = le / H, t = le - pl * H;
            const double g = gseq ? gseq[t] : 0.0;
            const T incoming = costs[e0 + le];
            const int slot = pl >= second;
            const int ws = per_episode ? slot : 0;
            double* const my_prev = prev0 ? prev0 + (slot ? A : 0) : nullptr;
            const T* const my_o = tile_o + j * po;
            const T* const my_a = tile_a + (j + 1) * pa;
            const double first = keep_builtin ? (double)incoming : 0.0;
            double acc;
            if constexpr (TRACK) {
                const double* const my_ref = ref0 + (ref_per_episode && slot ? ref_len : 0);
                int n_obs, n_act;
                ct_ref_rows(clock, t, n_obs, n_act);
                acc = ct_walk<true>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                    CtTracked{s_w[ws], s_target[ws], s_rcol, s_flags, my_ref + (long)n_obs * n_cols,
                                              my_ref + (long)n_act * n_cols},
                                    pa, t == 0, my_prev);
            } else {
                acc = ct_walk<true>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                    CtArrays{s_w[ws], s_target[ws]}, pa, t == 0, my_prev);
            }
            const T out = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
            costs[e0 + le] = out;
            s_gc[j] = g * (double)out;
            if (advance_prev && my_prev)        // (P = H = 1: this lane is its workgroup's only one)
                for (int c = 0; c < A; ++c) my_prev[c] = (double)my_a[c];
        }
        __syncthreads();
        if (q0 && j < my_p) {
            const int lo = j * H > c0 ? j * H : c0;
            const int hi = (j + 1) * H < c0 + mine ? (j + 1) * H : c0 + mine;
#pragma unroll 4
            for (int i = lo; i < hi; ++i) q += s_gc[i - c0];
        }
    }
    if (q0 && j < my_p) q0[p0 + j] = fabs(q) < (double)INFINITY ? q : (double)INFINITY;
}

int bad(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms", detail); }

template <typename T>
int launch(int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions, const double* d_terms,
           int n_terms, int keep_builtin, int terminal, void* d_costs, void* stream) {
    const long n = (long)P * H;
    const long row_bytes = (long)sizeof(T) * (ct_pitch(d_obs) + (d_actions ? ct_pitch(A) : 0));
    if (row_bytes > CT_LDS_BYTES) return bad("an observation and action row of more than 60 KiB");
    int rows = CT_ROWS;
    while (rows * row_bytes > CT_LDS_BYTES) rows >>= 1;
    const long blocks = (n + rows - 1) / rows;
    if (blocks > INT32_MAX) return bad("more than 2^31 workgroups");
    const size_t lds = (size_t)((rows * row_bytes + 7) / 8 * 8);
    hipLaunchKernelGGL(cost_terms_kernel<T>, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream,
                       (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, n, H, d_obs, A, rows, keep_builtin,
                       terminal, (T*)d_costs);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms", hipGetErrorString(e));
}

int bad_batch(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms_batch", detail); }

template <typename T>
int launch_batch(int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                 const double* d_terms, int n_terms, int per_episode, int keep_builtin, int terminal, void* d_costs,
                 const double* d_gseq, double* d_q0, void* stream) {
    const long np = (long)E * P;
    const long row_bytes = (long)sizeof(T) * (ct_pitch(d_obs) + (d_actions ? ct_pitch(A) : 0));
    if (row_bytes > CT_BATCH_LDS_BYTES) return bad_batch("an observation and action row of more than 56 KiB");
    int rows = CT_ROWS;
    while (rows * row_bytes > CT_BATCH_LDS_BYTES) rows >>= 1;
    int ppw = H >= rows ? 1 : rows / H;             // whole particles per workgroup ...
    if (per_episode && ppw > P) ppw = (int)P;       // ... of at most two episodes
    const long blocks = (np + ppw - 1) / ppw;
    if (blocks > INT32_MAX) return bad_batch("more than 2^31 workgroups");
    const size_t lds = (size_t)((rows * row_bytes + 7) / 8 * 8);
    hipLaunchKernelGGL(cost_terms_batch_kernel<T>, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream,
                       (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, np, (long)P, H, d_obs, A, rows, ppw,
                       per_episode, keep_builtin, terminal, (T*)d_costs, d_gseq, d_q0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms_batch", hipGetErrorString(e));
}

int bad_track(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms_track", detail); }

template <typename T>
int launch_track(int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions, const double* d_terms,
                 int n_terms, int keep_builtin, int terminal, const double* d_ref, int n_ref, int n_cols, int periodic,
                 int64_t* d_step, int64_t step_bias, int advance, void* d_costs, void* stream) {
    const long n = (long)P * H;
    const long row_bytes = (long)sizeof(T) * (ct_pitch(d_obs) + (d_actions ? ct_pitch(A) : 0));
    if (row_bytes > CT_LDS_BYTES) return bad_track("an observation and action row of more than 60 KiB");
    int rows = CT_ROWS;
    while (rows * row_bytes > CT_LDS_BYTES) rows >>= 1;
    const long blocks = (n + rows - 1) / rows;
    if (blocks > INT32_MAX) return bad_track("more than 2^31 workgroups");
    const size_t lds = (size_t)((rows * row_bytes + 7) / 8 * 8);
    hipLaunchKernelGGL(cost_terms_track_kernel<T>, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream,
                       (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, n, H, d_obs, A, rows, keep_builtin,
                       terminal, d_ref, n_ref, n_cols, periodic, d_step, step_bias, advance, (T*)d_costs);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms_track", hipGetErrorString(e));
}

int bad_track_batch(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms_track_batch", detail); }

template <typename T>
int launch_track_batch(int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                       const double* d_terms, int n_terms, int per_episode, int keep_builtin, int terminal,
                       const double* d_ref, int n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* d_step,
                       int64_t step_bias, void* d_costs, const double* d_gseq, double* d_q0, void* stream) {
    const long np = (long)E * P;
    const long row_bytes = (long)sizeof(T) * (ct_pitch(d_obs) + (d_actions ? ct_pitch(A) : 0));
    if (row_bytes > CT_BATCH_LDS_BYTES) return bad_track_batch("an observation and action row of more than 56 KiB");
    int rows = CT_ROWS;
    while (rows * row_bytes > CT_BATCH_LDS_BYTES) rows >>= 1;
    int ppw = H >= rows ? 1 : rows / H;                                     // whole particles per workgroup ...
    if ((per_episode || ref_per_episode) && ppw > P) ppw = (int)P;          // ... of at most two episodes
    const long blocks = (np + ppw - 1) / ppw;
    if (blocks > INT32_MAX) return bad_track_batch("more than 2^31 workgroups");
    const size_t lds = (size_t)((rows * row_bytes + 7) / 8 * 8);
    hipLaunchKernelGGL(cost_terms_track_batch_kernel<T>, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream,
                       (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, np, (long)P, H, d_obs, A, rows, ppw,
                       per_episode, keep_builtin, terminal, d_ref, n_ref, n_cols, ref_per_episode, periodic, d_step, step_bias,
                       (T*)d_costs, d_gseq, d_q0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms_track_batch", hipGetErrorString(e));
}

int bad_rate(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms_rate", detail); }

// the tile of the rate kernels: `rows` observation rows and rows + 1 action rows inside `budget` bytes -> rows, 0 if one does not fit
template <typename T>
int rate_rows(int d_obs, int A, long budget, size_t* lds) {
    const long row_bytes = (long)sizeof(T) * (ct_pitch(d_obs) + ct_pitch(A)), extra = (long)sizeof(T) * ct_pitch(A);
    if (row_bytes + extra > budget) return 0;
    int rows = CT_ROWS;
    while (rows * row_bytes + extra > budget) rows >>= 1;
    *lds = (size_t)((rows * row_bytes + extra + 7) / 8 * 8);
    return rows;
}

template <typename T>
int launch_rate(int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions, const double* d_terms,
                int n_terms, int keep_builtin, int terminal, const double* d_ref, int n_ref, int n_cols, int periodic,
                int64_t* d_step, int64_t step_bias, int advance, double* d_prev, void* d_costs, void* stream) {
    const long n = (long)P * H;
    size_t lds = 0;
    const int rows = rate_rows<T>(d_obs, A, CT_LDS_BYTES, &lds);
    if (!rows) return bad_rate("an observation row and two action rows of more than 60 KiB");
    const long blocks = (n + rows - 1) / rows;
    if (blocks > INT32_MAX) return bad_rate("more than 2^31 workgroups");
    auto* const kernel = d_ref ? cost_terms_rate_kernel<T, true> : cost_terms_rate_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream, (const T*)d_next_obs,
                       (const T*)d_actions, d_terms, n_terms, n, H, d_obs, A, rows, keep_builtin, terminal, d_ref, n_ref,
                       n_cols, periodic, d_step, step_bias, advance, d_prev, (T*)d_costs);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms_rate", hipGetErrorString(e));
}

int bad_rate_batch(const char* detail) { return set_error(MJMPC_E_BADARG, "mjmpc_cost_terms_rate_batch", detail); }

template <typename T>
int launch_rate_batch(int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                      const double* d_terms, int n_terms, int per_episode, int keep_builtin, int terminal,
                      const double* d_ref, int n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* d_step,
                      int64_t step_bias, double* d_prev, int advance_prev, void* d_costs, const double* d_gseq, double* d_q0,
                      void* stream) {
    const long np = (long)E * P;
    size_t lds = 0;
    const int rows = rate_rows<T>(d_obs, A, CT_BATCH_LDS_BYTES, &lds);
    if (!rows) return bad_rate_batch("an observation row and two action rows of more than 56 KiB");
    int ppw = H >= rows ? 1 : rows / H;                                             // whole particles per workgroup ...
    if ((per_episode || ref_per_episode || d_prev) && ppw > P) ppw = (int)P;        // ... of at most two episodes
    const long blocks = (np + ppw - 1) / ppw;
    if (blocks > INT32_MAX) return bad_rate_batch("more than 2^31 workgroups");
    auto* const kernel = d_ref ? cost_terms_rate_batch_kernel<T, true> : cost_terms_rate_batch_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CT_WG), lds, (hipStream_t)stream, (const T*)d_next_obs,
                       (const T*)d_actions, d_terms, n_terms, np, (long)P, H, d_obs, A, rows, ppw, per_episode, keep_builtin,
                       terminal, d_ref, n_ref, n_cols, ref_per_episode, periodic, d_step, step_bias, d_prev, advance_prev,
                       (T*)d_costs, d_gseq, d_q0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, "mjmpc_cost_terms_rate_batch", hipGetErrorString(e));
}

}  // namespace
}  // namespace mjmpc

extern "C" int mjmpc_cost_terms_rate(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                     const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal,
                                     const double* d_ref, int64_t n_ref, int n_cols, int periodic, int64_t* d_step,
                                     int64_t step_bias, int advance, double* d_prev_action, void* d_costs, void* stream) {
    using mjmpc::bad_rate;
    if (!d_next_obs || !d_actions || !d_terms || !d_costs) return bad_rate("null argument");
    if ((d_ref != nullptr) != (d_step != nullptr)) return bad_rate("d_ref and d_step go together");
    if (P < 1 || H < 1 || d_obs < 1 || A < 1) return bad_rate("needs P >= 1, H >= 1, d_obs >= 1 and A >= 1");
    if (P > ((int64_t)1 << 40)) return bad_rate("more than 2^40 particles");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return bad_rate("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad_rate("dtype must be MJMPC_F32 or MJMPC_F64");
    if (d_ref && (n_ref < 1 || n_ref > mjmpc::CT_MAX_REF_ROWS)) return bad_rate("n_ref must be 1 .. 2^20");
    if (d_ref && (n_cols < 1 || n_cols > mjmpc::CT_MAX_TERMS)) return bad_rate("n_cols must be 1 .. 128");
    if (advance && (P != 1 || H != 1))
        return bad_rate("advance needs P = H = 1 (one workgroup owns the counter and the previous action)");
    if (!d_ref) n_ref = n_cols = 1;
    if (dtype == MJMPC_F32)
        return mjmpc::launch_rate<float>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal, d_ref,
                                         (int)n_ref, n_cols, periodic != 0, d_step, step_bias, advance != 0, d_prev_action,
                                         d_costs, stream);
    return mjmpc::launch_rate<double>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal, d_ref,
                                      (int)n_ref, n_cols, periodic != 0, d_step, step_bias, advance != 0, d_prev_action, d_costs,
                                      stream);
}

extern "C" int mjmpc_cost_terms_rate_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                           const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                           int keep_builtin, int terminal, const double* d_ref, int64_t n_ref, int n_cols,
                                           int ref_per_episode, int periodic, const int64_t* d_step, int64_t step_bias,
                                           double* d_prev_actions, int advance_prev, void* d_costs, const double* d_gseq,
                                           double* d_q0, void* stream) {
    using mjmpc::bad_rate_batch;
    if (!d_next_obs || !d_actions || !d_terms || !d_costs) return bad_rate_batch("null argument");
    if ((d_ref != nullptr) != (d_step != nullptr)) return bad_rate_batch("d_ref and d_step go together");
    if (E < 1 || P < 1 || H < 1 || d_obs < 1 || A < 1)
        return bad_rate_batch("needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 1");
    if (P > ((int64_t)1 << 40) / E) return bad_rate_batch("more than 2^40 particles");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return bad_rate_batch("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad_rate_batch("dtype must be MJMPC_F32 or MJMPC_F64");
    if ((d_gseq != nullptr) != (d_q0 != nullptr)) return bad_rate_batch("d_gseq and d_q0 go together");
    if (d_ref && (n_ref < 1 || n_ref > mjmpc::CT_MAX_REF_ROWS)) return bad_rate_batch("n_ref must be 1 .. 2^20");
    if (d_ref && (n_cols < 1 || n_cols > mjmpc::CT_MAX_TERMS)) return bad_rate_batch("n_cols must be 1 .. 128");
    if (advance_prev && (P != 1 || H != 1))
        return bad_rate_batch("advance_prev needs P = H = 1 (one workgroup per episode owns its previous action)");
    if (!d_ref) { n_ref = n_cols = 1; ref_per_episode = 0; }
    if (dtype == MJMPC_F32)
        return mjmpc::launch_rate_batch<float>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                               keep_builtin, terminal, d_ref, (int)n_ref, n_cols, ref_per_episode != 0,
                                               periodic != 0, d_step, step_bias, d_prev_actions, advance_prev != 0, d_costs,
                                               d_gseq, d_q0, stream);
    return mjmpc::launch_rate_batch<double>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                            keep_builtin, terminal, d_ref, (int)n_ref, n_cols, ref_per_episode != 0,
                                            periodic != 0, d_step, step_bias, d_prev_actions, advance_prev != 0, d_costs,
                                            d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms_track(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                      const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal,
                                      const double* d_ref, int64_t n_ref, int n_cols, int periodic, int64_t* d_step,
                                      int64_t step_bias, int advance, void* d_costs, void* stream) {
    using mjmpc::bad_track;
    if (!d_next_obs || !d_terms || !d_costs || !d_ref || !d_step) return bad_track("null argument");
    if (P < 1 || H < 1 || d_obs < 1 || A < 0) return bad_track("needs P >= 1, H >= 1, d_obs >= 1 and A >= 0");
    if (P > ((int64_t)1 << 40)) return bad_track("more than 2^40 particles");
    if (d_actions && A < 1) return bad_track("actions of width 0");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return bad_track("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad_track("dtype must be MJMPC_F32 or MJMPC_F64");
    if (n_ref < 1 || n_ref > mjmpc::CT_MAX_REF_ROWS) return bad_track("n_ref must be 1 .. 2^20");
    if (n_cols < 1 || n_cols > mjmpc::CT_MAX_TERMS) return bad_track("n_cols must be 1 .. 128");
    if (advance && (P != 1 || H != 1)) return bad_track("advance needs P = H = 1 (one workgroup owns the counter)");
    if (dtype == MJMPC_F32)
        return mjmpc::launch_track<float>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal,
                                          d_ref, (int)n_ref, n_cols, periodic != 0, d_step, step_bias, advance != 0, d_costs,
                                          stream);
    return mjmpc::launch_track<double>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal, d_ref,
                                       (int)n_ref, n_cols, periodic != 0, d_step, step_bias, advance != 0, d_costs, stream);
}

extern "C" int mjmpc_cost_terms_track_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                            const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                            int keep_builtin, int terminal, const double* d_ref, int64_t n_ref, int n_cols,
                                            int ref_per_episode, int periodic, const int64_t* d_step, int64_t step_bias,
                                            void* d_costs, const double* d_gseq, double* d_q0, void* stream) {
    using mjmpc::bad_track_batch;
    if (!d_next_obs || !d_terms || !d_costs || !d_ref || !d_step) return bad_track_batch("null argument");
    if (E < 1 || P < 1 || H < 1 || d_obs < 1 || A < 0)
        return bad_track_batch("needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 0");
    if (P > ((int64_t)1 << 40) / E) return bad_track_batch("more than 2^40 particles");
    if (d_actions && A < 1) return bad_track_batch("actions of width 0");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return bad_track_batch("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad_track_batch("dtype must be MJMPC_F32 or MJMPC_F64");
    if ((d_gseq != nullptr) != (d_q0 != nullptr)) return bad_track_batch("d_gseq and d_q0 go together");
    if (n_ref < 1 || n_ref > mjmpc::CT_MAX_REF_ROWS) return bad_track_batch("n_ref must be 1 .. 2^20");
    if (n_cols < 1 || n_cols > mjmpc::CT_MAX_TERMS) return bad_track_batch("n_cols must be 1 .. 128");
    if (dtype == MJMPC_F32)
        return mjmpc::launch_track_batch<float>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                                keep_builtin, terminal, d_ref, (int)n_ref, n_cols, ref_per_episode != 0,
                                                periodic != 0, d_step, step_bias, d_costs, d_gseq, d_q0, stream);
    return mjmpc::launch_track_batch<double>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                             keep_builtin, terminal, d_ref, (int)n_ref, n_cols, ref_per_episode != 0,
                                             periodic != 0, d_step, step_bias, d_costs, d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                      const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                      int keep_builtin, int terminal, void* d_costs, const double* d_gseq, double* d_q0,
                                      void* stream) {
    using mjmpc::bad_batch;
    if (!d_next_obs || !d_terms || !d_costs) return bad_batch("null argument");
    if (E < 1 || P < 1 || H < 1 || d_obs < 1 || A < 0) return bad_batch("needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 0");
    if (P > ((int64_t)1 << 40) / E) return bad_batch("more than 2^40 particles");
    if (d_actions && A < 1) return bad_batch("actions of width 0");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return bad_batch("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad_batch("dtype must be MJMPC_F32 or MJMPC_F64");
    if ((d_gseq != nullptr) != (d_q0 != nullptr)) return bad_batch("d_gseq and d_q0 go together");
    if (dtype == MJMPC_F32)
        return mjmpc::launch_batch<float>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                          keep_builtin, terminal, d_costs, d_gseq, d_q0, stream);
    return mjmpc::launch_batch<double>(E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode != 0,
                                       keep_builtin, terminal, d_costs, d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                                const double* d_terms, int n_terms, int keep_builtin, int terminal, void* d_costs,
                                void* stream) {
    if (!d_next_obs || !d_terms || !d_costs) return mjmpc::bad("null argument");
    if (P < 1 || H < 1 || d_obs < 1 || A < 0) return mjmpc::bad("needs P >= 1, H >= 1, d_obs >= 1 and A >= 0");
    if (P > ((int64_t)1 << 40)) return mjmpc::bad("more than 2^40 particles");
    if (d_actions && A < 1) return mjmpc::bad("actions of width 0");
    if (n_terms < 1 || n_terms > mjmpc::CT_MAX_TERMS) return mjmpc::bad("n_terms must be 1 .. 128");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return mjmpc::bad("dtype must be MJMPC_F32 or MJMPC_F64");
    if (dtype == MJMPC_F32)
        return mjmpc::launch<float>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal, d_costs,
                                    stream);
    return mjmpc::launch<double>(P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal, d_costs,
                                 stream);
}
