// User-defined cost terms: a second, bandwidth-bound launch behind a rollout that turns the next
// observations and the actions of every (particle, step) into a cost from a table of terms.  The rollout kernels keep their
// built-in costs and are not touched: the terms live neither in the model block (its length is part of the ABI) nor in the
// rollout translation units (an edit there moves the register allocation of every instantiation).
//
// A table row is eight doubles - kind, source, index, weight, target, group, when, reserved (include/mjmpc_amd.h):
//   source 0       v = next_obs[p][t][index], as double
//   source 1       v = actions[p][t][index]
//   source 2       v = actions[p][t][index] - actions[p][t - 1][index], the action rate (rate entries only).  At t = 0 the
//                  step before is entry `index` of the launch's previous-action vector `prev` (float64 [A]); where that is
//                  NaN, or without `prev`, nothing has been applied yet and v = 0
//   reserved       0: the goal is the row's `target`.  1 + c (track and rate entries with a reference `ref`, float64
//                  [n_ref][n_cols]): the goal is column c of a reference row - row b + t + 1 for an observation, row b + t for an
//                  action (source 1 or 2), clamped to [0, n_ref - 1] or taken mod n_ref (`periodic`), b = *step + bias, a
//                  counter on the device: a captured graph or a launch tape freezes the pointer, not the value
//   r = v - goal
//   kind 0 ABS     w |r|
//   kind 1 SQUARE  w r^2
//   kind 2 NORM    consecutive rows of one group > 0: w_first sqrt(sum r^2), once, at the group's last row
//   kind 3 COS     w (1 - cos r), formed as 2 w sin^2(r / 2): no cancellation near r = 0
//   kind 4 ABOVE   w max(0, r)             kind 5 BELOW         w max(0, -r)            (4 .. 7: rate entries only)
//   kind 6 ABOVE_SQUARE  w max(0, r)^2     kind 7 BELOW_SQUARE  w max(0, -r)^2
//   kind 8 QUAD    consecutive rows of one group > 0, n <= 32 of them: w_first sum_i sum_j r_i Q_ij r_j, once, at the group's
//                  last row (quad entries only).  Q is the group's n x n matrix in the pool `quad` (float64 [quad_len], the
//                  groups' matrices back to back in table order, row-major, symmetric: the host stores (M + M') / 2); its
//                  offset is the sum of n^2 over the QUAD groups before it.  Q may be indefinite
//   kind 9 LINEAR  w r, signed (quad entries only)
//   when = 1       the row counts only at t = H - 1 and only if the launch says `terminal`
// The cost of (p, t) is the sum over the rows in row order, in double whatever the storage type, behind the incoming cost
// when keep_builtin is set; an incoming cost that is not finite leaves as +inf either way (a particle that reset
// under set_reset_returns("inf"), or diverged, weighs nothing in the updates).
//
// Shape: the elements e = p H + t of a launch are independent and their observation rows lie back to back, so a workgroup
// takes `rows` (64, fewer for very wide rows) consecutive elements, copies their rows into LDS with unit-stride loads (lane i
// reads word i of the tile) and then lane j walks the table over row j of the tile.  Read straight from memory, lane j's
// gathers would be d_obs words apart: one 64-byte request per lane and per row of the table.  The LDS rows are padded to an
// odd number of words, which spreads the lanes' column reads over all banks.  The table is decoded once per workgroup into
// LDS; every lane reads the same entry at the same time (a broadcast).
// The tile: `rows` observation rows, then - where the launch has actions - `rows` action rows; the rate kernels put one more
// action row in front of those, the row of the element before the tile's first (which may lie in another workgroup's tile),
// so lane j's action row is tile row j + 1 and its previous one tile row j, whatever j is: no lane goes to memory for it.
//
// Two kernel templates carry the eight entries: cost_terms_flat_kernel (one tile per workgroup) and cost_terms_batch_kernel
// (whole particles per workgroup, for the episode batches), each over <T, TRACK, RATE, QUAD>:
//   TRACK   rows may be tracked (`ref` given).  Off: the reference, the counter and the reference columns are compiled out.
//   RATE    source 2 and the kinds 4 .. 7, the leading action row, `prev`.  Off: they are compiled out, and a null `act` means
//           "no action tile".
//   QUAD    the kinds 8 and 9, the pool and the walking lanes' scratch (always with RATE: a quad table may hold any row).  Off:
//           they are compiled out; the sixteen instantiations without it are instruction for instruction what they were before
//           the flag existed (profiles/r21_quad_resources.txt)
// All are template flags and not run-time tests: that variant was measured slower (profiles/r19_rate.txt).
//
// QUAD's shape.  The walking lane parks r_i of a QUAD row in an LDS scratch behind the tile, laid out [i][lane]
// (64 doubles a row: lane-consecutive doubles, no bank conflict), and at the group's last row forms
// sum_i r_i (Q_ii r_i + 2 sum_{j<i} Q_ij r_j): the symmetry halves the scratch reads and the Q loads.  Q_ij is one address for all
// lanes and is read const __restrict__ through the cache (scalar loads, as the reference windows are).  Measured against it, the
// pool staged into LDS behind the scratch was 4.6 % faster with a pool of 245 doubles and no faster with 729 (47.1 / 87.8 us per
// launch at 4096 x 32 for a 14 x 14 with a 7 x 7 group / one 32 x 32 group, 16.5 / 19.5 us with the diagonals as SQUARE rows
// through the rate kernel: profiles/r21_quad.txt); it would take up to 32 KiB more from the tile, so Q stays in the cache.
// A row's place in its group, the group's size and its pool offset are worked out once per workgroup behind the decode, from
// LDS, and packed into one word a row.  The entry does not see the table (it is on the device), so the scratch is sized by the pool: no group is larger than
// n_cap = min(32, floor(sqrt(quad_len))) rows, the scratch is n_cap x 64 doubles (16 KiB at most) and comes out of the tile budget
// of the QUAD instantiations alone, with 1 KiB for the packed words.  Whatever the table says, a lane's scratch index stays below
// n_cap and a group's matrix inside quad_len: a group too long or a matrix past the pool's end is held inside both.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../include/mjmpc_amd.h"

namespace mjmpc {
int set_error(int code, const char* what, const char* detail);      // capi.hip: the message mjmpc_last_error() returns

namespace {

constexpr int CT_WG = 256;
constexpr int CT_ROWS = 64;                 // elements per workgroup: four wavefronts copy the tile, one walks the table.  Small
                                            // tiles put many workgroups in flight; measured against one-wavefront workgroups
                                            // and against a walk that fetches rows ahead (both slower): profiles/r16_cost_terms.txt
constexpr int CT_MAX_TERMS = 128;
constexpr int CT_MAX_REF_ROWS = 1 << 20;    // a lane adds its t to the launch's base time in 32 bits (ct_ref_rows)
constexpr int CT_LDS_BYTES = 60 * 1024;     // the tile's share of a workgroup's 64 KiB (the decoded table takes 3.5 - 4 KiB)
constexpr int CT_BATCH_LDS_BYTES = 56 * 1024;   // cost_terms_batch_kernel's tile: two sets of weights and targets and a chunk's
                                                // costs stand beside it (6 - 6.5 KiB)

// a decoded row's flags
constexpr int CT_ACTION = 1, CT_TERMINAL = 2, CT_GROUP_FIRST = 4, CT_GROUP_LAST = 8;
constexpr int CT_RATE = 16;                 // (only the RATE decode sets it: source 2)
constexpr int CT_MAX_QUAD = 32;             // rows of a QUAD group
constexpr int CT_MAX_QUAD_LEN = 4096;       // doubles of the pool: 128 rows in groups of at most 32
constexpr int CT_QUAD_STATIC = 1024;        // what the QUAD instantiations' static LDS takes from the tile budget (s_quad)
// a QUAD row's packed word (ct_decode_quad): its place in the group, the group's size (at its last row) and pool offset
constexpr int CT_Q_PLACE = 0x3f, CT_Q_SIZE_SHIFT = 6, CT_Q_OFFSET_SHIFT = 12;

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

// RATE: stage the action rows of elements [first, first + mine) behind tile row 0, and row first - 1 into it where there is one
template <typename T>
__device__ __forceinline__ void ct_stage_actions(const T* __restrict__ act, long first, int mine, int A, int pa, T* tile_a) {
    if (first > 0) ct_stage(act + (first - 1) * A, mine + 1, A, pa, tile_a);
    else ct_stage(act, mine, A, pa, tile_a + pa);
}

// decode the structural columns of a table (kind, source, index, group, when) into LDS: `terms` is [n_terms][8].
// RATE: a row of source 2 reads the action tile like one of source 1 and is marked CT_RATE.
template <bool RATE, bool QUAD = false>
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
        if constexpr (RATE) {
            if (row[1] == 2.0) f |= CT_RATE;
        }
        if constexpr (QUAD) {
            if (kind == 8) {
                if (k == 0 || (int)terms[8 * (k - 1)] != 8 || terms[8 * (k - 1) + 5] != group) f |= CT_GROUP_FIRST;
                if (k == n_terms - 1 || (int)terms[8 * (k + 1)] != 8 || terms[8 * (k + 1) + 5] != group) f |= CT_GROUP_LAST;
            }
        }
        s_kind[k] = kind;
        s_col[k] = (int)row[2];
        s_flags[k] = f;
    }
}

// QUAD, behind ct_decode and a barrier: row k's place i in its group, and at a group's last row its size n and the offset of its
// matrix - the sum of n^2 over the groups before it - packed into s_quad[k].  Held inside the scratch (i < n_cap, n <= n_cap) and
// the pool (offset + n^2 <= quad_len; n_cap^2 <= quad_len) whatever the table says: the host builder never writes such a table.
__device__ __forceinline__ void ct_decode_quad(const int* s_kind, const int* s_flags, int n_terms, int n_cap, int quad_len,
                                               int* s_quad) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        int word = 0;
        if (s_kind[k] == 8) {
            int run = 0;            // rows of the open group before row j
            long offset = 0;        // n^2 of the groups closed before row j
            for (int j = 0; j < k; ++j) {
                if (s_kind[j] != 8) continue;
                const int f = s_flags[j];
                if (f & CT_GROUP_FIRST) run = 0;
                ++run;
                if (f & CT_GROUP_LAST) { offset += (long)run * run; run = 0; }
            }
            const int fk = s_flags[k];
            if (fk & CT_GROUP_FIRST) run = 0;
            const int place = run < n_cap ? run : n_cap - 1;
            word = place;
            if (fk & CT_GROUP_LAST) {
                const int n = run + 1 < n_cap ? run + 1 : n_cap;
                if (offset + (long)n * n > quad_len) offset = 0;
                word |= (n << CT_Q_SIZE_SHIFT) | ((int)offset << CT_Q_OFFSET_SHIFT);
            }
        }
        s_quad[k] = word;
    }
}

// the weights and targets of a table into LDS
__device__ __forceinline__ void ct_decode_values(const double* __restrict__ terms, int n_terms, double* s_w, double* s_target) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        s_w[k] = terms[8 * k + 3];
        s_target[k] = terms[8 * k + 4];
    }
}

// TRACK: a table's reference columns into LDS, -1 for a row with a constant target.  A column beyond the reference (the host
// builder never writes one) is held inside it: the walk must not read past `ref` whatever the table says.
__device__ __forceinline__ void ct_decode_ref_cols(const double* __restrict__ terms, int n_terms, int n_cols, int* s_rcol) {
    for (int k = threadIdx.x; k < n_terms; k += CT_WG) {
        const int c = (int)terms[8 * k + 7] - 1;
        s_rcol[k] = c < 0 ? -1 : c < n_cols ? c : n_cols - 1;
    }
}

// TRACK: a launch's base time b, reduced once per workgroup (it is uniform) into 32 bits; a lane adds its t: n_ref <= 2^20
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

// QUAD: the scratch stands behind the tile (`end`: one past its last word), on the next double - where ct_tile()'s size ends
template <typename T>
__device__ __forceinline__ double* ct_scratch(double* raw, const T* end) {
    return raw + ((const char*)end - (const char*)raw + 7) / 8;
}

// where a walk takes row k's weight and goal from: two arrays in LDS ...
struct CtArrays {
    const double *w, *target;
    __device__ __forceinline__ double weight(int k) const { return w[k]; }
    __device__ __forceinline__ double goal(int k) const { return target[k]; }
};

// ... or (TRACK) the element's two reference rows, read through the cache (a launch's window is (H + 1) n_cols doubles, the
// same few KB for every workgroup), for a row with a reference column
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

// one element's walk over the table: its observation row my_o and action row my_a (LDS), `acc` the first addend.
// RATE: a CT_RATE row reads the action minus the action of the step before - the tile row in front of my_a (`pa` words), or
// at the first step of a plan entry `col` of `prev` (through the cache) - and the kinds 4 .. 7 exist.
// QUAD: the kinds 8 and 9 exist; `scr` is this lane's column of the scratch (entry i at scr[64 i]), `quad` the pool.
template <bool RATE, bool QUAD = false, typename T, typename V>
__device__ __forceinline__ double ct_walk(const int* s_kind, const int* s_col, const int* s_flags, int n_terms, const T* my_o,
                                          const T* my_a, bool last_step, double acc, const V values, int pa, bool first_step,
                                          const double* prev, const int* s_quad = nullptr, double* scr = nullptr,
                                          const double* __restrict__ quad = nullptr) {
    double sq = 0.0, w_group = 0.0;
    for (int k = 0; k < n_terms; ++k) {
        const int f = s_flags[k], kind = s_kind[k];
        if ((f & CT_TERMINAL) && !last_step) continue;
        double v = (double)((f & CT_ACTION) ? my_a[s_col[k]] : my_o[s_col[k]]);
        if constexpr (RATE) {
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
        if constexpr (QUAD) {
            if (kind == 8) {
                const int word = s_quad[k];
                if (f & CT_GROUP_FIRST) w_group = w;
                scr[CT_ROWS * (word & CT_Q_PLACE)] = r;
                if (f & CT_GROUP_LAST) {
                    const int n = (word >> CT_Q_SIZE_SHIFT) & CT_Q_PLACE;
                    const double* __restrict__ q_row = quad + (word >> CT_Q_OFFSET_SHIFT);
                    // (fma spelled out: left to the compiler, the flat and the batch kernel contracted these sums differently
                    //  and an episode of a batch was no longer the flat launch bit for bit)
                    double form = 0.0;
                    for (int i = 0; i < n; ++i, q_row += n) {
                        const double ri = scr[CT_ROWS * i];
                        double below = 0.0;
                        for (int c = 0; c < i; ++c) below = fma(q_row[c], scr[CT_ROWS * c], below);
                        form = fma(ri, fma(q_row[i], ri, 2.0 * below), form);
                    }
                    acc = fma(w_group, form, acc);
                }
                continue;
            }
            if (kind == 9) {
                acc = fma(w, r, acc);
                continue;
            }
        }
        if (kind == 0) {
            acc += w * fabs(r);
        } else if (kind == 1) {
            acc += w * (r * r);
        } else if (kind == 2) {
            if (f & CT_GROUP_FIRST) { sq = 0.0; w_group = w; }
            sq += r * r;
            if (f & CT_GROUP_LAST) acc += w_group * sqrt(sq);
        } else if (!RATE || kind == 3) {
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

// grid: ceil(n / rows) workgroups of CT_WG; dynamic LDS: ct_tile()'s.
// advance (host: only for P = H = 1, one workgroup): every lane takes its copy of the counter before the barrier; the one
// walking lane stores counter + 1 (TRACK) and its action row into `prev` (RATE, with a `prev`) behind its walk - the lane
// that read them.
// QUAD: dynamic LDS is the tile's and behind it quad_n x 64 doubles of scratch.
template <typename T, bool TRACK, bool RATE, bool QUAD = false>
__global__ __launch_bounds__(CT_WG) void cost_terms_flat_kernel(const T* __restrict__ nobs, const T* __restrict__ act,
                                                                const double* __restrict__ terms, int n_terms, long n, int H,
                                                                int d_obs, int A, int rows, int keep_builtin, int terminal,
                                                                const double* __restrict__ ref, int n_ref, int n_cols,
                                                                int periodic, int64_t* step, int64_t bias, int advance,
                                                                double* prev, T* __restrict__ costs,
                                                                const double* __restrict__ quad, int quad_len, int quad_n) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[CT_MAX_TERMS], s_target[CT_MAX_TERMS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[TRACK ? CT_MAX_TERMS : 1];
    __shared__ int s_quad[QUAD ? CT_MAX_TERMS : 1];
    const int po = ct_pitch(d_obs), pa = (RATE || act) ? ct_pitch(A) : 0;
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
    ct_decode<RATE, QUAD>(terms, n_terms, s_kind, s_col, s_flags);
    ct_decode_values(terms, n_terms, s_w, s_target);
    ct_stage(nobs + e0 * d_obs, mine, d_obs, po, tile_o);
    if constexpr (RATE) ct_stage_actions(act, e0, mine, A, pa, tile_a);
    else if (act) ct_stage(act + e0 * A, mine, A, pa, tile_a);
    __syncthreads();
    if constexpr (QUAD) {               // (the decoded kinds and group flags are in LDS now)
        ct_decode_quad(s_kind, s_flags, n_terms, quad_n, quad_len, s_quad);
        __syncthreads();
    }

    const int j = threadIdx.x;
    if (j >= mine) return;
    const long e = e0 + j;
    const int t = (TRACK || RATE || terminal) ? (int)(e % H) : 0;   // (a 64-bit remainder: not paid where nothing reads t)
    const T* const my_o = tile_o + j * po;
    const T* const my_a = tile_a + (j + RATE) * pa;
    const T incoming = costs[e];
    const double first = keep_builtin ? (double)incoming : 0.0;
    // QUAD: my column of the scratch behind the tile's (rows + 1) action rows
    double* const scr = QUAD ? ct_scratch(ct_tile_raw, tile_a + (long)(rows + 1) * pa) + j : nullptr;
    double acc;
    if constexpr (TRACK) {
        int n_obs, n_act;
        ct_ref_rows(clock, t, n_obs, n_act);
        acc = ct_walk<RATE, QUAD>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                  CtTracked{s_w, s_target, s_rcol, s_flags, ref + (long)n_obs * n_cols, ref + (long)n_act * n_cols},
                                  pa, t == 0, prev, s_quad, scr, quad);
    } else {
        acc = ct_walk<RATE, QUAD>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                  CtArrays{s_w, s_target}, pa, t == 0, prev, s_quad, scr, quad);
    }
    costs[e] = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
    if (advance) {                      // (n = 1: this lane is the launch's only one behind the barrier)
        if constexpr (TRACK) *step = now + 1;
        if constexpr (RATE) {
            if (prev)
                for (int c = 0; c < A; ++c) prev[c] = (double)my_a[c];
        }
    }
}

// The episode batches' launch: the costs of E P particles, [E P][H], with one table for all or one per episode
// (the structural columns are episode 0's; weight and target the particle's own episode's), and in the same launch the
// discounted cost-to-go q0[p] = sum_t gseq[t] cost[p][t] of the costs as stored, forward, every product and sum rounded.
// A workgroup owns `ppw` whole particles - as many as fit the tile's `rows` elements, one if H is longer, and no more than an
// episode holds where anything is per episode - and takes their ppw H elements in chunks of `rows`: stage (RATE: every chunk
// with the action row in front of it), walk (lane j = element j of the chunk), store the cost and leave gseq[t] cost in LDS,
// then thread s < ppw carries particle s's sum on over the chunk's elements of that particle.  So a particle's costs meet in
// one thread whatever H is, the products are formed by all lanes and only the additions are serial, and the observations are
// read once.  ppw <= P consecutive particles cross at most one episode boundary: two sets of weights and targets are decoded
// into LDS and a lane picks its episode's by its `slot`, as it picks its reference ([E][n_ref][n_cols] with ref_per_episode)
// and its row of `prev` ([E][A]).  The counter is only read: the batch classes' update launches advance it.
// advance_prev (host: only for P = H = 1, so a workgroup is one element): the element of episode e stores its action row into
// row e of `prev` behind its walk.
// grid: ceil(E P / ppw) workgroups of CT_WG; dynamic LDS as cost_terms_flat_kernel's
// (waves_per_eu 5: left alone the tracked instantiations take 97 - 100 VGPRs, one allocation step past the five waves per SIMD
// of the others; held to five they take 94 - 95, with no spill to scratch: profiles/r20_cost_terms_unify_resources.txt.
// The QUAD instantiations take 95 untracked and 94 tracked under it, five waves, nothing spilled to scratch: the attribute suits
// them as it does the rate instantiations they extend - profiles/r21_quad_resources.txt)
// QUAD: dynamic LDS is the tile's and behind it quad_n x 64 doubles of scratch, which every chunk reuses (s_gc is untouched).
template <typename T, bool TRACK, bool RATE, bool QUAD = false>
__global__ __launch_bounds__(CT_WG) __attribute__((amdgpu_waves_per_eu(5))) void cost_terms_batch_kernel(
    const T* __restrict__ nobs, const T* __restrict__ act, const double* __restrict__ terms, int n_terms, long np, long P, int H,
    int d_obs, int A, int rows, int ppw, int per_episode, int keep_builtin, int terminal, const double* __restrict__ ref,
    int n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* __restrict__ step, int64_t bias, double* prev,
    int advance_prev, T* __restrict__ costs, const double* __restrict__ gseq, double* __restrict__ q0,
    const double* __restrict__ quad, int quad_len, int quad_n) {
    extern __shared__ double ct_tile_raw[];
    __shared__ double s_w[2][CT_MAX_TERMS], s_target[2][CT_MAX_TERMS], s_gc[CT_ROWS];
    __shared__ int s_kind[CT_MAX_TERMS], s_col[CT_MAX_TERMS], s_flags[CT_MAX_TERMS], s_rcol[TRACK ? CT_MAX_TERMS : 1];
    __shared__ int s_quad[QUAD ? CT_MAX_TERMS : 1];
    const int po = ct_pitch(d_obs), pa = (RATE || act) ? ct_pitch(A) : 0;
    T* const tile_o = reinterpret_cast<T*>(ct_tile_raw);
    T* const tile_a = tile_o + (long)rows * po;
    const long p0 = (long)blockIdx.x * ppw;                         // my first particle
    const int my_p = np - p0 < ppw ? (int)(np - p0) : ppw;          // my particles
    const long e0 = p0 * H;
    const int my_n = my_p * H;                                      // my elements (ppw > 1 only where ppw H <= rows)
    CtClock clock{0, 1, 0};
    if constexpr (TRACK) {
        clock = ct_clock((long)(*step + bias), n_ref, periodic);
        ct_decode_ref_cols(terms, n_terms, n_cols, s_rcol);
    }
    // my first particle's episode, ep0, and the first of my particles that belongs to the episode after it, `second`: looked
    // for only where the tables, the references or the previous actions are per episode (the host keeps ppw <= P there).
    // (One table for all goes straight to its decode: with the split in front of this `if` the launch measured 3 % slower.)
    long ep0 = 0;
    int second = my_p;
    auto split = [&] {
        ep0 = p0 / P;
        if ((ep0 + 1) * P - p0 < my_p) second = (int)((ep0 + 1) * P - p0);
    };
    if (per_episode) {
        split();
        ct_decode_values(terms + ep0 * 8L * n_terms, n_terms, s_w[0], s_target[0]);
        if (second < my_p) ct_decode_values(terms + (ep0 + 1) * 8L * n_terms, n_terms, s_w[1], s_target[1]);
    } else {
        if ((TRACK && ref_per_episode) || (RATE && prev)) split();
        ct_decode_values(terms, n_terms, s_w[0], s_target[0]);
    }
    const long ref_len = (long)n_ref * n_cols;
    const double* const ref0 = TRACK ? ref + (ref_per_episode ? ep0 * ref_len : 0) : nullptr;
    double* const prev0 = RATE && prev ? prev + ep0 * A : nullptr;
    ct_decode<RATE, QUAD>(terms, n_terms, s_kind, s_col, s_flags);
    if constexpr (QUAD) {               // (the first chunk's barrier stands between these words and the walk)
        __syncthreads();
        ct_decode_quad(s_kind, s_flags, n_terms, quad_n, quad_len, s_quad);
    }
    double q = 0.0;                                                 // thread s < my_p: particle p0 + s's sum so far
    const int j = threadIdx.x;
    // QUAD: my column of the scratch behind the tile's (rows + 1) action rows; a lane's own, so every chunk reuses it
    double* const scr = QUAD ? ct_scratch(ct_tile_raw, tile_a + (long)(rows + 1) * pa) + j : nullptr;
    for (int c0 = 0; c0 < my_n; c0 += rows) {
        const int mine = my_n - c0 < rows ? my_n - c0 : rows;
        ct_stage(nobs + (e0 + c0) * d_obs, mine, d_obs, po, tile_o);
        if constexpr (RATE) ct_stage_actions(act, e0 + c0, mine, A, pa, tile_a);
        else if (act) ct_stage(act + (e0 + c0) * A, mine, A, pa, tile_a);
        __syncthreads();
        if (j < mine) {
            const int le = c0 + j, pl = le / H, t = le - pl * H;    // my element: particle pl of the workgroup's, step t
            const double g = gseq ? gseq[t] : 0.0;
            const T incoming = costs[e0 + le];
            const int slot = pl >= second;
            const int ws = per_episode ? slot : 0;
            double* const my_prev = prev0 ? prev0 + (slot ? A : 0) : nullptr;
            const T* const my_o = tile_o + j * po;
            const T* const my_a = tile_a + (j + RATE) * pa;
            const double first = keep_builtin ? (double)incoming : 0.0;
            double acc;
            if constexpr (TRACK) {
                const double* const my_ref = ref0 + (ref_per_episode && slot ? ref_len : 0);
                int n_obs, n_act;
                ct_ref_rows(clock, t, n_obs, n_act);
                acc = ct_walk<RATE, QUAD>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                          CtTracked{s_w[ws], s_target[ws], s_rcol, s_flags, my_ref + (long)n_obs * n_cols,
                                                    my_ref + (long)n_act * n_cols},
                                          pa, t == 0, my_prev, s_quad, scr, quad);
            } else {
                acc = ct_walk<RATE, QUAD>(s_kind, s_col, s_flags, n_terms, my_o, my_a, terminal && t == H - 1, first,
                                          CtArrays{s_w[ws], s_target[ws]}, pa, t == 0, my_prev, s_quad, scr, quad);
            }
            const T out = fabs((double)incoming) < (double)INFINITY ? (T)acc : (T)INFINITY;
            costs[e0 + le] = out;
            s_gc[j] = g * (double)out;
            if constexpr (RATE) {
                if (advance_prev && my_prev)        // (P = H = 1: this lane is its workgroup's only one)
                    for (int c = 0; c < A; ++c) my_prev[c] = (double)my_a[c];
            }
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

// ---- the host side: one tile sizing, one launch per kernel template, one check per concern ---------------------------------

int bad(const char* entry, const char* detail) { return set_error(MJMPC_E_BADARG, entry, detail); }

// the tile inside `budget` bytes: `rows` observation rows of `word` bytes a word, as many action rows where the launch has
// actions, and one more in front of those for a rate kernel; rows = 0: one row does not fit
struct CtTile {
    int rows;
    size_t lds;
};

CtTile ct_tile(long word, int d_obs, int A, bool actions, bool leading_row, long budget) {
    const long row_bytes = word * (ct_pitch(d_obs) + (actions ? ct_pitch(A) : 0)), extra = leading_row ? word * ct_pitch(A) : 0;
    if (row_bytes + extra > budget) return CtTile{0, 0};
    int rows = CT_ROWS;
    while (rows * row_bytes + extra > budget) rows >>= 1;
    return CtTile{rows, (size_t)((rows * row_bytes + extra + 7) / 8 * 8)};
}

// the quad entries' share of LDS: no group holds more rows than n_cap (n^2 <= quad_len), the scratch is n_cap x 64 doubles
struct CtQuad {
    int n_cap;
    long scratch;       // bytes, behind the tile
    long budget;        // the tile's, out of `whole` (CT_LDS_BYTES or CT_BATCH_LDS_BYTES)
};

CtQuad ct_quad(int quad_len, long whole) {
    int n = 1;
    while (n < CT_MAX_QUAD && (n + 1) * (n + 1) <= quad_len) ++n;
    const long scratch = 8L * CT_ROWS * n;
    return CtQuad{n, scratch, whole - CT_QUAD_STATIC - scratch};
}

// a quad entry's refusal of a row too wide, with the limit that holds for this pool
int ct_quad_too_wide(const char* entry, const CtQuad q) {
    char detail[160];
    snprintf(detail, sizeof detail, "an observation row and two action rows of more than %ld bytes (groups of up to %d rows take "
             "%ld bytes of scratch from the tile)", q.budget, q.n_cap, q.scratch);
    return bad(entry, detail);
}

// a launch of `blocks` workgroups in the storage type of `dtype`: `launch(zero of T)` issues it
template <typename Launch>
int ct_dispatch(const char* entry, long blocks, int dtype, Launch launch) {
    if (blocks > INT32_MAX) return bad(entry, "more than 2^31 workgroups");
    if (dtype == MJMPC_F32) launch(0.0f);
    else launch(0.0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, entry, hipGetErrorString(e));
}

// the flat entries: `rate` names the ones with the leading action row; d_ref, d_step and d_prev may be null; d_quad: the quad
// entry's pool (then `rate` is set)
int launch_flat(const char* entry, bool rate, int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal, const double* d_ref,
                int64_t n_ref, int n_cols, int periodic, int64_t* d_step, int64_t step_bias, int advance, double* d_prev,
                void* d_costs, void* stream, const double* d_quad = nullptr, int quad_len = 0) {
    const long n = (long)P * H;
    const CtQuad quad = d_quad ? ct_quad(quad_len, CT_LDS_BYTES) : CtQuad{0, 0, CT_LDS_BYTES};
    const CtTile tile = ct_tile(dtype == MJMPC_F32 ? 4 : 8, d_obs, A, d_actions != nullptr, rate, quad.budget);
    if (!tile.rows && d_quad) return ct_quad_too_wide(entry, quad);
    if (!tile.rows)
        return bad(entry, rate ? "an observation row and two action rows of more than 60 KiB"
                               : "an observation and action row of more than 60 KiB");
    if (!d_ref) n_ref = n_cols = 1;
    const long blocks = (n + tile.rows - 1) / tile.rows;
    return ct_dispatch(entry, blocks, dtype, [&](auto zero) {
        using T = decltype(zero);
        auto* const kernel =
            d_quad ? (d_ref ? cost_terms_flat_kernel<T, true, true, true> : cost_terms_flat_kernel<T, false, true, true>)
            : rate ? (d_ref ? cost_terms_flat_kernel<T, true, true> : cost_terms_flat_kernel<T, false, true>)
                   : (d_ref ? cost_terms_flat_kernel<T, true, false> : cost_terms_flat_kernel<T, false, false>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CT_WG), tile.lds + quad.scratch, (hipStream_t)stream,
                           (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, n, H, d_obs, A, tile.rows, keep_builtin,
                           terminal, d_ref, (int)n_ref, n_cols, periodic != 0, d_step, step_bias, advance != 0, d_prev,
                           (T*)d_costs, d_quad, quad_len, quad.n_cap);
    });
}

// the batch entries.  ppw: whole particles per workgroup, of at most two episodes; d_quad: as launch_flat's, one pool for all
int launch_batch(const char* entry, bool rate, int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                 const void* d_actions, const double* d_terms, int n_terms, int per_episode, int keep_builtin, int terminal,
                 const double* d_ref, int64_t n_ref, int n_cols, int ref_per_episode, int periodic, const int64_t* d_step,
                 int64_t step_bias, double* d_prev, int advance_prev, void* d_costs, const double* d_gseq, double* d_q0,
                 void* stream, const double* d_quad = nullptr, int quad_len = 0) {
    const long np = (long)E * P;
    const CtQuad quad = d_quad ? ct_quad(quad_len, CT_BATCH_LDS_BYTES) : CtQuad{0, 0, CT_BATCH_LDS_BYTES};
    const CtTile tile = ct_tile(dtype == MJMPC_F32 ? 4 : 8, d_obs, A, d_actions != nullptr, rate, quad.budget);
    if (!tile.rows && d_quad) return ct_quad_too_wide(entry, quad);
    if (!tile.rows)
        return bad(entry, rate ? "an observation row and two action rows of more than 56 KiB"
                               : "an observation and action row of more than 56 KiB");
    if (!d_ref) { n_ref = n_cols = 1; ref_per_episode = 0; }
    int ppw = H >= tile.rows ? 1 : tile.rows / H;
    if ((per_episode || ref_per_episode || d_prev) && ppw > P) ppw = (int)P;
    const long blocks = (np + ppw - 1) / ppw;
    return ct_dispatch(entry, blocks, dtype, [&](auto zero) {
        using T = decltype(zero);
        auto* const kernel =
            d_quad ? (d_ref ? cost_terms_batch_kernel<T, true, true, true> : cost_terms_batch_kernel<T, false, true, true>)
            : rate ? (d_ref ? cost_terms_batch_kernel<T, true, true> : cost_terms_batch_kernel<T, false, true>)
                   : (d_ref ? cost_terms_batch_kernel<T, true, false> : cost_terms_batch_kernel<T, false, false>);
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CT_WG), tile.lds + quad.scratch, (hipStream_t)stream,
                           (const T*)d_next_obs, (const T*)d_actions, d_terms, n_terms, np, (long)P, H, d_obs, A, tile.rows, ppw,
                           per_episode != 0, keep_builtin, terminal, d_ref, (int)n_ref, n_cols, ref_per_episode != 0,
                           periodic != 0, d_step, step_bias, d_prev, advance_prev != 0, (T*)d_costs, d_gseq, d_q0, d_quad,
                           quad_len, quad.n_cap);
    });
}

// The argument checks, one per concern: each returns its refusal or null.  An entry lists the ones that apply to it in its
// own order, with its own wording where the rule is its own, and refuses with the first that is not null.
const char* ct_first(std::initializer_list<const char*> refusals) {
    for (const char* r : refusals)
        if (r) return r;
    return nullptr;
}

const char* ct_not_null(bool all_given) { return all_given ? nullptr : "null argument"; }

const char* ct_together(const void* a, const void* b, const char* refusal) { return (a != nullptr) == (b != nullptr) ? nullptr : refusal; }

// every size at least 1, A at least min_A (`needs`: the entry's sentence), no action pointer with A = 0, E P <= 2^40
const char* ct_sizes(int E, int64_t P, int H, int d_obs, int A, int min_A, const void* d_actions, const char* needs) {
    if (E < 1 || P < 1 || H < 1 || d_obs < 1 || A < min_A) return needs;
    if (P > ((int64_t)1 << 40) / E) return "more than 2^40 particles";
    return d_actions && A < 1 ? "actions of width 0" : nullptr;
}

const char* ct_n_terms(int n_terms) { return n_terms < 1 || n_terms > CT_MAX_TERMS ? "n_terms must be 1 .. 128" : nullptr; }

const char* ct_dtype(int dtype) { return dtype != MJMPC_F32 && dtype != MJMPC_F64 ? "dtype must be MJMPC_F32 or MJMPC_F64" : nullptr; }

const char* ct_reference(const double* d_ref, int64_t n_ref, int n_cols) {
    if (d_ref && (n_ref < 1 || n_ref > CT_MAX_REF_ROWS)) return "n_ref must be 1 .. 2^20";
    return d_ref && (n_cols < 1 || n_cols > CT_MAX_TERMS) ? "n_cols must be 1 .. 128" : nullptr;
}

const char* ct_pool(const double* d_quad, int quad_len) {
    if (!d_quad) return "null d_quad";
    return quad_len < 1 || quad_len > CT_MAX_QUAD_LEN ? "quad_len must be 1 .. 4096" : nullptr;
}

const char* ct_advance(int advance, int64_t P, int H, const char* refusal) { return advance && (P != 1 || H != 1) ? refusal : nullptr; }

}  // namespace
}  // namespace mjmpc

using namespace mjmpc;

extern "C" int mjmpc_cost_terms(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                                const double* d_terms, int n_terms, int keep_builtin, int terminal, void* d_costs,
                                void* stream) {
    const char* const entry = "mjmpc_cost_terms";
    const char* const refusal = ct_first({ct_not_null(d_next_obs && d_terms && d_costs),
                                          ct_sizes(1, P, H, d_obs, A, 0, d_actions, "needs P >= 1, H >= 1, d_obs >= 1 and A >= 0"),
                                          ct_n_terms(n_terms), ct_dtype(dtype)});
    if (refusal) return bad(entry, refusal);
    return launch_flat(entry, false, dtype, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal,
                       nullptr, 0, 0, 0, nullptr, 0, 0, nullptr, d_costs, stream);
}

extern "C" int mjmpc_cost_terms_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                      const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                      int keep_builtin, int terminal, void* d_costs, const double* d_gseq, double* d_q0,
                                      void* stream) {
    const char* const entry = "mjmpc_cost_terms_batch";
    const char* const refusal =
        ct_first({ct_not_null(d_next_obs && d_terms && d_costs),
                  ct_sizes(E, P, H, d_obs, A, 0, d_actions, "needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 0"),
                  ct_n_terms(n_terms), ct_dtype(dtype), ct_together(d_gseq, d_q0, "d_gseq and d_q0 go together")});
    if (refusal) return bad(entry, refusal);
    return launch_batch(entry, false, dtype, E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode,
                        keep_builtin, terminal, nullptr, 0, 0, 0, 0, nullptr, 0, nullptr, 0, d_costs, d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms_track(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                      const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal,
                                      const double* d_ref, int64_t n_ref, int n_cols, int periodic, int64_t* d_step,
                                      int64_t step_bias, int advance, void* d_costs, void* stream) {
    const char* const entry = "mjmpc_cost_terms_track";
    const char* const refusal =
        ct_first({ct_not_null(d_next_obs && d_terms && d_costs && d_ref && d_step),
                  ct_sizes(1, P, H, d_obs, A, 0, d_actions, "needs P >= 1, H >= 1, d_obs >= 1 and A >= 0"), ct_n_terms(n_terms),
                  ct_dtype(dtype), ct_reference(d_ref, n_ref, n_cols),
                  ct_advance(advance, P, H, "advance needs P = H = 1 (one workgroup owns the counter)")});
    if (refusal) return bad(entry, refusal);
    return launch_flat(entry, false, dtype, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal,
                       d_ref, n_ref, n_cols, periodic, d_step, step_bias, advance, nullptr, d_costs, stream);
}

extern "C" int mjmpc_cost_terms_track_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                            const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                            int keep_builtin, int terminal, const double* d_ref, int64_t n_ref, int n_cols,
                                            int ref_per_episode, int periodic, const int64_t* d_step, int64_t step_bias,
                                            void* d_costs, const double* d_gseq, double* d_q0, void* stream) {
    const char* const entry = "mjmpc_cost_terms_track_batch";
    const char* const refusal =
        ct_first({ct_not_null(d_next_obs && d_terms && d_costs && d_ref && d_step),
                  ct_sizes(E, P, H, d_obs, A, 0, d_actions, "needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 0"),
                  ct_n_terms(n_terms), ct_dtype(dtype), ct_together(d_gseq, d_q0, "d_gseq and d_q0 go together"),
                  ct_reference(d_ref, n_ref, n_cols)});
    if (refusal) return bad(entry, refusal);
    return launch_batch(entry, false, dtype, E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode,
                        keep_builtin, terminal, d_ref, n_ref, n_cols, ref_per_episode, periodic, d_step, step_bias, nullptr, 0,
                        d_costs, d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms_rate(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                     const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal,
                                     const double* d_ref, int64_t n_ref, int n_cols, int periodic, int64_t* d_step,
                                     int64_t step_bias, int advance, double* d_prev_action, void* d_costs, void* stream) {
    const char* const entry = "mjmpc_cost_terms_rate";
    const char* const refusal = ct_first(
        {ct_not_null(d_next_obs && d_actions && d_terms && d_costs), ct_together(d_ref, d_step, "d_ref and d_step go together"),
         ct_sizes(1, P, H, d_obs, A, 1, d_actions, "needs P >= 1, H >= 1, d_obs >= 1 and A >= 1"), ct_n_terms(n_terms),
         ct_dtype(dtype), ct_reference(d_ref, n_ref, n_cols),
         ct_advance(advance, P, H, "advance needs P = H = 1 (one workgroup owns the counter and the previous action)")});
    if (refusal) return bad(entry, refusal);
    return launch_flat(entry, true, dtype, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal,
                       d_ref, n_ref, n_cols, periodic, d_step, step_bias, advance, d_prev_action, d_costs, stream);
}

extern "C" int mjmpc_cost_terms_rate_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                           const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                           int keep_builtin, int terminal, const double* d_ref, int64_t n_ref, int n_cols,
                                           int ref_per_episode, int periodic, const int64_t* d_step, int64_t step_bias,
                                           double* d_prev_actions, int advance_prev, void* d_costs, const double* d_gseq,
                                           double* d_q0, void* stream) {
    const char* const entry = "mjmpc_cost_terms_rate_batch";
    const char* const refusal = ct_first(
        {ct_not_null(d_next_obs && d_actions && d_terms && d_costs), ct_together(d_ref, d_step, "d_ref and d_step go together"),
         ct_sizes(E, P, H, d_obs, A, 1, d_actions, "needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 1"), ct_n_terms(n_terms),
         ct_dtype(dtype), ct_together(d_gseq, d_q0, "d_gseq and d_q0 go together"), ct_reference(d_ref, n_ref, n_cols),
         ct_advance(advance_prev, P, H, "advance_prev needs P = H = 1 (one workgroup per episode owns its previous action)")});
    if (refusal) return bad(entry, refusal);
    return launch_batch(entry, true, dtype, E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode,
                        keep_builtin, terminal, d_ref, n_ref, n_cols, ref_per_episode, periodic, d_step, step_bias,
                        d_prev_actions, advance_prev, d_costs, d_gseq, d_q0, stream);
}

extern "C" int mjmpc_cost_terms_quad(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                     const void* d_actions, const double* d_terms, int n_terms, int keep_builtin, int terminal,
                                     const double* d_ref, int64_t n_ref, int n_cols, int periodic, int64_t* d_step,
                                     int64_t step_bias, int advance, double* d_prev_action, const double* d_quad, int quad_len,
                                     void* d_costs, void* stream) {
    const char* const entry = "mjmpc_cost_terms_quad";
    const char* const refusal = ct_first(
        {ct_not_null(d_next_obs && d_actions && d_terms && d_costs), ct_together(d_ref, d_step, "d_ref and d_step go together"),
         ct_sizes(1, P, H, d_obs, A, 1, d_actions, "needs P >= 1, H >= 1, d_obs >= 1 and A >= 1"), ct_n_terms(n_terms),
         ct_dtype(dtype), ct_reference(d_ref, n_ref, n_cols), ct_pool(d_quad, quad_len),
         ct_advance(advance, P, H, "advance needs P = H = 1 (one workgroup owns the counter and the previous action)")});
    if (refusal) return bad(entry, refusal);
    return launch_flat(entry, true, dtype, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, keep_builtin, terminal,
                       d_ref, n_ref, n_cols, periodic, d_step, step_bias, advance, d_prev_action, d_costs, stream, d_quad,
                       quad_len);
}

extern "C" int mjmpc_cost_terms_quad_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                           const void* d_actions, const double* d_terms, int n_terms, int per_episode,
                                           int keep_builtin, int terminal, const double* d_ref, int64_t n_ref, int n_cols,
                                           int ref_per_episode, int periodic, const int64_t* d_step, int64_t step_bias,
                                           double* d_prev_actions, int advance_prev, const double* d_quad, int quad_len,
                                           void* d_costs, const double* d_gseq, double* d_q0, void* stream) {
    const char* const entry = "mjmpc_cost_terms_quad_batch";
    const char* const refusal = ct_first(
        {ct_not_null(d_next_obs && d_actions && d_terms && d_costs), ct_together(d_ref, d_step, "d_ref and d_step go together"),
         ct_sizes(E, P, H, d_obs, A, 1, d_actions, "needs E >= 1, P >= 1, H >= 1, d_obs >= 1 and A >= 1"), ct_n_terms(n_terms),
         ct_dtype(dtype), ct_together(d_gseq, d_q0, "d_gseq and d_q0 go together"), ct_reference(d_ref, n_ref, n_cols),
         ct_pool(d_quad, quad_len),
         ct_advance(advance_prev, P, H, "advance_prev needs P = H = 1 (one workgroup per episode owns its previous action)")});
    if (refusal) return bad(entry, refusal);
    return launch_batch(entry, true, dtype, E, P, H, d_obs, A, d_next_obs, d_actions, d_terms, n_terms, per_episode,
                        keep_builtin, terminal, d_ref, n_ref, n_cols, ref_per_episode, periodic, d_step, step_bias,
                        d_prev_actions, advance_prev, d_costs, d_gseq, d_q0, stream, d_quad, quad_len);
}
