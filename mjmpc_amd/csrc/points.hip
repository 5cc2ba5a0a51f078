// World positions of user-named points for the cost terms and, with MOTION, body axes and velocities beside them
// (DESIGN 12.5): a launch between a rollout and its cost launch that copies every observation row into an augmented row and
// appends, in double whatever the storage type, up to 16 outputs of three entries on any bodies and up to 16 differences of two
// outputs.  The cost kernels then read these entries as ordinary observation entries: nothing in cost_terms.hip or in a rollout
// translation unit changes.
//
// The program (float64 [n_rows + n_diff][16]; the row format: include/mjmpc_amd.h) is wave-uniform: every lane walks the same
// rows over its own qpos - one walk, pt_walk<T, MOTION>, for both entries.  A node row moves the frame as MuJoCo's
// mj_kinematics does, as the test oracle's kinematics() states it; a closing row writes an output.  The quaternions of qpos are
// used as stored - no normalised copy is written anywhere - and rotate as q / |q|, which is what the oracle's quat2mat does.
// Only the current frame (a position and a unit quaternion: 7 doubles) lives in registers; paths that share ancestors
// recompute them: no per-lane frame storage, no scratch.  Measured, the launch is bound by the nodes' arithmetic (2.5 - 4 us
// per node over 4096 x 32 rows, much of it the hinge's double-precision sincos), not by the bytes it moves:
// profiles/r25_points.txt.  The n_diff rows behind the walks are {5, a, b}: output a - output b, one double subtraction per
// component.
//
// The MOTION part (mjmpc_points_motion) carries, beside the frame, the world linear velocity v of the frame's origin and the
// world angular velocity w of the frame (6 more doubles), reads qvel - entries nq .. nq + nv of the row - at the dof address
// d_dofadr[k] of node row k, takes a closing row's slot and keep flag from the row and clears every slot first: one that no
// closing row names reads as 0.  Without it (mjmpc_points) a closing row is a point, the slots are the points in program order,
// every point closes its walk and nothing is cleared.  The kind branch is uniform, the dof addresses are wave-uniform reads
// like the rows.  Registers, LDS, scratch of the four instantiations: profiles/r27_points_one_walk.txt.
//
// The TREE part (mjmpc_points_tree) adds the centre of mass of a subtree and its velocity: a MASS row adds the
// current frame's group, weighted by its share of the subtree's mass, to two accumulators S and Sv (6 more doubles), SAVE and
// RESTORE rows put the frame with v and w away at a branch point and fetch it for the next child, so every body of the subtree
// is visited once, and the closing rows COM and COM_VELOCITY write S and Sv.  The saved frames live in LDS behind the parked
// outputs as doubles [level][component][lane] - 13 components, lane-consecutive like the outputs, 104 n_levels bytes a row -:
// a level is a run-time value, and a per-lane array indexed by one would go to scratch.  Every lane first writes the world
// frame at rest to its levels, so a RESTORE of a level never saved is defined.  Resources: profiles/r29_com_resources.txt.
//
// The ORIENT part (mjmpc_points_orient; with TREE) adds the orientation error of a body as three entries: the
// rotation vector Log(conj(a) * q_body * o) from a goal frame a - a constant world quaternion, or the frame a HOLD row took from
// an earlier path of the same walk, times a constant - to the body's frame.  The held quaternion h is 4 more doubles in
// registers; nothing more stands in LDS, so the tile is the tree entry's.  The log map is the header's, statement by statement.
// Resources: profiles/r30_orient_resources.txt.
//
// Shape (cost_terms.hip's): a workgroup takes `rows` consecutive observation rows - they lie back to back in memory -, copies
// them into LDS with unit-stride loads (odd row pitch: the lanes' column reads spread over the banks), lane j walks the program
// over row j and parks its outputs in LDS as doubles, laid out [entry][lane] (lane-consecutive, no bank conflict); then all
// lanes write the augmented tile, which is back to back in memory too, with unit stride: the observation's words as they came
// (bit for bit), the outputs rounded once to the storage type, the differences formed from the parked doubles and rounded once.
// Node rows are one address for all lanes, read const __restrict__ through the scalar cache; the joint-kind branch is uniform.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/mjmpc_amd.h"

namespace mjmpc {
int set_error(int code, const char* what, const char* detail);      // capi.hip: the message mjmpc_last_error() returns

namespace {

constexpr int PT_WG = 256;                  // threads of a workgroup and the most rows of its tile: one lane a row.  Tiles of 64
                                            // and 128 rows (as many threads) measured within 2 % of it: profiles/r25_points.txt
constexpr int PT_ROW = 16;                  // doubles of a program row
constexpr int PT_MAX_POINTS = 16, PT_MAX_DIFF = 16, PT_MAX_NODES = 33;
constexpr int PT_MAX_ROWS = PT_MAX_POINTS * (PT_MAX_NODES + 1);
constexpr int PT_LDS_BYTES = 60 * 1024;     // the tile's share of a workgroup's 64 KiB
constexpr int PT_MAX_LEVELS = 4;            // saved frames of a TREE program
constexpr int PT_LEVEL = 13;                // doubles of a saved frame: p, q, v, w

__host__ __device__ inline int pt_pitch(int n) { return n | 1; }

struct PtFrame {
    double p[3], q[4];      // origin in the world; orientation, a unit quaternion (w, x, y, z)
};

// v turned by the unit quaternion q: v + 2 w (u x v) + 2 u x (u x v)
__device__ __forceinline__ void pt_rotate(const double* q, double x, double y, double z, double* out) {
    const double tx = 2.0 * (q[2] * z - q[3] * y), ty = 2.0 * (q[3] * x - q[1] * z), tz = 2.0 * (q[1] * y - q[2] * x);
    out[0] = x + q[0] * tx + (q[2] * tz - q[3] * ty);
    out[1] = y + q[0] * ty + (q[3] * tx - q[1] * tz);
    out[2] = z + q[0] * tz + (q[1] * ty - q[2] * tx);
}

// q <- q * (w, x, y, z)
__device__ __forceinline__ void pt_mul(double* q, double w, double x, double y, double z) {
    const double a = q[0], b = q[1], c = q[2], d = q[3];
    q[0] = a * w - b * x - c * y - d * z;
    q[1] = a * x + b * w + c * z - d * y;
    q[2] = a * y - b * z + c * w + d * x;
    q[3] = a * z + b * y - c * x + d * w;
}

__device__ __forceinline__ void pt_cross(const double* a, const double* b, double* out) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// The rotation vector of the unit quaternion e (w, x, y, z), as include/mjmpc_amd.h states it: the half with w >= 0 is taken,
// s = |(x, y, z)|, and r = k (x, y, z) with k = 2 / w below s = 2^-26 (relative error s^2 / 3) and 2 atan2(s, w) / s from there
__device__ __forceinline__ void pt_log(const double* e, double* r) {
    const bool flip = e[0] < 0.0;
    const double w = flip ? -e[0] : e[0], x = flip ? -e[1] : e[1], y = flip ? -e[2] : e[2], z = flip ? -e[3] : e[3];
    const double s = sqrt(x * x + y * y + z * z);
    const double k = s < 0x1p-26 ? 2.0 / w : 2.0 * atan2(s, w) / s;
    r[0] = k * x; r[1] = k * y; r[2] = k * z;
}

// The output o of a closing row on the frame f: kind 0 POINT p + R off - without MOTION the only one - and, with v and w,
// 6 AXIS R a, 7 VELOCITY v + w x (R off), 8 ANGULAR w
template <bool MOTION>
__device__ __forceinline__ void pt_output(int kind, const PtFrame& f, const double* v, const double* w,
                                          const double* __restrict__ row, double* o) {
    if constexpr (MOTION) {
        if (kind == 8) {
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
            return;
        }
    }
    double t[3], c[3];
    pt_rotate(f.q, row[3], row[4], row[5], t);
    if (kind == 0) {
        o[0] = f.p[0] + t[0]; o[1] = f.p[1] + t[1]; o[2] = f.p[2] + t[2];
    } else if constexpr (MOTION) {
        if (kind == 7) {
            pt_cross(w, t, c);
            o[0] = v[0] + c[0]; o[1] = v[1] + c[1]; o[2] = v[2] + c[2];
        } else {
            o[0] = t[0]; o[1] = t[1]; o[2] = t[2];
        }
    }
}

// The walk over one row `my`: the frame and, with MOTION, its origin's velocity v and its angular velocity w; the outputs go
// to pts[(3 slot + c) * rows] (pts: this lane's column of the parked entries).  nv and dofadr are read with MOTION alone.
// TREE (with MOTION): the accumulators S and Sv of the MASS rows and the saved frames lv[(PT_LEVEL level + c) * rows] (lv:
// this lane's column of them), n_levels of them.  ORIENT (with TREE): the held quaternion h of the HOLD rows and the closing row
// ORIENTATION; in the other instantiations the kinds 14 and 15 are what they were.
template <typename T, bool MOTION, bool TREE, bool ORIENT>
__device__ __forceinline__ void pt_walk(const T* my, const double* __restrict__ prog, const int32_t* __restrict__ dofadr,
                                        int n_rows, int n_out, int nq, int nv, double* pts, int rows,
                                        [[maybe_unused]] double* lv, [[maybe_unused]] int n_levels) {
    static_assert(MOTION || !TREE, "the tree walk carries v and w");
    static_assert(TREE || !ORIENT, "the orientation walk is the tree walk's superset");
    // entry i of my qpos / qvel, held inside it whatever the tables say
    auto qpos = [&](int i) { return (double)my[i < 0 ? 0 : i < nq ? i : nq - 1]; };
    [[maybe_unused]] auto qvel = [&](int i) { return (double)my[nq + (i < 0 ? 0 : i < nv ? i : nv - 1)]; };
    if constexpr (MOTION)
        for (int e = 0; e < 3 * n_out; ++e) pts[e * rows] = 0.0;
    PtFrame f{{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0}};
    [[maybe_unused]] double v[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    [[maybe_unused]] double S[3] = {0.0, 0.0, 0.0}, Sv[3] = {0.0, 0.0, 0.0};
    [[maybe_unused]] double h[4] = {1.0, 0.0, 0.0, 0.0};       // ORIENT: the held quaternion, the identity until a HOLD row
    if constexpr (TREE) {                   // every level holds the world frame at rest until a SAVE says otherwise
        for (int l = 0; l < n_levels; ++l)
            for (int e = 0; e < PT_LEVEL; ++e) lv[(PT_LEVEL * l + e) * rows] = e == 3 ? 1.0 : 0.0;
    }
    int point = 0;                          // the closing rows so far: without MOTION a row's slot
    for (int k = 0; k < n_rows; ++k) {
        const double* __restrict__ row = prog + (long)PT_ROW * k;
        const int kind = (int)row[0];
        double t[3];
        [[maybe_unused]] double c[3];
        if constexpr (TREE) {
            if (kind == 9) {                // MASS: the group's centre c and its share of the subtree's mass; the frame is kept
                const double share = row[6];
                pt_rotate(f.q, row[3], row[4], row[5], t);
                pt_cross(w, t, c);
                S[0] += share * (f.p[0] + t[0]); S[1] += share * (f.p[1] + t[1]); S[2] += share * (f.p[2] + t[2]);
                Sv[0] += share * (v[0] + c[0]); Sv[1] += share * (v[1] + c[1]); Sv[2] += share * (v[2] + c[2]);
                continue;
            }
            if (kind == 10 || kind == 11) { // SAVE, RESTORE: the frame, v and w to and from a level; -1: the world frame at rest
                const int level = (int)row[1];
                const bool held = level >= 0 && level < n_levels;
                double* const at = lv + (long)PT_LEVEL * (held ? level : 0) * rows;
                if (kind == 10) {
                    if (held) {
                        for (int e = 0; e < 3; ++e) at[e * rows] = f.p[e];
                        for (int e = 0; e < 4; ++e) at[(3 + e) * rows] = f.q[e];
                        for (int e = 0; e < 3; ++e) at[(7 + e) * rows] = v[e];
                        for (int e = 0; e < 3; ++e) at[(10 + e) * rows] = w[e];
                    }
                } else if (held) {
                    for (int e = 0; e < 3; ++e) f.p[e] = at[e * rows];
                    for (int e = 0; e < 4; ++e) f.q[e] = at[(3 + e) * rows];
                    for (int e = 0; e < 3; ++e) v[e] = at[(7 + e) * rows];
                    for (int e = 0; e < 3; ++e) w[e] = at[(10 + e) * rows];
                } else {
                    f = PtFrame{{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0}};
                    v[0] = v[1] = v[2] = w[0] = w[1] = w[2] = 0.0;
                }
                continue;
            }
        }
        if constexpr (ORIENT) {
            if (kind == 14) {               // HOLD: the frame's orientation is put by; the next path starts at the world, at rest
                for (int e = 0; e < 4; ++e) h[e] = f.q[e];
                f = PtFrame{{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0}};
                v[0] = v[1] = v[2] = w[0] = w[1] = w[2] = 0.0;
                continue;
            }
        }
        // a closing row: its output into its slot; the frame kept or reset
        if (kind == 0 || (MOTION && !TREE && kind >= 6) || (TREE && ((kind >= 6 && kind <= 8) || kind >= 12))) {
            double o[3];
            if (ORIENT && kind == 15) {     // ORIENTATION: Log(conj(a) b), b = q o, a = g or h g
                double a[4] = {1.0, 0.0, 0.0, 0.0}, b[4] = {f.q[0], f.q[1], f.q[2], f.q[3]};
                if (row[11] != 0.0)
                    for (int e = 0; e < 4; ++e) a[e] = h[e];
                pt_mul(a, row[7], row[8], row[9], row[10]);
                pt_mul(b, row[3], row[4], row[5], row[6]);
                a[1] = -a[1]; a[2] = -a[2]; a[3] = -a[3];
                pt_mul(a, b[0], b[1], b[2], b[3]);
                pt_log(a, o);
            } else if (TREE && kind >= 12) {       // COM, COM_VELOCITY: the accumulators
                for (int e = 0; e < 3; ++e) o[e] = kind == 12 ? S[e] : Sv[e];
            } else {
                pt_output<MOTION>(kind, f, v, w, row, o);
            }
            const int slot = MOTION ? (int)row[2] : point;
            if (slot >= 0 && slot < n_out) {
                pts[(3 * slot + 0) * rows] = o[0];
                pts[(3 * slot + 1) * rows] = o[1];
                pts[(3 * slot + 2) * rows] = o[2];
            }
            ++point;
            if (!MOTION || row[1] == 0.0) {             // the next walk starts at the world frame, at rest
                f = PtFrame{{0.0, 0.0, 0.0}, {1.0, 0.0, 0.0, 0.0}};
                if constexpr (MOTION) v[0] = v[1] = v[2] = w[0] = w[1] = w[2] = 0.0;
                if constexpr (TREE) S[0] = S[1] = S[2] = Sv[0] = Sv[1] = Sv[2] = 0.0;
            }
            continue;
        }
        const int adr = (int)row[1];
        [[maybe_unused]] int dof = 0;
        if constexpr (MOTION) dof = dofadr[k];
        if (kind == 4) {                    // free: the frame is qpos' own, the linear rates the world's, the angular the body's
            const double qw = qpos(adr + 3), x = qpos(adr + 4), y = qpos(adr + 5), z = qpos(adr + 6);
            const double s = 1.0 / sqrt(qw * qw + x * x + y * y + z * z);
            f = PtFrame{{qpos(adr), qpos(adr + 1), qpos(adr + 2)}, {qw * s, x * s, y * s, z * s}};
            if constexpr (MOTION) {
                v[0] = qvel(dof); v[1] = qvel(dof + 1); v[2] = qvel(dof + 2);
                pt_rotate(f.q, qvel(dof + 3), qvel(dof + 4), qvel(dof + 5), w);
            }
            continue;
        }
        pt_rotate(f.q, row[3], row[4], row[5], t);
        if constexpr (MOTION) {
            pt_cross(w, t, c);
            v[0] += c[0]; v[1] += c[1]; v[2] += c[2];
        }
        f.p[0] += t[0]; f.p[1] += t[1]; f.p[2] += t[2];
        pt_mul(f.q, row[6], row[7], row[8], row[9]);
        if (kind == 2) {                    // slide: along the axis, no rotation
            const double d = qpos(adr) - row[2];
            pt_rotate(f.q, row[10], row[11], row[12], t);
            const double ad[3] = {t[0] * d, t[1] * d, t[2] * d};
            if constexpr (MOTION) {         // the displaced origin is carried round by w
                const double qd = qvel(dof);
                pt_cross(w, ad, c);
                v[0] += c[0] + t[0] * qd; v[1] += c[1] + t[1] * qd; v[2] += c[2] + t[2] * qd;
            }
            f.p[0] += ad[0]; f.p[1] += ad[1]; f.p[2] += ad[2];
            continue;
        }
        // hinge, ball: about the anchor, which stays where it is and moves as the frame before the joint moves it
        double anchor[3];
        pt_rotate(f.q, row[13], row[14], row[15], t);
        anchor[0] = f.p[0] + t[0]; anchor[1] = f.p[1] + t[1]; anchor[2] = f.p[2] + t[2];
        if constexpr (MOTION) {
            pt_cross(w, t, c);
            v[0] += c[0]; v[1] += c[1]; v[2] += c[2];              // (the anchor's velocity)
        }
        if (kind == 1) {
            const double half = 0.5 * (qpos(adr) - row[2]);
            double sn, cs;
            sincos(half, &sn, &cs);
            pt_mul(f.q, cs, row[10] * sn, row[11] * sn, row[12] * sn);
            if constexpr (MOTION) {
                const double qd = qvel(dof);
                pt_rotate(f.q, row[10], row[11], row[12], t);
                w[0] += t[0] * qd; w[1] += t[1] * qd; w[2] += t[2] * qd;
            }
        } else {
            const double qw = qpos(adr), x = qpos(adr + 1), y = qpos(adr + 2), z = qpos(adr + 3);
            const double s = 1.0 / sqrt(qw * qw + x * x + y * y + z * z);
            pt_mul(f.q, qw * s, x * s, y * s, z * s);
            if constexpr (MOTION) {
                pt_rotate(f.q, qvel(dof), qvel(dof + 1), qvel(dof + 2), t);
                w[0] += t[0]; w[1] += t[1]; w[2] += t[2];
            }
        }
        pt_rotate(f.q, row[13], row[14], row[15], t);
        f.p[0] = anchor[0] - t[0]; f.p[1] = anchor[1] - t[1]; f.p[2] = anchor[2] - t[2];
        if constexpr (MOTION) {
            pt_cross(w, t, c);
            v[0] -= c[0]; v[1] -= c[1]; v[2] -= c[2];
        }
    }
}

// grid: ceil(n / rows) workgroups of max(rows, 64) threads; dynamic LDS: rows x pitch(d_obs) words of T, then 3 n_points x rows doubles
// MOTION: n_points counts the output slots; nv and dofadr are read by that instantiation alone
// TREE: behind the parked outputs PT_LEVEL n_levels x rows doubles, the saved frames; n_levels is read by that instantiation alone
template <typename T, bool MOTION, bool TREE, bool ORIENT>
__global__ __launch_bounds__(PT_WG) void points_kernel(const T* __restrict__ obs, const double* __restrict__ prog, int n_rows,
                                                       int n_points, int n_diff, long n, int d_obs, int nq, int rows,
                                                       T* __restrict__ out, int nv, const int32_t* __restrict__ dofadr,
                                                       int n_levels) {
    extern __shared__ double pt_tile_raw[];
    __shared__ int s_da[PT_MAX_DIFF], s_db[PT_MAX_DIFF];
    const int po = pt_pitch(d_obs);
    T* const tile = reinterpret_cast<T*>(pt_tile_raw);
    double* const pts = pt_tile_raw + ((long)rows * po * sizeof(T) + 7) / 8;
    const long e0 = (long)blockIdx.x * rows;
    const int mine = n - e0 < rows ? (int)(n - e0) : rows;
    const int j = threadIdx.x, wg = blockDim.x;

    if (j < n_diff) {                       // a difference's two points, held below n_points whatever the table says
        const double* row = prog + (long)PT_ROW * (n_rows + j);
        const int a = (int)row[1], b = (int)row[2];
        s_da[j] = a < 0 ? 0 : a < n_points ? a : n_points - 1;
        s_db[j] = b < 0 ? 0 : b < n_points ? b : n_points - 1;
    }
    {                                       // the tile: unit stride over the lanes
        const T* __restrict__ src = obs + e0 * d_obs;
        const int total = mine * d_obs;
        int i = j, r = i / d_obs, c = i - r * d_obs;
        const int dr = wg / d_obs, dc = wg - dr * d_obs;
        for (; i < total; i += wg) {
            tile[r * po + c] = src[i];
            r += dr;
            c += dc;
            if (c >= d_obs) { c -= d_obs; ++r; }
        }
    }
    __syncthreads();

    if (j < mine)
        pt_walk<T, MOTION, TREE, ORIENT>(tile + j * po, prog, dofadr, n_rows, n_points, nq, nv, pts + j, rows,
                                 pts + (long)3 * n_points * rows + j, n_levels);
    __syncthreads();

    {                                       // the augmented tile: unit stride over the lanes
        const int d_pts = 3 * n_points, d_aug = d_obs + d_pts + 3 * n_diff;
        T* __restrict__ dst = out + e0 * d_aug;
        const long total = (long)mine * d_aug;
        int r = j / d_aug, c = j - r * d_aug;
        const int dr = wg / d_aug, dc = wg - dr * d_aug;
        for (long i = j; i < total; i += wg) {
            T v;
            if (c < d_obs) {
                v = tile[r * po + c];
            } else if (c < d_obs + d_pts) {
                v = (T)pts[(c - d_obs) * rows + r];
            } else {
                const int m = c - d_obs - d_pts, d = m / 3, ax = m - 3 * d;
                v = (T)(pts[(3 * s_da[d] + ax) * rows + r] - pts[(3 * s_db[d] + ax) * rows + r]);
            }
            dst[i] = v;
            r += dr;
            c += dc;
            if (c >= d_aug) { c -= d_aug; ++r; }
        }
    }
}

// The four entries: the checks, the tile - the largest power of two of rows up to PT_WG whose rows, parked outputs and saved
// frames fit PT_LDS_BYTES - and the launch.  `motion`: mjmpc_points_motion and mjmpc_points_tree, which alone read (and check)
// nv and dofadr and call their outputs n_out where mjmpc_points says n_points; `tree`: mjmpc_points_tree, which alone reads
// (and checks) n_levels; `orient`: mjmpc_points_orient, the tree entry with the rows HOLD and ORIENTATION.
int launch_points(const char* entry, bool motion, bool tree, bool orient, int dtype, int64_t N, int d_obs, int nq, int nv, const void* obs,
                  const double* prog, const int32_t* dofadr, int n_rows, int n_out, int n_diff, int n_levels, void* out,
                  void* stream) {
    auto bad = [&](const char* detail) { return set_error(MJMPC_E_BADARG, entry, detail); };
    if (!obs || !prog || !out) return bad("null pointer");
    if (motion && !dofadr) return bad("null d_dofadr: the node rows' qvel addresses");
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return bad("unknown dtype");
    if (N < 1 || d_obs < 1) return bad("N and d_obs must be >= 1");
    if (nq < 1 || nq > d_obs) return bad("nq must be in 1 .. d_obs: qpos opens the observation");
    if (motion && (nv < 1 || (long)nq + nv > d_obs)) return bad("nv must be >= 1 and nq + nv <= d_obs: qvel follows qpos");
    if (n_out < 1 || n_out > PT_MAX_POINTS) return bad(motion ? "n_out must be in 1 .. 16" : "n_points must be in 1 .. 16");
    if (n_diff < 0 || n_diff > PT_MAX_DIFF) return bad("n_diff must be in 0 .. 16");
    if (n_rows < n_out || n_rows > PT_MAX_ROWS)
        return bad(motion ? "n_rows must be in n_out .. 544 (16 paths of 33 nodes and an output)"
                          : "n_rows must be in n_points .. 544 (16 paths of 33 nodes and a point)");
    if (tree && (n_levels < 0 || n_levels > PT_MAX_LEVELS)) return bad("n_levels must be in 0 .. 4");
    const long word = dtype == MJMPC_F32 ? 4 : 8;
    const long pts_bytes = 8L * 3 * n_out + (tree ? 8L * PT_LEVEL * n_levels : 0);     // a row's parked outputs and saved frames
    if ((long)d_obs > (PT_LDS_BYTES - pts_bytes - 8) / word - 1)
        return bad(tree ? "an observation row, its outputs and its saved frames of more than 60 KiB"
                   : motion ? "an observation row and its outputs of more than 60 KiB"
                            : "an observation row and its points of more than 60 KiB");
    auto lds = [&](int r) { return (r * word * pt_pitch(d_obs) + 7) / 8 * 8 + r * pts_bytes; };
    int rows = PT_WG;
    while (lds(rows) > PT_LDS_BYTES) rows >>= 1;
    const long blocks = ((long)N + rows - 1) / rows;
    if (blocks > INT32_MAX) return bad("more than 2^31 workgroups");
    auto launch = [&](auto zero) {
        using T = decltype(zero);
        auto* const kernel = orient   ? points_kernel<T, true, true, true>
                             : tree   ? points_kernel<T, true, true, false>
                             : motion ? points_kernel<T, true, false, false>
                                      : points_kernel<T, false, false, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(rows < 64 ? 64 : rows), (size_t)lds(rows), (hipStream_t)stream,
                           (const T*)obs, prog, n_rows, n_out, n_diff, (long)N, d_obs, nq, rows, (T*)out, nv, dofadr, n_levels);
    };
    if (dtype == MJMPC_F32) launch(0.0f);
    else launch(0.0);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : set_error((int)e, entry, hipGetErrorString(e));
}

}  // namespace
}  // namespace mjmpc

extern "C" int mjmpc_points(int dtype, int64_t N, int d_obs, int nq, const void* d_obs_rows, const double* d_program, int n_rows,
                            int n_points, int n_diff, void* d_out, void* stream) {
    return mjmpc::launch_points("mjmpc_points", false, false, false, dtype, N, d_obs, nq, 0, d_obs_rows, d_program, nullptr, n_rows,
                                n_points, n_diff, 0, d_out, stream);
}

extern "C" int mjmpc_points_motion(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                                   const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, void* d_out, void* stream) {
    return mjmpc::launch_points("mjmpc_points_motion", true, false, false, dtype, N, d_obs, nq, nv, d_obs_rows, d_program, d_dofadr,
                                n_rows, n_out, n_diff, 0, d_out, stream);
}

extern "C" int mjmpc_points_tree(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                                 const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, int n_levels, void* d_out,
                                 void* stream) {
    return mjmpc::launch_points("mjmpc_points_tree", true, true, false, dtype, N, d_obs, nq, nv, d_obs_rows, d_program, d_dofadr,
                                n_rows, n_out, n_diff, n_levels, d_out, stream);
}

extern "C" int mjmpc_points_orient(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                                   const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, int n_levels, void* d_out,
                                   void* stream) {
    return mjmpc::launch_points("mjmpc_points_orient", true, true, true, dtype, N, d_obs, nq, nv, d_obs_rows, d_program, d_dofadr,
                                n_rows, n_out, n_diff, n_levels, d_out, stream);
}
