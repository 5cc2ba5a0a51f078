// extern "C" entry points declared in include/mjmpc_amd.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/mjmpc_amd.h"
#include "arm_model.h"
#include "analytic_rollout.h"
#include "arm_rollout.h"
#include "noise_mt.h"
#include "tree_model.h"
#include "tree_rollout.h"
#include "update.h"

// failure counter (one unsigned) followed by the phase-clock slots of developer builds (arm_rollout.hip, Stamps)
constexpr size_t MJMPC_DIAG_BYTES = 8 * (2 + 64);      // counters, then the developer clocks of -DMJMPC_STAMPS builds (4 waves x 16)

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace
namespace mjmpc {
// (comm.hip reports through the same thread-local message as the entry points of this file)
int set_error(int code, const char* what, const char* detail) { return fail(code, "%s: %s", what, detail); }
}  // namespace mjmpc
namespace {

int hip_fail(hipError_t e, const char* what) {
    return fail((int)e, "%s: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                \
    do {                                             \
        hipError_t e_ = (expr);                      \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

}  // namespace

// The element type of a launch from the ABI's dtype code: f(float()) or f(double()) issues the launch(es) and returns
// their hipError_t, `what` names them in the error message.
template <typename F>
static int with_dtype(int dtype, const char* what, F&& f) {
    hipError_t e;
    if (dtype == MJMPC_F32) e = f(float());
    else if (dtype == MJMPC_F64) e = f(double());
    else return fail(MJMPC_E_BADARG, "unknown dtype %d", dtype);
    if (e != hipSuccess) return hip_fail(e, what);
    return 0;
}

/* ---- the engine core: what the arm and the tree engine are on the host, once ------------------------------------------ */
struct engine_core {
    int device = 0;
    int nv = 0, nu = 0, d_obs = 0;
    float* model_f32 = nullptr;
    double* model_f64 = nullptr;
    double* state = nullptr;        // MJMPC_ARM_STATE_LEN / MJMPC_TREE_DEVICE_STATE_LEN
    unsigned* diag = nullptr;
    double* pinned = nullptr;       // host staging for set_state: a ring of 4 state vectors, one event each
    hipEvent_t staged[4] = {nullptr, nullptr, nullptr, nullptr};
    int stage_next = 0;
    int n_shards = 1;               // > 1: model_f32 / model_f64 hold one block per shard
    double* shard_states = nullptr; // n_state_shards state vectors (per-shard start states)
    int n_state_shards = 0;
    double* reset_rec = nullptr;    // n_shards records: MuJoCo's reset on instability (RolloutFusion / TreeFusion::reset_rec)
    int inf_on_reset = 0;           // mjmpc_*_set_reset_returns
    std::vector<double*> reset_retired;     // reset records that were replaced: bound launchers / captured graphs carry the
                                            // pointer by value (RolloutFusion, MonoStep), so they stay allocated until destroy
};

template <typename T>
static const T* model(const engine_core* h) {
    if constexpr (std::is_same<T, float>::value) return h->model_f32;
    else return h->model_f64;
}

// create: the device and pinned memory every engine owns, and the upload of its one model block
static int core_create(engine_core* h, const double* blob, int n_blob, size_t state_len, size_t diag_bytes) {
    std::vector<float> f32(blob, blob + n_blob);
    HIP_TRY(hipMalloc(&h->model_f32, sizeof(float) * n_blob));
    HIP_TRY(hipMalloc(&h->model_f64, sizeof(double) * n_blob));
    HIP_TRY(hipMalloc(&h->state, sizeof(double) * state_len));
    HIP_TRY(hipMalloc(&h->diag, diag_bytes));
    HIP_TRY(hipHostMalloc(&h->pinned, sizeof(double) * state_len * 4));
    for (int k = 0; k < 4; ++k) HIP_TRY(hipEventCreateWithFlags(&h->staged[k], hipEventDisableTiming));
    HIP_TRY(hipMemcpy(h->model_f32, f32.data(), sizeof(float) * n_blob, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->model_f64, blob, sizeof(double) * n_blob, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(h->state, 0, sizeof(double) * state_len));
    HIP_TRY(hipMemset(h->diag, 0, diag_bytes));
    return 0;
}

// destroy (also of a half-created engine: everything that is not there yet is null)
static void core_free(engine_core* h) {
    hipSetDevice(h->device);
    hipFree(h->model_f32);
    hipFree(h->model_f64);
    hipFree(h->state);
    hipFree(h->diag);
    hipFree(h->shard_states);
    hipFree(h->reset_rec);
    for (double* p : h->reset_retired) hipFree(p);
    if (h->pinned) hipHostFree(h->pinned);
    for (int k = 0; k < 4; ++k) if (h->staged[k]) hipEventDestroy(h->staged[k]);
}

static int core_dims(const engine_core* h, int* nv, int* nu, int* d_obs) {
    if (!h) return fail(MJMPC_E_BADARG, "null engine");
    if (nv) *nv = h->nv;
    if (nu) *nu = h->nu;
    if (d_obs) *d_obs = h->d_obs;
    return 0;
}

// set_state: pack(stage) writes the state vector into a pinned slot, which is copied to the device on `s`.
// Staging ring: wait only for the copy that last used THIS slot (four calls ago), never for the stream - a
// captured control iteration still running on `s` keeps running while the next state is being staged.
template <typename Pack>
static int core_set_state(engine_core* h, size_t state_len, hipStream_t s, Pack&& pack) {
    HIP_TRY(hipSetDevice(h->device));
    const int slot = h->stage_next;
    h->stage_next = (slot + 1) & 3;
    HIP_TRY(hipEventSynchronize(h->staged[slot]));
    double* stage = h->pinned + (size_t)slot * state_len;
    pack(stage);
    HIP_TRY(hipMemcpyAsync(h->state, stage, sizeof(double) * state_len, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->staged[slot], s));
    return 0;
}

// set_shard_models: n_shards validated blocks (host, blob_len each) replace the engine's.  make_records(&rec) builds the
// reset records of the NEW blocks before anything is committed: if that (or an allocation, or a copy) fails the engine
// keeps its old models, shard count and records.
template <typename MakeRecords>
static int core_swap_models(engine_core* h, const double* blobs, int n_shards, size_t blob_len, MakeRecords&& make_records) {
    const size_t n = (size_t)n_shards * blob_len;
    std::vector<float> f32(blobs, blobs + n);
    HIP_TRY(hipDeviceSynchronize());
    float* m32 = nullptr;
    double* m64 = nullptr;
    HIP_TRY(hipMalloc(&m32, sizeof(float) * n));
    if (hipError_t e = hipMalloc(&m64, sizeof(double) * n); e != hipSuccess) {
        hipFree(m32);
        return hip_fail(e, "hipMalloc");
    }
    hipError_t e = hipMemcpy(m32, f32.data(), sizeof(float) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m64, blobs, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(m32);
        hipFree(m64);
        return hip_fail(e, "hipMemcpy");
    }
    double* rec = nullptr;
    if (int rc = make_records(&rec); rc != 0) {
        hipFree(m32);
        hipFree(m64);
        return rc;
    }
    hipFree(h->model_f32);
    hipFree(h->model_f64);
    h->model_f32 = m32;
    h->model_f64 = m64;
    h->n_shards = n_shards;
    if (h->reset_rec) h->reset_retired.push_back(h->reset_rec);     // (launchers bound earlier still point at it)
    h->reset_rec = rec;
    return 0;
}

// set_shard_states: room for n_shards state vectors (0: none)
static int core_resize_shard_states(engine_core* h, int n_shards, size_t state_len) {
    if (n_shards == h->n_state_shards) return 0;
    HIP_TRY(hipDeviceSynchronize());
    hipFree(h->shard_states);
    h->shard_states = nullptr;
    h->n_state_shards = 0;
    if (n_shards > 0) HIP_TRY(hipMalloc(&h->shard_states, sizeof(double) * state_len * n_shards));
    h->n_state_shards = n_shards;
    return 0;
}

// (`host` is pageable memory: the call returns when the copy has been made)
static int core_upload_shard_states(engine_core* h, const double* host, size_t n_doubles, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(h->shard_states, host, sizeof(double) * n_doubles, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

static int read_counter(const engine_core* h, int index, uint32_t* count) {
    if (!h || !count) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());
    unsigned c = 0;
    HIP_TRY(hipMemcpy(&c, h->diag + index, sizeof(unsigned), hipMemcpyDeviceToHost));
    *count = c;
    return 0;
}

static int set_reset_returns(engine_core* h, int inf_returns) {
    if (!h) return fail(MJMPC_E_BADARG, "null argument");
    h->inf_on_reset = inf_returns ? 1 : 0;
    return 0;
}

/* ---- arm engine: what it adds to the core ------------------------------------------------------------------------------ */
struct mjmpc_arm_s : engine_core {
    bool xj = false;                // slide joints / friction loss: launches go to the extended-joint build (arm_blob_is_xj)
    // mjmpc_arm_mppi_step: the rollout workgroups' records.  The pointer travels to the kernels BY VALUE (MonoStep), so a
    // captured graph holds it: the buffer only ever GROWS, and a buffer it outgrew stays allocated until the handle is
    // destroyed (mono_retired) - a graph captured at one (P, H) survives later calls at another
    double* mono_tree = nullptr;
    size_t mono_cap = 0;            // doubles
    std::vector<double*> mono_retired;
};
constexpr int ARM_DIAG_ENV_RESETS = 2;      // (diag: [0] solver failures, [1] resets, [2] resets of the real env)

// which build of the arm kernels an engine's launches go to: the extended-joint one (arm_rollout_xj.hip) when some block of its
// model has a slide joint or a dof with friction loss
static bool arm_blob_is_xj(const double* blobs, int n_shards) {
    for (int s = 0; s < n_shards; ++s)
        for (int l = 0; l < mjmpc::LANES; ++l) {
            const double* b = blobs + (size_t)s * mjmpc::ARM_BLOB_LEN;
            if (b[mjmpc::O_JTYPE + l] != 0.0 || b[mjmpc::O_FLOSS + l] > 0.0) return true;
        }
    return false;
}
template <typename T, typename... A>
static hipError_t arm_rollout_launch(const mjmpc_arm_s* h, A&&... a) {
    return h->xj ? mjmpc::launch_arm_rollout_xj<T>(a...) : mjmpc::launch_arm_rollout<T>(a...);
}
template <typename T, typename... A>
static hipError_t arm_finish_launch(const mjmpc_arm_s* h, A&&... a) {
    return h->xj ? mjmpc::launch_arm_mppi_finish_xj<T>(a...) : mjmpc::launch_arm_mppi_finish<T>(a...);
}

static mjmpc::RolloutFusion arm_fuse(const mjmpc_arm_s* h) {
    mjmpc::RolloutFusion f;
    f.reset_rec = h->reset_rec;
    f.inf_on_reset = h->inf_on_reset;
    return f;
}

// The reset records of `n_shards` model blocks (host, ARM_BLOB_LEN each): per block ONE substep of the f64 kernel itself
// from the reset state (qpos0 = 0, zero velocity, zero controls) on a copy of the block with frame_skip 1 - state_out
// receives the state after it, the next observation's site entries are the site at the reset state.  Synchronous; called
// when the engine is created and when its model blocks are replaced.
// The records are returned in *out and the handle is NOT touched: the caller commits them together with the model blocks
// (core_swap_models), so that a failure here leaves the engine as it was; the launches count into a scratch
// counter block of their own, not into the engine's live diagnostics.
static int arm_make_reset_records(mjmpc_arm_s* h, const double* blobs, int n_shards, double** out) {
    const size_t L = (size_t)mjmpc::ARM_BLOB_LEN, R = (size_t)mjmpc::ARM_RESET_LEN;
    const int dobs = 2 * h->nv + 6;
    double *rec = nullptr, *tmp = nullptr;
    HIP_TRY(hipMalloc(&rec, sizeof(double) * R * n_shards));
    // scratch: model block | state (19) | mean (8) | cost (1) | next observation (dobs) | counters (MJMPC_DIAG_BYTES)
    const size_t nscr = L + MJMPC_ARM_STATE_LEN + 8 + 1 + dobs + MJMPC_DIAG_BYTES / sizeof(double) + 1;
    hipError_t e = hipMalloc(&tmp, sizeof(double) * nscr);
    if (e == hipSuccess) e = hipMemset(tmp, 0, sizeof(double) * nscr);
    if (e == hipSuccess) e = hipMemset(rec, 0, sizeof(double) * R * n_shards);
    std::vector<double> b(L);
    double *st = tmp + L, *mean = st + MJMPC_ARM_STATE_LEN, *cost = mean + 8, *nobs = cost + 1;
    unsigned* sdiag = (unsigned*)(nobs + dobs);
    for (int k = 0; k < n_shards && e == hipSuccess; ++k) {
        std::memcpy(b.data(), blobs + (size_t)k * L, sizeof(double) * L);
        b[mjmpc::O_FRAME_SKIP] = 1.0;
        e = hipMemcpy(tmp, b.data(), sizeof(double) * L, hipMemcpyHostToDevice);
        if (e != hipSuccess) break;
        double* rk = rec + (size_t)k * R;
        e = arm_rollout_launch<double>(h, tmp, st, 1, 1, h->nu, mean, nullptr, cost, nullptr, nullptr, nobs, rk, sdiag, nullptr);
        if (e == hipSuccess) e = hipMemcpy(rk + 2 * mjmpc::LANES, nobs + 2 * h->nv, sizeof(double) * 3, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) break;
        double host[mjmpc::ARM_RESET_LEN];          // sin / cos of the record's qpos (the kernels carry them beside q)
        e = hipMemcpy(host, rk, sizeof(double) * 19, hipMemcpyDeviceToHost);
        for (int l = 0; l < mjmpc::LANES; ++l) {
            const bool slide = b[mjmpc::O_JTYPE + l] != 0.0;     // (a slide joint's coordinate is a length: the kernels keep (0, 1))
            host[19 + l] = slide ? 0.0 : std::sin(host[l]);
            host[19 + mjmpc::LANES + l] = slide ? 1.0 : std::cos(host[l]);
        }
        if (e == hipSuccess) e = hipMemcpy(rk + 19, host + 19, sizeof(double) * 16, hipMemcpyHostToDevice);
    }
    hipFree(tmp);
    if (e != hipSuccess) {
        hipFree(rec);
        return hip_fail(e, "reset record");
    }
    *out = rec;
    return 0;
}

static int shard_fusion(const mjmpc_arm_s* h, int64_t P, mjmpc::RolloutFusion& fuse) {
    if (h->n_state_shards > 1) {
        if (P % h->n_state_shards != 0 || (P / h->n_state_shards) % mjmpc::LANES != 0)
            return fail(MJMPC_E_BADARG, "with per-shard start states P / n_shards must be a multiple of 8");
        fuse.state_shard_size = (long)(P / h->n_state_shards);
    }
    if (h->n_shards <= 1) return 0;
    if (P % h->n_shards != 0) return fail(MJMPC_E_BADARG, "P = %lld is not divisible by %d shards", (long long)P, h->n_shards);
    const long ss = (long)(P / h->n_shards);
    if (ss % mjmpc::LANES != 0) return fail(MJMPC_E_BADARG, "with per-shard models a shard must hold a multiple of 8 particles (got %ld)", ss);
    fuse.shard_size = ss;
    return 0;
}

// what mjmpc_arm_rollout / _rollout_cl / _rollout_fused do between their null checks and their launch: the sizes, the device,
// the engine's fusion with its shard arithmetic, and the start state(s) the launch reads
static int arm_rollout_begin(const mjmpc_arm_s* h, int64_t P, int H, mjmpc::RolloutFusion* fuse, const double** st) {
    if (P < 0 || H < 0) return fail(MJMPC_E_BADARG, "negative size");
    HIP_TRY(hipSetDevice(h->device));
    *fuse = arm_fuse(h);
    if (int rc = shard_fusion(h, P, *fuse)) return rc;
    *st = fuse->state_shard_size > 0 ? h->shard_states : h->state;
    return 0;
}

// room for the records of a fused iteration / a sampled rollout at (P, H): grow only, never under a capture (an allocation
// would invalidate it), and never free what an earlier graph may still point at
static int arm_grow_mono(mjmpc_arm_s* h, size_t need, hipStream_t s) {
    if (need <= h->mono_cap) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(MJMPC_E_BADARG, "the record buffer must grow for this (P, H): call once outside stream capture first");
    double* bigger = nullptr;
    HIP_TRY(hipMalloc(&bigger, sizeof(double) * need));
    if (h->mono_tree) h->mono_retired.push_back(h->mono_tree);
    h->mono_tree = bigger;
    h->mono_cap = need;
    return 0;
}

/* ---- tree engine: what it adds to the core ----------------------------------------------------------------------------- */
static_assert(MJMPC_TREE_BLOB_LEN == mjmpc::TREE_BLOB_LEN && MJMPC_TREE_DEVICE_STATE_LEN == mjmpc::TREE_STATE_LEN &&
              MJMPC_TREE_STATE_LEN == mjmpc::TREE_PUBLIC_STATE_LEN, "include/mjmpc_amd.h and csrc/tree_model.h disagree");
#define MJMPC_TREE_DIAG_BYTES (8 + 8 * mjmpc::TREE_STAT_SLOTS + 8)  /* counters, the developer clocks of -DTREE_STATS builds, the real env's resets (TREE_DIAG_ENV_RESETS) */

struct mjmpc_tree_s : engine_core {
    int max_path = 0, nq = 0;
    bool full = false;              // slide joints, springs, friction cones, > 8 contact points or a medium: the full kernel
    int gen = 0;                    // T_GEN: 1 ball / free joints, friction loss, boxes, equalities, tendon limits (the general
                                    // instantiation), 2 round 5's record kinds on top (instantiations of their own)
    std::vector<double> topo;       // create-time topology tables (shard blocks must match them)
    int integrator = MJMPC_INTEGRATOR_EULER;    // mjmpc_tree_create_ex: every launch (the reset records' too) steps with it
    double* zero_action = nullptr;  // [32] zeros (the kinematics-only launch of mjmpc_tree_rollout_cl)
    double* scratch = nullptr;      // [8] a place for that launch's cost
    // mjmpc_tree_set_batch_models: batch_sets * batch_k model blocks for the episode batches' rollouts, apart from the engine's
    // own (which keep stepping the batch's real envs), with their reset records and their kernel choice
    float* batch_f32 = nullptr;
    double* batch_f64 = nullptr;
    double* batch_rec = nullptr;
    int batch_sets = 0, batch_k = 0;
    bool batch_full = false;
    // mjmpc_tree_set_env_model: the block the device-resident real env steps with instead of shard 0's (null: shard 0's)
    float* env_f32 = nullptr;
    double* env_f64 = nullptr;
    double* env_rec = nullptr;
    bool env_full = false;
    std::vector<void*> env_retired; // replaced env blocks / records: a captured env step carries the pointers by value
};

// MuJoCo's layout (qpos[nq], qvel[nv], target[3]) -> the device state vector: one coordinate per LINK, a ball joint's
// quaternion as x, y, z in its three links' entries and w in its first link's w entry, a free joint's translations relative
// to the body position (the links are slides from there)
static void tree_pack_state(const mjmpc_tree_s* h, const double* qpos, const double* qvel, const double* target, double* st) {
    std::memset(st, 0, sizeof(double) * MJMPC_TREE_DEVICE_STATE_LEN);
    const double* b = h->topo.data();
    for (int l = 0; l < h->nv; ++l) {
        const int kind = (int)b[mjmpc::T_JTYPE + l], adr = (int)b[mjmpc::T_QADR + l];
        st[mjmpc::TREE_QW + l] = 1.0;
        if (kind == mjmpc::LINK_BALL_X) {
            // the device quaternion is relative to the qpos0 pose: q_link = conj(q0) * qpos (a free joint's qpos is absolute)
            const double w0 = b[mjmpc::T_QW0 + l], x0 = -b[mjmpc::T_QOFF + l], y0 = -b[mjmpc::T_QOFF + l + 1], z0 = -b[mjmpc::T_QOFF + l + 2];
            const double w = qpos[adr], x = qpos[adr + 1], y = qpos[adr + 2], z = qpos[adr + 3];
            st[mjmpc::TREE_QW + l] = w0 * w - x0 * x - y0 * y - z0 * z;
            st[l] = w0 * x + x0 * w + y0 * z - z0 * y;
            st[l + 1] = w0 * y - x0 * z + y0 * w + z0 * x;
            st[l + 2] = w0 * z + x0 * y - y0 * x + z0 * w;
        } else if (kind <= mjmpc::LINK_SLIDE) {
            st[l] = qpos[adr] - b[mjmpc::T_QOFF + l];
        }
        st[mjmpc::TL + l] = qvel[l];
    }
    std::memcpy(st + 2 * mjmpc::TL, target, sizeof(double) * 3);
}
static void tree_unpack_state(const mjmpc_tree_s* h, const double* st, double* qpos, double* qvel) {
    const double* b = h->topo.data();
    for (int l = 0; l < h->nv; ++l) {
        const int kind = (int)b[mjmpc::T_JTYPE + l], adr = (int)b[mjmpc::T_QADR + l];
        if (kind == mjmpc::LINK_BALL_X) {          // qpos = q0 * q_link
            const double w0 = b[mjmpc::T_QW0 + l], x0 = b[mjmpc::T_QOFF + l], y0 = b[mjmpc::T_QOFF + l + 1], z0 = b[mjmpc::T_QOFF + l + 2];
            const double w = st[mjmpc::TREE_QW + l], x = st[l], y = st[l + 1], z = st[l + 2];
            qpos[adr] = w0 * w - x0 * x - y0 * y - z0 * z;
            qpos[adr + 1] = w0 * x + x0 * w + y0 * z - z0 * y;
            qpos[adr + 2] = w0 * y - x0 * z + y0 * w + z0 * x;
            qpos[adr + 3] = w0 * z + x0 * y - y0 * x + z0 * w;
        } else if (kind <= mjmpc::LINK_SLIDE) {
            qpos[adr] = st[l] + b[mjmpc::T_QOFF + l];
        }
        qvel[l] = st[mjmpc::TL + l];
    }
}

static bool tree_blob_is_full(const double* blob, int nv) {
    bool full = blob[mjmpc::T_ANY_FRICTION] != 0.0 || (int)blob[mjmpc::T_N_SPHERE] > 8 || blob[mjmpc::T_DENSITY] > 0.0 ||
                blob[mjmpc::T_VISCOSITY] > 0.0 || blob[mjmpc::T_GEN] != 0.0;
    for (int l = 0; l < nv; ++l) full = full || (int)blob[mjmpc::T_JTYPE + l] == 2 || blob[mjmpc::T_STIFFNESS + l] != 0.0;
    return full;
}

// the tables a shard block must share with the engine's create-time block: they fix the kernel instantiation, the
// launch shape and the factorisation schedule (dynamics randomization edits masses, inertias, damping, contact radii and
// friction - never the tree)
static bool tree_same_topology(const double* a, const double* b) {
    auto same = [&](int off, int n) { return std::memcmp(a + off, b + off, sizeof(double) * n) == 0; };
    return same(mjmpc::T_PARENT, mjmpc::TL) && same(mjmpc::T_EPARENT, mjmpc::TL) && same(mjmpc::T_SUBSIZE, mjmpc::TL) && same(mjmpc::T_ANC, 5 * mjmpc::TL) &&
           same(mjmpc::T_JTYPE, mjmpc::TL) && same(mjmpc::T_ACT, mjmpc::TL) && same(mjmpc::T_DEPTH, mjmpc::TL) &&
           same(mjmpc::T_N_ROUNDS, 1) && same(mjmpc::T_ELIM, (mjmpc::TL - 1) * mjmpc::TL) && same(mjmpc::T_NV, 1) &&
           same(mjmpc::T_NU, 1) && same(mjmpc::T_TASK, 1) && same(mjmpc::T_OBS_SKIP, 1) && same(mjmpc::T_JUMPS, 1) &&
           same(mjmpc::T_NQ, 1) && same(mjmpc::T_QADR, mjmpc::TL) && same(mjmpc::T_HAS_BALL, 1) && same(mjmpc::T_QW0, mjmpc::TL);
}

// what a set of model blocks must pass before it replaces or joins the engine's (mjmpc_tree_set_shard_models, _set_batch_models,
// _set_env_model): the engine's topology and dimensions, its kernel instantiation; *full = the kernel choice of the set
static int tree_check_blocks(const mjmpc_tree_s* h, const double* blobs, int n, bool* full, const char* what) {
    *full = false;
    for (int s = 0; s < n; ++s) {
        const double* b = blobs + (size_t)s * mjmpc::TREE_BLOB_LEN;
        if ((int)b[mjmpc::T_N_SPHERE] > mjmpc::TREE_MAX_SPHERES || !tree_same_topology(b, h->topo.data()))
            return fail(MJMPC_E_BADMODEL, "%s %d does not have the engine's topology / dimensions", what, s);
        *full = *full || tree_blob_is_full(b, h->nv);
        if ((int)b[mjmpc::T_GEN] != h->gen)
            return fail(MJMPC_E_BADMODEL, "%s %d needs a different kernel instantiation than the engine's model", what, s);
    }
    return 0;
}

// n model blocks (host) -> device copies in both precisions
static int tree_upload_blocks(const double* blobs, int n, float** m32_out, double** m64_out) {
    const size_t len = (size_t)n * mjmpc::TREE_BLOB_LEN;
    std::vector<float> f32(blobs, blobs + len);
    float* m32 = nullptr;
    double* m64 = nullptr;
    HIP_TRY(hipMalloc(&m32, sizeof(float) * len));
    hipError_t e = hipMalloc(&m64, sizeof(double) * len);
    if (e == hipSuccess) e = hipMemcpy(m32, f32.data(), sizeof(float) * len, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m64, blobs, sizeof(double) * len, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(m32);
        hipFree(m64);
        return hip_fail(e, "model block upload");
    }
    *m32_out = m32;
    *m64_out = m64;
    return 0;
}

// what every rollout launch of the engine carries besides its own fusions: the reset records (one per model shard; shard >= 0:
// a launch that runs that one shard's model block)
static mjmpc::TreeFusion tree_fuse(const mjmpc_tree_s* h, int shard = -1) {
    mjmpc::TreeFusion f;
    if (h->reset_rec) {
        f.reset_rec = h->reset_rec + (shard > 0 && h->n_shards > 1 ? (size_t)shard * mjmpc::TREE_RESET_LEN : 0);
        f.reset_stride = (shard < 0 && h->n_shards > 1) ? mjmpc::TREE_RESET_LEN : 0;
    }
    f.inf_on_reset = h->inf_on_reset;
    return f;
}

// One launch of the tree kernel, by name: a call site says what is special about it, tree_launch adds what the handle knows
// (max_path, full, nv, nu, gen, integrator, diag).  Made for the engine's model blocks - all of them (shard < 0) or one
// (shard >= 0) - with the fusion every launch on them carries (tree_fuse).
struct TreeCall {
    size_t model_offset = 0;        // scalars from the start of model_f32 / model_f64
    int n_model_shards = 1;
    const double* state = nullptr;
    long P = 1;
    int H = 1;
    const double* mean = nullptr;
    const void* noise = nullptr;    // noise, cost, act, obs, nobs: of the launch's precision
    void* cost = nullptr;
    void* act = nullptr;
    void* obs = nullptr;
    void* nobs = nullptr;
    double* state_out = nullptr;
    const double* clw = nullptr;
    double* site_out = nullptr;
    int n_state_shards = 1;
    mjmpc::TreeFusion fuse;
    // a launch on blocks that are not (yet) the engine's (tree_make_reset_records): their device copy, of the launch's
    // precision, their kernel choice and a counter block of their own
    const void* other_model = nullptr;
    bool other_full = false;
    unsigned* other_diag = nullptr;

    TreeCall() = default;
    explicit TreeCall(const mjmpc_tree_s* h, int shard = -1)
        : model_offset(shard > 0 && h->n_shards > 1 ? (size_t)shard * mjmpc::TREE_BLOB_LEN : 0),
          n_model_shards(shard < 0 ? h->n_shards : 1), fuse(tree_fuse(h, shard)) {}
};

template <typename T>
static hipError_t tree_launch(const mjmpc_tree_s* h, const TreeCall& c, hipStream_t s) {
    const T* m = c.other_model ? (const T*)c.other_model : model<T>(h) + c.model_offset;
    return mjmpc::launch_tree_rollout<T>(m, c.n_model_shards, h->max_path, c.other_model ? c.other_full : h->full, h->nv, c.state,
                                         c.P, c.H, h->nu, c.mean, (const T*)c.noise, (T*)c.cost, (T*)c.act, (T*)c.obs,
                                         (T*)c.nobs, c.other_model ? c.other_diag : h->diag, s, c.state_out, c.clw, c.site_out,
                                         c.n_state_shards, h->gen, c.fuse, h->integrator);
}
static int tree_issue(const mjmpc_tree_s* h, int dtype, const TreeCall& c, hipStream_t s, const char* what) {
    return with_dtype(dtype, what, [&](auto tag) { return tree_launch<decltype(tag)>(h, c, s); });
}

// The reset records of `n_shards` model blocks (host, TREE_BLOB_LEN each): per block ONE substep of the f64 kernel itself
// from the reset state (qpos0 = the device's zero coordinates and identity quaternions, zero velocity, zero controls) on a
// copy of the block with frame_skip 1 - state_out receives the state after it, site_out / axis_out the site and the object
// axis at the reset state (under RK4: at the substep's last stage, where mj_RungeKutta leaves them).  Synchronous; called when the engine is created and when its model blocks are replaced.
// (as arm_make_reset_records: the records come back in *out, `full` is the kernel choice of the NEW blocks, the launches count
// into a scratch counter block)
static int tree_make_reset_records(mjmpc_tree_s* h, const double* blobs, int n_shards, bool full, double** out) {
    const size_t L = (size_t)mjmpc::TREE_BLOB_LEN, R = (size_t)mjmpc::TREE_RESET_LEN;
    double *rec = nullptr, *tmp = nullptr, *st = nullptr;
    unsigned* sdiag = nullptr;
    HIP_TRY(hipMalloc(&rec, sizeof(double) * R * n_shards));
    hipError_t e = hipMalloc(&tmp, sizeof(double) * L);
    if (e == hipSuccess) e = hipMalloc(&sdiag, MJMPC_TREE_DIAG_BYTES);
    if (e == hipSuccess) e = hipMemset(sdiag, 0, MJMPC_TREE_DIAG_BYTES);
    if (e == hipSuccess) e = hipMalloc(&st, sizeof(double) * mjmpc::TREE_STATE_LEN);
    if (e == hipSuccess) e = hipMemset(rec, 0, sizeof(double) * R * n_shards);
    std::vector<double> b(L), s0(mjmpc::TREE_STATE_LEN, 0.0);
    for (int l = 0; l < mjmpc::TL; ++l) s0[mjmpc::TREE_QW + l] = 1.0;
    if (e == hipSuccess) e = hipMemcpy(st, s0.data(), sizeof(double) * s0.size(), hipMemcpyHostToDevice);
    for (int k = 0; k < n_shards && e == hipSuccess; ++k) {
        std::memcpy(b.data(), blobs + (size_t)k * L, sizeof(double) * L);
        b[mjmpc::T_FRAME_SKIP] = 1.0;
        e = hipMemcpy(tmp, b.data(), sizeof(double) * L, hipMemcpyHostToDevice);
        if (e != hipSuccess) break;
        double* rk = rec + (size_t)k * R;
        TreeCall c;                 // (one particle, one step, zero controls; no reset record: this launch makes it)
        c.other_model = tmp;
        c.other_full = full;
        c.other_diag = sdiag;
        c.state = st;
        c.mean = h->zero_action;
        c.cost = h->scratch;
        c.state_out = rk;
        c.site_out = rk + mjmpc::TREE_STATE_LEN;
        c.fuse.axis_out = rk + mjmpc::TREE_STATE_LEN + 3;
        e = tree_launch<double>(h, c, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    hipFree(tmp);
    hipFree(st);
    hipFree(sdiag);
    if (e != hipSuccess) {
        hipFree(rec);
        return hip_fail(e, "reset record");
    }
    *out = rec;
    return 0;
}

// what mjmpc_tree_rollout / _rollout_cl / _rollout_fused do between their null checks and their launch: the sizes, the shard
// arithmetic, the device, and the call on all model blocks from the start state(s)
static int tree_rollout_begin(const mjmpc_tree_s* h, int64_t P, int H, TreeCall* c) {
    if (P < 0 || H < 0) return fail(MJMPC_E_BADARG, "negative size");
    const int nss = h->n_state_shards > 1 ? h->n_state_shards : 1;
    if (P % h->n_shards != 0 || P % nss != 0)
        return fail(MJMPC_E_BADARG, "%lld particles do not divide into %d shards", (long long)P, std::max(h->n_shards, nss));
    HIP_TRY(hipSetDevice(h->device));
    *c = TreeCall(h);
    c->state = nss > 1 ? h->shard_states : h->state;
    c->n_state_shards = nss;
    c->P = (long)P;
    c->H = H;
    return 0;
}

// what every batch entry point asks of the engine: one model block, 1 .. 65535 state shards (grid rows), and - given a
// particle count - the same number of particles per shard
static int tree_batch_shape(const mjmpc_tree_s* h, int64_t P_total, int* E) {
    if (!h) return fail(MJMPC_E_BADARG, "null engine");
    if (h->n_shards > 1) return fail(MJMPC_E_BADARG, "an episode batch runs one model block; the engine has %d", h->n_shards);
    const int e = h->n_state_shards;
    if (e < 1 || e > 65535)
        return fail(MJMPC_E_BADARG, "an episode batch needs 1 .. 65535 state shards (mjmpc_tree_set_shard_states); the engine has %d", e);
    if (P_total < 1 || P_total % e != 0)
        return fail(MJMPC_E_BADARG, "%lld particles do not divide into %d episodes", (long long)P_total, e);
    *E = e;
    return 0;
}

extern "C" {

int mjmpc_abi_version(void) { return MJMPC_ABI_VERSION; }

const char* mjmpc_last_error(void) { return g_err; }

int mjmpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mjmpc_graph_kernel_nodes(void* hip_graph, int64_t* n_out) {
    if (!hip_graph || !n_out) return fail(MJMPC_E_BADARG, "null argument");
    size_t n = 0;
    HIP_TRY(hipGraphGetNodes((hipGraph_t)hip_graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) HIP_TRY(hipGraphGetNodes((hipGraph_t)hip_graph, nodes.data(), &n));
    int64_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        HIP_TRY(hipGraphNodeGetType(nodes[i], &t));
        k += t == hipGraphNodeTypeKernel;
    }
    n_out[0] = k;
    n_out[1] = (int64_t)n;
    return 0;
}

// An order-independent signature of a captured graph: n_out[0] = sum over its KERNEL nodes of a hash of (function, grid,
// block, dynamic LDS), n_out[1] = the same over every node's type.  (Argument VALUES are out of the runtime's reach - a
// kernel node's parameter array comes without sizes - but they are the recorded ones by construction; what can differ
// between an iteration and its tape is which kernels run and in what shape.)
int mjmpc_graph_signature(void* hip_graph, uint64_t* n_out) {
    if (!hip_graph || !n_out) return fail(MJMPC_E_BADARG, "null argument");
    size_t n = 0;
    HIP_TRY(hipGraphGetNodes((hipGraph_t)hip_graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) HIP_TRY(hipGraphGetNodes((hipGraph_t)hip_graph, nodes.data(), &n));
    auto mix = [](uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; };
    uint64_t ksum = 0, tsum = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        HIP_TRY(hipGraphNodeGetType(nodes[i], &t));
        tsum += mix(1469598103934665603ull, (uint64_t)t);
        if (t != hipGraphNodeTypeKernel) continue;
        hipKernelNodeParams kp;
        HIP_TRY(hipGraphKernelNodeGetParams(nodes[i], &kp));
        uint64_t h = 1469598103934665603ull;
        h = mix(h, (uint64_t)(uintptr_t)kp.func);
        h = mix(h, ((uint64_t)kp.gridDim.x << 32) | kp.gridDim.y);
        h = mix(h, ((uint64_t)kp.gridDim.z << 32) | kp.blockDim.x);
        h = mix(h, ((uint64_t)kp.blockDim.y << 32) | kp.blockDim.z);
        h = mix(h, (uint64_t)kp.sharedMemBytes);
        ksum += h;
    }
    n_out[0] = ksum;
    n_out[1] = tsum;
    return 0;
}

/* ---- arm engine ------------------------------------------------------------------------------------- */
int mjmpc_arm_create(const double* blob, int n_blob, int device, mjmpc_arm_t* out) {
    if (!blob || !out) return fail(MJMPC_E_BADARG, "null argument");
    if (n_blob != mjmpc::ARM_BLOB_LEN) return fail(MJMPC_E_BADMODEL, "model blob has %d scalars, expected %d", n_blob, (int)mjmpc::ARM_BLOB_LEN);
    const int nv = (int)blob[mjmpc::O_NV];
    if (nv < 1 || nv > mjmpc::MAX_LINKS) return fail(MJMPC_E_BADMODEL, "nv = %d outside 1..%d", nv, mjmpc::MAX_LINKS);
    if (mjmpc_device_count() <= device) return fail(MJMPC_E_NOGPU, "HIP device %d not present", device);
    HIP_TRY(hipSetDevice(device));
    mjmpc_arm_s* h = new mjmpc_arm_s();
    h->device = device;
    h->nv = nv;
    h->nu = (int)blob[mjmpc::O_NU] >= 1 && (int)blob[mjmpc::O_NU] <= nv ? (int)blob[mjmpc::O_NU] : nv;
    h->d_obs = 2 * nv + 6;
    h->xj = arm_blob_is_xj(blob, 1);
    int rc = core_create(h, blob, n_blob, MJMPC_ARM_STATE_LEN, MJMPC_DIAG_BYTES);
    if (rc == 0) rc = arm_make_reset_records(h, blob, 1, &h->reset_rec);
    if (rc != 0) {          // a failed allocation leaves nothing behind
        mjmpc_arm_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int mjmpc_arm_set_shard_models(mjmpc_arm_t h, const double* blobs, int n_shards) {
    if (!h || !blobs || n_shards < 1) return fail(MJMPC_E_BADARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    for (int s = 0; s < n_shards; ++s)
        if ((int)blobs[(size_t)s * mjmpc::ARM_BLOB_LEN + mjmpc::O_NV] != h->nv)
            return fail(MJMPC_E_BADMODEL, "shard %d has a different nv", s);
    const bool xj_old = h->xj;
    const int rc = core_swap_models(h, blobs, n_shards, mjmpc::ARM_BLOB_LEN, [&](double** rec) {
        h->xj = arm_blob_is_xj(blobs, n_shards);        // (the record launches run the build the NEW blocks need)
        return arm_make_reset_records(h, blobs, n_shards, rec);
    });
    if (rc != 0) h->xj = xj_old;
    return rc;
}

int mjmpc_arm_set_shard_states(mjmpc_arm_t h, const double* states, int n_shards, void* stream) {
    if (!h || (n_shards > 0 && !states) || n_shards < 0) return fail(MJMPC_E_BADARG, "bad argument");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = core_resize_shard_states(h, n_shards, MJMPC_ARM_STATE_LEN)) return rc;
    if (n_shards == 0) return 0;
    return core_upload_shard_states(h, states, (size_t)n_shards * MJMPC_ARM_STATE_LEN, (hipStream_t)stream);
}

int mjmpc_arm_destroy(mjmpc_arm_t h) {
    if (!h) return 0;
    core_free(h);
    hipFree(h->mono_tree);
    for (double* p : h->mono_retired) hipFree(p);
    delete h;
    return 0;
}

int mjmpc_arm_dims(mjmpc_arm_t h, int* nv, int* nu, int* d_obs) { return core_dims(h, nv, nu, d_obs); }

int mjmpc_arm_set_state(mjmpc_arm_t h, const double* qpos, const double* qvel, const double* target_pos,
                        void* stream) {
    if (!h || !qpos || !qvel || !target_pos) return fail(MJMPC_E_BADARG, "null argument");
    return core_set_state(h, MJMPC_ARM_STATE_LEN, (hipStream_t)stream, [&](double* stage) {
        std::memset(stage, 0, sizeof(double) * MJMPC_ARM_STATE_LEN);
        std::memcpy(stage, qpos, sizeof(double) * h->nv);
        std::memcpy(stage + mjmpc::LANES, qvel, sizeof(double) * h->nv);
        std::memcpy(stage + 2 * mjmpc::LANES, target_pos, sizeof(double) * 3);
    });
}

double* mjmpc_arm_state_ptr(mjmpc_arm_t h) { return h ? h->state : nullptr; }

int mjmpc_arm_rollout(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                      void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream) {
    if (!h || !d_mean || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    mjmpc::RolloutFusion fuse;
    const double* st = nullptr;
    if (int rc = arm_rollout_begin(h, P, H, &fuse, &st)) return rc;
    return with_dtype(dtype, "arm_rollout launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_rollout_launch<T>(h, model<T>(h), st, (long)P, H, h->nu, d_mean, (const T*)d_noise, (T*)d_costs, (T*)d_actions,
                                     (T*)d_obs, (T*)d_next_obs, nullptr, h->diag, (hipStream_t)stream, fuse);
    });
}

int mjmpc_arm_rollout_cl(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_weights, const void* d_noise,
                         void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream) {
    if (!h || !d_weights || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    mjmpc::RolloutFusion fuse;
    const double* st = nullptr;
    if (int rc = arm_rollout_begin(h, P, H, &fuse, &st)) return rc;
    fuse.clw = d_weights;
    return with_dtype(dtype, "arm_rollout_cl launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_rollout_launch<T>(h, model<T>(h), st, (long)P, H, h->nu, d_weights, (const T*)d_noise, (T*)d_costs,
                                     (T*)d_actions, (T*)d_obs, (T*)d_next_obs, nullptr, h->diag, (hipStream_t)stream, fuse);
    });
}

int mjmpc_arm_rollout_fused(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                            const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                            double* d_q0, void* stream) {
    if (!h || !d_mean || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    if ((d_q0 != nullptr) != (d_gseq != nullptr)) return fail(MJMPC_E_BADARG, "d_q0 and d_gseq go together");
    mjmpc::RolloutFusion fuse;
    const double* st = nullptr;
    if (int rc = arm_rollout_begin(h, P, H, &fuse, &st)) return rc;
    fuse.filt = d_filter_coeffs;
    fuse.gseq = d_gseq;
    fuse.q0_out = d_q0;
    return with_dtype(dtype, "arm_rollout_fused launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_rollout_launch<T>(h, model<T>(h), st, (long)P, H, h->nu, d_mean, (const T*)d_noise, (T*)d_costs, (T*)d_actions,
                                     nullptr, nullptr, nullptr, h->diag, (hipStream_t)stream, fuse);
    });
}

int mjmpc_arm_mppi_step(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, double* d_mean_out,
                        const double* d_gseq, const double* d_filter_coeffs, const double* d_chol, uint64_t seed,
                        uint64_t offset, int64_t particle_offset, int64_t* d_step_counter, double lam, double step_size,
                        int shift_mode, double* d_action_out, double* h_action_slots, double* d_record, int env_step,
                        void* d_step_cost, void* d_step_next_obs, void* d_costs, void* d_actions, double* d_q0, void* stream) {
    if (!h || !d_mean || !d_gseq || !d_chol) return fail(MJMPC_E_BADARG, "null argument");
    if (!d_record && shift_mode != -2 && (!d_mean_out || d_mean_out == d_mean))
        return fail(MJMPC_E_BADARG, "d_mean_out must be a buffer of its own (the finish launch reads d_mean while it writes)");
    if (P < 1 || H < 1) return fail(MJMPC_E_BADARG, "P and H must be positive");
    if (!(lam > 0) || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad lam / shift_mode");
    const bool rollout_only = shift_mode == -2;         // (measurement: the first launch alone, records left in the engine)
    if (h->n_shards > 1 || h->n_state_shards > 1)
        return fail(MJMPC_E_BADARG, "the fused iteration runs one model and one start state (no per-shard blocks)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const long groups = mjmpc::arm_rollout_groups((long)P);
    if (int rc = arm_grow_mono(h, (size_t)mjmpc::mono_record_doubles(groups, H, h->nu), s)) return rc;
    mjmpc::MonoStep mo;             // (travels to both kernels by value, as a kernel argument)
    mo.chol = d_chol;
    mo.seed = seed;
    mo.offset = offset;
    mo.particle_offset = (long)particle_offset;
    mo.d_step = (const long long*)d_step_counter;
    mo.lam = lam;
    mo.step_size = step_size;
    mo.shift_mode = shift_mode;
    mo.tree = h->mono_tree;
    mo.action_out = d_action_out;
    mo.action_host = h_action_slots;
    mo.step_counter = (long long*)d_step_counter;
    mo.record = d_record;
    mo.state_io = h->state;
    mo.step_cost = d_step_cost;
    mo.step_nobs = d_step_next_obs;
    mo.reset_rec = h->reset_rec;
    const int do_env = (env_step && !d_record) ? 1 : 0;
    mjmpc::RolloutFusion fuse = arm_fuse(h);
    fuse.filt = d_filter_coeffs;
    fuse.gseq = d_gseq;
    fuse.q0_out = d_q0;
    return with_dtype(dtype, "arm_mppi_step launch", [&](auto tag) {
        using T = decltype(tag);
        hipError_t e = arm_rollout_launch<T>(h, model<T>(h), h->state, (long)P, H, h->nu, d_mean, nullptr, (T*)d_costs,
                                             (T*)d_actions, nullptr, nullptr, nullptr, h->diag, s, fuse, &mo);
        if (e == hipSuccess && !rollout_only)
            e = arm_finish_launch<T>(h, model<T>(h), h->mono_tree, groups, H, h->nu, d_mean, d_mean_out, mo, do_env, h->diag, s);
        return e;
    });
}

int mjmpc_arm_rollout_sampled(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const double* d_gseq,
                              const double* d_filter_coeffs, const double* d_chol, int chol_full, uint64_t seed, uint64_t offset,
                              int64_t particle_offset, const int64_t* d_step_counter, void* d_costs, void* d_actions,
                              double* d_q0, void* stream) {
    if (!h || !d_mean || !d_gseq || !d_chol) return fail(MJMPC_E_BADARG, "null argument");
    if (P < 1 || H < 1) return fail(MJMPC_E_BADARG, "P and H must be positive");
    if (h->n_shards > 1 || h->n_state_shards > 1)
        return fail(MJMPC_E_BADARG, "sampled rollouts run one model and one start state (no per-shard blocks)");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const long groups = mjmpc::arm_rollout_groups((long)P);
    // (the launch also leaves its softmax partials)
    if (int rc = arm_grow_mono(h, (size_t)mjmpc::mono_record_doubles(groups, H, h->nu), s)) return rc;
    mjmpc::MonoStep mo;
    mo.chol = d_chol;
    mo.chol_full = chol_full ? 1 : 0;
    mo.seed = seed;
    mo.offset = offset;
    mo.particle_offset = (long)particle_offset;
    mo.d_step = (const long long*)d_step_counter;
    mo.lam = 1.0;
    mo.shift_mode = -2;
    mo.tree = h->mono_tree;
    mjmpc::RolloutFusion fuse = arm_fuse(h);
    fuse.filt = d_filter_coeffs;
    fuse.gseq = d_gseq;
    fuse.q0_out = d_q0;
    return with_dtype(dtype, "arm_rollout_sampled launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_rollout_launch<T>(h, model<T>(h), h->state, (long)P, H, h->nu, d_mean, nullptr, (T*)d_costs, (T*)d_actions,
                                     nullptr, nullptr, nullptr, h->diag, s, fuse, &mo);
    });
}

int mjmpc_arm_mppi_combine(mjmpc_arm_t h, int dtype, const double* d_records, int n_records, int H, const double* d_mean,
                           double* d_mean_out, int64_t* d_step_counter, double step_size, int shift_mode,
                           double* d_action_out, double* h_action_slots, int env_step, void* d_step_cost,
                           void* d_step_next_obs, void* stream) {
    if (!h || !d_records || !d_mean || !d_mean_out || d_mean_out == d_mean) return fail(MJMPC_E_BADARG, "null / aliased argument");
    if (n_records < 1 || H < 1 || shift_mode > 1 || shift_mode < -1) return fail(MJMPC_E_BADARG, "bad n_records / H / shift_mode");
    if (env_step && (h->n_shards > 1 || h->n_state_shards > 1))
        return fail(MJMPC_E_BADARG, "the fused env step runs one model and one state (no per-shard blocks)");
    HIP_TRY(hipSetDevice(h->device));
    mjmpc::MonoStep mo;
    mo.step_size = step_size;
    mo.shift_mode = shift_mode;
    mo.action_out = d_action_out;
    mo.action_host = h_action_slots;
    mo.step_counter = (long long*)d_step_counter;
    mo.state_io = h->state;
    mo.step_cost = d_step_cost;
    mo.step_nobs = d_step_next_obs;
    mo.reset_rec = h->reset_rec;
    return with_dtype(dtype, "arm_mppi_combine launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_finish_launch<T>(h, model<T>(h), d_records, n_records, H, h->nu, d_mean, d_mean_out, mo, env_step ? 1 : 0,
                                    h->diag, (hipStream_t)stream);
    });
}

int mjmpc_arm_step_state(mjmpc_arm_t h, int dtype, const double* d_action, void* d_cost, void* d_next_obs,
                         void* stream) {
    if (!h || !d_action || !d_cost) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    return with_dtype(dtype, "arm_step_state launch", [&](auto tag) {
        using T = decltype(tag);
        return arm_rollout_launch<T>(h, model<T>(h), h->state, 1, 1, h->nu, d_action, nullptr, (T*)d_cost, nullptr, nullptr,
                                     (T*)d_next_obs, h->state, h->diag, (hipStream_t)stream, arm_fuse(h));
    });
}

int mjmpc_arm_get_state(mjmpc_arm_t h, double* qpos, double* qvel, void* stream) {
    if (!h || !qpos || !qvel) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    double st[MJMPC_ARM_STATE_LEN];
    HIP_TRY(hipMemcpyAsync(st, h->state, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::memcpy(qpos, st, sizeof(double) * h->nv);
    std::memcpy(qvel, st + mjmpc::LANES, sizeof(double) * h->nv);
    return 0;
}

/* ---- episode batches: the engine's E state shards are the batch's E real envs -------------------------- */
// E of a batch call on this engine; refuses what the twins do not run
static int arm_batch_shape(const mjmpc_arm_s* h, int* E) {
    if (h->n_state_shards < 1) return fail(MJMPC_E_BADARG, "the engine has no state shards (mjmpc_arm_set_shard_states)");
    if (h->n_state_shards > 65535) return fail(MJMPC_E_BADARG, "%d state shards: a batch holds at most 65535 episodes", h->n_state_shards);
    if (h->n_shards > 1) return fail(MJMPC_E_BADARG, "an episode batch runs one model block (the engine holds %d)", h->n_shards);
    if (h->xj) return fail(MJMPC_E_BADARG, "extended-joint models (slide joints / friction loss) have no episode-batch kernels: use the tree engine");
    *E = h->n_state_shards;
    return 0;
}

// the batch rollout of both entries; d_next_obs: dtype [P_total][H][d_obs] or null
static int arm_rollout_batch(mjmpc_arm_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                             const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions, double* d_q0,
                             void* d_next_obs, void* stream) {
    if (!h || !d_means || !d_noise || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    if ((d_q0 != nullptr) != (d_gseq != nullptr)) return fail(MJMPC_E_BADARG, "d_q0 and d_gseq go together");
    if (H < 1) return fail(MJMPC_E_BADARG, "horizon %d", H);
    int E = 0;
    if (int rc = arm_batch_shape(h, &E)) return rc;
    if (P_total < 1 || P_total % E != 0)
        return fail(MJMPC_E_BADARG, "P_total = %lld is not divisible by %d episodes", (long long)P_total, E);
    if ((P_total / E) % mjmpc::LANES != 0)
        return fail(MJMPC_E_BADARG, "an episode must hold a multiple of 8 particles (got %lld)", (long long)(P_total / E));
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return fail(MJMPC_E_BADARG, "unknown dtype %d", dtype);
    HIP_TRY(hipSetDevice(h->device));
    mjmpc::RolloutFusion fuse = arm_fuse(h);
    fuse.state_shard_size = (long)(P_total / E);        // (also the rows of episode e's mean: d_means + e H A)
    fuse.filt = d_filter_coeffs;
    fuse.gseq = d_gseq;
    fuse.q0_out = d_q0;
    return with_dtype(dtype, "arm_rollout_fused_batch launch", [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::launch_arm_rollout<T>(model<T>(h), h->shard_states, (long)P_total, H, h->nu, d_means, (const T*)d_noise,
                                            (T*)d_costs, (T*)d_actions, nullptr, (T*)d_next_obs, nullptr, h->diag,
                                            (hipStream_t)stream, fuse, nullptr, 1);
    });
}

int mjmpc_arm_rollout_fused_batch(mjmpc_arm_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                                  const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                                  double* d_q0, void* stream) {
    return arm_rollout_batch(h, dtype, P_total, H, d_means, d_noise, d_filter_coeffs, d_gseq, d_costs, d_actions, d_q0, nullptr,
                             stream);
}

int mjmpc_arm_rollout_fused_batch_obs(mjmpc_arm_t h, int dtype, int64_t P_total, int H, const double* d_means,
                                      const void* d_noise, const double* d_filter_coeffs, const double* d_gseq, void* d_costs,
                                      void* d_actions, double* d_q0, void* d_next_obs, void* stream) {
    return arm_rollout_batch(h, dtype, P_total, H, d_means, d_noise, d_filter_coeffs, d_gseq, d_costs, d_actions, d_q0,
                             d_next_obs, stream);
}

int mjmpc_arm_step_shard_states(mjmpc_arm_t h, int dtype, const double* d_actions, void* d_costs, void* d_next_obs, void* stream) {
    if (!h || !d_actions || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    int E = 0;
    if (int rc = arm_batch_shape(h, &E)) return rc;
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return fail(MJMPC_E_BADARG, "unknown dtype %d", dtype);
    HIP_TRY(hipSetDevice(h->device));
    // mjmpc_arm_step_state once per workgroup: one live particle, one env step, no noise, the engine's model block and reset
    // record; workgroup e reads action e and advances state shard e in place
    mjmpc::RolloutFusion fuse = arm_fuse(h);
    fuse.state_shard_size = mjmpc::LANES;
    return with_dtype(dtype, "arm_step_shard_states launch", [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::launch_arm_rollout<T>(model<T>(h), h->shard_states, (long)E, 1, h->nu, d_actions, nullptr, (T*)d_costs,
                                            nullptr, nullptr, (T*)d_next_obs, h->shard_states, h->diag, (hipStream_t)stream,
                                            fuse, nullptr, 2);
    });
}

int mjmpc_arm_get_shard_states(mjmpc_arm_t h, double* qpos, double* qvel, void* stream) {
    if (!h || !qpos || !qvel) return fail(MJMPC_E_BADARG, "null argument");
    if (h->n_state_shards < 1) return fail(MJMPC_E_BADARG, "the engine has no state shards (mjmpc_arm_set_shard_states)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t L = MJMPC_ARM_STATE_LEN;
    std::vector<double> st((size_t)h->n_state_shards * L);
    HIP_TRY(hipMemcpyAsync(st.data(), h->shard_states, sizeof(double) * st.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k < h->n_state_shards; ++k) {
        std::memcpy(qpos + (size_t)k * h->nv, st.data() + (size_t)k * L, sizeof(double) * h->nv);
        std::memcpy(qvel + (size_t)k * h->nv, st.data() + (size_t)k * L + mjmpc::LANES, sizeof(double) * h->nv);
    }
    return 0;
}

int mjmpc_arm_solver_failures(mjmpc_arm_t h, uint32_t* count) { return read_counter(h, 0, count); }
int mjmpc_arm_diverged(mjmpc_arm_t h, uint32_t* count) { return read_counter(h, 1, count); }
int mjmpc_arm_env_resets(mjmpc_arm_t h, uint32_t* count) { return read_counter(h, ARM_DIAG_ENV_RESETS, count); }
int mjmpc_arm_set_reset_returns(mjmpc_arm_t h, int inf_returns) { return set_reset_returns(h, inf_returns); }

#ifdef MJMPC_STAMPS
// developer builds only (not declared in include/mjmpc_amd.h): read and clear the phase clocks
extern "C" int mjmpc_debug_stamps(mjmpc_arm_t h, unsigned long long* out32) {
    if (!h || !out32) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out32, (char*)h->diag + 16, 8 * 64, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset((char*)h->diag + 16, 0, 8 * 64));
    return 0;
}
#endif

/* ---- tree engine ------------------------------------------------------------------------------------ */
#ifdef TREE_STATS
// developer builds only (not declared in include/mjmpc_amd.h): read and clear the phase clocks / iteration counts
extern "C" int mjmpc_debug_tree_stats(mjmpc_tree_t h, unsigned long long* out48) {
    if (!h || !out48) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out48, (char*)h->diag + 8, 8 * mjmpc::TREE_STAT_SLOTS, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset((char*)h->diag + 8, 0, 8 * mjmpc::TREE_STAT_SLOTS));
    return 0;
}
#endif

int mjmpc_tree_create(const double* blob, int n_blob, int device, mjmpc_tree_t* out) {
    return mjmpc_tree_create_ex(blob, n_blob, device, MJMPC_INTEGRATOR_EULER, out);
}

static int tree_create_impl(mjmpc_tree_s* h, const double* blob, int n_blob) {
    if (int rc = core_create(h, blob, n_blob, MJMPC_TREE_DEVICE_STATE_LEN, MJMPC_TREE_DIAG_BYTES)) return rc;
    HIP_TRY(hipMalloc(&h->zero_action, sizeof(double) * 40));
    HIP_TRY(hipMemset(h->zero_action, 0, sizeof(double) * 40));
    h->scratch = h->zero_action + 32;
    return tree_make_reset_records(h, blob, 1, h->full, &h->reset_rec);
}

int mjmpc_tree_create_ex(const double* blob, int n_blob, int device, int integrator, mjmpc_tree_t* out) {
    if (!blob || !out) return fail(MJMPC_E_BADARG, "null argument");
    if (integrator != MJMPC_INTEGRATOR_EULER && integrator != MJMPC_INTEGRATOR_RK4)
        return fail(MJMPC_E_BADARG, "unknown integrator %d", integrator);
    if (n_blob != mjmpc::TREE_BLOB_LEN)
        return fail(MJMPC_E_BADMODEL, "tree model blob has %d scalars, expected %d", n_blob, (int)mjmpc::TREE_BLOB_LEN);
    const int nv = (int)blob[mjmpc::T_NV];
    if (nv < 1 || nv > mjmpc::TL) return fail(MJMPC_E_BADMODEL, "nv = %d outside 1..%d", nv, mjmpc::TL);
    if ((int)blob[mjmpc::T_N_SPHERE] > mjmpc::TREE_MAX_SPHERES) return fail(MJMPC_E_BADMODEL, "too many contact points");
    const int nu = (int)blob[mjmpc::T_NU], task = (int)blob[mjmpc::T_TASK], skip = (int)blob[mjmpc::T_OBS_SKIP];
    if (nu < 1 || nu > nv || task < 0 || task > 2 || skip < 0 || skip >= nv)
        return fail(MJMPC_E_BADMODEL, "nu = %d, task = %d, obs_skip = %d do not fit nv = %d", nu, task, skip, nv);
    if (mjmpc_device_count() <= device) return fail(MJMPC_E_NOGPU, "HIP device %d not present", device);
    HIP_TRY(hipSetDevice(device));
    mjmpc_tree_s* h = new mjmpc_tree_s();
    h->device = device;
    h->nv = nv;
    h->nu = (int)blob[mjmpc::T_NU];
    h->nq = (int)blob[mjmpc::T_NQ];
    if (h->nq < nv || h->nq > mjmpc::TREE_NQ_MAX) {
        delete h;
        return fail(MJMPC_E_BADMODEL, "nq = %d does not fit nv = %d", (int)blob[mjmpc::T_NQ], nv);
    }
    h->d_obs = (int)blob[mjmpc::T_TASK] == 1 ? h->nq + nv - (int)blob[mjmpc::T_OBS_SKIP] : h->nq + nv + 6;
    h->full = tree_blob_is_full(blob, nv);
    h->gen = (int)blob[mjmpc::T_GEN];
    for (int l = 0; l < nv; ++l) h->max_path = std::max(h->max_path, (int)blob[mjmpc::T_DEPTH + l] + 1);
    h->topo.assign(blob, blob + n_blob);
    h->integrator = integrator;
    if (integrator == MJMPC_INTEGRATOR_RK4 && (nv > 16 || h->gen >= 3)) {
        delete h;
        return fail(MJMPC_E_BADMODEL, "RK4 runs models of up to 16 dofs without elliptic friction cones (nv = %d, gen = %d)", nv,
                    (int)blob[mjmpc::T_GEN]);
    }
    if (int rc = tree_create_impl(h, blob, n_blob)) {       // a failed allocation leaves nothing behind
        mjmpc_tree_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int mjmpc_tree_set_shard_models(mjmpc_tree_t h, const double* blobs, int n_shards) {
    if (!h || !blobs || n_shards < 1) return fail(MJMPC_E_BADARG, "bad argument");
    if (h->n_state_shards > 1 && n_shards > 1 && n_shards != h->n_state_shards)
        return fail(MJMPC_E_BADARG, "%d model shards but %d per-shard start states", n_shards, h->n_state_shards);
    HIP_TRY(hipSetDevice(h->device));
    bool full = false;
    if (int rc = tree_check_blocks(h, blobs, n_shards, &full, "shard")) return rc;
    const int rc = core_swap_models(h, blobs, n_shards, mjmpc::TREE_BLOB_LEN,
                                    [&](double** rec) { return tree_make_reset_records(h, blobs, n_shards, full, rec); });
    if (rc == 0) h->full = full;    // of the NEW set of blocks (they replace the old ones)
    return rc;
}

int mjmpc_tree_set_batch_models(mjmpc_tree_t h, const double* blobs, int n_sets, int K) {
    if (n_sets < 0) return fail(MJMPC_E_BADARG, "n_sets = %d is negative", n_sets);
    if (n_sets > 0 && K < 1) return fail(MJMPC_E_BADARG, "K = %d model shards per episode", K);
    if (n_sets > 0 && !blobs) return fail(MJMPC_E_BADARG, "null model blocks");
    if (!h) return fail(MJMPC_E_BADARG, "null engine");
    HIP_TRY(hipSetDevice(h->device));
    float* m32 = nullptr;
    double *m64 = nullptr, *rec = nullptr;
    bool full = false;
    if (n_sets > 0) {
        if (n_sets != 1 && n_sets != h->n_state_shards)
            return fail(MJMPC_E_BADARG, "%d sets of model blocks: one for every episode, or one per state shard (%d)", n_sets,
                        h->n_state_shards);
        if (K > 65535 || (int64_t)n_sets * K > (1 << 20))
            return fail(MJMPC_E_BADARG, "%d sets of %d model shards are more than a batch launch takes", n_sets, K);
        const int n = n_sets * K;
        if (int rc = tree_check_blocks(h, blobs, n, &full, "batch block")) return rc;
        HIP_TRY(hipDeviceSynchronize());
        if (int rc = tree_upload_blocks(blobs, n, &m32, &m64)) return rc;
        if (int rc = tree_make_reset_records(h, blobs, n, full, &rec)) {
            hipFree(m32);
            hipFree(m64);
            return rc;
        }
    }
    HIP_TRY(hipDeviceSynchronize());        // (no launch that reads the old blocks is still running)
    hipFree(h->batch_f32);
    hipFree(h->batch_f64);
    hipFree(h->batch_rec);
    h->batch_f32 = m32;
    h->batch_f64 = m64;
    h->batch_rec = rec;
    h->batch_sets = n_sets;
    h->batch_k = n_sets > 0 ? K : 0;
    h->batch_full = full;
    return 0;
}

int mjmpc_tree_set_env_model(mjmpc_tree_t h, const double* blob) {
    if (!h) return fail(MJMPC_E_BADARG, "null engine");
    HIP_TRY(hipSetDevice(h->device));
    float* m32 = nullptr;
    double *m64 = nullptr, *rec = nullptr;
    bool full = false;
    if (blob) {
        if (int rc = tree_check_blocks(h, blob, 1, &full, "env block")) return rc;
        HIP_TRY(hipDeviceSynchronize());
        if (int rc = tree_upload_blocks(blob, 1, &m32, &m64)) return rc;
        if (int rc = tree_make_reset_records(h, blob, 1, full, &rec)) {
            hipFree(m32);
            hipFree(m64);
            return rc;
        }
    }
    for (void* p : {(void*)h->env_f32, (void*)h->env_f64, (void*)h->env_rec})
        if (p) h->env_retired.push_back(p);     // (env steps captured earlier still point at them)
    h->env_f32 = m32;
    h->env_f64 = m64;
    h->env_rec = rec;
    h->env_full = full;
    return 0;
}

int mjmpc_tree_set_shard_states(mjmpc_tree_t h, const double* states, int n_shards, void* stream) {
    if (!h || (n_shards > 0 && !states) || n_shards < 0) return fail(MJMPC_E_BADARG, "bad argument");
    if (h->n_shards > 1 && n_shards > 1 && n_shards != h->n_shards)
        return fail(MJMPC_E_BADARG, "%d per-shard start states but %d model shards", n_shards, h->n_shards);
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = core_resize_shard_states(h, n_shards, MJMPC_TREE_DEVICE_STATE_LEN)) return rc;
    if (n_shards == 0) return 0;
    std::vector<double> packed((size_t)n_shards * MJMPC_TREE_DEVICE_STATE_LEN);
    for (int k = 0; k < n_shards; ++k) {
        const double* pub = states + (size_t)k * MJMPC_TREE_STATE_LEN;     // qpos[40] | qvel[32] | target[3] | -
        tree_pack_state(h, pub, pub + mjmpc::TREE_NQ_MAX, pub + mjmpc::TREE_NQ_MAX + mjmpc::TL,
                        packed.data() + (size_t)k * MJMPC_TREE_DEVICE_STATE_LEN);
    }
    return core_upload_shard_states(h, packed.data(), packed.size(), (hipStream_t)stream);
}

int mjmpc_tree_destroy(mjmpc_tree_t h) {
    if (!h) return 0;
    core_free(h);
    hipFree(h->zero_action);
    for (void* p : {(void*)h->batch_f32, (void*)h->batch_f64, (void*)h->batch_rec, (void*)h->env_f32, (void*)h->env_f64,
                    (void*)h->env_rec})
        hipFree(p);
    for (void* p : h->env_retired) hipFree(p);
    delete h;
    return 0;
}

int mjmpc_tree_dims(mjmpc_tree_t h, int* nv, int* nu, int* d_obs) { return core_dims(h, nv, nu, d_obs); }

int mjmpc_tree_nq(mjmpc_tree_t h) { return h ? h->nq : -1; }

int mjmpc_tree_set_state(mjmpc_tree_t h, const double* qpos, const double* qvel, const double* target_pos,
                         void* stream) {
    if (!h || !qpos || !qvel || !target_pos) return fail(MJMPC_E_BADARG, "null argument");
    return core_set_state(h, MJMPC_TREE_DEVICE_STATE_LEN, (hipStream_t)stream,
                          [&](double* stage) { tree_pack_state(h, qpos, qvel, target_pos, stage); });
}

int mjmpc_tree_rollout(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                       void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream) {
    if (!h || !d_mean || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    TreeCall c;
    if (int rc = tree_rollout_begin(h, P, H, &c)) return rc;
    c.mean = d_mean;
    c.noise = d_noise;
    c.cost = d_costs;
    c.act = d_actions;
    c.obs = d_obs;
    c.nobs = d_next_obs;
    return tree_issue(h, dtype, c, (hipStream_t)stream, "tree_rollout launch");
}

int mjmpc_tree_rollout_fused(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                             const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions, double* d_q0,
                             void* stream) {
    if (!h || !d_mean || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    if ((d_q0 != nullptr) != (d_gseq != nullptr)) return fail(MJMPC_E_BADARG, "d_q0 and d_gseq go together");
    TreeCall c;
    if (int rc = tree_rollout_begin(h, P, H, &c)) return rc;
    c.mean = d_mean;
    c.noise = d_noise;
    c.cost = d_costs;
    c.act = d_actions;
    c.fuse.filt = d_filter_coeffs;
    c.fuse.gseq = d_gseq;
    c.fuse.q0_out = d_q0;
    return tree_issue(h, dtype, c, (hipStream_t)stream, "tree_rollout_fused launch");
}

int mjmpc_tree_rollout_cl(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_weights, const void* d_noise,
                          void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream) {
    if (!h || !d_weights || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    TreeCall c;
    if (int rc = tree_rollout_begin(h, P, H, &c)) return rc;
    hipStream_t s = (hipStream_t)stream;
    // the first action depends on the fresh observation, whose tracked site comes out of a kinematics pass: a
    // one-particle, one-step launch per start state (its cost lands in the workspace and is discarded) leaves it in
    // the state vector
    for (int k = 0; k < c.n_state_shards; ++k) {
        double* sk = (c.n_state_shards > 1 ? h->shard_states : h->state) + (size_t)k * MJMPC_TREE_DEVICE_STATE_LEN;
        TreeCall kin(h, k);
        kin.state = sk;
        kin.mean = h->zero_action;
        kin.cost = h->scratch;
        kin.site_out = sk + 2 * mjmpc::TL + 3;
        if (int rc = tree_issue(h, dtype, kin, s, "tree_rollout_cl launch")) return rc;
    }
    c.mean = d_weights;
    c.clw = d_weights;
    c.noise = d_noise;
    c.cost = d_costs;
    c.act = d_actions;
    c.obs = d_obs;
    c.nobs = d_next_obs;
    return tree_issue(h, dtype, c, s, "tree_rollout_cl launch");
}

int mjmpc_tree_step_state(mjmpc_tree_t h, int dtype, const double* d_action, void* d_cost, void* d_next_obs, void* stream) {
    if (!h || !d_action || !d_cost) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    TreeCall c(h, 0);       // one particle, one env step, no noise, shard 0's model; the state vector is advanced in place
    c.state = h->state;
    c.mean = d_action;
    c.cost = d_cost;
    c.nobs = d_next_obs;
    c.state_out = h->state;
    if (h->env_f64) {       // mjmpc_tree_set_env_model: the real env's own block and reset record
        c.other_model = dtype == MJMPC_F32 ? (const void*)h->env_f32 : (const void*)h->env_f64;
        c.other_full = h->env_full;
        c.other_diag = h->diag;
        c.fuse.reset_rec = h->env_rec;
        c.fuse.reset_stride = 0;
    }
    return tree_issue(h, dtype, c, (hipStream_t)stream, "tree_step_state launch");
}

int mjmpc_tree_get_state(mjmpc_tree_t h, double* qpos, double* qvel, void* stream) {
    if (!h || !qpos || !qvel) return fail(MJMPC_E_BADARG, "null argument");
    HIP_TRY(hipSetDevice(h->device));
    double st[MJMPC_TREE_DEVICE_STATE_LEN];
    HIP_TRY(hipMemcpyAsync(st, h->state, sizeof(st), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    tree_unpack_state(h, st, qpos, qvel);
    return 0;
}

/* ---- episode batches: the engine's E state shards are the batch's E real envs ---------------------------- */
// the batch rollout of both entries; d_next_obs: dtype [P_total][H][d_obs] or null
static int tree_rollout_batch(mjmpc_tree_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                              const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions, double* d_q0,
                              void* d_next_obs, void* stream) {
    if (!h || !d_means || !d_noise || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    if ((d_q0 != nullptr) != (d_gseq != nullptr)) return fail(MJMPC_E_BADARG, "d_q0 and d_gseq go together");
    if (H < 1) return fail(MJMPC_E_BADARG, "horizon %d", H);
    int E = 0;
    if (int rc = tree_batch_shape(h, P_total, &E)) return rc;
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return fail(MJMPC_E_BADARG, "unknown dtype %d", dtype);
    HIP_TRY(hipSetDevice(h->device));
    TreeCall c(h);
    c.state = h->shard_states;
    c.n_state_shards = E;
    c.P = (long)P_total;
    c.H = H;
    c.mean = d_means;
    c.noise = d_noise;
    c.cost = d_costs;
    c.act = d_actions;
    c.nobs = d_next_obs;
    c.fuse.filt = d_filter_coeffs;
    c.fuse.gseq = d_gseq;
    c.fuse.q0_out = d_q0;
    c.fuse.mean_stride = (long)H * h->nu;       // episode e's mean: d_means + e H A
    c.fuse.batch_k = 1;
    if (h->batch_sets > 0) {        // mjmpc_tree_set_batch_models: row (e, k) runs block set(e) K + k of the stored blocks
        const int K = h->batch_k;
        if (h->batch_sets != 1 && h->batch_sets != E)
            return fail(MJMPC_E_BADARG, "%d sets of batch model blocks but %d state shards", h->batch_sets, E);
        if (P_total % ((int64_t)E * K) != 0)
            return fail(MJMPC_E_BADARG, "%lld particles do not divide into %d episodes of %d model shards", (long long)P_total, E, K);
        c.other_model = dtype == MJMPC_F32 ? (const void*)h->batch_f32 : (const void*)h->batch_f64;
        c.other_full = h->batch_full;
        c.other_diag = h->diag;
        c.n_model_shards = h->batch_sets * K;
        c.fuse.reset_rec = h->batch_rec;
        c.fuse.reset_stride = c.n_model_shards > 1 ? mjmpc::TREE_RESET_LEN : 0;
        c.fuse.batch_k = K;
    }
    return tree_issue(h, dtype, c, (hipStream_t)stream, "tree_rollout_fused_batch launch");
}

int mjmpc_tree_rollout_fused_batch(mjmpc_tree_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                                   const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                                   double* d_q0, void* stream) {
    return tree_rollout_batch(h, dtype, P_total, H, d_means, d_noise, d_filter_coeffs, d_gseq, d_costs, d_actions, d_q0, nullptr,
                              stream);
}

int mjmpc_tree_rollout_fused_batch_obs(mjmpc_tree_t h, int dtype, int64_t P_total, int H, const double* d_means,
                                       const void* d_noise, const double* d_filter_coeffs, const double* d_gseq, void* d_costs,
                                       void* d_actions, double* d_q0, void* d_next_obs, void* stream) {
    return tree_rollout_batch(h, dtype, P_total, H, d_means, d_noise, d_filter_coeffs, d_gseq, d_costs, d_actions, d_q0,
                              d_next_obs, stream);
}

int mjmpc_tree_step_shard_states(mjmpc_tree_t h, int dtype, const double* d_actions, void* d_costs, void* d_next_obs, void* stream) {
    if (!h || !d_actions || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    int E = 0;
    if (int rc = tree_batch_shape(h, h->n_state_shards, &E)) return rc;
    if (dtype != MJMPC_F32 && dtype != MJMPC_F64) return fail(MJMPC_E_BADARG, "unknown dtype %d", dtype);
    HIP_TRY(hipSetDevice(h->device));
    // mjmpc_tree_step_state once per row: one particle, one env step, no noise, the model block's instantiation and reset
    // record; row e reads action e and advances state shard e in place
    TreeCall c(h, 0);
    c.state = h->shard_states;
    c.n_state_shards = E;
    c.P = E;
    c.mean = d_actions;
    c.cost = d_costs;
    c.nobs = d_next_obs;
    c.state_out = h->shard_states;
    c.fuse.mean_stride = h->nu;
    c.fuse.state_out_stride = mjmpc::TREE_STATE_LEN;
    return tree_issue(h, dtype, c, (hipStream_t)stream, "tree_step_shard_states launch");
}

int mjmpc_tree_get_shard_states(mjmpc_tree_t h, double* qpos, double* qvel, void* stream) {
    if (!h || !qpos || !qvel) return fail(MJMPC_E_BADARG, "null argument");
    if (h->n_state_shards < 1) return fail(MJMPC_E_BADARG, "the engine has no state shards (mjmpc_tree_set_shard_states)");
    HIP_TRY(hipSetDevice(h->device));
    const size_t L = MJMPC_TREE_DEVICE_STATE_LEN;
    std::vector<double> st((size_t)h->n_state_shards * L);
    HIP_TRY(hipMemcpyAsync(st.data(), h->shard_states, sizeof(double) * st.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    for (int k = 0; k < h->n_state_shards; ++k)
        tree_unpack_state(h, st.data() + (size_t)k * L, qpos + (size_t)k * h->nq, qvel + (size_t)k * h->nv);
    return 0;
}

int mjmpc_tree_solver_failures(mjmpc_tree_t h, uint32_t* count) { return read_counter(h, 0, count); }
int mjmpc_tree_diverged(mjmpc_tree_t h, uint32_t* count) { return read_counter(h, 1, count); }
int mjmpc_tree_env_resets(mjmpc_tree_t h, uint32_t* count) { return read_counter(h, mjmpc::TREE_DIAG_ENV_RESETS, count); }
int mjmpc_tree_set_reset_returns(mjmpc_tree_t h, int inf_returns) { return set_reset_returns(h, inf_returns); }

int mjmpc_analytic_rollout(int kind, const double* d_params, int n_state, int n_action, const double* d_state, int dtype,
                           int64_t P, int H, const double* d_mean, const void* d_noise, void* d_costs, void* d_actions,
                           void* d_obs, void* d_next_obs, int closed_loop_linear, void* stream) {
    if (!d_params || !d_state || !d_mean || !d_costs) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, "analytic rollout launch", [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::launch_analytic_rollout<T>(kind, d_params, n_state, n_action, d_state, (long)P, H, d_mean, (const T*)d_noise,
                                                 (T*)d_costs, (T*)d_actions, (T*)d_obs, (T*)d_next_obs, (hipStream_t)stream,
                                                 closed_loop_linear);
    });
}

// ---- update / noise entry points -------------------------------------------------------------------
// (a launch that has no element type: its hipError_t as the entry point's return code)
static int plain(hipError_t e, const char* what) { return e != hipSuccess ? hip_fail(e, what) : 0; }

// what every episode-batch entry point asks of its shape: a grid row per episode (1 .. 65535), sizes of at least one and
// A within the limit of its kernels (INT_MAX: none); checks that belong to one controller follow at the call
static int batch_shape(int E, int64_t P, int H, int A, int A_max, const char* what) {
    if (E < 1 || E > 65535) return fail(MJMPC_E_BADARG, "%s: %d episodes outside 1 .. 65535", what, E);
    if (P < 1 || H < 1 || A < 1) return fail(MJMPC_E_BADARG, "%s: bad sizes P = %lld, H = %d, A = %d", what, (long long)P, H, A);
    if (A > A_max) return fail(MJMPC_E_BADARG, "%s: A = %d above %d, the limit of its kernels", what, A, A_max);
    return 0;
}

int64_t mjmpc_update_workspace_bytes(int64_t P, int H, int A) {
    return (int64_t)sizeof(double) * mjmpc::update_workspace_doubles((long)P, H, A);
}

int mjmpc_softmax_record_len(int H, int A, int tbw) { return 2 * (tbw ? H : 1) + H * A + A * A; }

int mjmpc_traj_cost(int dtype, int64_t P, int H, int A, const void* d_costs, const double* d_gseq, int gamma_zero,
                    void* d_ws, void* stream) {
    if (!d_costs || !d_gseq || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::traj_cost<T>((const T*)d_costs, nullptr, nullptr, nullptr, d_gseq, gamma_zero, 1.0, 1, 0, (long)P, H, A,
                                   (double*)d_ws, (hipStream_t)stream);
    });
}

double* mjmpc_workspace_q0(void* d_ws, int64_t P, int H, int A) {
    return mjmpc::workspace_q0((double*)d_ws, (long)P, H, A);
}

int mjmpc_td_lambda_returns(int dtype, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                            const void* d_qvals, const double* d_mean, const double* d_covinv, const double* d_wseq,
                            int wseq_has_zero, double beta, int alpha, double gamma, double td_lam, void* d_returns,
                            void* d_ws, void* stream) {
    if (!d_costs || !d_returns || !d_ws || (H > 1 && !d_wseq)) return fail(MJMPC_E_BADARG, "null argument");
    if (alpha == 0 && (!d_actions || !d_mean || !d_covinv)) return fail(MJMPC_E_BADARG, "control cost needs actions, mean, cov^-1");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::td_lambda_returns<T>((const T*)d_costs, (const T*)d_actions, (const T*)d_qvals, d_mean, d_covinv, d_wseq,
                                           wseq_has_zero, beta, alpha, gamma, td_lam, (long)P, H, A, (T*)d_returns,
                                           (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_softmax_stats(int dtype, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                        const double* d_mean, const double* d_covinv, const double* d_gseq, int gamma_zero,
                        double lam, int alpha, int tbw, int want_cov, double* d_record, void* d_ws, void* stream) {
    if (!d_costs || !d_actions || !d_mean || !d_gseq || !d_record || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (alpha == 0 && !d_covinv) return fail(MJMPC_E_BADARG, "alpha == 0 needs d_covinv");
    if (tbw && want_cov) return fail(MJMPC_E_BADARG, "time_based_weights and want_cov are exclusive");
    if (!(lam > 0)) return fail(MJMPC_E_BADARG, "lam must be positive");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::softmax_stats<T>((const T*)d_costs, (const T*)d_actions, d_mean, d_covinv, d_gseq, gamma_zero, lam, alpha,
                                       tbw, want_cov, (long)P, H, A, d_record, (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_softmax_combine(const double* d_records, int G, int H, int A, int tbw, double lam, double step_size,
                          int cov_mode, double P_total, double* d_mean, double* d_cov, double* d_value,
                          double* d_wnorm, void* stream) {
    if (!d_records || !d_mean || G < 1) return fail(MJMPC_E_BADARG, "bad argument");
    if (cov_mode && !d_cov) return fail(MJMPC_E_BADARG, "cov_mode needs d_cov");
    return plain(mjmpc::softmax_combine(d_records, G, H, A, tbw, lam, step_size, cov_mode, P_total, d_mean, d_cov, d_value,
                                        d_wnorm, (hipStream_t)stream), __func__);
}

int mjmpc_softmax_weights(int64_t P, int H, int A, const double* d_wnorm, void* d_ws, double* d_weights,
                          void* stream) {
    if (!d_wnorm || !d_ws || !d_weights) return fail(MJMPC_E_BADARG, "null argument");
    return plain(mjmpc::softmax_weights((long)P, d_wnorm, (double*)d_ws, H, A, d_weights, (hipStream_t)stream), __func__);
}

int mjmpc_cem_elite_sums(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_q_all,
                         int64_t P_all, int64_t offset, int64_t k, double* d_sum_record, void* d_ws, void* stream) {
    if (!d_actions || !d_sum_record || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_elite_sums<T>((const T*)d_actions, d_q_all, (long)P_all, (long)offset, (long)k, (long)P, H, A,
                                        d_sum_record, (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_cem_elite_cov(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_mean,
                        const double* d_sum_records, int G, double* d_cov_record, void* d_ws, void* stream) {
    if (!d_actions || !d_mean || !d_sum_records || !d_cov_record || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_elite_cov<T>((const T*)d_actions, d_mean, d_sum_records, G, (long)P, H, A, d_cov_record,
                                       (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_cem_final(const double* d_cov_records, int G, int64_t P, int H, int A, double n_elite, int full_cov,
                    double step_size, double* d_mean, double* d_cov, void* d_ws, void* stream) {
    if (!d_cov_records || !d_mean || !d_cov || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return plain(mjmpc::cem_final(d_cov_records, G, (long)P, H, A, n_elite, full_cov, step_size, d_mean, d_cov,
                                  (double*)d_ws, (hipStream_t)stream), __func__);
}

int mjmpc_cem_combine(const double* d_records, int G, int H, int A, double n_elite, int full_cov, double step_size,
                      double* d_mean, double* d_cov, void* stream) {
    if (!d_records || !d_mean || !d_cov) return fail(MJMPC_E_BADARG, "null argument");
    return plain(mjmpc::cem_combine(d_records, G, H, A, n_elite, full_cov, step_size, d_mean, d_cov, (hipStream_t)stream),
                 __func__);
}

int mjmpc_cem_fused_supported(int64_t P_all, int64_t P, int64_t k, int H, int A) {
    return mjmpc::cem_fused_supported((long)P_all, (long)P, (long)k, H, A) ? 1 : 0;
}

int mjmpc_cem_select_moments(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_q_all, int64_t P_all,
                             int64_t offset, int64_t k, const double* d_mean, const double* d_cov,
                             const int64_t* d_step_counter, void* d_ws, void* stream) {
    if (!d_actions || !d_mean || !d_cov || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (!mjmpc::cem_fused_supported(d_q_all ? (long)P_all : (long)P, (long)P, (long)k, H, A))
        return fail(MJMPC_E_BADARG, "shape outside the fused CEM step (mjmpc_cem_fused_supported)");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_select_moments<T>((const T*)d_actions, d_q_all, (long)P_all, (long)offset, (long)k, (long)P, H, A,
                                            d_mean, d_cov, (const long long*)d_step_counter, (double*)d_ws,
                                            (hipStream_t)stream);
    });
}

int mjmpc_cem_record(int64_t P, int H, int A, int64_t k, const double* d_mean, double* d_record, void* d_ws, void* stream) {
    if (!d_mean || !d_record || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return plain(mjmpc::cem_record((long)k, (long)P, H, A, d_mean, d_record, (double*)d_ws, (hipStream_t)stream), __func__);
}

int mjmpc_cem_finish(int dtype, int64_t P, int H, int A, int64_t k, const double* d_records, int G, double n_elite,
                     int full_cov, double step_size, int shift_mode, double* d_mean, double* d_cov, double* d_chol,
                     int* d_status, const double* d_grow_diag, double grow_scale, double* d_action_out,
                     double* h_action_pinned, int64_t* d_step_counter, void* d_next_noise, uint64_t seed, uint64_t offset,
                     int64_t particle_offset, void* d_ws, void* stream) {
    if (!d_mean || !d_cov || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (shift_mode > 1) return fail(MJMPC_E_BADARG, "shift_mode must be < 0 (none), 0 (null) or 1 (repeat)");
    if (!mjmpc::cem_fused_supported((long)P, (long)P, (long)k, H, A))
        return fail(MJMPC_E_BADARG, "shape outside the fused CEM step (mjmpc_cem_fused_supported)");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_finish<T>(d_records, G, (long)k, (long)P, H, A, n_elite, full_cov, step_size, shift_mode, d_mean, d_cov,
                                    d_chol, d_status, d_grow_diag, grow_scale, d_action_out, h_action_pinned,
                                    (long long*)d_step_counter, (T*)d_next_noise, seed, offset, (long)particle_offset,
                                    (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_rs_best(int dtype, int64_t P, int H, int A, const void* d_actions, int64_t offset, double* d_record,
                  void* d_ws, void* stream) {
    if (!d_actions || !d_record || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::rs_best<T>((const T*)d_actions, (long)offset, (long)P, H, A, d_record, (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_rs_combine(const double* d_records, int G, int H, int A, double step_size, double* d_mean, void* stream) {
    if (!d_records || !d_mean || G < 1) return fail(MJMPC_E_BADARG, "bad argument");
    return plain(mjmpc::rs_combine(d_records, G, H, A, step_size, d_mean, (hipStream_t)stream), __func__);
}

static int fused_update(int dtype, int64_t P, int H, int A, const double* d_q0, const void* d_actions, double lam,
                        double step_size, int shift_mode, double* d_mean, double* d_action_out, double* d_record,
                        double* d_value, double* h_action_mapped, int64_t* d_step_counter, void* d_ws, void* stream,
                        const mjmpc::NextNoise* next) {
    if (!d_actions || !d_mean || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (!(lam > 0) || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad lam / shift_mode");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::mppi_fused_update<T>(d_q0, (const T*)d_actions, lam, step_size, shift_mode, (long)P, H, A, d_mean,
                                           d_action_out, d_record, d_value, (double*)d_ws, (hipStream_t)stream,
                                           h_action_mapped, (long long*)d_step_counter, next);
    });
}

int mjmpc_mppi_fused_update(int dtype, int64_t P, int H, int A, const double* d_q0, const void* d_actions, double lam,
                            double step_size, int shift_mode, double* d_mean, double* d_action_out, double* d_record,
                            double* d_value, double* h_action_mapped, int64_t* d_step_counter, void* d_ws,
                            void* stream) {
    return fused_update(dtype, P, H, A, d_q0, d_actions, lam, step_size, shift_mode, d_mean, d_action_out, d_record,
                        d_value, h_action_mapped, d_step_counter, d_ws, stream, nullptr);
}

int mjmpc_mppi_fused_update_draw_next(int dtype, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                                      double lam, double step_size, int shift_mode, double* d_mean,
                                      double* d_action_out, double* d_record, double* d_value, double* h_action_mapped,
                                      int64_t* d_step_counter, void* d_ws, void* d_next_noise, const double* d_chol,
                                      uint64_t seed, uint64_t offset, int64_t particle_offset, const int64_t* d_step,
                                      int chol_is_diagonal, void* stream) {
    if (!d_next_noise || !d_chol) return fail(MJMPC_E_BADARG, "null noise buffer or Cholesky factor");
    mjmpc::NextNoise nn{d_next_noise, d_chol, seed, offset, (long)particle_offset, (const long long*)d_step,
                        chol_is_diagonal};
    return fused_update(dtype, P, H, A, d_q0, d_actions, lam, step_size, shift_mode, d_mean, d_action_out, d_record,
                        d_value, h_action_mapped, d_step_counter, d_ws, stream, &nn);
}

int64_t mjmpc_update_batch_workspace_bytes(int E, int64_t P, int H, int A) {
    if (int rc = batch_shape(E, P, H, A, INT_MAX, __func__)) return rc;
    return (int64_t)sizeof(double) * mjmpc::mppi_fused_batch_workspace_doubles(E, (long)P, H, A);
}

int mjmpc_mppi_fused_update_batch(int dtype, int E, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                                  const double* d_lam, const double* d_step_size, int shift_mode, double* d_means,
                                  double* d_actions_out, int64_t* d_step_counter, void* d_ws, void* stream) {
    if (!d_q0 || !d_actions || !d_lam || !d_step_size || !d_means || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, P, H, A, INT_MAX, __func__)) return rc;
    if (shift_mode < -1 || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad shift_mode %d", shift_mode);
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::mppi_fused_update_batch<T>(E, d_q0, (const T*)d_actions, d_lam, d_step_size, shift_mode, (long)P, H, A,
                                                 d_means, d_actions_out, (long long*)d_step_counter, (double*)d_ws,
                                                 (hipStream_t)stream);
    });
}

int mjmpc_cem_batch_supported(int E, int64_t P, int64_t k_max, int H, int A) {
    return mjmpc::cem_batch_supported(E, (long)P, (long)k_max, H, A) ? 1 : 0;
}

static int cem_batch_shape(int E, int64_t P, int64_t k_max, int H, int A, const char* what) {
    if (int rc = batch_shape(E, P, H, A, INT_MAX, what)) return rc;
    if (!mjmpc::cem_batch_supported(E, (long)P, (long)k_max, H, A))
        return fail(MJMPC_E_BADARG, "shape outside the batched fused CEM step (mjmpc_cem_batch_supported): P = %lld, "
                    "k_max = %lld, H = %d, A = %d; it takes A <= 8, A <= H + 1, P <= 32768, 1 <= k <= P",
                    (long long)P, (long long)k_max, H, A);
    return 0;
}

int64_t mjmpc_cem_batch_workspace_bytes(int E, int64_t P, int64_t k_max, int H, int A) {
    if (int rc = cem_batch_shape(E, P, k_max, H, A, __func__)) return rc;
    return (int64_t)sizeof(double) * mjmpc::cem_batch_workspace_doubles(E, (long)P, H, A);
}

int mjmpc_cem_select_moments_batch(int dtype, int E, int64_t P, int H, int A, const void* d_actions, const double* d_q0,
                                   const int64_t* d_k, const double* d_means, const double* d_covs,
                                   const int64_t* d_step_counter, void* d_ws, void* stream) {
    if (!d_actions || !d_q0 || !d_k || !d_means || !d_covs || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = cem_batch_shape(E, P, 1, H, A, __func__)) return rc;
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_select_moments_batch<T>(E, (const T*)d_actions, d_q0, (const long long*)d_k, (long)P, H, A, d_means,
                                                  d_covs, (const long long*)d_step_counter, (double*)d_ws,
                                                  (hipStream_t)stream);
    });
}

int mjmpc_cem_finish_batch(int dtype, int E, int64_t P, int H, int A, const int64_t* d_k, int full_cov,
                           const double* d_step_size, int shift_mode, double* d_means, double* d_covs, double* d_chols,
                           int* d_status, const double* d_grow_diag, const double* d_grow_scale, double* d_actions_out,
                           int64_t* d_step_counter, void* d_next_noise, const uint64_t* d_seeds, uint64_t offset, void* d_ws,
                           void* stream) {
    if (!d_k || !d_step_size || !d_means || !d_covs || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    if (d_next_noise && !d_seeds) return fail(MJMPC_E_BADARG, "d_next_noise without d_seeds");
    if (shift_mode > 1) return fail(MJMPC_E_BADARG, "shift_mode must be < 0 (none), 0 (null) or 1 (repeat)");
    if (int rc = cem_batch_shape(E, P, 1, H, A, __func__)) return rc;
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::cem_finish_batch<T>(E, (const long long*)d_k, (long)P, H, A, full_cov, d_step_size, shift_mode, d_means,
                                          d_covs, d_chols, d_status, d_grow_diag, d_grow_scale, d_actions_out,
                                          (long long*)d_step_counter, (T*)d_next_noise, (const unsigned long long*)d_seeds,
                                          offset, (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_mppi_fused_combine(const double* d_records, int G, double P_total, int H, int A, double lam, double step_size,
                             int shift_mode, double* d_mean, double* d_action_out, double* d_value,
                             double* h_action_mapped, int64_t* d_step_counter, void* stream) {
    if (!d_records || !d_mean || G < 1) return fail(MJMPC_E_BADARG, "null argument");
    if (!(lam > 0) || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad lam / shift_mode");
    return plain(mjmpc::mppi_fused_combine(d_records, G, P_total, lam, step_size, shift_mode, H, A, d_mean, d_action_out,
                                           d_value, h_action_mapped, (long long*)d_step_counter, (hipStream_t)stream),
                 __func__);
}

int mjmpc_q0_sum(int64_t P, int H, int A, double* d_out, void* d_ws, void* stream) {
    if (!d_out || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return plain(mjmpc::q0_sum((long)P, H, A, d_out, (double*)d_ws, (hipStream_t)stream), __func__);
}

int mjmpc_shift_mean(double* d_mean, int H, int A, int mode, const double* d_row, void* stream) {
    if (!d_mean || (mode == 2 && !d_row) || mode < 0 || mode > 2) return fail(MJMPC_E_BADARG, "bad argument");
    return plain(mjmpc::shift_mean(d_mean, H, A, mode, d_row, (hipStream_t)stream), __func__);
}

int mjmpc_step_tail(double* d_mean, int H, int A, int shift_mode, const double* d_row, double* d_action_out,
                    double* h_action_mapped, int64_t* d_step_counter, double* d_cov, const double* d_cov_diag,
                    double cov_scale, void* stream) {
    if (!d_mean || (shift_mode == 2 && !d_row) || shift_mode < 0 || shift_mode > 2 || A < 1 || A > 64 || H < 1)
        return fail(MJMPC_E_BADARG, "bad argument");
    return plain(mjmpc::step_tail(d_mean, H, A, shift_mode, d_row, d_action_out, h_action_mapped, (long long*)d_step_counter,
                                  d_cov, d_cov_diag, cov_scale, (hipStream_t)stream), __func__);
}

int mjmpc_cholesky_lower(const double* d_cov, int A, double* d_chol, int* d_status, void* stream) {
    if (!d_cov || !d_chol || A < 1 || A > 64) return fail(MJMPC_E_BADARG, "bad argument (A <= 64)");
    return plain(mjmpc::cholesky_lower(d_cov, A, d_chol, d_status, (hipStream_t)stream), __func__);
}

// (A <= 64 below: the Cholesky kernel and the tail take a thread per action channel of one wavefront)
int mjmpc_cholesky_lower_batch(int E, const double* d_covs, int A, double* d_chols, int* d_status, void* stream) {
    if (!d_covs || !d_chols) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, 1, 1, A, 64, __func__)) return rc;
    return plain(mjmpc::cholesky_lower_batch(E, d_covs, A, d_chols, d_status, (hipStream_t)stream), __func__);
}

int64_t mjmpc_dmd_batch_workspace_bytes(int E, int64_t P, int H, int A) {
    if (int rc = batch_shape(E, P, H, A, 64, __func__)) return rc;
    return (int64_t)sizeof(double) * mjmpc::dmd_batch_workspace_doubles(E, (long)P, H, A);
}

int mjmpc_dmd_update_batch(int dtype, int E, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                           const double* d_gseq, const double* d_lam, const double* d_step_size, int cov_mode,
                           const double* d_beta, int shift_mode, double* d_means, double* d_covs, double* d_actions_out,
                           int64_t* d_step_counter, void* d_ws, void* stream) {
    if (!d_costs || !d_actions || !d_gseq || !d_lam || !d_step_size || !d_beta || !d_means || !d_covs || !d_ws)
        return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, P, H, A, 64, __func__)) return rc;
    if (cov_mode != 1 && cov_mode != 2) return fail(MJMPC_E_BADARG, "cov_mode %d (1 diagonal, 2 full)", cov_mode);
    if (shift_mode < 0 || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad shift_mode %d", shift_mode);
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::dmd_update_batch<T>(E, (const T*)d_costs, (const T*)d_actions, d_gseq, d_lam, d_step_size, cov_mode, d_beta,
                                          shift_mode, (long)P, H, A, d_means, d_covs, d_actions_out,
                                          (long long*)d_step_counter, (double*)d_ws, (hipStream_t)stream);
    });
}

int mjmpc_mppiq_batch_supported(int E, int64_t P, int H, int A, int time_based_weights) {
    return mjmpc::mppiq_batch_supported(E, (long)P, H, A, time_based_weights) ? 1 : 0;
}

static int mppiq_batch_shape(int E, int64_t P, int H, int A, int tbw, const char* what) {
    if (int rc = batch_shape(E, P, H, A, 64, what)) return rc;
    if (!mjmpc::mppiq_batch_supported(E, (long)P, H, A, tbw))
        return fail(MJMPC_E_BADARG, "H = %d above 512 with time-based weights (mjmpc_mppiq_batch_supported)", H);
    return 0;
}

int64_t mjmpc_mppiq_batch_workspace_bytes(int E, int64_t P, int H, int A, int time_based_weights) {
    if (int rc = mppiq_batch_shape(E, P, H, A, time_based_weights, __func__)) return rc;
    return (int64_t)sizeof(double) * mjmpc::mppiq_batch_workspace_doubles(E, (long)P, H, A, time_based_weights);
}

int mjmpc_mppiq_update_batch(int dtype, int E, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                             const double* d_beta, const double* d_step_size, const double* d_td_lam, const double* d_wseq,
                             const int* d_wseq_has_zero, double gamma, int alpha, const double* d_covinv,
                             int time_based_weights, int shift_mode, double* d_means, double* d_actions_out,
                             int64_t* d_step_counter, void* d_ws, void* stream) {
    if (!d_costs || !d_actions || !d_beta || !d_step_size || !d_td_lam || !d_wseq || !d_wseq_has_zero || !d_means || !d_ws)
        return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = mppiq_batch_shape(E, P, H, A, time_based_weights, __func__)) return rc;
    if (alpha != 0 && alpha != 1) return fail(MJMPC_E_BADARG, "alpha %d (0: control cost on, 1: off)", alpha);
    if (alpha == 0 && !d_covinv) return fail(MJMPC_E_BADARG, "alpha = 0 needs d_covinv");
    if (shift_mode < 0 || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad shift_mode %d", shift_mode);
    const double* covinv = alpha == 0 ? d_covinv : nullptr;
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::mppiq_update_batch<T>(E, (const T*)d_costs, (const T*)d_actions, d_beta, d_step_size, d_td_lam, d_wseq,
                                            d_wseq_has_zero, gamma, covinv, time_based_weights, shift_mode, (long)P, H, A,
                                            d_means, d_actions_out, (long long*)d_step_counter, (double*)d_ws,
                                            (hipStream_t)stream);
    });
}

int mjmpc_rs_batch_supported(int E, int64_t P, int H, int A) { return mjmpc::rs_batch_supported(E, (long)P, H, A) ? 1 : 0; }

int mjmpc_rs_update_batch(int dtype, int E, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                          const double* d_step_size, int shift_mode, double* d_means, double* d_actions_out,
                          int64_t* d_step_counter, int64_t* d_best, void* stream) {
    if (!d_q0 || !d_actions || !d_step_size || !d_means) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, P, H, A, INT_MAX, __func__)) return rc;
    if (!mjmpc::rs_batch_supported(E, (long)P, H, A))
        return fail(MJMPC_E_BADARG, "A = %d outside 1 .. 256 (mjmpc_rs_batch_supported)", A);
    if (shift_mode < 0 || shift_mode > 1) return fail(MJMPC_E_BADARG, "bad shift_mode %d", shift_mode);
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::rs_update_batch<T>(E, d_q0, (const T*)d_actions, d_step_size, shift_mode, (long)P, H, A, d_means,
                                         d_actions_out, (long long*)d_step_counter, (long long*)d_best, (hipStream_t)stream);
    });
}

int mjmpc_cov_add_diag(double* d_cov, int A, const double* d_diag, double scale, void* stream) {
    if (!d_cov || A < 1 || A > 64) return fail(MJMPC_E_BADARG, "bad argument (A <= 64)");
    return plain(mjmpc::cov_add_diag(d_cov, A, d_diag, scale, (hipStream_t)stream), __func__);
}

int mjmpc_filter_noise(int dtype, void* d_noise, int64_t P, int H, int A, const double* d_coeffs, void* stream) {
    if (!d_noise || !d_coeffs) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::filter_noise<T>((T*)d_noise, (long)P, H, A, d_coeffs, (hipStream_t)stream);
    });
}

int mjmpc_color_noise(int dtype, void* d_noise, int64_t rows, int A, const double* d_B, void* stream) {
    if (!d_noise || !d_B) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::color_rows<T>((T*)d_noise, (long)rows, A, d_B, (hipStream_t)stream);
    });
}

int64_t mjmpc_mt19937_workspace_bytes(int64_t n_normals) { return (int64_t)mjmpc::mt_workspace_bytes((long)n_normals); }

int mjmpc_sample_noise_mt19937(int dtype, void* d_noise, int64_t n_normals, double scale, uint64_t seed,
                               const int64_t* d_step, void* d_ws, int* d_status, void* stream) {
    if (!d_noise || !d_ws) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::sample_noise_mt19937<T>((T*)d_noise, (long)n_normals, scale, seed, (const long long*)d_step, d_ws,
                                              d_status, (hipStream_t)stream);
    });
}

int64_t mjmpc_mt19937_stream_words(int64_t n_normals) { return 4 * (int64_t)mjmpc::mt_attempts_for((long)n_normals); }

int mjmpc_sample_noise_mt19937_jump(int dtype, void* d_noise, int64_t n_normals, double scale, uint64_t seed,
                                    const int64_t* d_step, const int32_t* d_jump_idx, const int32_t* d_jump_starts,
                                    int64_t head_words, int64_t seg_words, int n_segments, int64_t first_normal,
                                    void* d_ws, int* d_status, void* stream) {
    if (!d_noise || !d_ws || first_normal < 0) return fail(MJMPC_E_BADARG, "null argument");
    if (n_segments > 0) {
        if (!d_jump_idx || !d_jump_starts) return fail(MJMPC_E_BADARG, "jump tables missing");
        if (head_words < 19936 || head_words > 19968 || (head_words & 3) || seg_words < 2 * 624)
            return fail(MJMPC_E_BADARG, "head_words must be a multiple of 4 in [19936, 19968], seg_words >= 1248");
        if (n_segments > mjmpc::MT_MAX_SEGMENTS) return fail(MJMPC_E_BADARG, "too many segments (max 64)");
        if (head_words + seg_words * (int64_t)n_segments < mjmpc_mt19937_stream_words(first_normal + n_normals))
            return fail(MJMPC_E_BADARG, "segments do not cover the stream");
    }
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::sample_noise_mt19937<T>((T*)d_noise, (long)n_normals, scale, seed, (const long long*)d_step, d_ws,
                                              d_status, (hipStream_t)stream, d_jump_idx, d_jump_starts, (long)head_words,
                                              (long)seg_words, n_segments, (long)first_normal);
    });
}

int mjmpc_sample_noise(int dtype, void* d_noise, int64_t P, int H, int A, const double* d_chol,
                       const double* d_coeffs, uint64_t seed, uint64_t offset, int64_t particle_offset,
                       const int64_t* d_step, int chol_is_diagonal, void* stream) {
    if (!d_noise || !d_chol) return fail(MJMPC_E_BADARG, "null argument");
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::sample_noise<T>((T*)d_noise, (long)P, H, A, d_chol, d_coeffs, seed, offset, (long)particle_offset,
                                      (const long long*)d_step, (hipStream_t)stream, chol_is_diagonal);
    });
}

int mjmpc_sample_noise_batch(int dtype, int E, void* d_noise, int64_t P, int H, int A, const double* d_chols,
                             const uint64_t* d_seeds, uint64_t offset, const int64_t* d_step, void* stream) {
    if (!d_noise || !d_chols || !d_seeds) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, P, H, A, INT_MAX, __func__)) return rc;
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::sample_noise_batch<T>((T*)d_noise, E, (long)P, H, A, d_chols, (const unsigned long long*)d_seeds, offset,
                                            (const long long*)d_step, (hipStream_t)stream);
    });
}

int mjmpc_sample_noise_cov_batch(int dtype, int E, void* d_noise, int64_t P, int H, int A, const double* d_chols,
                                 const double* d_coeffs, const uint64_t* d_seeds, uint64_t offset, const int64_t* d_step,
                                 int chol_is_diagonal, void* stream) {
    if (!d_noise || !d_chols || !d_seeds) return fail(MJMPC_E_BADARG, "null argument");
    if (int rc = batch_shape(E, P, H, A, 64, __func__)) return rc;
    return with_dtype(dtype, __func__, [&](auto tag) {
        using T = decltype(tag);
        return mjmpc::sample_noise_cov_batch<T>((T*)d_noise, E, (long)P, H, A, d_chols, d_coeffs,
                                                (const unsigned long long*)d_seeds, offset, (const long long*)d_step,
                                                (hipStream_t)stream, chol_is_diagonal);
    });
}

}  // extern "C"
