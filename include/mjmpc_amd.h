/*
 * mjmpc_amd - C ABI of the MI355X-native sampling-MPC rollout engine.
 *
 * This is the drop-in boundary UNDER the Python callables the reference exposes
 * (`set_sim_state_fn(state)`, `rollout_fn(P, H, mean, noise, mode)`, and the controllers'
 * `_update_distribution`).  The reference is pure Python, so a maintainer binds this library with
 * ctypes (INTEGRATION.md shows the stub); mjmpc_amd/_lib.py is that binding for this repo.
 *
 * Conventions
 *   - plain C types only; every `d_*` pointer is a DEVICE pointer on the engine's GPU, laid out
 *     exactly like the reference's C-order float64 numpy arrays unless `dtype` says f32;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous
 *     on that stream unless stated otherwise;
 *   - return value: 0 on success, otherwise a negative MJMPC_E_* code or a positive hipError_t;
 *     mjmpc_last_error() gives a thread-local message.
 */
#ifndef MJMPC_AMD_H
#define MJMPC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a blob / state layout, a buffer size or a signature changes incompatibly; mjmpc_amd/_lib.py refuses a
 * library whose mjmpc_abi_version() differs from the one it was written for.
 *   1: rounds 1-3.
 *   2: round 4 - MJMPC_TREE_BLOB_LEN 3116 -> 3929 (solref / solimp scalars replaced by the table of solver sets, new
 *      field order), MJMPC_TREE_STATE_LEN 70 -> 78 (qpos[40] | qvel[32] | target[3] | 3 reserved), tree set / get state
 *      take qpos[nq], and mjmpc_step_tail writes A + 1 doubles into h_action_mapped (action + completion flag). */
/*   3: round 5 - rollouts emulate MuJoCo's reset on instability (finite costs where version 2 returned +inf;
 *      mjmpc_arm_diverged). */
/*   4: round 6 - mjmpc_{arm,tree}_env_resets (resets of the device-resident REAL env, counted apart from the rollouts'),
 *      mjmpc_{arm,tree}_set_reset_returns (+inf returns for particles that reset, as an engine option);
 *      MJMPC_ARM_BLOB_LEN 229 -> 255 (joint type, friction loss, nu: the arm engine takes slide joints, dry friction and
 *      fewer motors than dofs). */
/*   (entry points that are only ADDED keep the version - every existing caller still works: the episode batches', the
 *      device-resident particle filter's, mjmpc_tree_set_batch_models, mjmpc_tree_set_env_model, the CEM episode batches'
 *      the DMD-MPC episode batches', mjmpc_cost_terms, mjmpc_cost_terms_track / _track_batch, mjmpc_cost_terms_rate /
 *      _rate_batch, mjmpc_cost_terms_quad / _quad_batch, mjmpc_points, mjmpc_points_motion, mjmpc_points_tree and
 *      mjmpc_points_orient.) */
#define MJMPC_ABI_VERSION 4

#define MJMPC_F32 0
#define MJMPC_F64 1

#define MJMPC_E_BADARG (-1)
#define MJMPC_E_BADMODEL (-2)
#define MJMPC_E_NOGPU (-3)

/* Length and layout of the compiled-arm constant block (float64 scalars), produced by
 * mjmpc_amd/models/compile.py::compile_arm and mirrored by mjmpc_amd/csrc/arm_model.h.  Per-link
 * fields are [component][8 lanes]:
 *   off[3][8] axis[3][8] mass[8] com[3][8] inertia[6][8] armature[8] damping[8] range_lo[8]
 *   range_hi[8] limited[8] gear[8] ctrl_lo[8] ctrl_hi[8] dof_invweight0[8] nv timestep frame_skip
 *   site_link site_pos[3] n_sphere sph_link sph_pos[3] sph_r sph_margin sph_invweight plane_n[3]
 *   plane_d sol_K sol_B sol_dmin sol_dmax sol_width sol_mid sol_power gravity[3]
 *   jtype[8] (0 hinge, 1 slide) frictionloss[8] floss_D[8] floss_B nu                           */
#define MJMPC_ARM_BLOB_LEN 255
/* Device state vector of an arm engine: qpos[8] | qvel[8] | target_pos[3]  (float64). */
#define MJMPC_ARM_STATE_LEN 19

typedef struct mjmpc_arm_s* mjmpc_arm_t;

int mjmpc_abi_version(void);
const char* mjmpc_last_error(void);
/* Number of visible HIP devices (0 when there is no GPU / no driver). */
int mjmpc_device_count(void);
/* n_out[0] = kernel nodes, n_out[1] = nodes of any kind of a captured hipGraph_t (a host-side check: the controller
 * compares the captured control iteration with a capture of its own launch tape before it trusts the tape; no reference
 * counterpart). */
int mjmpc_graph_kernel_nodes(void* hip_graph, int64_t* n_out);
/* n_out[0] = an order-independent hash over the graph's kernel nodes of (function, grid, block, dynamic LDS), n_out[1] =
 * the same over all nodes' types: the second half of that check - the tape must launch the same kernels in the same shapes,
 * not merely as many (argument values cannot be read back from a kernel node; they are the recorded ones). */
int mjmpc_graph_signature(void* hip_graph, uint64_t* n_out);

/* ---- arm engine: replaces the SubprocVecEnv worker pool for reacher_7dof-v0 ------------------
 * reference: mjmpc/envs/vec_env/subproc_vec_env.py:91-111 (worker start-up),
 *            mjmpc/envs/gym_env_wrapper.py:16-40 (env construction).                             */
int mjmpc_arm_create(const double* model_blob, int n_blob, int device, mjmpc_arm_t* out);
int mjmpc_arm_destroy(mjmpc_arm_t h);
int mjmpc_arm_dims(mjmpc_arm_t h, int* nv, int* nu, int* d_obs);

/* Dynamics randomization: SubprocVecEnv.randomize_dynamics (subproc_vec_env.py:304-312) gives every
 * worker its own perturbed model (gym_env_wrapper.py:367-416).  Here: n_shards model blocks
 * (float64 [n_shards][MJMPC_ARM_BLOB_LEN], HOST pointer); afterwards particles
 * [k*P/n_shards, (k+1)*P/n_shards) of every rollout use block k (P/n_shards must be a multiple of 8).
 * The single-particle mjmpc_arm_step_state keeps using block 0.  Synchronises the device.        */
int mjmpc_arm_set_shard_models(mjmpc_arm_t h, const double* model_blobs, int n_shards);

/* set_sim_state_fn: SubprocVecEnv.set_env_state (subproc_vec_env.py:235-251) ->
 * Reacher7DOFEnv.set_env_state (mjmpc/envs/basic/reacher_env.py:87-99).  HOST pointers
 * (qpos[nv], qvel[nv], target_pos[3]); copied to the engine's device state on `stream`.         */
int mjmpc_arm_set_state(mjmpc_arm_t h, const double* qpos, const double* qvel, const double* target_pos,
                        void* stream);
/* Per-shard start states: SubprocVecEnv.set_env_state with a list of one state dict per worker
 * (subproc_vec_env.py:242-251).  states = float64 [n_shards][MJMPC_ARM_STATE_LEN] (HOST pointer, layout
 * qpos[8] | qvel[8] | target[3]); afterwards particles of shard k start from states[k] (P / n_shards must
 * be a multiple of 8).  n_shards = 0 returns to the single engine state.                           */
int mjmpc_arm_set_shard_states(mjmpc_arm_t h, const double* states, int n_shards, void* stream);
/* Device pointer to the state vector, for callers that keep the control loop on the GPU.        */
double* mjmpc_arm_state_ptr(mjmpc_arm_t h);

/* rollout_fn: SubprocVecEnv.rollout (subproc_vec_env.py:128-135,161-186) ->
 * GymEnvWrapper.rollout mode="open_loop" (gym_env_wrapper.py:89-156) -> Reacher7DOFEnv.step
 * (reacher_env.py:29-39).  Every particle starts from the engine state.
 *   d_mean     float64 [H][A]                    (always float64: controller state)
 *   d_noise    dtype   [P][H][A]   or NULL      (NULL = mean-only rollout)
 *   d_costs    dtype   [P][H]                    = -reward
 *   d_actions  dtype   [P][H][A]   or NULL      = mean + noise, UNCLIPPED (gym_env_wrapper.py:151)
 *   d_obs      dtype   [P][H][2nv+6] or NULL    observation BEFORE each step
 *   d_next_obs dtype   [P][H][2nv+6] or NULL    observation AFTER each step
 * `dones` are identically zero (reacher_env.py:39) and are not produced.                         */
int mjmpc_arm_rollout(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                      void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream);

/* rollout_fn with mode="closed_loop_linear" (gym_env_wrapper.py:135-136): the nominal action of every
 * step is d_weights^T [obs; 1], obs being the observation before the step; d_weights is float64
 * [(2nv+7)][A] (the reference's `mean` argument in that mode).  Other arrays as in mjmpc_arm_rollout. */
int mjmpc_arm_rollout_cl(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_weights, const void* d_noise,
                         void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream);

/* The same rollout with two optional fusions for a device-resident control iteration:
 *   d_filter_coeffs float64[3] or NULL: d_noise holds RAW samples and the recursive filter of
 *                   control_utils.generate_noise (control_utils.py:32-33) is applied inside the kernel;
 *   d_gseq float64[H] + d_q0 float64[P] (both or neither): d_q0[p] = sum_t gseq[t] * cost[p][t], i.e.
 *                   control_utils.cost_to_go(costs, gamma_seq)[:,0] (control_utils.py:37-46), so the
 *                   update does not have to re-read the costs.  No observations are produced.     */
int mjmpc_arm_rollout_fused(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                            const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                            double* d_q0, void* stream);

/* One Controller.optimize() of MPPI / DMD-MPC without covariance adaptation (controller.py:207-257: generate_rollouts ->
 * _update_distribution -> _get_next_action -> _shift) plus env.step of the closed loop (examples/example_mpc.py:165-168)
 * in TWO launches, for a diagonal action covariance, per-particle softmax weights and no control cost (mppi.py:69-97 with
 * alpha = 1, gaussian_dmd.py:65-104 with update_cov = False):
 *   1. the rollout kernel draws the samples itself - the Philox stream of mjmpc_sample_noise (diag(d_chol) colours it,
 *      d_filter_coeffs float64[3] or NULL filters it as control_utils.py:32-33), keyed by (seed, offset + *d_step_counter,
 *      particle_offset + particle, channel, t) -, keeps its particles' actions in LDS and leaves one softmax record
 *      {max, S, W[H][A]} per workgroup;
 *   2. the finish kernel (H workgroups) merges the records: d_mean_out <- shift((1 - step_size) d_mean + step_size W / S)
 *      (shift_mode 0 'null', 1 'repeat', < 0 none; d_mean_out must NOT alias d_mean, which the launch only reads); the
 *      action (row 0 of the updated mean) goes to d_action_out (device float64[A], may be NULL) and to h_action_slots
 *      (MAPPED PINNED host float64[2][A + 1], may be NULL: slot (*d_step_counter & 1) receives the action and then, as
 *      completion flag, the new step count); *d_step_counter advances; env_step != 0: the engine state advances by one
 *      env step with that action (d_step_cost dtype[1], d_step_next_obs dtype[d_obs], may be NULL).
 *   Sharded runs pass d_record (float64 [2 + H*A]): step 2 then leaves this GPU's record {max, S, W} there and nothing
 *   else (all-gather, then mjmpc_arm_mppi_combine, which also steps the env); d_mean_out is not used.
 * d_gseq float64[H] (gamma_seq, no zero entry).  d_costs / d_actions (dtype [P][H] / [P][H][A]) and d_q0 (float64 [P])
 * are optional outputs.  One model block and one start state only.  shift_mode = -2 issues launch 1 alone (the records
 * stay in the engine): what bench.py times as the dominant kernel.
 * Lifetime / hipGraph rule: every parameter - including the pointer to the engine's per-workgroup record buffer - travels
 * to the two kernels BY VALUE, so a captured graph holds them.  The record buffer only grows and an outgrown buffer stays
 * allocated until mjmpc_arm_destroy, so a graph captured at one (P, H) stays valid after calls at another; a call that
 * would have to GROW the buffer while its stream is capturing returns MJMPC_E_BADARG (call once outside the capture first). */
int mjmpc_arm_mppi_step(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, double* d_mean_out,
                        const double* d_gseq, const double* d_filter_coeffs, const double* d_chol, uint64_t seed,
                        uint64_t offset, int64_t particle_offset, int64_t* d_step_counter, double lam, double step_size,
                        int shift_mode, double* d_action_out, double* h_action_slots, double* d_record, int env_step,
                        void* d_step_cost, void* d_step_next_obs, void* d_costs, void* d_actions, double* d_q0, void* stream);

/* The rollout of mjmpc_arm_mppi_step on its own, for updates other than MPPI's (CEM: cem.py:65-95): the kernel draws its
 * samples itself - the Philox stream of mjmpc_sample_noise keyed by (seed, offset + *d_step_counter, particle_offset +
 * particle, channel, t), coloured by d_chol (chol_full != 0: the whole lower triangle, an adapting full covariance; 0: its
 * diagonal) and filtered by d_filter_coeffs (NULL: none) - and writes costs [P][H] (optional), actions [P][H][A] (optional)
 * and d_q0 float64 [P] = sum_t gseq[t] cost[p][t] (optional).  Graph-capture rule as mjmpc_arm_mppi_step. */
int mjmpc_arm_rollout_sampled(mjmpc_arm_t h, int dtype, int64_t P, int H, const double* d_mean, const double* d_gseq,
                              const double* d_filter_coeffs, const double* d_chol, int chol_full, uint64_t seed, uint64_t offset,
                              int64_t particle_offset, const int64_t* d_step_counter, void* d_costs, void* d_actions,
                              double* d_q0, void* stream);

/* Sharded runs (one rank per GPU): what follows the all-gather of the per-GPU records that mjmpc_arm_mppi_step left
 * (d_record != NULL) - ONE launch that merges the n_records gathered records [max | S | W[H*A]] in rank order (bit-identical
 * on every rank), updates the mean (mppi.py:69-82) into d_mean_out (a buffer of its own) already shifted
 * (olgaussian_mpc.py:116-129), publishes the action into slot (step & 1) of h_action_slots (mapped pinned [2][A+1], value
 * then step count), advances the step counter and, with env_step != 0, steps the device-resident real env.  The
 * parameters travel by value as kernel arguments: a captured graph that holds this launch is valid for as long as the
 * buffers it was given (d_records, d_mean, d_mean_out, the counters, the pinned slots) live. */
int mjmpc_arm_mppi_combine(mjmpc_arm_t h, int dtype, const double* d_records, int n_records, int H, const double* d_mean,
                           double* d_mean_out, int64_t* d_step_counter, double step_size, int shift_mode,
                           double* d_action_out, double* h_action_slots, int env_step, void* d_step_cost,
                           void* d_step_next_obs, void* stream);

/* env.step of the "real" environment kept on the device (examples/example_mpc.py:168 ->
 * Reacher7DOFEnv.step, reacher_env.py:29-39): advances the engine state IN PLACE by one env step
 * under d_action (float64 [A]), writes the step cost (= -reward, dtype[1]) and, if not NULL, the
 * resulting observation (dtype[2nv+6]).                                                          */
int mjmpc_arm_step_state(mjmpc_arm_t h, int dtype, const double* d_action, void* d_cost, void* d_next_obs,
                         void* stream);
/* The engine state read back: qpos[nv], qvel[nv] (host; synchronises the stream), as mjmpc_tree_get_state. */
int mjmpc_arm_get_state(mjmpc_arm_t h, double* qpos, double* qvel, void* stream);
/* Episode batches on the arm engine, as the tree engine's below: E independent closed-loop MPC episodes side by side.  The
 * engine's E = n_state_shards start states (mjmpc_arm_set_shard_states, 1 <= E <= 65535; a batch of one episode sets one
 * shard) are the batch's E real envs.  MJMPC_E_BADARG, before any launch: no state shards; more than one model block
 * (mjmpc_arm_set_shard_models); an extended-joint model (slide joints / friction loss: the tree engine runs those batches).
 * mjmpc_arm_rollout_fused_batch: mjmpc_arm_rollout_fused with one mean per state shard - d_means float64 [E][H][nu];
 * particles [e P_total / E, (e + 1) P_total / E) start from state shard e and follow mean e; P_total % E == 0 and
 * (P_total / E) % 8 == 0 (a particle group never straddles two episodes), d_noise required, d_q0 and d_gseq both or
 * neither.  The launch shape is chosen from the TOTAL grid, as mjmpc_arm_rollout_fused chooses it for P = P_total: each
 * episode's rows are, bit for bit, those rows of a plain launch of all P_total particles under episode e's state and mean. */
int mjmpc_arm_rollout_fused_batch(mjmpc_arm_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                                  const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                                  double* d_q0, void* stream);
/* mjmpc_arm_rollout_fused_batch with the next observations of every (particle, step) as well: d_next_obs dtype
 * [P_total][H][d_obs] or NULL (then it is mjmpc_arm_rollout_fused_batch); episode e's rows carry site - target with state
 * shard e's target.  Costs, actions and q0 are those of mjmpc_arm_rollout_fused_batch, bit for bit. */
int mjmpc_arm_rollout_fused_batch_obs(mjmpc_arm_t h, int dtype, int64_t P_total, int H, const double* d_means,
                                      const void* d_noise, const double* d_filter_coeffs, const double* d_gseq, void* d_costs,
                                      void* d_actions, double* d_q0, void* d_next_obs, void* stream);
/* env.step of every episode's real env in one launch (as mjmpc_arm_step_state per state shard, bit for bit, resets
 * counted as there): d_actions float64 [E][nu], d_costs dtype [E], d_next_obs dtype [E][d_obs] or NULL; every state shard is
 * advanced in place. */
int mjmpc_arm_step_shard_states(mjmpc_arm_t h, int dtype, const double* d_actions, void* d_costs, void* d_next_obs, void* stream);
/* The E state shards read back: qpos [E][nv], qvel [E][nv] (host; synchronises the stream). */
int mjmpc_arm_get_shard_states(mjmpc_arm_t h, double* qpos, double* qvel, void* stream);

/* ---- tree engine: the same worker-pool replacement for models the serial-chain arm engine cannot hold ----------
 * (SURVEY 8f rank 4): a kinematic TREE of up to 32 hinge / slide dofs (the reference's vendored sawyer.xml, swimmer.xml
 * and half_cheetah.xml; a synthetic 24-dof hand, and that hand holding a 6-dof pen): gravity, joint limits and springs,
 * motors or position servos on a subset of the joints, MuJoCo's inertia-box fluid model, up to 16 contact points -
 * sphere- or capsule-end / plane, or sphere / capsule geom-geom pairs - frictionless or with pyramidal friction cones.
 * Reward and observation follow the block's task: 0 = reach (reacher_env.py:29-47, d_obs = 2 nv + 6), 1 = forward
 * progress (swimmer.py:10-24, half_cheetah.py:10-25, d_obs = 2 nv - obs_skip), 2 = reorient an object (the shape of
 * pen-v0's reward, examples/configs/hand/pen-v0.yml:8; d_obs = 2 nv + 6).  Constant block (MJMPC_TREE_BLOB_LEN float64)
 * produced by mjmpc_amd/models/compile_tree.py::compile_tree and mirrored by mjmpc_amd/csrc/tree_model.h; per-link
 * fields are [component][32 lanes], links numbered depth-first:
 *   off[3][32] axis[3][32] mass[32] com[3][32] inertia[6][32] armature damping range_lo range_hi limited gear ctrl_lo
 *   ctrl_hi dof_invweight0 stiffness springref (each [32]) fbox[3][32] frot[9][32] kpg[32] kvg[32] tau0[32] (affine actuator bias at the joint: -gear^2 b1, -gear^2 b2, gear b0; servos: kpg = gear^2 kp)
 *   tau_lo[32] tau_hi[32] (the actuator's forcerange at the joint, +-inf without one) tcoef[32] tpartner[32] tpcoef[32]
 *   (actuators on fixed tendons: the dof's coefficient, the tendon's other dof and its coefficient)
 *   nv timestep frame_skip jumps site_link site_pos[3] n_sphere plane_n[3] plane_d
 *   gravity[3] nu task ctrl_cost obs_skip density viscosity any_friction site_axis[3] target_dir[3]
 *   soltab[8][7] (the model's distinct solver-parameter sets {K, B, dmin, dmax, width, mid, power} - MuJoCo's solref /
 *   solimp after refsafe and clamping; a contact record names its own in slot [21]) dofcls[32] (the dof's limit-row set +
 *   8 * its friction-loss-row set)
 *   spheres[16][24] = {link A, start[3], rA, margin, invweight, mu, capsule axis / segment vector on A [3], depth of
 *   link A in the elimination tree, kind (0 sphere-plane, 1 geom-geom), link B, start on B [3], rB, segment vector on B [3]}
 *   parent subsize anc[5][32] ancmask[2][32] jtype act eparent (parent in the elimination tree of the factorisation)
 *   depth[32] n_rounds elim[31][32]
 *   (elimination lists of the tree-sparse L'DL: the descendants of every link sorted by height, packed
 *   k | distance << 8 | height << 16, -1 ends)
 * Same call shapes and reference counterparts as the arm engine (subproc_vec_env.py:91-111, 128-186, 235-251);
 * target_pos is ignored by task 1.                                                                                  */
#define MJMPC_TREE_BLOB_LEN 3961
/* Round 4, the GENERAL instantiation (block field `gen`; models without these features run the earlier kernels unchanged):
 * ball and free joints (quaternion links: qpos has nq >= nv entries in MuJoCo's layout, d_obs = nq + nv + 6 or nq + nv -
 * obs_skip), joint anchors off the body origin, explicit inertials, box geoms (eight corner points against the plane, one
 * point against a sphere), static geoms of the world body (link -1), friction-loss rows (dof_frictionloss), connect and
 * joint equalities, limits of fixed tendons over one or two joints.  The block then continues
 *   gen nq has_ball frictionloss[32] qadr[32] qoff[32] pext[16][24] qw0[32]
 * (pext: what the new record kinds need beyond spheres[.][24]; layout in csrc/tree_model.h). */
/* A state vector as the C ABI takes it (mjmpc_tree_set_shard_states): MuJoCo's layout, qpos[40] (nq entries used) |
 * qvel[32] | target_pos[3] | 3 reserved (float64). */
#define MJMPC_TREE_STATE_LEN 78
/* The device-resident state vector: one coordinate per link - qpos[32] | qvel[32] | target_pos[3] | site of the fresh
 * observation[3] (filled by mjmpc_tree_rollout_cl) | quaternion w[32] (a ball joint keeps x, y, z in its three links'
 * qpos entries and w here). */
#define MJMPC_TREE_DEVICE_STATE_LEN 102
typedef struct mjmpc_tree_s* mjmpc_tree_t;
int mjmpc_tree_create(const double* model_blob, int n_blob, int device, mjmpc_tree_t* out);
/* The integrator of MJCF <option integrator>: Euler (MuJoCo's semi-implicit mj_Euler, implicit in joint damping; what
 * mjmpc_tree_create makes) or RK4 (mj_RungeKutta with four stages: four forward evaluations per substep, joint damping
 * explicit; models of up to 16 dofs without elliptic friction cones - MJMPC_E_BADMODEL otherwise).  It is not in the
 * model blob, whose layout and length stay as above: the engine is created with it, every launch of the engine (its reset
 * records included) steps with it, and mjmpc_tree_set_shard_models keeps it.  The flat blob of the reference-side
 * physics (RawModel.to_flat) carries no integrator either: the reference oracle simulates Euler only. */
#define MJMPC_INTEGRATOR_EULER 0
#define MJMPC_INTEGRATOR_RK4 1
int mjmpc_tree_create_ex(const double* model_blob, int n_blob, int device, int integrator, mjmpc_tree_t* out);
int mjmpc_tree_destroy(mjmpc_tree_t h);
int mjmpc_tree_dims(mjmpc_tree_t h, int* nv, int* nu, int* d_obs);
/* entries of qpos in MuJoCo's layout (nv + one per ball / free joint); mjmpc_tree_set_state / _get_state take and return
 * qpos[nq], qvel[nv] in that layout */
int mjmpc_tree_nq(mjmpc_tree_t h);
/* SubprocVecEnv.randomize_dynamics for the tree engine (subproc_vec_env.py:304-312, gym_env_wrapper.py:367-416): n_shards
 * model blocks [n_shards][MJMPC_TREE_BLOB_LEN] of the engine's topology; from then on shard i of a rollout (particles
 * [i P / n_shards, (i + 1) P / n_shards), P % n_shards == 0) simulates block i. */
int mjmpc_tree_set_shard_models(mjmpc_tree_t h, const double* model_blobs, int n_shards);
/* set_sim_state_fn (subproc_vec_env.py:235-251), asynchronous on `stream` like mjmpc_arm_set_state (pinned staging ring). */
int mjmpc_tree_set_state(mjmpc_tree_t h, const double* qpos, const double* qvel, const double* target_pos, void* stream);
/* One start state per shard, as mjmpc_arm_set_shard_states (SubprocVecEnv.set_env_state with one dict per worker,
 * subproc_vec_env.py:242-251): states = float64 [n_shards][MJMPC_TREE_STATE_LEN] (HOST pointer, layout qpos[40] | qvel[32] |
 * target[3] | 3 unused, MuJoCo's qpos layout); particles of shard k then start from states[k].  With per-shard models the two shard counts
 * must agree.  n_shards = 0 returns to the single engine state. */
int mjmpc_tree_set_shard_states(mjmpc_tree_t h, const double* states, int n_shards, void* stream);
int mjmpc_tree_rollout(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                       void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream);
/* mjmpc_tree_rollout with the two fusions of mjmpc_arm_rollout_fused (round 4): d_filter_coeffs float64[3] or NULL - d_noise
 * holds RAW samples, filtered inside the kernel (control_utils.py:32-33); d_gseq float64[H] + d_q0 float64[P] (both or
 * neither) - d_q0[p] = sum_t gseq[t] * cost[p][t] = cost_to_go(costs, gamma_seq)[:, 0] (control_utils.py:37-46; +inf for a
 * diverged rollout).  No observations. */
int mjmpc_tree_rollout_fused(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_mean, const void* d_noise,
                             const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                             double* d_q0, void* stream);
/* The "real" environment kept on the device, as mjmpc_arm_step_state (env.step of the reference's closed loop,
 * examples/example_mpc.py:165-168): one env step from the engine's state with d_action (device float64[nu]), the state
 * advanced in place; d_cost dtype[1], d_next_obs dtype[d_obs] or NULL.  mjmpc_tree_get_state reads qpos / qvel back. */
int mjmpc_tree_step_state(mjmpc_tree_t h, int dtype, const double* d_action, void* d_cost, void* d_next_obs, void* stream);
int mjmpc_tree_get_state(mjmpc_tree_t h, double* qpos, double* qvel, void* stream);
/* Episode batches: E independent closed-loop MPC episodes side by side (the reference runs them one after another,
 * examples/job_script.py:80-99 and the episode loop of examples/example_mpc.py).  The engine's E = n_state_shards start
 * states (mjmpc_tree_set_shard_states, 1 <= E <= 65535) are the batch's E real envs; the engine must hold one model block
 * (MJMPC_E_BADARG after mjmpc_tree_set_shard_models with more than one; a batch's per-shard models go through
 * mjmpc_tree_set_batch_models below).
 * mjmpc_tree_rollout_fused_batch: mjmpc_tree_rollout_fused (rollout, gym_env_wrapper.py:125-153) with one mean per state
 * shard - d_means float64 [E][H][nu]; particles [e P_total / E, (e + 1) P_total / E) start from state shard e and follow
 * mean e; P_total % E == 0.  Each episode's particles compute the bits a single-state engine computes for them. */
int mjmpc_tree_rollout_fused_batch(mjmpc_tree_t h, int dtype, int64_t P_total, int H, const double* d_means, const void* d_noise,
                                   const double* d_filter_coeffs, const double* d_gseq, void* d_costs, void* d_actions,
                                   double* d_q0, void* stream);
/* mjmpc_tree_rollout_fused_batch with the next observations of every (particle, step) as well: d_next_obs dtype
 * [P_total][H][d_obs] or NULL (then it is mjmpc_tree_rollout_fused_batch); episode e's rows are those mjmpc_tree_rollout writes
 * on a single-state engine at state e, also under mjmpc_tree_set_batch_models. */
int mjmpc_tree_rollout_fused_batch_obs(mjmpc_tree_t h, int dtype, int64_t P_total, int H, const double* d_means,
                                       const void* d_noise, const double* d_filter_coeffs, const double* d_gseq, void* d_costs,
                                       void* d_actions, double* d_q0, void* d_next_obs, void* stream);
/* env.step of every episode's real env in one launch (examples/example_mpc.py:165-168, as mjmpc_tree_step_state per state
 * shard, bit for bit, resets counted as there): d_actions float64 [E][nu], d_costs dtype [E], d_next_obs dtype [E][d_obs]
 * or NULL; every state shard is advanced in place. */
int mjmpc_tree_step_shard_states(mjmpc_tree_t h, int dtype, const double* d_actions, void* d_costs, void* d_next_obs, void* stream);
/* Dynamics-randomized episode batches (the reference's example_mpc.py --dyn_randomize_config, whose randomized sim_env
 * only does rollouts while the true env stays nominal): n_sets * K model blocks [n_sets][K][MJMPC_TREE_BLOB_LEN] of the
 * engine's topology and kernel instantiation (as mjmpc_tree_set_shard_models checks them), kept apart from the engine's own
 * block, with their reset records.  From then on mjmpc_tree_rollout_fused_batch runs E * K rows: row (e, k) holds the
 * particles [(e K + k) P_total / (E K), (e K + k + 1) P_total / (E K)), starts from state shard e, follows mean e and
 * simulates block [set(e)][k], set(e) = 0 with n_sets = 1 (every episode the same K blocks) and e with n_sets = E = the
 * number of state shards (MJMPC_E_BADARG for any other n_sets); P_total % (E K) == 0, K <= 65535.  Each row computes the bits
 * shard k of a single-state engine with these K blocks (mjmpc_tree_set_shard_models) computes for its particles.
 * mjmpc_tree_step_shard_states keeps stepping the E real envs with the engine's own block.  n_sets = 0 (model_blobs and K
 * ignored) drops the stored blocks: the batch rolls out the engine's own block again.  Synchronises the device. */
int mjmpc_tree_set_batch_models(mjmpc_tree_t h, const double* model_blobs, int n_sets, int K);
/* The model of the device-resident real env: with a block (MJMPC_TREE_BLOB_LEN scalars, checked as above)
 * mjmpc_tree_step_state steps the engine's state with it and its own reset record instead of shard 0's block - after
 * mjmpc_tree_set_shard_models the reference's pairing of a randomized sim_env with a nominal true env; an env step captured
 * in a hipGraph AFTER this call does the same (one captured before keeps the block it was captured with, which stays
 * allocated).  NULL restores the default, shard 0's block.  Rollouts are not affected. */
int mjmpc_tree_set_env_model(mjmpc_tree_t h, const double* model_blob);
/* The E state shards read back in MuJoCo's layout (quaternions included): qpos [E][nq], qvel [E][nv] (host; synchronises
 * the stream), as mjmpc_tree_get_state for the single state. */
int mjmpc_tree_get_shard_states(mjmpc_tree_t h, double* qpos, double* qvel, void* stream);
/* rollout(mode="closed_loop_linear") (gym_env_wrapper.py:135-136) as mjmpc_arm_rollout_cl: d_weights float64 [(d_obs + 1)][nu],
 * the nominal action of a step is weights' [observation the step starts from; 1]. */
int mjmpc_tree_rollout_cl(mjmpc_tree_t h, int dtype, int64_t P, int H, const double* d_weights, const void* d_noise,
                          void* d_costs, void* d_actions, void* d_obs, void* d_next_obs, void* stream);
int mjmpc_tree_solver_failures(mjmpc_tree_t h, uint32_t* count);
/* Resets since create: particle-substeps in which MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc [EXT] would have found a NaN
 * or an entry beyond mjMAXVAL = 1e10 in qpos / qvel / qacc and called mj_resetData (the rollouts of
 * mjmpc/envs/gym_env_wrapper.py:125-153 run through mj_step).  The kernels do what MuJoCo does: the particle goes on from
 * qpos0 with zero velocity, and with zero controls until its env step ends (mj_resetData zeroes data.ctrl, which
 * do_simulation wrote once before its frame_skip substeps), so its costs stay finite.  Not counted by
 * mjmpc_*_solver_failures.  (Since ABI version 3; before, such particles carried a +inf return.) */
int mjmpc_tree_diverged(mjmpc_tree_t h, uint32_t* count);
int mjmpc_arm_diverged(mjmpc_arm_t h, uint32_t* count);
/* The resets among them that happened to the REAL env kept on the device (mjmpc_*_step_state, the env step inside
 * mjmpc_arm_mppi_step / mjmpc_arm_mppi_combine): there the reference does not go on silently - mujoco-py's default warning
 * callback raises MujocoException out of sim.step() in the worker that steps the env (mjmpc/envs/gym_env_wrapper.py:
 * 64-66 -> reacher_env.py:29-39).  The host side (the engines' check_env_resets, mjmpc_amd/envs/_resets.py) reads this counter where it
 * synchronises anyway and raises / warns.  Since ABI version 4. */
int mjmpc_tree_env_resets(mjmpc_tree_t h, uint32_t* count);
int mjmpc_arm_env_resets(mjmpc_arm_t h, uint32_t* count);
/* inf_returns != 0: a rollout particle that resets costs +inf from that env step on (its return +inf: no weight in the
 * softmax updates, last in the elite ranking) instead of the finite costs of MuJoCo's reset state - a blown-up particle whose
 * reset pose happens to be cheap cannot pull the mean towards the action sequence that blew it up.  Default 0 (what the
 * reference's workers return).  Applies to launches issued afterwards; captured launchers keep what they were made with.
 * Since ABI version 4. */
int mjmpc_tree_set_reset_returns(mjmpc_tree_t h, int inf_returns);
int mjmpc_arm_set_reset_returns(mjmpc_arm_t h, int inf_returns);

/* rollout_fn over the reference's two analytic numpy envs (stateless; every pointer is a device
 * pointer): kind 0 = PendulumEnv (mjmpc/envs/basic/pendulum.py:33-50; d_params = [max_speed,
 * max_torque, dt, g, m, l], d_state = [th, thdot], observations have 3 entries), kind 1 = LQREnv
 * (mjmpc/envs/basic/lqr.py:31-35; d_params = [A | B | Q | R] row-major, d_state = x[n_state],
 * n_state, n_action <= 8).  Arrays as in mjmpc_arm_rollout (costs = -reward).  closed_loop_linear != 0:
 * d_mean is the (d_obs+1, n_action) weight matrix of mode "closed_loop_linear"
 * (mjmpc/envs/gym_env_wrapper.py:135-136), action = W^T [obs; 1] + noise.                          */
#define MJMPC_ENV_PENDULUM 0
#define MJMPC_ENV_LQR 1
int mjmpc_analytic_rollout(int kind, const double* d_params, int n_state, int n_action, const double* d_state, int dtype,
                           int64_t P, int H, const double* d_mean, const void* d_noise, void* d_costs, void* d_actions,
                           void* d_obs, void* d_next_obs, int closed_loop_linear, void* stream);

/* Number of (particle, substep) constraint solves whose active set had not settled after the
 * iteration cap since engine creation (synchronises the device).  0 in every test.               */
int mjmpc_arm_solver_failures(mjmpc_arm_t h, uint32_t* count);

/* ---- the exchange of a sharded run, issued from the library ---------------------------------------
 * reference: SubprocVecEnv gathers its workers' results through pipes (mjmpc/envs/vec_env/subproc_vec_env.py:161-186); here
 * each rank (one process per GPU) contributes one small float64 record per control iteration and every rank combines the
 * gathered records identically.  The all-gather is RCCL's, on the iteration's stream; issuing it through this
 * ABI instead of torch.distributed makes the sharded iteration a sequence of LIBRARY calls, which runs from the launch tape
 * / as direct launches like the one-GPU loop (no hipGraph replay gap).  RCCL is bound at run time (dlopen of the copy the
 * process already holds); without it these entries fail with MJMPC_E_NOGPU and callers keep torch.distributed.
 *   mjmpc_comm_unique_id   rank 0: 128 opaque bytes (ncclGetUniqueId) to hand to every rank by any means
 *   mjmpc_comm_create      every rank, collectively (ncclCommInitRank) on HIP device `device`
 *   mjmpc_comm_all_gather_f64   d_recv[world][count] <- every rank's d_send[count] (device pointers; may be captured)  */
#define MJMPC_COMM_ID_BYTES 128
typedef struct mjmpc_comm_s* mjmpc_comm_t;
int mjmpc_comm_unique_id(void* id_out);
int mjmpc_comm_create(const void* id_bytes, int world_size, int rank, int device, mjmpc_comm_t* out);
int mjmpc_comm_all_gather_f64(mjmpc_comm_t c, const double* d_send, double* d_recv, int64_t count, void* stream);
int mjmpc_comm_destroy(mjmpc_comm_t c);

/* ---- sampling-distribution updates: the device side of Controller._update_distribution --------
 * All functions below are stateless; `d_ws` is a caller-owned device workspace of at least
 * mjmpc_update_workspace_bytes(P, H, A) bytes that carries intermediate results between the
 * calls of one update (per-particle costs, elite flags).  P is the number of particles ON THIS
 * GPU.  "Records" are small float64 vectors designed to be all-gathered across GPUs (one
 * collective per control iteration) and combined identically on every rank:
 *   softmax record  [ xmax[Hw] | S[Hw] | W[H*A] | C[A*A] ]   Hw = time_based_weights ? H : 1
 *   CEM sum record  [ n_elite_local | sum over local elites of actions[H*A] ]
 *   CEM cov record  [ sum over local elites and t of (d - dbar)(d - dbar)^T  [A*A] ]
 *   RS record       [ min q0 | global particle index | actions[H*A] of that particle ]
 * d_gseq is Controller.gamma_seq (controller.py:71) as float64[H]; gamma_zero = any(gseq == 0)
 * (control_utils.cost_to_go returns its input unchanged in that case, control_utils.py:41-42).
 * Diverged rollouts: for every entry below a return (cost-to-go or d_q0) that is not finite - +inf, -inf, NaN of either sign -
 * means zero weight / ranked last, so the result is the update over the particles with a finite return, also where a whole
 * workgroup's block, a whole record or a whole merge slice has none (a record without a finite return is {-inf, 0, 0...}).
 * A row or run with NO finite return is outside that promise: the softmax entries give it a NaN mean, as the plain
 * arithmetic does, the selections particle 0 / the first k by index; in a batch it leaves the other rows alone.        */
int64_t mjmpc_update_workspace_bytes(int64_t P, int H, int A);
int mjmpc_softmax_record_len(int H, int A, int time_based_weights);

/* cost_to_go (mjmpc/utils/control_utils.py:37-46) of the local particles, [:,0] column, left in
 * the workspace for the CEM / random-shooting calls; mjmpc_workspace_q0 returns its device address. */
int mjmpc_traj_cost(int dtype, int64_t P, int H, int A, const void* d_costs, const double* d_gseq, int gamma_zero,
                    void* d_ws, void* stream);
double* mjmpc_workspace_q0(void* d_ws, int64_t P, int H, int A);

/* MPPIQ.calculate_returns + _control_costs (mjmpc/control/mppiq.py:104-136): TD(lambda) returns
 * d_returns (dtype [P][H]) from the per-step costs (+ beta * per-step control cost when alpha == 0; then
 * d_actions, d_mean, d_covinv are read) and the optional Q estimates d_qvals (dtype [P][H]; NULL = the
 * reference's default: zero except the last step's own cost).  d_wseq (float64 [H-1]) =
 * cumprod(1, gamma*td_lam, ...) (mppiq.py:120); wseq_has_zero selects cost_to_go's pass-through branch
 * (control_utils.py:39-40).  Feed d_returns to mjmpc_softmax_stats with gamma_zero = 1, alpha = 1.   */
int mjmpc_td_lambda_returns(int dtype, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                            const void* d_qvals, const double* d_mean, const double* d_covinv, const double* d_wseq,
                            int wseq_has_zero, double beta, int alpha, double gamma, double td_lam, void* d_returns,
                            void* d_ws, void* stream);

/* MPPI._exp_util + _control_costs (mjmpc/control/mppi.py:84-111), DMDMPC._exp_util
 * (gaussian_dmd.py:94-104), PFMPC._exp_util (particle_filter_controller.py:104-113): exponentiated
 * cost weights reduced to this GPU's softmax record.  d_covinv (float64 [A][A]) is read only when
 * alpha == 0 (control cost on); want_cov adds the weighted scatter C used by DMD-MPC.             */
int mjmpc_softmax_stats(int dtype, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                        const double* d_mean, const double* d_covinv, const double* d_gseq, int gamma_zero,
                        double lam, int alpha, int time_based_weights, int want_cov, double* d_record, void* d_ws,
                        void* stream);
/* MPPI._update_distribution (mppi.py:69-82) / DMDMPC._update_distribution (gaussian_dmd.py:65-91)
 * / _calc_val (mppi.py:113-131, gaussian_dmd.py:126-139) from G gathered records.
 * cov_mode: 0 leave cov, 1 diagonal update, 2 full update.  d_cov, d_value, d_wnorm may be NULL;
 * d_wnorm receives {global max, global normaliser} for mjmpc_softmax_weights.                     */
int mjmpc_softmax_combine(const double* d_records, int G, int H, int A, int time_based_weights, double lam,
                          double step_size, int cov_mode, double P_total, double* d_mean, double* d_cov,
                          double* d_value, double* d_wnorm, void* stream);
/* normalised per-particle weights (PFMPC resampling input), float64 [P] */
int mjmpc_softmax_weights(int64_t P, int H, int A, const double* d_wnorm, void* d_ws, double* d_weights,
                          void* stream);

/* CEM._update_distribution (mjmpc/control/cem.py:63-86) in three steps.  Elite = the k particles
 * with the smallest (q0, global index); d_q_all is the all-gathered q0 of every GPU (NULL = this
 * GPU holds all particles; `offset` is then ignored) and `offset` the global index of local particle 0.
 * The local elite rows are kept as a list in d_ws, which mjmpc_cem_elite_cov reads: call them in this order
 * on the same workspace.                                                                             */
int mjmpc_cem_elite_sums(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_q_all,
                         int64_t P_all, int64_t offset, int64_t k, double* d_sum_record, void* d_ws, void* stream);
int mjmpc_cem_elite_cov(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_mean,
                        const double* d_sum_records, int G, double* d_cov_record, void* d_ws, void* stream);
int mjmpc_cem_final(const double* d_cov_records, int G, int64_t P, int H, int A, double n_elite, int full_cov,
                    double step_size, double* d_mean, double* d_cov, void* d_ws, void* stream);
/* The sharded form with ONE record exchange after the q0 gather (two collectives per iteration): each GPU
 * calls mjmpc_cem_elite_sums, then mjmpc_cem_elite_cov with ITS OWN sum record (G = 1: scatter about its own mean
 * delta) and all-gathers  rec_g = { sum record [1 + H*A] | cov record [A*A] };  this call pools them (pairwise-
 * variance identity; exactly the two-pass np.cov / np.var of cem.py:76-80 when G = 1) and updates mean and cov.   */
int mjmpc_cem_combine(const double* d_records, int G, int H, int A, double n_elite, int full_cov, double step_size,
                      double* d_mean, double* d_cov, void* stream);

/* The fused CEM step (round 4; cem.py:65-95 in two launches beside the rollout instead of nine):
 *   mjmpc_cem_select_moments  the elite threshold (k-th smallest q0, ties by particle index, exactly as
 *       mjmpc_cem_elite_sums), the elite list, and per workgroup {rows, sum of elite action rows, scatter of their deltas
 *       about a provisional centre} - every workgroup repeats the selection and takes a slice of the elite rows; it also
 *       snapshots mean, cov and *d_step_counter for the finish launch.  q0 is read from d_ws (mjmpc_workspace_q0) or,
 *       sharded, from the gathered d_q_all [P_all] with this GPU's block at `offset`;
 *   mjmpc_cem_record          (sharded runs) the partials -> this GPU's record {n | sum a [H*A] | scatter about its own
 *       mean [A*A]}, the layout mjmpc_cem_combine pools; all-gather it;
 *   mjmpc_cem_finish          d_records == NULL: one GPU, the partials in d_ws; else the G gathered records.  New mean and
 *       covariance (np.var ddof 0 / np.cov ddof 1 over the H k elite deltas, step-size blend), cov += grow_scale *
 *       diag(d_grow_diag) (CEM._shift, cem.py:94; NULL: identity), its lower Cholesky factor -> d_chol (may be NULL;
 *       positive semi-definite input as mjmpc_cholesky_lower, *d_status = 1 if indefinite), the action (row 0 of the new
 *       mean) -> d_action_out / h_action_pinned (mapped pinned, A + 1 doubles, may be NULL: the action, then - behind a
 *       system-scope fence - the new step count as a completion flag the host can poll while the launch is still
 *       drawing), the horizon shift (0 'null', 1 'repeat', < 0 none), *d_step_counter = snapshot + 1, and - d_next_noise != NULL - the RAW Philox samples of the next
 *       control step, [P][H][A] of dtype, coloured by the new factor: the stream of mjmpc_sample_noise(..., filter NULL,
 *       seed, offset, particle_offset, d_step_counter), sample for sample.
 * mjmpc_cem_fused_supported: A <= 8, A <= H + 1, P_all <= 32768, the moment tiles fit the workspace (else use the
 * separate entries above).  Same workspace for the three calls; d_mean / d_cov as given to the first. */
int mjmpc_cem_fused_supported(int64_t P_all, int64_t P, int64_t k, int H, int A);
int mjmpc_cem_select_moments(int dtype, int64_t P, int H, int A, const void* d_actions, const double* d_q_all, int64_t P_all,
                             int64_t offset, int64_t k, const double* d_mean, const double* d_cov,
                             const int64_t* d_step_counter, void* d_ws, void* stream);
int mjmpc_cem_record(int64_t P, int H, int A, int64_t k, const double* d_mean, double* d_record, void* d_ws, void* stream);
int mjmpc_cem_finish(int dtype, int64_t P, int H, int A, int64_t k, const double* d_records, int G, double n_elite,
                     int full_cov, double step_size, int shift_mode, double* d_mean, double* d_cov, double* d_chol,
                     int* d_status, const double* d_grow_diag, double grow_scale, double* d_action_out,
                     double* h_action_pinned, int64_t* d_step_counter, void* d_next_noise, uint64_t seed, uint64_t offset,
                     int64_t particle_offset, void* d_ws, void* stream);

/* RandomShooting._update_distribution (mjmpc/control/random_shooting.py:52-62). */
int mjmpc_rs_best(int dtype, int64_t P, int H, int A, const void* d_actions, int64_t offset, double* d_record,
                  void* d_ws, void* stream);
int mjmpc_rs_combine(const double* d_records, int G, int H, int A, double step_size, double* d_mean, void* stream);

/* MPPI._update_distribution (mppi.py:69-82, time_based_weights off, alpha == 1) + the action read-out
 * (olgaussian_mpc.py:71) + OLGaussianMPC._shift (olgaussian_mpc.py:116-129) in two launches.
 * d_q0: float64[P] cost-to-go (NULL = the one mjmpc_traj_cost left in d_ws).  shift_mode: -1 none,
 * 0 'null', 1 'repeat'.  d_action_out (float64[A]), d_record ([xmax | S | W[H*A]], the softmax record
 * without its covariance block) and d_value (_calc_val, mppi.py:113-131) may be NULL.  For a captured
 * control iteration: *d_step_counter (device int64) is incremented (the noise stream index of the next step),
 * and h_action_mapped (device-visible pinned host memory, float64[A+1]) also receives the action followed by
 * the new step count, written last behind a system-scope fence: a host polling entry [A] can read the action
 * as soon as this kernel has produced it, while later work of the same stream is still running.            */
int mjmpc_mppi_fused_update(int dtype, int64_t P, int H, int A, const double* d_q0, const void* d_actions, double lam,
                            double step_size, int shift_mode, double* d_mean, double* d_action_out, double* d_record,
                            double* d_value, double* h_action_mapped, int64_t* d_step_counter, void* d_ws,
                            void* stream);

/* The same, and in the same two launches the RAW samples of the next control step are drawn into d_next_noise
 * (dtype [P][H][A], unfiltered: mjmpc_arm_rollout_fused filters on the fly) - extra workgroups of the first
 * launch, as mjmpc_sample_noise(dtype, d_next_noise, P, H, A, d_chol, NULL, seed, offset, particle_offset,
 * d_step, chol_is_diagonal) would draw them.  The rollout that read d_next_noise has finished by then, and
 * *d_step still holds the current step when it is read (the counter moves in the second launch), so `offset`
 * is normally 1.  Saves the sampler's own launch on the critical path of a captured control iteration.     */
int mjmpc_mppi_fused_update_draw_next(int dtype, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                                      double lam, double step_size, int shift_mode, double* d_mean,
                                      double* d_action_out, double* d_record, double* d_value, double* h_action_mapped,
                                      int64_t* d_step_counter, void* d_ws, void* d_next_noise, const double* d_chol,
                                      uint64_t seed, uint64_t offset, int64_t particle_offset, const int64_t* d_step,
                                      int chol_is_diagonal, void* stream);

/* Episode batches: E independent MPPI updates (mppi.py:69-82 + olgaussian_mpc.py:71 + olgaussian_mpc.py:116-129, one per
 * episode of the reference's episode loop, examples/job_script.py:80-99) in two launches, grid row e = episode e.  Each row
 * is exactly mjmpc_mppi_fused_update of P particles: d_q0 float64 [E][P], d_actions dtype [E][P][H][A], d_lam and
 * d_step_size float64 [E] (device), d_means float64 [E][H][A] (updated and shifted in place), d_actions_out float64 [E][A]
 * (may be NULL); *d_step_counter (may be NULL) is incremented once - the episodes advance together.  d_ws: at least
 * mjmpc_update_batch_workspace_bytes(E, P, H, A) bytes.  1 <= E <= 65535. */
int64_t mjmpc_update_batch_workspace_bytes(int E, int64_t P, int H, int A);
int mjmpc_mppi_fused_update_batch(int dtype, int E, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                                  const double* d_lam, const double* d_step_size, int shift_mode, double* d_means,
                                  double* d_actions_out, int64_t* d_step_counter, void* d_ws, void* stream);

/* Episode batches of the fused CEM step: E independent CEM updates (cem.py:65-95, one per episode of the reference's
 * episode loop) in the same two launches, grid row e = episode e, no host synchronisation.
 *   mjmpc_cem_select_moments_batch  row e is exactly mjmpc_cem_select_moments on one GPU (d_q_all == NULL) for its P
 *       particles with k = d_k[e] (device int64 [E]): the k-th smallest (q0, particle index) threshold, the elite list and
 *       the per-workgroup partials, with the slice sizes and the merge order of the single launch of P particles; and the
 *       snapshots of ITS mean and covariance and of *d_step_counter.  d_actions dtype [E][P][H][A], d_q0 float64 [E][P],
 *       d_means float64 [E][H][A], d_covs float64 [E][A][A].
 *   mjmpc_cem_finish_batch          row e is exactly mjmpc_cem_finish with d_records == NULL, G = 1, n_elite = d_k[e],
 *       step size d_step_size[e], growth d_grow_scale[e] * diag(d_grow_diag[e]) (float64 [E][A] / [E]; NULL: identity /
 *       no growth), factor -> d_chols [E][A][A] (may be NULL), d_status[e] = 1 (int [E], sticky, may be NULL) if row e's
 *       covariance is indefinite or not finite, action -> d_actions_out [E][A] (may be NULL), horizon shift, and -
 *       d_next_noise != NULL - row e's RAW Philox samples of the next step, sample for sample the stream of
 *       mjmpc_sample_noise(dtype, d_next_noise + e P H A, P, H, A, d_chols + e A A, NULL, d_seeds[e], offset, 0,
 *       d_step_counter, 0).  *d_step_counter (may be NULL) is advanced once, by row 0; every row takes the step from the
 *       snapshot the select launch made, never from the counter.
 * The host sees k only through d_k, so the workspace - mjmpc_cem_batch_workspace_bytes(E, P, k_max, H, A) bytes, the same
 * d_ws for both calls - holds any 1 <= d_k[e] <= P (k_max is validated, not a size); a row with d_k[e] outside that range
 * is left untouched and flagged in d_status[e].  mjmpc_cem_batch_supported(E, P, k_max, H, A): 1 <= E <= 65535,
 * 1 <= k_max <= P, and mjmpc_cem_fused_supported(P, P, k, H, A) for every row (A <= 8, A <= H + 1, P <= 32768). */
int mjmpc_cem_batch_supported(int E, int64_t P, int64_t k_max, int H, int A);
int64_t mjmpc_cem_batch_workspace_bytes(int E, int64_t P, int64_t k_max, int H, int A);
int mjmpc_cem_select_moments_batch(int dtype, int E, int64_t P, int H, int A, const void* d_actions, const double* d_q0,
                                   const int64_t* d_k, const double* d_means, const double* d_covs,
                                   const int64_t* d_step_counter, void* d_ws, void* stream);
int mjmpc_cem_finish_batch(int dtype, int E, int64_t P, int H, int A, const int64_t* d_k, int full_cov,
                           const double* d_step_size, int shift_mode, double* d_means, double* d_covs, double* d_chols,
                           int* d_status, const double* d_grow_diag, const double* d_grow_scale, double* d_actions_out,
                           int64_t* d_step_counter, void* d_next_noise, const uint64_t* d_seeds, uint64_t offset, void* d_ws,
                           void* stream);

/* Episode batches of DMD-MPC's covariance-adapting step (gaussian_dmd.py:65-113 with update_cov, one per episode of the
 * reference's episode loop): grid row e = episode e, no host synchronisation, nothing exchanged between rows.
 *   mjmpc_cholesky_lower_batch    row e is exactly mjmpc_cholesky_lower(d_covs + e A A, A, d_chols + e A A, d_status + e) on
 *       its block: d_covs / d_chols float64 [E][A][A]; d_status int [E] (may be NULL), d_status[e] = 1 if row e's covariance
 *       is indefinite or not finite - sticky, and only that row's.  One launch.  A <= 64.
 *   mjmpc_sample_noise_cov_batch  row e is exactly mjmpc_sample_noise(dtype, d_noise + e P H A, P, H, A, d_chols + e A A,
 *       d_coeffs, d_seeds[e], offset, 0, d_step, chol_is_diagonal) on its slice: d_noise dtype [E][P][H][A], d_seeds uint64
 *       [E] (device), one step counter d_step (may be NULL) and one d_coeffs (float64 [3]; NULL leaves the samples raw) for
 *       all rows.  The draw is one launch of the kernel mjmpc_sample_noise would pick (all channels of a (particle, t-quad)
 *       per thread for a general factor with A <= 8, per element above that and for chol_is_diagonal), the filter a second
 *       launch over the E P particles - per (particle, channel), the instructions of the single pass.
 *   mjmpc_dmd_update_batch        row e is exactly mjmpc_softmax_stats(dtype, P, H, A, d_costs + e P H, d_actions + e P H A,
 *       d_means + e H A, NULL, d_gseq, gamma_zero = 0, d_lam[e], alpha = 1, time_based_weights = 0, want_cov = 1, record,
 *       ws), then mjmpc_softmax_combine(record, G = 1, H, A, 0, d_lam[e], d_step_size[e], cov_mode, P, d_means + e H A,
 *       d_covs + e A A, NULL, NULL), then mjmpc_step_tail(d_means + e H A, H, A, shift_mode, NULL, d_actions_out + e A, NULL,
 *       counter, d_covs + e A A, NULL, d_beta[e]) on its slices: the same 16 particles per partial, the same merge tree
 *       over the ceil(P / 16) partials, the same combine with one record, the covariance scatter about the mean from before
 *       the update.  d_costs dtype [E][P][H], d_actions dtype [E][P][H][A], d_gseq float64 [H] without zeros, d_lam (> 0:
 *       only the host can check it), d_step_size and d_beta float64 [E] (device), cov_mode 1 (diagonal) or 2 (full),
 *       shift_mode 0 'null' or 1 'repeat', d_means float64 [E][H][A] and d_covs float64 [E][A][A] (updated in place; the means
 *       shifted, the covariances grown by d_beta[e] I), d_actions_out float64 [E][A] (may be NULL).  *d_step_counter (may be
 *       NULL) is advanced once, by row 0 of the last launch; no row reads it.  Three launches (cost-to-go weights + their
 *       maximum; partial moments; record + combine + tail).  d_ws: mjmpc_dmd_batch_workspace_bytes(E, P, H, A) bytes, 8-byte
 *       aligned (negative for bad sizes).
 * 1 <= E <= 65535, A <= 64 (MJMPC_E_BADARG otherwise). */
int mjmpc_cholesky_lower_batch(int E, const double* d_covs, int A, double* d_chols, int* d_status, void* stream);
int mjmpc_sample_noise_cov_batch(int dtype, int E, void* d_noise, int64_t P, int H, int A, const double* d_chols,
                                 const double* d_coeffs, const uint64_t* d_seeds, uint64_t offset, const int64_t* d_step,
                                 int chol_is_diagonal, void* stream);
int64_t mjmpc_dmd_batch_workspace_bytes(int E, int64_t P, int H, int A);
int mjmpc_dmd_update_batch(int dtype, int E, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                           const double* d_gseq, const double* d_lam, const double* d_step_size, int cov_mode,
                           const double* d_beta, int shift_mode, double* d_means, double* d_covs, double* d_actions_out,
                           int64_t* d_step_counter, void* d_ws, void* stream);

/* Episode batches of the MPPIQ step (mppiq.py:73-136 without Q estimates, one per episode of the reference's episode loop):
 * three launches, grid row e = episode e, no host synchronisation.  Row e is exactly mjmpc_td_lambda_returns(dtype, P, H, A,
 * d_costs + e P H, d_actions + e P H A, NULL, d_means + e H A, d_covinv + e A A, d_wseq + e max(H-1, 1), d_wseq_has_zero[e],
 * d_beta[e], alpha, gamma, d_td_lam[e], returns, ws), then mjmpc_softmax_stats(dtype, P, H, A, returns, d_actions + e P H A,
 * d_means + e H A, NULL, any d_gseq, gamma_zero = 1, d_beta[e], alpha = 1, time_based_weights, want_cov = 0, record, ws), then
 * mjmpc_softmax_combine(record, G = 1, H, A, time_based_weights, d_beta[e], d_step_size[e], cov_mode = 0, P, d_means + e H A,
 * NULL, NULL, NULL), then mjmpc_step_tail(d_means + e H A, H, A, shift_mode, NULL, d_actions_out + e A, NULL, counter, NULL,
 * NULL, 0) on its slices: the returns rounded to dtype before the weights read them, the same 16 particles per partial, the
 * same merge tree over the ceil(P / 16) partials, the same combine with one record and H weight columns (time_based_weights)
 * or one.  d_costs dtype [E][P][H], d_actions dtype [E][P][H][A], d_beta (> 0: only the host can check it), d_step_size and
 * d_td_lam float64 [E] (device), d_wseq float64 [E][max(H-1, 1)] = cumprod(1, gamma d_td_lam[e], ...) per row and
 * d_wseq_has_zero int [E] (device), alpha 0 (control cost on: d_covinv float64 [E][A][A] is read) or 1 (d_covinv may be NULL),
 * shift_mode 0 'null' or 1 'repeat', d_means float64 [E][H][A] (updated and shifted in place), d_actions_out float64 [E][A]
 * (may be NULL).  *d_step_counter (may be NULL) is advanced once, by row 0 of the last launch; no row reads it.  Launches:
 * returns + weights + their column maxima; partial moments; record + combine + tail.
 * mjmpc_mppiq_batch_supported: 1 <= E <= 65535, P >= 1, H >= 1, 1 <= A <= 64 (the tail's limit) and, with time_based_weights,
 * H <= 512 (the partial launch's 8 * 16 * H bytes of LDS within 64 KB).  d_ws: mjmpc_mppiq_batch_workspace_bytes(E, P, H, A,
 * time_based_weights) bytes, 8-byte aligned (negative for unsupported sizes).  MJMPC_E_BADARG otherwise, before any launch. */
int mjmpc_mppiq_batch_supported(int E, int64_t P, int H, int A, int time_based_weights);
int64_t mjmpc_mppiq_batch_workspace_bytes(int E, int64_t P, int H, int A, int time_based_weights);
int mjmpc_mppiq_update_batch(int dtype, int E, int64_t P, int H, int A, const void* d_costs, const void* d_actions,
                             const double* d_beta, const double* d_step_size, const double* d_td_lam, const double* d_wseq,
                             const int* d_wseq_has_zero, double gamma, int alpha, const double* d_covinv,
                             int time_based_weights, int shift_mode, double* d_means, double* d_actions_out,
                             int64_t* d_step_counter, void* d_ws, void* stream);

/* Episode batches of the random-shooting step (random_shooting.py:52-62, one per episode of the reference's episode loop):
 * one launch, grid row e = episode e, no host synchronisation, no workspace.  Row e is mjmpc_rs_best(dtype, P, H, A,
 * d_actions + e P H A, 0, record, ws) on the cost-to-go d_q0 + e P, then mjmpc_rs_combine(record, 1, H, A, d_step_size[e],
 * d_means + e H A), then mjmpc_step_tail(d_means + e H A, H, A, shift_mode, NULL, d_actions_out + e A, NULL, counter, NULL,
 * NULL, 0): the particle with the first minimum of its cost-to-go (numpy.argmin: ties go to the lowest index), mean <-
 * (1 - step) mean + step * its actions, the action read-out and the horizon shift.  A row without a finite cost-to-go
 * selects particle 0, as numpy.argmin does for a row of +inf (and as the single calls do).  d_q0 float64 [E][P] (a value that
 * is not finite compares as +inf), d_actions dtype [E][P][H][A], d_step_size float64 [E] (device), shift_mode 0 'null' or 1 'repeat', d_means float64
 * [E][H][A] (updated and shifted in place), d_actions_out float64 [E][A] (may be NULL), d_best int64 [E] (may be NULL): the
 * selected particle of every row.  *d_step_counter (may be NULL) is advanced once, by row 0; no row reads it.
 * mjmpc_rs_batch_supported(E, P, H, A): 1 <= E <= 65535, P >= 1, H >= 1, 1 <= A <= 256 (MJMPC_E_BADARG otherwise). */
int mjmpc_rs_batch_supported(int E, int64_t P, int H, int A);
int mjmpc_rs_update_batch(int dtype, int E, int64_t P, int H, int A, const double* d_q0, const void* d_actions,
                          const double* d_step_size, int shift_mode, double* d_means, double* d_actions_out,
                          int64_t* d_step_counter, int64_t* d_best, void* stream);

/* Sharded MPPI: the G all-gathered records d_records (float64 [G][2 + H*A], as left in d_record by
 * mjmpc_mppi_fused_update with step_size 0, shift_mode -1) merged in rank order -> mean update, action read-out,
 * shift, step counter and the mapped host copy with its completion flag, exactly as the single-GPU call does
 * (P_total = particles over all ranks; every rank computes the bit-identical result).                      */
int mjmpc_mppi_fused_combine(const double* d_records, int G, double P_total, int H, int A, double lam, double step_size,
                             int shift_mode, double* d_mean, double* d_action_out, double* d_value,
                             double* h_action_mapped, int64_t* d_step_counter, void* stream);

/* sum of q0 over local particles (CEM / RandomShooting _calc_val: cem.py:107-112) -> d_out[0] */
int mjmpc_q0_sum(int64_t P, int H, int A, double* d_out, void* d_ws, void* stream);

/* OLGaussianMPC._shift (mjmpc/control/olgaussian_mpc.py:116-129).  mode 0 'null', 1 'repeat',
 * 2 the appended row is read from d_row ('random': drawn by the host from np.random).            */
int mjmpc_shift_mean(double* d_mean, int H, int A, int mode, const double* d_row, void* stream);
/* The tail of Controller.optimize (controller.py:240-257: `_get_next_action`, `num_steps += 1`, `_shift`) in ONE launch
 * for device-resident controllers: d_action_out (float64 [A]) / h_action_mapped (float64 [A + 1], mapped pinned host
 * memory: the action, then - behind a system-scope fence - the new step count as a completion flag; 0 without a
 * counter) <- mean[0], either may be NULL; the shift of mjmpc_shift_mean; *d_step_counter += 1 (may be NULL); and, when
 * d_cov is not NULL, cov += cov_scale * diag(d_cov_diag) as in mjmpc_cov_add_diag (cem.py:89-95,
 * gaussian_dmd.py:107-113).  A <= 64.                                                                          */
int mjmpc_step_tail(double* d_mean, int H, int A, int shift_mode, const double* d_row, double* d_action_out,
                    double* h_action_mapped, int64_t* d_step_counter, double* d_cov, const double* d_cov_diag,
                    double cov_scale, void* stream);

/* Covariance kept on the device (CEM cem.py:75-95, DMDMPC with update_cov gaussian_dmd.py:77-113): the lower
 * Cholesky factor d_chol (float64 [A][A]) that mjmpc_sample_noise colours its normals with, computed from the
 * device-resident d_cov (np.linalg.cholesky's role inside control_utils.generate_noise:28-29); *d_status (device
 * int, may be NULL) is set to 1 if d_cov is not positive definite.  mjmpc_cov_add_diag: cov += scale * diag(d_diag)
 * (the shift's `+ beta * diag(init_cov)` / `+ beta * I`; d_diag NULL = identity).  A <= 64.                  */
int mjmpc_cholesky_lower(const double* d_cov, int A, double* d_chol, int* d_status, void* stream);
int mjmpc_cov_add_diag(double* d_cov, int A, const double* d_diag, double scale, void* stream);

/* The recursive filter of generate_noise alone (control_utils.py:32-33), in place on d_noise [P][H][A]. */
int mjmpc_filter_noise(int dtype, void* d_noise, int64_t P, int H, int A, const double* d_coeffs, void* stream);
/* noise[row][:] <- noise[row][:] B for `rows` rows of A scalars, B float64 [A][A] row-major: the colouring step of
 * np.random.multivariate_normal (control_utils.py:30), B = sqrt(s)[:, None] * v from the SVD of cov (host, LAPACK),
 * applied to the standard-normal stream mjmpc_sample_noise_mt19937[_jump] regenerates with scale 1.          */
int mjmpc_color_noise(int dtype, void* d_noise, int64_t rows, int A, const double* d_B, void* stream);

/* control_utils.generate_noise (mjmpc/utils/control_utils.py:24-34), SEED-IDENTICAL mode for an isotropic
 * covariance c*I: d_noise[0..n_normals) = scale * the numpy legacy stream `np.random.seed(seed + *d_step);
 * standard_normal(n_normals)` (MT19937 + polar method), regenerated on the device, unfiltered (C order over
 * (P,H,A); scale = sqrt(c)).  Stream alignment is exact; values agree with numpy to <= 2 ulp (log()).
 * d_ws: mjmpc_mt19937_workspace_bytes(n_normals) bytes, 16-byte aligned.  *d_status (device int, may be
 * NULL) is set to 1 if the generated margin of polar attempts did not suffice.                    */
int64_t mjmpc_mt19937_workspace_bytes(int64_t n_normals);
int mjmpc_sample_noise_mt19937(int dtype, void* d_noise, int64_t n_normals, double scale, uint64_t seed,
                               const int64_t* d_step, void* d_ws, int* d_status, void* stream);

/* The same stream produced in parallel.  MT19937's recurrence is serial, but its state transition is linear
 * over GF(2): the state J words ahead is the XOR of the word windows x[i .. i+624) over the set bits i of
 * t^J mod phi (phi = the generator's characteristic polynomial).  One workgroup generates the first
 * head_words (a multiple of 4 in [19936, 19968]) words serially; workgroup g of n_segments (<= 64) then starts directly at word
 * head_words + g*seg_words.  d_jump_idx / d_jump_starts[n_segments+1] (device int32) hold the set-bit lists
 * of t^(head_words + g*seg_words) mod phi, g >= 1 (entry 0 empty), as computed by
 * mjmpc_amd/control/mt_jump.py; the segments must cover mjmpc_mt19937_stream_words(n_normals) words.
 * n_segments == 0 behaves as mjmpc_sample_noise_mt19937.  Output is bit-identical for any segmentation.
 * first_normal > 0 (particle sharding): d_noise[0..n_normals) receives normals [first_normal, first_normal +
 * n_normals) of the one global stream - the polar method's rejections make positions data dependent, so a rank
 * regenerates the stream up to the end of its block; workspace, segments and stream_words are then those of
 * first_normal + n_normals.                                                                                   */
int64_t mjmpc_mt19937_stream_words(int64_t n_normals);
int mjmpc_sample_noise_mt19937_jump(int dtype, void* d_noise, int64_t n_normals, double scale, uint64_t seed,
                                    const int64_t* d_step, const int32_t* d_jump_idx, const int32_t* d_jump_starts,
                                    int64_t head_words, int64_t seg_words, int n_segments, int64_t first_normal,
                                    void* d_ws, int* d_status, void* stream);

/* control_utils.generate_noise (mjmpc/utils/control_utils.py:24-34), performance mode: Philox
 * normals coloured by the lower Cholesky factor d_chol (float64 [A][A]) and filtered in place with
 * d_coeffs (float64 [3]; NULL leaves the samples raw for mjmpc_arm_rollout_fused to filter).  Same distribution as the reference, different bit stream; `offset`
 * plays the role of num_steps in base_seed = seed_val + num_steps (olgaussian_mpc.py:91);
 * `particle_offset` is the global index of local particle 0, so that a sharded run draws exactly
 * the samples a single GPU would draw for the same particles.  d_step (device int64, may be NULL)
 * is added to `offset` on the device, so that a captured hipGraph can advance the stream itself.
 * chol_is_diagonal != 0 promises that d_chol has no off-diagonal entries (skips the colouring loop). */
int mjmpc_sample_noise(int dtype, void* d_noise, int64_t P, int H, int A, const double* d_chol,
                       const double* d_coeffs, uint64_t seed, uint64_t offset, int64_t particle_offset,
                       const int64_t* d_step, int chol_is_diagonal, void* stream);

/* Episode batches: the RAW samples of E episodes in one launch (control_utils.py:24-34 of every episode, unfiltered as
 * mjmpc_tree_rollout_fused_batch takes them).  Row e of d_noise (dtype [E][P][H][A]) is exactly what
 * mjmpc_sample_noise(dtype, d_noise + e P H A, P, H, A, d_chols + e A A, NULL, d_seeds[e], offset, 0, d_step, 1) draws:
 * d_chols float64 [E][A][A] DIAGONAL factors, d_seeds uint64 [E] (device), one step counter d_step (may be NULL) for all. */
int mjmpc_sample_noise_batch(int dtype, int E, void* d_noise, int64_t P, int H, int A, const double* d_chols,
                             const uint64_t* d_seeds, uint64_t offset, const int64_t* d_step, void* stream);

/* PFMPC with the particle set on the device (mjmpc/control/particle_filter_controller.py:92-174; csrc/pfmpc.hip).  The set
 * d_set (float64 [M][H][A]), its mean (float64 [H][A]) and the weights are float64; random numbers are the Philox stream of
 * mjmpc_sample_noise.  One control step is  delta -> rollout -> weights -> resample -> gather_shift -> finish.
 * d_ws: mjmpc_pf_workspace_bytes(M, H, A) bytes, 8-byte aligned, the same for resample, gather_shift and finish.
 *
 * mjmpc_pf_weights   d_weights[p] = softmax_p((-1 / lam) d_q0[p]) (:104-113; a non-finite q0 weighs nothing), one workgroup,
 *                    fixed summation tree.  d_first (device float64, may be NULL) receives the resampling's first pointer,
 *                    random.uniform(0, 1 / M)'s formula on a Philox uniform: (1.0 / M) * double(u), u = (float(c0) + 0.5f) *
 *                    2^-32, c0 the first word of the block keyed (seed, offset + *d_step, chan = 2^64 - 1, quad 0) in
 *                    mjmpc_sample_noise's key layout (no particle's channel index reaches that chan).
 * mjmpc_pf_resample  the systematic resampling (:159-171): d_idx[m] = first i whose running sum of d_weights reaches the
 *                    pointer *d_first + m / M, capped at M - 1; -1 (the last particle, as numpy's index -1) for a pointer
 *                    <= 0.  The running sum is the strictly sequential left-to-right float64 sum - np.cumsum's bits -: one
 *                    lane adds (M dependent additions), so the launch is linear in M.  One workgroup.
 * mjmpc_pf_gather_shift  d_set_out[m] = d_set[d_idx[m]] (must not alias d_set), shifted unless shift_mode < 0 (:127-150):
 *                    rows move up by one, every row gets + jitter - mjmpc_sample_noise(MJMPC_F64, ., M, H, A, d_chol,
 *                    d_coeffs, seed, offset, 0, d_step, chol_is_diagonal = 1) element for element, drawn in the kernel -, then
 *                    the last row becomes 0 (shift_mode 0, 'null') or the jittered row H - 2 (1, 'repeat').  d_gathered
 *                    (float64 [M][H][A], may be NULL) receives the unshifted survivors; per-workgroup sums of them stay in
 *                    d_ws for mjmpc_pf_finish.
 * mjmpc_pf_finish    d_mean = the mean of the unshifted survivors (:97; fixed summation tree, no atomics), d_action_out
 *                    (float64 [A], may be NULL) = d_mean[0], *d_step_counter += 1 (may be NULL).
 * mjmpc_pf_delta     d_delta (dtype [M][H][A]) = d_set - d_mean: the deviations a rollout takes beside d_mean (:74-90).   */
int64_t mjmpc_pf_workspace_bytes(int64_t M, int H, int A);
int mjmpc_pf_weights(int64_t M, const double* d_q0, double lam, uint64_t seed, uint64_t offset, const int64_t* d_step,
                     double* d_weights, double* d_first, void* stream);
int mjmpc_pf_resample(int64_t M, const double* d_weights, const double* d_first, int32_t* d_idx, void* d_ws, void* stream);
int mjmpc_pf_gather_shift(int64_t M, int H, int A, const double* d_set, const int32_t* d_idx, int shift_mode,
                          const double* d_chol, const double* d_coeffs, uint64_t seed, uint64_t offset, const int64_t* d_step,
                          double* d_set_out, double* d_gathered, void* d_ws, void* stream);
int mjmpc_pf_finish(int64_t M, int H, int A, const void* d_ws, double* d_mean, double* d_action_out, int64_t* d_step_counter,
                    void* stream);
int mjmpc_pf_delta(int dtype, int64_t M, int H, int A, const double* d_set, const double* d_mean, void* d_delta, void* stream);

/* Episode batches of the PFMPC step: E independent particle sets, the episode on a grid axis, no host
 * synchronisation.  Row e of every launch executes the single launch's instructions on episode e's slices - d_sets float64
 * [E][M][H][A], d_means float64 [E][H][A], d_q0 / d_weights float64 [E][M], d_first float64 [E], d_idx int32 [E][M], d_lams
 * float64 [E] (> 0: only the host can check it), d_seeds uint64 [E], d_chols float64 [E][A][A] (the jitters' factors), d_delta
 * dtype [E][M][H][A], d_gathered float64 [E][M][H][A] (may be NULL), d_actions float64 [E][A] (may be NULL) -; nothing is
 * exchanged between rows and no workgroup straddles two rows.  M, H, A, shift_mode, d_coeffs, offset and d_step are shared by
 * the batch; the Philox key's particle index is the index inside the episode.  *d_step_counter (may be NULL) is advanced
 * once, by row 0 of mjmpc_pf_finish_batch: the episodes advance together.  1 <= E <= 65535; the other refusals are those of
 * the single entry points.  d_ws: mjmpc_pf_batch_workspace_bytes(E, M, H, A) = E * mjmpc_pf_workspace_bytes(M, H, A) bytes
 * (0 for bad sizes), 8-byte aligned, the same for resample, gather_shift and finish: the running sums [E][M], then the
 * partial sums [E][nb][H A]. */
int64_t mjmpc_pf_batch_workspace_bytes(int E, int64_t M, int H, int A);
int mjmpc_pf_delta_batch(int dtype, int E, int64_t M, int H, int A, const double* d_sets, const double* d_means, void* d_delta,
                         void* stream);
int mjmpc_pf_weights_batch(int E, int64_t M, const double* d_q0, const double* d_lams, const uint64_t* d_seeds, uint64_t offset,
                           const int64_t* d_step, double* d_weights, double* d_first, void* stream);
int mjmpc_pf_resample_batch(int E, int64_t M, const double* d_weights, const double* d_first, int32_t* d_idx, void* d_ws,
                            void* stream);
int mjmpc_pf_gather_shift_batch(int E, int64_t M, int H, int A, const double* d_sets, const int32_t* d_idx, int shift_mode,
                                const double* d_chols, const double* d_coeffs, const uint64_t* d_seeds, uint64_t offset,
                                const int64_t* d_step, double* d_sets_out, double* d_gathered, void* d_ws, void* stream);
int mjmpc_pf_finish_batch(int E, int64_t M, int H, int A, const void* d_ws, double* d_means, double* d_actions,
                          int64_t* d_step_counter, void* stream);

/* User-defined cost terms: a second launch behind mjmpc_{arm,tree}_rollout / _rollout_cl / _step_state that turns
 * the next observations (d_next_obs, dtype [P][H][d_obs]) and the actions (d_actions, dtype [P][H][A]; may be NULL if no row
 * reads an action) of every (particle, step) into a cost, in place in d_costs (dtype [P][H]).  d_terms: float64 [n_terms][8]
 * on the device, 1 <= n_terms <= 128, a row being  kind, source, index, weight, target, group, when, reserved:
 *   v = next_obs[p][t][index] (source 0) or actions[p][t][index] (source 1) as double,  r = v - target;
 *   kind 0 ABS  w |r|;   1 SQUARE  w r^2;   3 COS  w (1 - cos r);
 *   kind 2 NORM: consecutive rows of kind 2 with the same group > 0 add  w_first sqrt(sum r^2)  once, at the group's last row;
 *   when = 1: the row counts only at t = H - 1, and only if `terminal` is non-zero (a real env's step is no plan's last step).
 * cost[p][t] = the sum over the rows in row order, accumulated in double and rounded to dtype; with keep_builtin the cost
 * already in d_costs is the first addend.  The incoming cost is read either way: where it is not finite the outgoing cost is
 * +inf (a particle that reset under set_reset_returns "inf" keeps weighing nothing).  The table's contents - kinds, indices
 * inside d_obs / A, contiguous groups with one `when`, finite numbers - are the caller's to check (envs/cost_terms.py does):
 * the kernel assumes a valid table.  Refused before anything is launched: null d_next_obs / d_terms / d_costs, P < 1, H < 1,
 * d_obs < 1, A < 0, n_terms outside 1 .. 128, an unknown dtype, a row of more than 60 KiB. */
int mjmpc_cost_terms(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                     const double* d_terms, int n_terms, int keep_builtin, int terminal, void* d_costs, void* stream);

/* mjmpc_cost_terms for an episode batch, one launch: the costs of E * P particles (d_costs dtype [E P][H],
 * d_next_obs dtype [E P][H][d_obs], d_actions dtype [E P][H][A] or NULL; the episode of particle p is p / P) with the row
 * semantics of mjmpc_cost_terms.  per_episode = 0: d_terms is float64 [n_terms][8]; per_episode = 1: [E][n_terms][8] - kind,
 * source, index, group and when are read from episode 0's rows (the caller checks that the episodes agree), weight and target
 * from the particle's own episode.  The costs are bit for bit those of mjmpc_cost_terms on that episode's rows with that
 * episode's table.  d_gseq (float64 [H]) and d_q0 (float64 [E P]) go together or are both NULL: q0[p] = the sum over
 * t = 0 .. H - 1, in this order, of gseq[t] * (double)cost[p][t] with the costs as stored (rounded to dtype), every product and
 * every sum rounded on its own (no fused multiply-add), +inf where the sum is not finite.  Refused before anything is
 * launched: null d_next_obs / d_terms / d_costs, E, P, H or d_obs < 1, A < 0, actions with A < 1, n_terms outside 1 .. 128, an
 * unknown dtype, one of d_gseq / d_q0 without the other, a row of more than 56 KiB. */
int mjmpc_cost_terms_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                           const double* d_terms, int n_terms, int per_episode, int keep_builtin, int terminal, void* d_costs,
                           const double* d_gseq, double* d_q0, void* stream);

/* Cost terms that track a reference trajectory: mjmpc_cost_terms with a goal that moves with env time.  A row
 * whose `reserved` column holds 1 + c (c >= 0) takes its goal from column c of d_ref, float64 [n_ref][n_cols] on the device
 * (reference row n = the goal for env time n), instead of its `target` column; rows with reserved = 0 are as ever.  d_step is
 * an int64 counter ON THE DEVICE, read by the kernel - a captured graph or a launch tape freezes the pointer, not the value.
 * With the base time b = *d_step + step_bias, element (p, t) compares an observation row with reference row b + t + 1 and an
 * action row with reference row b + t; a row index outside [0, n_ref - 1] is clamped to it (periodic = 0: the last goal is
 * held) or taken mod n_ref, non-negative (periodic != 0).  Everything else - kinds, groups, when, keep_builtin, non-finite
 * incoming costs, the order and the rounding - is mjmpc_cost_terms': r = v - goal is one subtraction, so a reference that is
 * constant in time costs bit for bit what the same table with that target does.  advance != 0: the launch leaves *d_step + 1
 * in the counter, behind its reads; only for P = H = 1 (the controlled env's step: one workgroup).  Refused before anything
 * is launched: what mjmpc_cost_terms refuses, null d_ref / d_step, n_ref outside 1 .. 2^20, n_cols outside 1 .. 128,
 * advance with P * H != 1.  A tracked row's column c < n_cols is the caller's to check (envs/cost_terms.py does). */
int mjmpc_cost_terms_track(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                           const double* d_terms, int n_terms, int keep_builtin, int terminal, const double* d_ref,
                           int64_t n_ref, int n_cols, int periodic, int64_t* d_step, int64_t step_bias, int advance,
                           void* d_costs, void* stream);

/* mjmpc_cost_terms_batch with tracked rows.  ref_per_episode = 0: d_ref is float64 [n_ref][n_cols]; ref_per_episode = 1:
 * [E][n_ref][n_cols], a particle reads its own episode's.  The counter is only read (the episode batches' update launches
 * advance theirs).  Costs and cost-to-go are bit for bit those of mjmpc_cost_terms_track per episode and of
 * mjmpc_cost_terms_batch's cost-to-go.  Refused: what mjmpc_cost_terms_batch refuses, null d_ref / d_step, n_ref outside
 * 1 .. 2^20, n_cols outside 1 .. 128. */
int mjmpc_cost_terms_track_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                 const void* d_actions, const double* d_terms, int n_terms, int per_episode, int keep_builtin,
                                 int terminal, const double* d_ref, int64_t n_ref, int n_cols, int ref_per_episode, int periodic,
                                 const int64_t* d_step, int64_t step_bias, void* d_costs, const double* d_gseq, double* d_q0,
                                 void* stream);

/* Action-rate rows and one-sided kinds: mjmpc_cost_terms_track with two more sources of cost.  The entry serves
 * every row of the entries above and
 *   source 2, the action rate:  v = (double)actions[p][t][index] - (double)actions[p][t-1][index]  for t >= 1, and for t = 0
 *     v = (double)actions[p][0][index] - d_prev_action[index], d_prev_action being float64 [A] on the device: the action last
 *     applied to the controlled env.  An entry that is NaN says that no action has been applied yet: v = 0 for it, as for every
 *     entry when d_prev_action is NULL.  r = v - target (or the tracked goal: a tracked rate row reads the ACTION-time
 *     reference row b + t), and every kind applies, NORM groups over rate rows included;
 *   kind 4 ABOVE  w max(0, r);   5 BELOW  w max(0, -r);   6 ABOVE_SQUARE  w max(0, r)^2;   7 BELOW_SQUARE  w max(0, -r)^2:
 *     zero on one side of the bound `target` (or the tracked goal).
 * The subtraction of the two actions is one correctly rounded double operation on values that convert exactly; order,
 * rounding, `when`, keep_builtin and non-finite incoming costs are mjmpc_cost_terms'.  d_actions is required.  d_ref and
 * d_step go together: both NULL for a table without tracked rows (n_ref, n_cols, periodic and step_bias are then ignored).
 * advance != 0 (only for P = H = 1): behind its reads the launch leaves *d_step + 1 in the counter, where one is given, and
 * the element's action row, as double, in d_prev_action, where that is given - the controlled env's step records the action
 * it applied in the launch that costs it, so a captured graph or a launch tape carries it along.  Refused before anything
 * is launched: null d_next_obs / d_actions / d_terms / d_costs, one of d_ref / d_step without the other, P, H, d_obs or A < 1,
 * n_terms outside 1 .. 128, an unknown dtype, with a reference n_ref outside 1 .. 2^20 or n_cols outside 1 .. 128, advance
 * with P * H != 1, an observation row and two action rows of more than 60 KiB. */
int mjmpc_cost_terms_rate(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                          const double* d_terms, int n_terms, int keep_builtin, int terminal, const double* d_ref,
                          int64_t n_ref, int n_cols, int periodic, int64_t* d_step, int64_t step_bias, int advance,
                          double* d_prev_action, void* d_costs, void* stream);

/* mjmpc_cost_terms_track_batch with the rows of mjmpc_cost_terms_rate.  d_prev_actions: float64 [E][A] or NULL, a particle
 * reads its own episode's row at t = 0.  advance_prev != 0 (only for P = H = 1): the element of episode e stores its action
 * row, as double, into row e behind its reads.  The counter is only read.  Costs and cost-to-go are bit for bit those of
 * mjmpc_cost_terms_rate per episode and of mjmpc_cost_terms_batch's cost-to-go.  Refused: what mjmpc_cost_terms_rate
 * refuses (E < 1, one of d_gseq / d_q0 without the other, advance_prev with P * H != 1; the row limit is 56 KiB). */
int mjmpc_cost_terms_rate_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                const void* d_actions, const double* d_terms, int n_terms, int per_episode, int keep_builtin,
                                int terminal, const double* d_ref, int64_t n_ref, int n_cols, int ref_per_episode, int periodic,
                                const int64_t* d_step, int64_t step_bias, double* d_prev_actions, int advance_prev,
                                void* d_costs, const double* d_gseq, double* d_q0, void* stream);

/* Quadratic forms and signed linear rows: mjmpc_cost_terms_rate with two more kinds.  The entry serves every row
 * of the entries above and
 *   kind 8 QUAD: consecutive rows of kind 8 with one group > 0 form a vector r_i = v_i - goal_i, i = 0 .. n-1, n <= 32, every
 *     row with its own source (0, 1 or 2), index and target or reference column.  At the group's last row the group adds
 *     w_first * sum_i sum_j r_i Q_ij r_j once, w_first being the first row's weight; `when` is the group's (all rows share it).
 *     Q is the group's matrix in the pool d_quad, float64 [quad_len] on the device: the groups' matrices back to back in table
 *     order, each n x n, row-major and symmetric (the kernel reads the diagonal and the entries below it, twice each).  A group's
 *     offset is the sum of n^2 over the QUAD groups before it.  Q need not be positive semi-definite;
 *   kind 9 LINEAR: w r, signed.
 * Order, rounding, `when`, keep_builtin, non-finite incoming costs, d_ref / d_step, advance and d_prev_action are
 * mjmpc_cost_terms_rate's; a table without a row of kind 8 or 9 gives that entry's result bit for bit.  The kernel never reads
 * beyond quad_len and never holds more than min(32, floor(sqrt(quad_len))) entries of a group, whatever the table says.  The
 * groups' scratch comes out of the tile: the row limit is 59 KiB less 512 bytes for every row the largest possible group has
 * (43 KiB at quad_len = 4096).  Refused before anything is launched: what mjmpc_cost_terms_rate refuses, null d_quad, quad_len
 * outside 1 .. 4096, an observation row and two action rows beyond that limit (the message names it in bytes). */
int mjmpc_cost_terms_quad(int dtype, int64_t P, int H, int d_obs, int A, const void* d_next_obs, const void* d_actions,
                          const double* d_terms, int n_terms, int keep_builtin, int terminal, const double* d_ref,
                          int64_t n_ref, int n_cols, int periodic, int64_t* d_step, int64_t step_bias, int advance,
                          double* d_prev_action, const double* d_quad, int quad_len, void* d_costs, void* stream);

/* mjmpc_cost_terms_rate_batch with the rows of mjmpc_cost_terms_quad; one pool d_quad for all episodes.  Costs and cost-to-go
 * are bit for bit those of mjmpc_cost_terms_quad per episode and of mjmpc_cost_terms_batch's cost-to-go.  Refused: what
 * mjmpc_cost_terms_rate_batch refuses, null d_quad, quad_len outside 1 .. 4096; the row limit is 55 KiB less the scratch. */
int mjmpc_cost_terms_quad_batch(int dtype, int E, int64_t P, int H, int d_obs, int A, const void* d_next_obs,
                                const void* d_actions, const double* d_terms, int n_terms, int per_episode, int keep_builtin,
                                int terminal, const double* d_ref, int64_t n_ref, int n_cols, int ref_per_episode, int periodic,
                                const int64_t* d_step, int64_t step_bias, double* d_prev_actions, int advance_prev,
                                const double* d_quad, int quad_len, void* d_costs, const double* d_gseq, double* d_q0,
                                void* stream);

/* World positions of points on any bodies as observation entries and, through mjmpc_points_motion, body axes and
 * velocities beside them: one launch in front of any cost entry above, one walk in csrc/points.hip behind both.
 * For each of N observation rows (d_obs_rows, dtype [N][d_obs]; N = P H, or E P H for an episode batch: rows are independent)
 * the kernel reads qpos - nq entries in MuJoCo's layout, from entry 0 of the row, as the reach / orient observation has them -,
 * runs the points program over it in double and writes the augmented row d_out, dtype [N][d_obs + 3 n_points + 3 n_diff]: the
 * observation's d_obs entries bit for bit, then world x, y, z of every point in program order, then a - b of every difference,
 * one double subtraction per component; every new entry is rounded once to dtype.  The cost entries then take d_out with
 * d_obs + 3 n_points + 3 n_diff as their d_obs.  The positions are those of the row's own qpos (the built-in `site` block of
 * the observation lags one substep).
 *
 * The points program d_program is float64 [n_rows + n_diff][16] on the device.  Its first n_rows rows hold, for every point
 * in turn, the nodes of the path from the root to the point's body in order - one per jointed body; a body without a joint is
 * folded into the fixed pose of the node (or the point) behind it by the host, so a path holds at most 33 nodes - and then the
 * point itself, which closes the path:
 *   [0] kind: 0 POINT, 1 HINGE, 2 SLIDE, 3 BALL, 4 FREE          [1] the joint's qpos address   [2] qpos0 (hinge, slide)
 *   [3 .. 5]   node: the body's position in the frame before it; POINT: the point's position in the frame of the last node
 *   [6 .. 9]   node: the body's orientation in the frame before it, a unit quaternion (w, x, y, z)
 *   [10 .. 12] the joint's unit axis in the body frame (hinge, slide)
 *   [13 .. 15] the joint's anchor in the body frame (hinge, ball)
 * A path starts at the world frame.  A node moves the frame to frame o (position, orientation) and applies its joint: a hinge
 * turns the frame by q - qpos0 about the axis through the anchor and a ball by qpos[adr .. adr + 4], the anchor held fixed; a
 * slide moves it by q - qpos0 along the axis; a free joint replaces the frame by qpos[adr .. adr + 3], qpos[adr + 3 .. adr + 7]
 * (MuJoCo's mj_kinematics).  The quaternions of qpos rotate as q / |q|.  The last n_diff rows are {5, a, b, 0 ..}: point a minus
 * point b, both indices in program order.  The table's contents are the caller's to check (envs/cost_terms.py builds it); the
 * kernel holds every qpos address inside nq and every point index inside n_points whatever the table says.
 *
 * mjmpc_points_motion adds to this, with n_out output slots of three entries for n_points:
 *   qvel       entries nq .. nq + nv of a row (nq + nv <= d_obs) with MuJoCo's meaning: a hinge's or slide's dof is a rate about
 *              or along the joint axis, a hinge turning about its anchor; a ball joint's three dofs are the angular velocity in
 *              the child body's frame; a free joint's six are the linear velocity in the world frame, then the angular
 *              velocity in the body's frame
 *   d_dofadr   int32 [n_rows] on the device: each node row's first qvel address (ignored for closing rows: the 16 columns of a
 *              node row are all taken, so the addresses stand beside the table).  Node rows themselves are unchanged
 *   the walk   carries beside the frame the world linear velocity v of its origin and its world angular velocity w:
 *                fixed pose  v += w x (R pos)
 *                slide       v += w x (a d) + a qd             (a: the axis in the world, d = q - qpos0)
 *                hinge       the anchor's velocity v + w x r_a is taken; w += a qd; the origin's is the anchor's - w x (R' local)
 *                ball        as the hinge, with w += R' omega_local
 *                free        v = qvel[0 .. 3], w = R qvel[3 .. 6]
 *   closing rows are {kind, keep, slot, x, y, z, 0 ..} (mjmpc_points: kind 0 with keep and slot 0 - every point closes its walk,
 *              and the slots are the points in program order):
 *                [0] kind   0 POINT: p + R (x, y, z)    6 AXIS: R (x, y, z)    7 VELOCITY: v + w x (R (x, y, z))    8 ANGULAR: w
 *                [1] keep   1: the next closing row stands on the same frame, which is kept; 0: the next row starts at the world
 *                           frame, at rest
 *                [2] slot   the output's place in d_out: entries d_obs + 3 slot .. + 3
 *                [3 .. 5]   the offset (POINT, VELOCITY) or the axis (AXIS) in the frame of the last node
 *              so all outputs on one body share one walk (a point and its velocity are nodes + 2 rows) and slots need not be in
 *              program order.  The trailing n_diff rows {5, a, b} index output slots
 *   guards     every dof address is held inside nv and every slot inside n_out whatever the tables say (a closing row with a
 *              slot outside writes nothing); a slot that no closing row names reads as 0.
 *
 * MJMPC_E_BADARG before anything is launched: a null pointer, an unknown dtype, N or d_obs below 1, nq outside 1 .. d_obs,
 * n_points (n_out) outside 1 .. 16, n_diff outside 0 .. 16, n_rows outside n_points (n_out) .. 544, an observation row that
 * does not fit the tile with its points or outputs (60 KiB of LDS); mjmpc_points_motion also a null d_dofadr, nv below 1 or
 * nq + nv above d_obs. */
int mjmpc_points(int dtype, int64_t N, int d_obs, int nq, const void* d_obs_rows, const double* d_program, int n_rows,
                 int n_points, int n_diff, void* d_out, void* stream);

/* Body axes and velocities beside the points: mjmpc_points with qvel, the dof addresses and the further closing
 * rows, all described above. */
int mjmpc_points_motion(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                        const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, void* d_out, void* stream);

/* The centre of mass of a subtree of bodies and its velocity beside the points, axes and velocities:
 * mjmpc_points_motion - every row kind above with the same meaning, the same d_dofadr, slots and guards - with two
 * accumulators S and Sv beside the walk, n_levels saved frames (0 .. 4) and the row kinds
 *   9 MASS          {9, 0, 0, cx, cy, cz, share}   on the current frame: S += share (p + R c), Sv += share (v + w x (R c)), with
 *                                                  c the centre of mass of the node's rigid group in the node's frame and share
 *                                                  its mass over the subtree's (the host divides, the kernel never does).  The
 *                                                  frame is kept
 *   10 SAVE         {10, level}                    the frame, v and w are stored at `level`
 *   11 RESTORE      {11, level}                    they are loaded from `level`; level -1 is the world frame at rest
 *   12 COM          {12, keep, slot}               a closing row (keep and slot as above) that writes S to `slot`
 *   13 COM_VELOCITY {13, keep, slot}               a closing row that writes Sv to `slot`
 * S and Sv are zero at the program's start and are zeroed again whenever a closing row with keep = 0 resets the frame.  A
 * centre of mass is one walk of its own: the nodes of the path from the root to the subtree's root body, then the subtree in
 * depth-first order - every rigid group its node row and its MASS row, a SAVE in front of the first child of a node with
 * several children in the walk, a RESTORE in front of each further child (a level is free again once its last child has
 * begun; several root bodies restore to level -1) - then COM and, on the same walk, COM_VELOCITY.  So every jointed body of the
 * subtree is visited once.
 *   guards     every level holds the world frame at rest until a SAVE names it, so a RESTORE of a level never saved gives that; a
 *              SAVE with a level outside 0 .. n_levels - 1 writes nothing and a RESTORE with one gives the world frame at rest;
 *              slots, qpos and dof addresses are held as in mjmpc_points_motion.
 * The saved frames stand in the tile beside a row's outputs: 104 n_levels more bytes a row.  MJMPC_E_BADARG before anything is
 * launched: what mjmpc_points_motion refuses, n_levels outside 0 .. 4, an observation row that does not fit the tile with its
 * outputs and saved frames. */
int mjmpc_points_tree(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                      const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, int n_levels, void* d_out, void* stream);

/* The orientation error of a body as three entries beside everything above: mjmpc_points_tree - every row kind
 * above with the same meaning, the same arguments, tile, slots and guards - with a held quaternion h beside the walk and two
 * row kinds, which have this meaning at this entry only:
 *   14 HOLD         {14}                           h <- the frame's orientation f.q; the frame, v and w go back to the world
 *                                                  frame at rest; S and Sv are left alone
 *   15 ORIENTATION  {15, keep, slot, ow, ox, oy, oz, gw, gx, gy, gz, rel}
 *                                                  a closing row (keep and slot as above): b = f.q * o, a = rel ? h * g : g,
 *                                                  e = conj(a) * b, and Log(e) goes to `slot`: the rotation vector theta u that
 *                                                  takes the goal frame a to the body's frame b, written in the goal frame
 * h is the identity at the program's start, so rel = 1 with no HOLD before it reads the world frame.  o and g are unit
 * quaternions (w, x, y, z), normalised by the host.  An absolute orientation (rel = 0) shares its body's walk with the other
 * outputs on that body; a relative one is a walk of its own: the path to the other body, HOLD, the path to the body, the
 * closing row.
 *
 * The log map, for e = (w, x, y, z), in double:
 *   if w < 0, all four are negated (w == 0 keeps the stored sign);
 *   s = sqrt(x^2 + y^2 + z^2);
 *   k = 2 / w if s < 2^-26 (relative error s^2 / 3 < 1e-16), else k = 2 atan2(s, w) / s;
 *   r = k (x, y, z).
 * So theta = |r| lies in [0, pi], e the identity gives exactly 0, and near theta = pi the sign of r follows that of w.
 * MJMPC_E_BADARG before anything is launched: what mjmpc_points_tree refuses. */
int mjmpc_points_orient(int dtype, int64_t N, int d_obs, int nq, int nv, const void* d_obs_rows, const double* d_program,
                        const int32_t* d_dofadr, int n_rows, int n_out, int n_diff, int n_levels, void* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MJMPC_AMD_H */
