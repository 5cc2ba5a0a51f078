// The body of the rollout kernels (arm_rollout.hip), #included inside each __global__ function - the barrier shapes' kernel
// (SOLO / DUO) and the flag shapes' kernel - after it has defined  `constexpr int SHAPE`  (1 SOLO, 2 DUO, 12 / 14 the flag shapes
// with two / four wavefronts),  `const MonoStep* mop`  and  `double* state_out`.  One text, two kernels.
    // (the including kernel also provides  `constexpr bool DUO` (SHAPE == 2), `QUAD` (SHAPE > 10: the flag-synchronised shapes)
    // and  `constexpr int NW`  = wavefronts per particle group)
    constexpr int STRIDE = PSTRIDE;
    __shared__ __attribute__((aligned(16))) T lds[LANES * STRIDE + ARM_BLOB_LEN + 3];
    // (the including kernel also provides `qflag_ptr qf` - the flag shapes' hand-over flags in LDS - and `int seq`, their substep number)
    extern __shared__ __attribute__((aligned(16))) double dyn_lds[];     // MONO: scratch [MONO_RED] | action tile T[8][H A]
    static_assert(!((DUO || QUAD) && CL), "the closed-loop-linear variant runs one wave per particle group");
    static_assert(!(MONO && (CL || STEP)), "the one-launch iteration is open-loop MPPI");
    constexpr int NT = 64 * NW;
    const int lane = threadIdx.x & 63;
    const int wave = NW > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const int l8 = lane_link(lane), g = lane_slot(lane);
    // (EB && STEP: workgroup e is env e of P = E - its one live particle sits in slot 0 and is record e of cost / next_obs)
    const long pid = (EB && STEP) ? (g == 0 ? (long)blockIdx.x : P) : (long)blockIdx.x * LANES + g;
    const bool live = pid < P;
    for (int k = threadIdx.x; k < LANES * STRIDE; k += NT) lds[k] = T(0);
    if constexpr (QUAD) { if (threadIdx.x < QF_COUNT) q_write(qf, threadIdx.x, 0); }
    T* ldsModel = lds + LANES * STRIDE;
    ResetCtl rc;
    rc.count = live;
    // my model block's reset record: its address waits in LDS for the rare path (held in scalar registers through the
    // rollout it cost this kernel spills in its hot loops)
    __shared__ const double* s_reset_rec;
    if (threadIdx.x == 0) {
        const double* r = fuse.reset_rec;
        if (r && fuse.shard_size > 0) r += ((long)blockIdx.x * LANES / fuse.shard_size) * ARM_RESET_LEN;
        s_reset_rec = r;
    }
    auto record = []() -> const double* { return *(const double* volatile*)&s_reset_rec; };
    const bool resets = fuse.reset_rec != nullptr;
    if (fuse.shard_size > 0) model += ((long)blockIdx.x * LANES / fuse.shard_size) * ARM_BLOB_LEN;
    if (fuse.state_shard_size > 0) state += ((long)blockIdx.x * LANES / fuse.state_shard_size) * (2 * LANES + 3);
    if constexpr (EB) mean += ((long)blockIdx.x * LANES / fuse.state_shard_size) * ((long)H * A);       // my episode's mean row
    for (int k = threadIdx.x; k < ARM_BLOB_LEN; k += NT) ldsModel[k] = model[k];
    __syncthreads();
    T* ldsM = lds + g * STRIDE;
    Model<T, (DUO || QUAD)> M{ldsModel, l8};
    M.cache();
    ArmInts I;
    I.site_link = (int)model[O_SITE_LINK];
    I.n_sphere = (int)model[O_N_SPHERE];
    I.sph_link = (int)model[O_SPH_LINK];
    I.frame_skip = (int)model[O_FRAME_SKIP];
    I.nv = (int)model[O_NV];
    const int nv = I.nv;
    const int dobs = 2 * nv + 6;

    T q = (T)state[l8], v = (T)state[LANES + l8], aw = T(0);
    const T tgt[3] = {(T)state[2 * LANES], (T)state[2 * LANES + 1], (T)state[2 * LANES + 2]};
    if (l8 >= nv) { q = T(0); v = T(0); }
    T sinq, cosq;
    sincos_(q, sinq, cosq);
    if constexpr (XJ) { if (M.xj_slide()) { sinq = T(0); cosq = T(1); } }
    if (resets) {
        // the launch's reset options (RST_REAL, RST_INF) into this wave's flags word - launches that have none write nothing
        const int ropts = (STEP ? RST_REAL : 0) | (fuse.inf_on_reset ? RST_INF : 0);
        if (ropts) {
            if (DUO && wave == 1) rflags_set<SOLVE>(ldsM, ropts);
            else if (QUAD && wave == 1) rflags_set<QSOLVE>(ldsM, ropts);
            else if (QUAD && wave == 2) rflags_set<QAUX>(ldsM, ropts);
            else if (QUAD && wave == 3) rflags_set<QMASS>(ldsM, ropts);
            else rflags_set<SOLO>(ldsM, ropts);
        }
        if (DUO && wave == 1) reset_check_start<SOLVE>(rc, q, v, lane, ldsM);
        else if (QUAD && wave == 1) reset_check_start<QSOLVE>(rc, q, v, lane, ldsM);
        else if (QUAD && wave == 2) reset_check_start<QAUX>(rc, q, v, lane, ldsM);
        else if (QUAD && wave == 3) reset_check_start<QMASS>(rc, q, v, lane, ldsM);
        else reset_check_start<SOLO>(rc, q, v, lane, ldsM);
    }
    const int site_lane = lane_of_link(lane, I.site_link);
    int rows = 0;
    T cq = q, cv = v, chand[3] = {T(0), T(0), T(0)};
    const bool has_u = l8 < A;
    Stamps ST;
    ST.begin();
    double fb0 = 1.0, fb1 = 0.0, fb2 = 0.0, e1 = 0.0, e2 = 0.0, q0acc = 0.0;
    if (fuse.filt) { fb0 = fuse.filt[0]; fb1 = fuse.filt[1]; fb2 = fuse.filt[2]; }

    // fresh observation after set_env_state (sim.forward()): the site position at the start state is
    // needed BEFORE the first step when the policy is closed-loop; one extra kinematics pass provides it
    if constexpr (CL) {
        T qq = q, vv = v, aa = aw, ss = sinq, cc = cosq;
        int rr = 0;
        T s0[3];
        bool fs0;
        arm_front<SOLO>(M, I, qq, vv, aa, ss, cc, rr, T(0), ldsM, lane, l8, s0, (unsigned*)nullptr, fs0, ST);
        arm_back<SOLO>(M, qq, vv, aa, ss, cc, ldsM, l8, fs0, ST);
        for (int k = 0; k < 3; ++k) chand[k] = __shfl(s0[k], site_lane);
    }

    constexpr int R = QUAD ? QDYN : (DUO ? DYN : SOLO);
    const int HA = H * A;
    T* actT = (T*)(dyn_lds + MONO_RED);          // MONO: the actions of my workgroup's particles, [8][H A]
    if (DUO && wave == 1) {         // the SOLVE wave: no inputs, no records - mass matrix, constraints, solves
        if constexpr (DUO) {
            bool fs;
            T nosite[3];
            for (int t = 0; t < H; ++t)
                for (int sub = 0; sub < I.frame_skip; ++sub) {
                    arm_front<SOLVE>(M, I, q, v, aw, sinq, cosq, rows, T(0), ldsM, lane, l8, nosite, diag, fs, ST, &rc);
                    arm_back<SOLVE>(M, q, v, aw, sinq, cosq, ldsM, l8, fs, ST, lane, &rc, nullptr, record);
                }
            ST.flush(diag, 1, lane);
        }
        if constexpr (!MONO) return;
    } else if (QUAD && wave >= 1) { // flag shapes: the waves beside the one that owns inputs and records (flag_front)
        if constexpr (QUAD) {
            bool fs;
            T nosite[3];
#define MJMPC_FLAG_LOOP(ROLE_)                                                                                              \
            for (int t = 0; t < H; ++t)                                                                                     \
                for (int sub = 0; sub < I.frame_skip; ++sub) {                                                              \
                    ++seq;                                                                                                  \
                    flag_front<ROLE_, NW>(M, I, q, v, aw, sinq, cosq, rows, T(0), ldsM, qf, seq, lane, l8, nosite, diag, fs, ST, &rc); \
                    arm_back<ROLE_>(M, q, v, aw, sinq, cosq, ldsM, l8, fs, ST, lane, &rc, nullptr, record, qf, seq);       \
                }
            if (wave == 1) { MJMPC_FLAG_LOOP(QSOLVE) }
            else if (wave == 2) { MJMPC_FLAG_LOOP(QAUX) }
            else { MJMPC_FLAG_LOOP(QMASS) }
#undef MJMPC_FLAG_LOOP
            ST.flush(diag, wave, lane);
        }
        if constexpr (!MONO) return;
    } else {

    // inputs of step t+1 are fetched while step t computes (a lone wave would otherwise sit out the full
    // HBM latency of its noise load at the top of every env step)
    T eps_next = T(0);
    double mean_next = 0.0, gs_next = (fuse.gseq && H > 0) ? fuse.gseq[0] : 0.0;   // (a load consumed in the iteration
    // that issues it would make its s_waitcnt also wait for the prefetches issued before it)
    // MONO: the raw sample of (particle, channel l8, step t) is drawn here instead of loaded - the same Philox block the
    // sampler kernel (noise.hip) would have used for it: one block yields the normals of steps 4k ... 4k + 3
    const bool sampled = MONO && has_u && live;
    float z_keep[3] = {0.0f, 0.0f, 0.0f};
    // (three normals live across env steps.  The sampler's parameters are read ONCE: a draw sits between E2 and E3 of a
    // substep, in the DYN wave's slack, and a global load per env step - even a cache hit - outlasted that slack:
    // hoisting them costs 16 AGPRs and 1.5 us less per launch)
    double chol_h = 0.0;
    double chol_row[LANES - 1];             // full covariance: my row of the factor (entries b <= l8)
    bool chol_full = false;
    unsigned long long seed_h = 0ull, off_h = 0ull, key_h = 0ull;
    if constexpr (MONO) {
        chol_full = mop->chol_full != 0;
        if (sampled) chol_h = mop->chol[l8 * A + l8];
#pragma unroll
        for (int b = 0; b < LANES - 1; ++b) chol_row[b] = (chol_full && sampled && b <= l8 && b < A) ? mop->chol[l8 * A + b] : 0.0;
        seed_h = mop->seed;
        off_h = mop->offset + (mop->d_step ? (unsigned long long)*mop->d_step : 0ull);
        key_h = (unsigned long long)((pid + mop->particle_offset) * A + l8);
    }
    auto draw = [&](int t) -> T {
        const double chol_aa = chol_h;
        float z = 0.0f;
        if (sampled) {
            if (!(t & 3)) {
                float q4[4];
                normal_quad(seed_h, off_h, key_h, (unsigned)(t >> 2), q4);
                z = q4[0];
                z_keep[0] = q4[1];
                z_keep[1] = q4[2];
                z_keep[2] = q4[3];
            } else {
                z = (t & 3) == 1 ? z_keep[0] : ((t & 3) == 2 ? z_keep[1] : z_keep[2]);
            }
        }
        if (chol_full) {
            // eps[a] = sum_{b <= a} L[a][b] z_b in noise_full_kernel's order: the channels' normals by DPP broadcast inside
            // the particle's 8 lanes (every lane takes part: the broadcasts run outside the `sampled` branch)
            double x = 0.0;
            float zb;
            zb = bcast<0>(z); if (chol_row[0] != 0.0) x += chol_row[0] * (double)zb;
            zb = bcast<1>(z); if (chol_row[1] != 0.0) x += chol_row[1] * (double)zb;
            zb = bcast<2>(z); if (chol_row[2] != 0.0) x += chol_row[2] * (double)zb;
            zb = bcast<3>(z); if (chol_row[3] != 0.0) x += chol_row[3] * (double)zb;
            zb = bcast<4>(z); if (chol_row[4] != 0.0) x += chol_row[4] * (double)zb;
            zb = bcast<5>(z); if (chol_row[5] != 0.0) x += chol_row[5] * (double)zb;
            zb = bcast<6>(z); if (chol_row[6] != 0.0) x += chol_row[6] * (double)zb;
            return (T)x;
        }
        return (T)(chol_aa * (double)z);
    };
    if (has_u && H > 0) {
        if constexpr (!CL) mean_next = mean[l8];
        if constexpr (!MONO) { if (noise && live) eps_next = noise[(pid * H) * A + l8]; }
    }
    if constexpr (MONO) { if (H > 0) { const T e0 = draw(0); if (sampled) eps_next = e0; } }    // (every lane: DPP broadcasts)

    for (int t = 0; t < H; ++t) {
        T u = T(0);
        const T eps_cur = eps_next;
        const double mean_cur = mean_next, gs_cur = gs_next;
        if (fuse.gseq && t + 1 < H) gs_next = fuse.gseq[t + 1];
        if (has_u && t + 1 < H) {
            if constexpr (!CL) mean_next = mean[(t + 1) * A + l8];
            if constexpr (!MONO) { if (noise && live) eps_next = noise[(pid * H + t + 1) * A + l8]; }
        }
        if constexpr (CL) {         // u = clw^T [q, v, hand, hand - target, 1]
            const int wl = has_u ? l8 : 0;
            double uu = fuse.clw[(2 * nv + 6) * A + wl];
            cl_accumulate<0, T>(fuse.clw, A, nv, wl, cq, cv, uu);
            for (int k = 0; k < 3; ++k)
                uu += fuse.clw[(2 * nv + k) * A + wl] * (double)chand[k] +
                      fuse.clw[(2 * nv + 3 + k) * A + wl] * (double)(chand[k] - tgt[k]);
            u = has_u ? (T)uu : T(0);
        }
        if (has_u) {
            if constexpr (!CL) u = (T)mean_cur;
            if (MONO ? sampled : (noise && live)) {
                T eps = eps_cur;
                if (fuse.filt) {            // eps[t] = b0 eps[t] + b1 eps[t-1] + b2 eps[t-2], t >= 2
                    const double f = t >= 2 ? fb0 * (double)eps + fb1 * e1 + fb2 * e2 : (double)eps;
                    e2 = e1;
                    e1 = f;
                    eps = (T)f;
                }
                u += eps;
            }
            if (act && live) act[(pid * H + t) * A + l8] = u;        // unclipped (gym_env_wrapper.py:151)
            if constexpr (MONO) actT[g * HA + t * A + l8] = u;
        }
        // MuJoCo clamps ctrl, not the record
        const T tau_act = M.link(O_GEAR) * fmin(fmax(u, M.link(O_CTRL_LO)), M.link(O_CTRL_HI));
        T site[3];
        bool fs = false;
        if (__builtin_expect(rc.any, 0)) rflags_set<R>(ldsM, rflags<R>(ldsM) & (2 | RST_EVER | RST_OPTS));     // a new env step: do_simulation writes data.ctrl again (a pending reset stays)
        for (int sub = 0; sub < I.frame_skip; ++sub) {
            if ((R == DYN || R == QDYN) && sub > 0) arm_back<R>(M, q, v, aw, sinq, cosq, ldsM, l8, fs, ST, lane, &rc, diag, record, qf, seq);
            if constexpr (QUAD) {
                ++seq;
                flag_front<R, NW>(M, I, q, v, aw, sinq, cosq, rows, tau_act, ldsM, qf, seq, lane, l8, site, diag, fs, ST, &rc);
            } else {
                arm_front<R>(M, I, q, v, aw, sinq, cosq, rows, tau_act, ldsM, lane, l8, site, diag, fs, ST, &rc);
            }
            if constexpr (R == SOLO) arm_back<R>(M, q, v, aw, sinq, cosq, ldsM, l8, fs, ST, lane, &rc, diag, record);
            if (t == 0 && sub == 0 && obs)                  // fresh observation after set_env_state
                for (int k = 0; k < 3; ++k) chand[k] = __shfl(site[k], site_lane);
        }
        // DYN: the last substep is integrated further down - the cost record needs only its kinematics and is
        // written while the SOLVE wave is still solving
        for (int k = 0; k < 3; ++k) site[k] = __shfl(site[k], site_lane);
        // (the last substep ended in mj_checkAcc's reset: mj_forward ran again from the reset state, site_xpos is that state's)
        if (R == SOLO && __builtin_expect(rc.any, 0)) {
            if (rflags<R>(ldsM) & 4)
                for (int k = 0; k < 3; ++k) site[k] = (T)record()[2 * LANES + k];
        }
        // Take delivery of the prefetched inputs HERE, before this step's stores are issued: loads and stores share
        // one in-order counter (vmcnt), and the register hand-over the compiler otherwise places on the loop's
        // back-edge waits with vmcnt(0) - i.e. for the cost / observation stores just issued (~2000 cycles per step).
        asm volatile("" : "+v"(eps_next), "+v"(mean_next), "+v"(gs_next));
        // reward = -(|h-g|_1 + 5 |h-g|_2), h = site_xpos lagging one substep (reacher_env.py:31-35)
        T dx = site[0] - tgt[0], dy = site[1] - tgt[1], dz = site[2] - tgt[2];
        T cst = fabs(dx) + fabs(dy) + fabs(dz) + T(5) * sqrt_(dx * dx + dy * dy + dz * dz);
        // RolloutFusion::inf_on_reset: a particle that has reset costs +inf from that env step on (no weight in the updates)
        if (__builtin_expect(rc.any, 0)) { if ((rflags<R>(ldsM) & (RST_INF | RST_EVER)) == (RST_INF | RST_EVER)) cst = T(INFINITY); }
        if (live && l8 == 0 && (!MONO || cost)) cost[pid * H + t] = cst;
        if (fuse.gseq) q0acc += gs_cur * (double)cst;
        // MONO: the next step's sample, drawn while the SOLVE wave is still iterating (DUO) / once per env step (SOLO)
        if constexpr (MONO) { if (t + 1 < H) { const T en = draw(t + 1); if (sampled) eps_next = en; } }
        if constexpr (R == DYN || R == QDYN) {
            arm_back<R>(M, q, v, aw, sinq, cosq, ldsM, l8, fs, ST, lane, &rc, diag, record, qf, seq);
            if (__builtin_expect(rc.any, 0)) {
                // (inf_on_reset: the env step's last substep reset the particle after its cost had been written)
                if ((rflags<R>(ldsM) & (RST_INF | RST_EVER)) == (RST_INF | RST_EVER) && !(cst == T(INFINITY))) {    // (finite or NaN so far)
                    if (live && l8 == 0 && (!MONO || cost)) cost[pid * H + t] = T(INFINITY);
                    if (fuse.gseq) q0acc = INFINITY;
                }
            }
            if (__builtin_expect(rc.any, 0) && !(rflags<R>(ldsM) & RST_INF)) {
                // the last substep ended in mj_checkAcc's reset: site_xpos is the reset state's (mj_forward ran again) - the
                // cost written ahead of the integration above is written again
                // (the substep began from a state mj_checkPos / mj_checkVel passed: its site and the cost from it are finite)
                if (rflags<R>(ldsM) & 4) {
                    T ex = site[0] - tgt[0], ey = site[1] - tgt[1], ez = site[2] - tgt[2];
                    const T c_old = fabs(ex) + fabs(ey) + fabs(ez) + T(5) * sqrt_(ex * ex + ey * ey + ez * ez);
                    for (int k = 0; k < 3; ++k) site[k] = (T)record()[2 * LANES + k];
                    ex = site[0] - tgt[0]; ey = site[1] - tgt[1]; ez = site[2] - tgt[2];
                    const T c_new = fabs(ex) + fabs(ey) + fabs(ez) + T(5) * sqrt_(ex * ex + ey * ey + ez * ez);
                    if (live && l8 == 0 && (!MONO || cost)) cost[pid * H + t] = c_new;
                    if (fuse.gseq) q0acc += fuse.gseq[t] * ((double)c_new - (double)c_old);
                }
            }
        }
        if (live && (obs || nobs)) {
            const long o = (pid * H + t) * dobs;
            if (obs) {
                if (l8 < nv) { obs[o + l8] = cq; obs[o + nv + l8] = cv; }
                if (l8 < 3) {
                    T hh = l8 == 0 ? chand[0] : (l8 == 1 ? chand[1] : chand[2]);
                    T gg = l8 == 0 ? tgt[0] : (l8 == 1 ? tgt[1] : tgt[2]);
                    obs[o + 2 * nv + l8] = hh;
                    obs[o + 2 * nv + 3 + l8] = hh - gg;
                }
            }
            if (nobs) {
                if (l8 < nv) { nobs[o + l8] = q; nobs[o + nv + l8] = v; }
                if (l8 < 3) {
                    T hh = l8 == 0 ? site[0] : (l8 == 1 ? site[1] : site[2]);
                    T gg = l8 == 0 ? tgt[0] : (l8 == 1 ? tgt[1] : tgt[2]);
                    nobs[o + 2 * nv + l8] = hh;
                    nobs[o + 2 * nv + 3 + l8] = hh - gg;
                }
            }
        }
        cq = q;
        cv = v;
        for (int k = 0; k < 3; ++k) chand[k] = site[k];
        ST.mark(14);    // observation records, loop
    }
    ST.flush(diag, 0, lane);
    if (QUAD && diag && lane == 0 && q_read(qf, QF_STUCK)) atomicAdd(diag, 0x10000u);     // a hand-over timed out: the results are void
    // A rollout that diverged numerically (MuJoCo would have reset that simulation, DESIGN 7) carries a non-finite return: it
    // leaves the update as +inf - zero weight in the softmax updates, last in the elite ranking - instead of poisoning
    // the mean with a NaN
    if (!(fabs(q0acc) < INFINITY)) q0acc = INFINITY;
    if (fuse.q0_out && live && l8 == 0) fuse.q0_out[pid] = q0acc;
    // "real env" stepping on the device: particle 0 writes its final (qpos, qvel) back into a state vector
    // (EB: every workgroup's live particle, into its own state shard)
    if (state_out && (EB ? live : pid == 0) && l8 < nv) {
        double* so = EB ? state_out + (long)blockIdx.x * (2 * LANES + 3) : state_out;
        so[l8] = (double)q;
        so[LANES + l8] = (double)v;
    }
    if constexpr (MONO) { if (l8 == 0) dyn_lds[g] = live ? q0acc : INFINITY; }     // cost-to-go of my particle
    }   // (wave 0 / the one wave)
    if constexpr (MONO)
        mono_record<T, NT>(mop->lam, mop->tree + (long)blockIdx.x * (2 + HA), HA, dyn_lds, actT);
