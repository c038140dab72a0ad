// The tracker step of the PARC hot path: the fused post-physics pass (observation, reward, termination), the reference state, the
// observation gather of the other layouts, the device-side resets and the fail rates, written for gfx950 (MI355X): 64-lane wavefronts,
// 16-lane body groups, LDS-staged observation rows.  The stand-alone heightmap gather is in parc_hfgather.hip, the motion library and
// character-model kernels in parc_motion.hip, the motion optimiser's primitives in parc_pose_opt.hip, the learner's returns in
// parc_returns.hip.  C-ABI in include/parc_hip.h.  Reference citations are relative to the reference root.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_math.h"
#include "parc_math_pk.h"
#include "parc_fk_group.h"      // GRP, shfl16, sum16, any16, fk_consts_of, group_fk
#include "parc_hf_lookup.h"     // hf_lookup, hf_env_params
#include "parc_pose_lane.h"     // model_ok, joint_rot_to_dof
#include "parc_motion_query.h"  // make_query, query_quat, lerp_ref, query_root_pos

// the timing-ablation bits of track_post_kernel exist only in the diagnostics build (-DPARC_DIAG_BUILD)
#ifdef PARC_DIAG_BUILD
#define PARC_DIAG(...) __VA_ARGS__
#else
#define PARC_DIAG(...)
#endif

// 4 floats moved by one 16-byte instruction from / to an address that is only 4-byte aligned (global memory takes it)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
// The observation rows are written with the non-temporal hint: a launch ends when its last dirty line has left the XCD's L2 (the L2s
// of the 8 XCDs are not coherent, the next kernel may read the row from another one), and 22 MB of rows held back until then were a
// 1 us tail; streamed out as they are produced they overlap the pose arithmetic (15.8 -> 14.7 us per launch, same box).
#ifndef POST_PLAIN_STORES
#define POST_STORE4(p, v) __builtin_nontemporal_store((v), reinterpret_cast<f4u *>(p))
#else
#define POST_STORE4(p, v) (*reinterpret_cast<f4u *>(p) = (v))
#endif

// joint_dof_to_rot (parc_pose_lane.h) with the joint's constants already at hand (type, first dof, hinge axis)
// Both joint kinds end in axis_angle_to_quat (exp_map_to_quat of parc_math.h = the steps below, then that call): the lanes of a group
// differ in kind, so each kind's branch only prepares (axis, angle) and the common tail is issued once instead of once per kind.
PARC_DEV q4 joint_dof_to_rot(int jt, int d, v3 ax, const float *dof, int stride) {
    float an = 0.f;
    if (jt == PARC_JOINT_HINGE) {
        an = dof[d * stride];
    } else if (jt == PARC_JOINT_SPHERICAL) {
        const v3 em = mk3(dof[d * stride], dof[(d + 1) * stride], dof[(d + 2) * stride]);
        float a = fsqrt(dot3(em, em));
        const float ia = frcp(a);
        ax = v3{em.x * ia, em.y * ia, em.z * ia};
        if (!(a < 3.1415925f)) a = normalize_angle(a);       // identity below pi
        if (!(fabsf(a) > 1e-5f)) {
            ax = mk3(0.f, 0.f, 1.f);
            a = 0.f;
        }
        an = a;
    }
    const q4 q = axis_angle_to_quat(ax, an);
    return (jt == PARC_JOINT_HINGE || jt == PARC_JOINT_SPHERICAL) ? q : mk4(0.f, 0.f, 0.f, 1.f);
}

// ---- the same on two poses per lane (parc_math_pk.h): the cross-lane moves are per component, the arithmetic is packed
PARC_DEV f2 shfl16(f2 v, int src) { return f2{shfl16(v.x, src), shfl16(v.y, src)}; }
PARC_DEV q4p shfl16(q4p q, int src) { return q4p{shfl16(q.x, src), shfl16(q.y, src), shfl16(q.z, src), shfl16(q.w, src)}; }
PARC_DEV v3p shfl16(v3p v, int src) { return v3p{shfl16(v.x, src), shfl16(v.y, src), shfl16(v.z, src)}; }
template <bool LEAF_ROT = true>
PARC_DEV void group_fk(const fk_consts &k, int max_depth, v3p root_pos, q4p root_rot, q4p jq, v3p &pos, q4p &rot) {
    q4p lq = sp4(mk4(0.f, 0.f, 0.f, 1.f));
    if (k.dep > 0) lq = quat_mul(sp4(k.lrot), jq);
    const v3p lt = sp3(k.lt);
    pos = root_pos;
    rot = root_rot;
    for (int lev = 1; lev <= max_depth; ++lev) {
        v3p pp = shfl16(pos, k.par);
        q4p pr = shfl16(rot, k.par);
        if (k.dep == lev) {
            pos = pp + quat_rotate(pr, lt);
            if (LEAF_ROT || lev < max_depth) rot = quat_mul(pr, lq);
        }
    }
}

// =============================================================================================
// Fused post-physics pass.  A pose (simulated character, reference at t, targets at t+dt_s - two of those per group) is handled by a
// 16-lane group, lane b = body b; every wave writes the observation columns it produces itself.
// =============================================================================================
#define POST_EPB 4            // envs per workgroup
#define POST_MAX_THREADS 384  // 64 * (3 + (PARC_MAX_TAR_STEPS + 1) / 2): character, reference, target waves (two target steps per lane), heightmap wave
#define POST_MAX_ROW 1408
#define POST_STAGE_T 248      // two target steps of one env: 2 (9 + 6 (PARC_MAX_BODIES - 1) + 3 PARC_MAX_KEY_BODIES) = 246 floats
#define POST_STAGE_C 192      // the character's own columns: 12 + 6 (PARC_MAX_BODIES - 1) + PARC_MAX_DOFS + 3 PARC_MAX_KEY_BODIES = 190 floats
// Kernel arguments passed by value are loaded by the compiler in the entry block, all of them, and then live in scalar registers
// for the whole kernel: with ~2 KB of argument structs that is far more than the 102 SGPRs a wave has, and the overflow is kept in
// VGPR lanes (v_writelane at entry, v_readlane at every use - vector-issue slots).  kernarg_late hands out a pointer to a struct
// inside the kernel-argument segment that the optimiser cannot see through, so loads through it stay where they are written.
// Offsets = the by-value parameters of track_post_kernel in order, each 8-byte aligned (checked against the code object's
// metadata by tools/check_kernarg_offsets.py).
#define KARG_ALIGN8(x) (((x) + 7) & ~(size_t)7)
#define KARG_OFF_ML KARG_ALIGN8(sizeof(parc_char_model_t))
#define KARG_OFF_TER KARG_ALIGN8(KARG_OFF_ML + sizeof(parc_motion_lib_t))
#define KARG_OFF_CFG KARG_ALIGN8(KARG_OFF_TER + sizeof(parc_terrain_t))
#define KARG_OFF_BUF KARG_ALIGN8(KARG_OFF_CFG + sizeof(parc_track_cfg_t))
template <typename T>
PARC_DEV const __attribute__((address_space(4))) T *kernarg_late(size_t off) {
    const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const __attribute__((address_space(4))) T *)(p + off);
}

#ifndef POST_MIN_WAVES
// 6 waves per workgroup at <= 72 VGPRs: four workgroups per CU, all 1024 workgroups of a 4096-env launch resident in one round
// (measured, profiles/r03_wg_residency.txt: 6-wave workgroups stay one round at 72 VGPRs and need two at 80, 5-wave ones stay one round
// up to 80; until round 3 the kernel ran 8 waves per workgroup at 64 VGPRs)
#define POST_MIN_WAVES 7
#endif

// The columns a 16-lane group has written to its LDS segment go to the observation row as 16-byte stores, 4 consecutive floats per lane:
// the launch is bound by the number of vector-memory instructions (a wave-wide store of one float per lane at a 24-byte stride costs the
// CU's address path the same ~22 cycles as a store of 16 contiguous bytes per lane), so 23 strided stores of a target wave become 5.
// LDS operations of one wave complete in order: the wave barrier + fences only keep the compiler from moving them.
PARC_DEV void stage_out(const float *seg, float *dst, int n, int b) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n4 = n >> 2;
    for (int c = b; c < n4; c += GRP) {
        const float4 v = *reinterpret_cast<const float4 *>(seg + 4 * c);
        f4u o;
        o.x = v.x, o.y = v.y, o.z = v.z, o.w = v.w;
        POST_STORE4(dst + 4 * c, o);
    }
    for (int i = 4 * n4 + b; i < n; i += GRP) dst[i] = seg[i];
}

// Workgroup = POST_EPB envs, one ROLE per wave so no wave diverges:
//   wave 0          the simulated character of the 4 envs   (4 x 16 body lanes)  -> its own observation columns
//   wave 1          their reference poses at t                                   -> reward, done
//   wave 2 + p      target steps 2p and 2p + 1 of the 4 envs, one in each half of packed float2 values (p < ceil(S / 2))
//   last wave       the 4 x 441 heightmap samples (only launched with PARC_POST_HF)
// Phase 0 (28 lanes of wave 0: per-env and per-query scalars -> LDS) is the only thing the one barrier waits for; behind it the waves
// never meet again: each collects the columns it produces in an LDS segment of its own and writes them as 16-byte stores (stage_out).
__global__ __launch_bounds__(POST_MAX_THREADS, POST_MIN_WAVES) void track_post_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_terrain_t ter,
                                                                     parc_track_cfg_t cfg, parc_env_buffers_t buf,
                                                                     const int64_t *__restrict__ env_ids, int n_total, int what,
                                                                     const float *__restrict__ ray_xy) {
    __shared__ __attribute__((aligned(16))) float envd[POST_EPB][20];   // root pos 3 | root rot 4 | heading^-1 4 | env id | root vel 3 | ang vel 3
    __shared__ __attribute__((aligned(16))) float qryd[1 + PARC_MAX_TAR_STEPS][POST_EPB][12];   // idx0 idx1 blend - | loop shift xyz, time | tile offset xy, motion end
    __shared__ float tgt_xy[POST_EPB][2];
    // per-wave staging of the observation columns a wave produces (see stage_out): never shared between waves, no barrier
    __shared__ __attribute__((aligned(16))) float stage_t[(PARC_MAX_TAR_STEPS + 1) / 2][POST_EPB][POST_STAGE_T];
    __shared__ __attribute__((aligned(16))) float stage_c[POST_EPB][POST_STAGE_C];
    // per-body constants of the tree walk + the body's key slot, loaded once per workgroup (by the reference wave, which has nothing
    // else to do in front of the barrier) instead of as four (character and reference wave: nine) vector loads in every pose wave: lrot 4 | lt 3, parent | depth, key slot,
    // | joint type, first dof, - | hinge axis 3, -
    __shared__ __attribute__((aligned(16))) float bodyk[GRP][16];
    PARC_DIAG(if (what & 0x100000) return;)          // (timing diagnostic: the launch alone)
    const int tid = threadIdx.x;
    const int wv = tid >> 6, gg = (tid & 63) >> 4, b = tid & 15;
    const int B = m.num_bodies, J = B - 1, D = m.dof_size, K = cfg.num_key_bodies, S = cfg.num_tar_steps;
    const int H = (S + 1) >> 1;                          // target waves: two target steps per lane
    const bool is_char = wv == 0, is_ref = wv == 1, is_tar = wv >= 2 && wv < 2 + H, is_gat = wv == 2 + H;
    const int le = gg;
    const int el = blockIdx.x * POST_EPB + le;
    const bool masked = (what & PARC_POST_MASKED) != 0;
    if (masked) {
        // device-side reset: nothing to do for a workgroup whose envs all kept running (uniform: every wave leaves)
        int any = 0;
#pragma unroll
        for (int k = 0; k < POST_EPB; ++k) {
            int ek = blockIdx.x * POST_EPB + k;
            if (ek < n_total) any |= buf.env_mask[ek];
        }
        if (!any) return;
    }
    const bool live = el < n_total && (!masked || buf.env_mask[el] != 0);
    const int RS = cfg.obs_dim;
    const int Wc = 12 + 6 * J + D + 3 * K;   // char_obs width (136)
    const int Wt = 9 + 6 * J + 3 * K;        // one target step (105)
    const int row_len = cfg.obs_dim - cfg.num_ray_points;  // 871
    const bool valid = b < B;

    // ---- phase 0 (wave 0): the per-env and per-query scalars, ONE lane each instead of once per 16-lane group in
    // every wave: lane l -> env l & 3, query l >> 2 (0 = reference at t, s + 1 = target step s)
    if (wv == 0 && tid < POST_EPB * (1 + S)) {
        const int ple = tid & (POST_EPB - 1), pq = tid >> 2;
        const int pel = min((int)blockIdx.x * POST_EPB + ple, n_total - 1);
        const int pe = env_ids ? (int)env_ids[pel] : pel;
        const int64_t mid = buf.motion_ids[pe];
        // dataset clips: env time + the clip time the episode started at (dm_env.py:597-602); generated plans: the plan clock itself
        // (mgdm_env.py:476-480), handed over in the same per-env slot so that it is the exact number and not a rounded sum
        const float mtime = (what & PARC_POST_PLAN_CLOCK) ? buf.motion_time_offsets[pe] : buf.time_buf[pe] + buf.motion_time_offsets[pe];
        if (pq == 0) {
            const float *prs = buf.root_state + (size_t)pe * 13;
            const q4 cr = ld4(prs + 3);
            // global_obs (ig_char_env.py:585-590, mgdm_dm_util.py:476-500): the observation stays in world axes - the "heading frame" every
            // wave rotates into is the identity, and a target's key bodies are not offset by its root (selector in ed[4].z)
            const q4 hi = cfg.global_obs ? mk4(0.f, 0.f, 0.f, 1.f) : calc_heading_quat_inv_alg(cr);
            float4 *ed = reinterpret_cast<float4 *>(envd[ple]);
            ed[0] = make_float4(prs[0], prs[1], prs[2], cr.x);
            ed[1] = make_float4(cr.y, cr.z, cr.w, hi.x);
            ed[2] = make_float4(hi.y, hi.z, hi.w, __int_as_float(pe));
            ed[3] = make_float4(prs[7], prs[8], prs[9], prs[10]);
            ed[4] = make_float4(prs[11], prs[12], cfg.global_obs ? 0.f : 1.f, 0.f);
        }
        // K3 index part: MotionLib.calc_motion_frame at t (ref) or t + dt_s (targets); dm_env.py:570-582, mgdm_dm_util.py:279-302
        const float t = mtime + (pq > 0 ? cfg.tar_dt[pq - 1] : 0.f);
        const frame_query fq = make_query(ml, mid, t);
        // The frame rows themselves (root position included) are loaded by the pose lanes after the barrier, together with the
        // quaternions: this lane only publishes what does not need them - indices, blend, the loop shift of wrapping clips
        // (motion_lib.py:458-475) and the tile offset (_move_to_motion_terrain dm_env.py:604-615) - so the barrier is reached one
        // memory round trip earlier.
        v3 shift = mk3(0.f, 0.f, 0.f);
        if (fq.wrap) {
            const float *d = ml.pos_delta + 3 * mid;
            shift = mk3(fq.loop_phase * d[0], fq.loop_phase * d[1], fq.loop_phase * d[2]);
        }
        float4 *qd = reinterpret_cast<float4 *>(qryd[pq][ple]);
        qd[0] = make_float4(__int_as_float(fq.idx0), __int_as_float(fq.idx1), fq.blend, 0.f);
        // (reference query only) env time and the motion-end flag of DeepMimicEnv.update_done, dm_env.py:746-783: the clip
        // length / loop mode were just loaded for the query, the termination code reads the result from LDS
        const int motion_end = (pq == 0) && !(what & PARC_POST_PLAN_CLOCK) && (mtime >= ml.length[mid]) && (ml.loop_mode[mid] != 1);
        qd[1] = make_float4(shift.x, shift.y, shift.z, buf.time_buf[pe]);
        qd[2] = make_float4(buf.motion_xy_offset[2 * pe] - buf.env_offsets[3 * pe], buf.motion_xy_offset[2 * pe + 1] - buf.env_offsets[3 * pe + 1],
                            __int_as_float(motion_end), 0.f);
    }
    // xy target resample (PARC_POST_TARGETS): lanes 4 (1 + S) .. 4 (2 + S) - 1 of wave 0, one per env
    if (wv == 0 && tid >= POST_EPB * (1 + S) && tid < POST_EPB * (2 + S)) {
        const int ple = tid - POST_EPB * (1 + S);
        const int pel = blockIdx.x * POST_EPB + ple;
        const int pelc = min(pel, n_total - 1);
        const int pe = env_ids ? (int)env_ids[pelc] : pelc;
        float tx = buf.target_xy[2 * pe], ty = buf.target_xy[2 * pe + 1];
        if ((what & PARC_POST_TARGETS) && pel < n_total && (!masked || buf.env_mask[pe] != 0)) {
            // DeepMimicEnv._update_motion_targets  dm_env.py:617-654
            const float tm = buf.time_buf[pe];
            if (tm >= buf.next_target_time[pe]) {
                const float *u = buf.target_rand + 3 * (size_t)pe;
                const float fut = u[0] * (cfg.target_future_max - cfg.target_future_min) + cfg.target_future_min;
                const int64_t mid = buf.motion_ids[pe];
                const frame_query fq = make_query(ml, mid, tm + buf.motion_time_offsets[pe] + fut);
                const v3 pr = query_root_pos(ml, fq, mid);
                // N(0, 0.05) noise from the two remaining uniforms (Box-Muller)
                const float rr = 0.05f * fsqrt(-2.0f * __logf(fmaxf(1.0f - u[1], 1e-12f)));
                float sn, cs;
                fsincos(6.283185307179586f * u[2], sn, cs);
                tx = pr.x + buf.motion_xy_offset[2 * pe] - buf.env_offsets[3 * pe] + rr * cs;
                ty = pr.y + buf.motion_xy_offset[2 * pe + 1] - buf.env_offsets[3 * pe + 1] + rr * sn;
                float *wt = const_cast<float *>(buf.target_xy);
                wt[2 * pe] = tx;
                wt[2 * pe + 1] = ty;
                buf.next_target_time[pe] = tm + fut;
            }
        }
        tgt_xy[ple][0] = tx;
        tgt_xy[ple][1] = ty;
    }
    // K5 fused: RefCharEnv._refresh_ray_obs_hfs (mgdm_dm_util.py:158-179) for the 4 envs of this workgroup, by a wave of its own (the
    // last one, launched only when PARC_POST_HF is asked for): 16 lanes per env, 28 points per lane, same affine cell-unit form as
    // hf_gather_kernel.  The heightmap columns need the simulated root state only, nothing of phase 0: the wave derives the map of its
    // envs while wave 0 walks the dependent loads of phase 0, and walks its points while the pose waves work - nobody waits for it.
    // (Until round 3 all waves but wave 0 shared the gather in front of the barrier: 3.2 us during which no pose wave computed.)
    hf_env_prm gpr;
    int ghe = 0;
    bool glive = false;
    if (is_gat) {
        const int hel = (int)blockIdx.x * POST_EPB + gg;
        const int helc = min(hel, n_total - 1);
        ghe = env_ids ? (int)env_ids[helc] : helc;
        gpr = hf_env_params<true>(ghe, buf.root_state, buf.env_offsets, ter, 1.0f / ter.dx, 1.0f / ter.dy);
        glive = hel < n_total && (!masked || buf.env_mask[helc] != 0);
    }
    PARC_DIAG(if (what & 0x200000) return;)          // (timing diagnostic: launch + phase 0 + heightmap gather, no barrier)
    if (is_ref && gg == 0) {
        const fk_consts k = fk_consts_of(m, b);
        int ks = -1;
        for (int i = 0; i < K; ++i)
            if (cfg.key_body_ids[i] == b) ks = i;
        float4 *bk = reinterpret_cast<float4 *>(bodyk[b]);
        bk[0] = make_float4(k.lrot.x, k.lrot.y, k.lrot.z, k.lrot.w);
        bk[1] = make_float4(k.lt.x, k.lt.y, k.lt.z, __int_as_float(k.par));
        const bool jv = b > 0 && b < B;
        bk[2] = make_float4(__int_as_float(k.dep), __int_as_float(ks), __int_as_float(jv ? m.joint_type[b] : -1), __int_as_float(jv ? m.dof_idx[b] : 0));
        bk[3] = jv ? make_float4(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2], 0.f) : make_float4(0.f, 0.f, 1.f, 0.f);
    }
    __syncthreads();
    const int key_slot = __float_as_int(bodyk[b][9]);
    auto joint_rot_lds = [&](const float *dof2) {                // K1 (kin_char_model.py:478-491) on the staged joint constants
        const float4 k3 = reinterpret_cast<const float4 *>(bodyk[b])[3];
        return joint_dof_to_rot(__float_as_int(bodyk[b][10]), __float_as_int(bodyk[b][11]), mk3(k3.x, k3.y, k3.z), dof2, 2);
    };
    auto fk_consts_lds = [&]() {                                 // read where the walk starts, not held in registers until then
        fk_consts k;
        const float4 k0 = reinterpret_cast<const float4 *>(bodyk[b])[0], k1 = reinterpret_cast<const float4 *>(bodyk[b])[1];
        k.lrot = mk4(k0.x, k0.y, k0.z, k0.w);
        k.lt = mk3(k1.x, k1.y, k1.z);
        k.par = __float_as_int(k1.w);
        k.dep = __float_as_int(bodyk[b][8]);
        return k;
    };
    // diagnostic role ablations (timing only): bits 16/17/18 drop the target / reference / character waves
    PARC_DIAG(if (((what & 0x10000) && is_tar) || ((what & 0x20000) && is_ref) || ((what & 0x40000) && is_char)) return;)
    if (is_gat) {
        PARC_DIAG(if (what & 0x80000) return;)                   // (timing diagnostic: no heightmap wave)
        const int P = cfg.num_ray_points;
        const float max_i = (float)(ter.dim_x - 1), max_j = (float)(ter.dim_y - 1);
        // straight into the observation row; the 441 columns are a third of the row's bytes.  The launch is bound by the NUMBER of
        // vector-memory instructions its waves issue (about 22 cycles of a CU's address path each, whatever they move), so a lane takes
        // 4 consecutive points: their (x, y) pairs arrive as two 16-byte loads and leave as one 16-byte store, 4 scattered cell reads
        // in between - 7 instructions per 4 points instead of 12.
        float *hrow = buf.obs + (size_t)ghe * RS + (RS - P);
        auto cell = [&](float rx, float ry) {
            float ui = fmaf(rx, gpr.ax, fmaf(ry, gpr.bx, gpr.cx));
            float uj = fmaf(rx, gpr.ay, fmaf(ry, gpr.by, gpr.cy));
            ui = __builtin_amdgcn_fmed3f(rintf(ui), 0.f, max_i);
            uj = __builtin_amdgcn_fmed3f(rintf(uj), 0.f, max_j);
            return __builtin_amdgcn_fmed3f(ter.hf[(int)ui * ter.dim_y + (int)uj] - gpr.gz, cfg.min_obs_h, cfg.max_obs_h);
        };
        const int full = P >> 2;                                 // chunks of 4 points
#pragma unroll 2
        for (int c = glive ? b : full; c < full; c += GRP) {
            const f4u r0 = *reinterpret_cast<const f4u *>(ray_xy + 8 * c), r1 = *reinterpret_cast<const f4u *>(ray_xy + 8 * c + 4);
            f4u h;
            h.x = cell(r0.x, r0.y);
            h.y = cell(r0.z, r0.w);
            h.z = cell(r1.x, r1.y);
            h.w = cell(r1.z, r1.w);
            POST_STORE4(hrow + 4 * c, h);
        }
        for (int p = glive ? 4 * full + b : P; p < P; p += GRP) hrow[p] = cell(ray_xy[2 * p], ray_xy[2 * p + 1]);
        return;
    }
    if (is_ref && !(what & PARC_POST_REWARD_DONE)) return;      // the reference wave computes reward / termination; the reference STATE is ref_state_group's

    // ---- target waves: DeepMimicEnv.compute_tar_obs + compute_tar_obs  dm_env.py:686-718, mgdm_dm_util.py:462-519
    // Wave 2 + p carries target steps 2p and 2p + 1 of the 4 envs, one in each component of float2 values: the clip
    // sampling (K3), the tree walk (K2) and the heading-frame epilogue (K7) of both steps issue as packed multiply-adds.
    if (is_tar) {
        if (!((what & PARC_POST_OBS) && live)) return;          // (a whole 16-lane group: the cross-lane moves stay inside a group)
        const int sA = 2 * (wv - 2), sB = sA + 1;                // adjacent steps: their columns are one contiguous run of the row
        const bool hasB = sB < S;                                // odd S: the last wave's second component repeats step sA and stores nothing
        const int qB = hasB ? sB : sA;
        const int e = __float_as_int(envd[le][11]);
        float *row = buf.obs + (size_t)e * RS;
        const float4 a0 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[0], a1 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[1],
                     a2 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[2];
        const float4 b0 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[0], b1 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[1],
                     b2 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[2];
        const float *rA0 = ml.frames + (size_t)__float_as_int(a0.x) * ml.row_stride, *rA1 = ml.frames + (size_t)__float_as_int(a0.y) * ml.row_stride;
        const float *rB0 = ml.frames + (size_t)__float_as_int(b0.x) * ml.row_stride, *rB1 = ml.frames + (size_t)__float_as_int(b0.y) * ml.row_stride;
        const f2 blend = mk2(a0.z, b0.z);
        q4p jq = sp4(mk4(0.f, 0.f, 0.f, 1.f));
        if (valid) {
            const float4 xa = *reinterpret_cast<const float4 *>(rA0 + 4 * b), ya = *reinterpret_cast<const float4 *>(rA1 + 4 * b);
            const float4 xb = *reinterpret_cast<const float4 *>(rB0 + 4 * b), yb = *reinterpret_cast<const float4 *>(rB1 + 4 * b);
            jq = slerp(q4p{mk2(xa.x, xb.x), mk2(xa.y, xb.y), mk2(xa.z, xb.z), mk2(xa.w, xb.w)},
                       q4p{mk2(ya.x, yb.x), mk2(ya.y, yb.y), mk2(ya.z, yb.z), mk2(ya.w, yb.w)}, blend);
        }
        PARC_DIAG(if ((what & 0x400000) && jq.x.x != 123.f) return;)       // (timing diagnostic: a target wave up to its blended joint rotations)
        // root position: lerp of the two rows, + loop shift, + tile offset (the order of query_root_pos and dm_env.py:604-615)
        v3p p_root;
        {
            const float *pa0 = rA0 + ml.off_pos, *pa1 = rA1 + ml.off_pos, *pb0 = rB0 + ml.off_pos, *pb1 = rB1 + ml.off_pos;
            p_root = v3p{lerp_ref(mk2(pa0[0], pb0[0]), mk2(pa1[0], pb1[0]), blend), lerp_ref(mk2(pa0[1], pb0[1]), mk2(pa1[1], pb1[1]), blend),
                         lerp_ref(mk2(pa0[2], pb0[2]), mk2(pa1[2], pb1[2]), blend)};
            p_root = p_root + v3p{mk2(a1.x, b1.x), mk2(a1.y, b1.y), mk2(a1.z, b1.z)};
            p_root.x += mk2(a2.x, b2.x);
            p_root.y += mk2(a2.y, b2.y);
        }
        if (valid) {
            const f2 ct = lerp_ref(mk2(rA0[ml.off_contacts + b], rB0[ml.off_contacts + b]), mk2(rA1[ml.off_contacts + b], rB1[ml.off_contacts + b]), blend);
            row[Wc + S * Wt + sA * B + b] = ct.x;
            if (hasB) row[Wc + S * Wt + sB * B + b] = ct.y;
        }
        // The tree walk starts from (root position, root rotation) in lane 0 and overwrites every other lane at its level, so the lanes'
        // own joint rotations serve as the initial value; the root pose is fetched from lane 0 again afterwards instead of being kept
        // in 14 registers through the walk.
        v3p pos;
        q4p rot;
        group_fk<false>(fk_consts_lds(), m.max_depth, p_root, jq, jq, pos, rot);
        asm volatile("" ::: "memory");                          // the simulated root pose and heading are only needed from here on
        PARC_DIAG(if ((what & 0x800000) && pos.x.x != 123.f) return;)      // (timing diagnostic: a target wave up to the end of its tree walk)
        p_root = shfl16(pos, 0);
        const float4 e0 = reinterpret_cast<const float4 *>(envd[le])[0], e1 = reinterpret_cast<const float4 *>(envd[le])[1],
                     e2 = reinterpret_cast<const float4 *>(envd[le])[2];
        const v3p c_pos = sp3(mk3(e0.x, e0.y, e0.z));
        const q4p hinv = sp4(mk4(e1.w, e2.x, e2.y, e2.z));
        float *seg = stage_t[wv - 2][le];                        // step sA at seg[0, Wt), step sB at seg[Wt, 2 Wt)
        const v3p rpo = quat_rotate(hinv, p_root - c_pos);
        if (b == 0) {
            seg[0] = rpo.x.x, seg[1] = rpo.y.x, seg[2] = rpo.z.x;
            seg[Wt] = rpo.x.y, seg[Wt + 1] = rpo.y.y, seg[Wt + 2] = rpo.z.y;
        }
        // lane 0: heading-relative root rotation at o+3 (the lane's own quaternion IS the root rotation); lane b: joint b-1 at
        // o + 9 + 6 (b-1) = o + 3 + 6 b
        const q4p hr = quat_mul(hinv, jq);
        if (valid) {
            f2 tn[6];
            quat_to_tan_norm(b == 0 ? hr : jq, tn);
#pragma unroll
            for (int k = 0; k < 6; ++k) seg[3 + 6 * b + k] = tn[k].x, seg[Wt + 3 + 6 * b + k] = tn[k].y;
        }
        if (key_slot >= 0) {
            const v3p kp = quat_rotate(hinv, pos - p_root) + envd[le][18] * rpo;     // (+ rpo unless global_obs)
            float *ka = seg + 9 + 6 * J + 3 * key_slot;
            ka[0] = kp.x.x, ka[1] = kp.y.x, ka[2] = kp.z.x;
            ka[Wt] = kp.x.y, ka[Wt + 1] = kp.y.y, ka[Wt + 2] = kp.z.y;
        }
        PARC_DIAG(if ((what & 0x1000000) && seg[b] != 123.f) return;)      // (timing diagnostic: a target wave without its stores)
        stage_out(seg, row + Wc + sA * Wt, hasB ? 2 * Wt : Wt, b);
        return;
    }

    const int e = __float_as_int(envd[le][11]);
    const float *dofs = buf.dof_state + (size_t)e * D * 2;  // interleaved pos,vel
    // every wave writes its own columns of the observation row straight to memory as it produces them: after the first barrier the
    // waves of a workgroup never meet again, so the stores of the early finishers overlap the arithmetic of the late ones (until
    // round 3 the rows were assembled in LDS and streamed out behind a second barrier: 3.6 of 17.7 us with every SIMD idle)
    float *row = buf.obs + (size_t)e * RS;

    // ---- phase A: every group gets its pose (root transform + one joint rotation per lane)
    frame_query fq;
    q4 jq = mk4(0.f, 0.f, 0.f, 1.f);
    v3 p_root = mk3(0.f, 0.f, 0.f);
    q4 r_root = mk4(0.f, 0.f, 0.f, 1.f);
    if (is_char) {
        p_root = mk3(envd[le][0], envd[le][1], envd[le][2]);
        r_root = mk4(envd[le][3], envd[le][4], envd[le][5], envd[le][6]);
        if (valid && b > 0) jq = joint_rot_lds(dofs);      // K1 (kin_char_model.py:478-491)
    } else {
        const float4 q0 = reinterpret_cast<const float4 *>(qryd[0][le])[0];
        const float4 q1 = reinterpret_cast<const float4 *>(qryd[0][le])[1];
        const float4 q2 = reinterpret_cast<const float4 *>(qryd[0][le])[2];
        fq.idx0 = __float_as_int(q0.x);
        fq.idx1 = __float_as_int(q0.y);
        fq.blend = q0.z;
        fq.row0 = ml.frames + (size_t)fq.idx0 * ml.row_stride;
        fq.row1 = ml.frames + (size_t)fq.idx1 * ml.row_stride;
        if (valid) jq = query_quat(fq, b);
        {
            // root position: lerp of the two rows, + loop shift, + tile offset (the order of query_root_pos and dm_env.py:604-615)
            const float *p0 = fq.row0 + ml.off_pos, *p1 = fq.row1 + ml.off_pos;
            p_root = mk3(lerp_ref(p0[0], p1[0], fq.blend), lerp_ref(p0[1], p1[1], fq.blend), lerp_ref(p0[2], p1[2], fq.blend));
            p_root = p_root + mk3(q1.x, q1.y, q1.z);
            p_root.x += q2.x;
            p_root.y += q2.y;
        }
        r_root = shfl16(jq, 0);
    }
    // ---- phase B: K2 forward kinematics, level-synchronous inside the 16-lane group
    // (kept in the reference's composition order root -> leaf: slerp between nearly identical frames returns slightly
    // non-unit quaternions, for which the rotation formula is not associative, so a reassociated tree walk - e.g. pointer
    // doubling in the root frame - drifts ~1e-4 from the reference's body positions)
    v3 pos;
    q4 rot;
    group_fk<false>(fk_consts_lds(), m.max_depth, p_root, r_root, jq, pos, rot);

    // the simulated root pose and heading are only needed from here on: read them after the tree walk (11 fewer live
    // registers through it; the compiler barrier keeps the LDS reads from being hoisted back up)
    asm volatile("" ::: "memory");
    const float4 e0 = reinterpret_cast<const float4 *>(envd[le])[0], e1 = reinterpret_cast<const float4 *>(envd[le])[1],
                 e2 = reinterpret_cast<const float4 *>(envd[le])[2];
    const v3 c_pos = mk3(e0.x, e0.y, e0.z);
    const q4 c_rot = mk4(e0.w, e1.x, e1.y, e1.z);
    const q4 hinv = mk4(e1.w, e2.x, e2.y, e2.z);

    // ---- phase C: per-group epilogues
    if (is_char) {
        if ((what & PARC_POST_OBS) && live) {
            // compute_char_obs  envs/ig_char_env.py:582-626 (global_obs False, no root height); the Wc columns are collected in the
            // wave's LDS segment and leave as 16-byte stores (stage_out)
            float *seg = stage_c[le];
            if (b == 0) {
                quat_to_tan_norm(quat_mul(hinv, c_rot), seg);
                st3(seg + 6, quat_rotate(hinv, ld3(envd[le] + 12)));     // simulated root velocities, staged by phase 0
                st3(seg + 9, quat_rotate(hinv, ld3(envd[le] + 15)));
            } else if (valid) {
                quat_to_tan_norm(jq, seg + 12 + 6 * (b - 1));
            }
            #pragma unroll 1
            for (int d = b; d < D; d += GRP) seg[12 + 6 * J + d] = dofs[2 * d + 1];
            if (key_slot >= 0) st3(seg + 12 + 6 * J + D + 3 * key_slot, quat_rotate(hinv, pos - c_pos));
            stage_out(seg, row, Wc, b);
            // char contacts  ig_parkour_env.py:841-848
            if (valid) {
                v3 f = ld3(buf.contact_forces + ((size_t)e * B + b) * 3);
                row[Wc + S * Wt + S * B + b] = fsqrt(dot3(f, f)) > cfg.contact_eps ? 1.f : 0.f;
            }
        }
        if ((what & PARC_POST_OBS) && b == 0 && live) {
            // values of the optional observation columns (has_target_xy_obs ig_parkour_env.py:1212-1224: the xy target seen from the
            // root, rotate_2d_vec(target - root_xy, -heading) = the heading-inverse rotation of (dx, dy, 0); global_root_height_obs
            // ig_char_env.py:618-620: root height) for parc_assemble_obs
            float *aux = kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF)->obs_aux;
            if (aux) {
                const q4 th = kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG)->global_obs ? calc_heading_quat_inv_alg(c_rot) : hinv;   // always the heading
                const v3 lt = quat_rotate(th, mk3(tgt_xy[le][0] - c_pos.x, tgt_xy[le][1] - c_pos.y, 0.f));
                reinterpret_cast<float4 *>(aux)[e] = make_float4(c_pos.z, lt.x, lt.y, 0.f);
            }
        }
        if ((what & PARC_POST_REWARD_DONE) && b == 0 && live) {
            // task terms  ig_parkour_env.py:1346-1393 (logged; they scale the reward only if rel_task_w > 0).  They read the simulated
            // root and the xy target only - nothing of the reference pose - so the character wave, the first to finish, computes them
            // instead of the reward wave, whose instruction stream is the longest of the workgroup.
            const auto &rbuf = *kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF);
            const auto &rcfg = *kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG);
            const int N = rbuf.reward_terms_stride > 0 ? rbuf.reward_terms_stride : rbuf.num_envs;
            float tx = tgt_xy[le][0] - c_pos.x, ty = tgt_xy[le][1] - c_pos.y;
            float terr = tx * tx + ty * ty;
            float task_r1 = fexp(-0.075f * terr);
            float tl = fsqrt(terr);
            float itl = frcp(tl);
            float dxn = tl > 0.01f ? tx * itl : 0.f, dyn = tl > 0.01f ? ty * itl : 0.f;
            float mve = fmaxf(2.0f - (dxn * envd[le][12] + dyn * envd[le][13]), 0.f);
            float min_vel_r = fexp(-(mve * mve));
            // heading direction (cos h, sin h) = normalised xy of the rotated x axis
            float ha = 1.0f - 2.0f * (c_rot.y * c_rot.y + c_rot.z * c_rot.z), hb = 2.0f * (c_rot.w * c_rot.z + c_rot.x * c_rot.y);
            float hn2 = ha * ha + hb * hb;
            float hir = __builtin_amdgcn_rsqf(hn2);
            float chd = hn2 > 0.f ? ha * hir : 1.0f, shd = hn2 > 0.f ? hb * hir : 0.0f;
            float he = fmaxf(1.0f - (dxn * chd + dyn * shd), 0.f);
            float task2 = min_vel_r * fexp(-(he * he));
            float task_r = rcfg.task1_w * task_r1 + rcfg.task2_w * task2;
            if (terr < rcfg.target_radius * rcfg.target_radius) task_r = 1.0f;
            rbuf.reward_terms[6 * (size_t)N + e] = task_r1;
            rbuf.reward_terms[7 * (size_t)N + e] = task2;
            rbuf.reward_terms[8 * (size_t)N + e] = task_r;
        }
    }
    // ---- reference wave, part 1 (before the barrier, while the target waves are still busy): reference state out
    // Everything the reference wave does lives in this one branch (its values never meet the other roles' registers), including
    // its own copies of the two barriers: it requests the simulator outputs it needs, writes the reference state, meets the
    // other waves at B1, passes B2 at once, and finishes reward / termination while they gather the heightmap and copy out.
    if (is_ref) {
      // the reference wave is the only user of most output pointers and of the reward / termination parameters: it reads them from the
      // kernel-argument block HERE (see kernarg_late) instead of having them loaded at kernel entry and kept in - or spilled from -
      // scalar registers by every wave
      const auto &rbuf = *kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF);
      const auto &rcfg = *kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG);
      const v3 r_pos = p_root;
      const q4 r_rot = r_root;
      const q4 rq = jq;
      float r_contact = 0.f;
      v3 r_vel = mk3(0.f, 0.f, 0.f), r_avel = mk3(0.f, 0.f, 0.f);
      if (what & (PARC_POST_REF | PARC_POST_REWARD_DONE)) {
        // DeepMimicEnv._update_ref_motion  dm_env.py:570-595
        r_contact = valid ? lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend) : 0.f;
        r_vel = ld3(fq.row0 + ml.off_root_vel);
        r_avel = ld3(fq.row0 + ml.off_root_ang_vel);
    }
        if (what & (PARC_POST_REF | PARC_POST_REWARD_DONE)) {
            if (what & PARC_POST_REWARD_DONE) {
                // compute_deepmimic_reward  mgdm_dm_util.py:327-390 (track_root, track_root_h)
                float pose_e = 0.f, vel_e = 0.f, key_e = 0.f, cpen = 0.f;
                int pose_fail = 0, fall_contact = 0, fall_height = 0;
                const v3 sim_pos = ld3(rbuf.rigid_body_state + ((size_t)e * B + (valid ? b : 0)) * 13);
                const v3 sim_root = shfl16(sim_pos, 0);          // body 0 is the root
                const v3 sim_f = ld3(rbuf.contact_forces + ((size_t)e * B + (valid ? b : 0)) * 3);
                // rotation differences, one evaluation for the group: lane b > 0 its joint (simulated vs reference), lane 0 - which has no
                // joint - the ROOT rotation difference that the reward's root term and the termination test need (same function, same inputs
                // as a second call by lane 0 alone would see)
                float rot_diff = 0.f;
                if (valid) {
                    // the simulated character's joint rotation (K1), computed here too: taking it from the character wave would need a
                    // second barrier, and with it every wave of the workgroup would wait for the slowest one
                    q4 cj = c_rot;
                    if (b > 0) cj = joint_rot_lds(dofs);
                    q4 rj = rq;                                         // (lane 0: rq = r_rot, the reference root rotation)
                    if (!rcfg.track_root && b == 0) {                   // convert_to_local (mgdm_dm_util.py:304-325,358-360): heading-relative root rotations
                        cj = quat_mul(calc_heading_quat_inv_alg(c_rot), c_rot);
                        rj = quat_mul(calc_heading_quat_inv_alg(r_rot), r_rot);
                    }
                    rot_diff = quat_diff_angle(cj, rj);
                    if (b > 0) pose_e = rcfg.joint_err_w[b - 1] * rot_diff * rot_diff;
                }
                #pragma unroll 1
                for (int d = b; d < D; d += GRP) {
                    float dv = fq.row0[ml.off_dof_vel + d] - dofs[2 * d + 1];
                    vel_e += rcfg.dof_err_w[d] * dv * dv;
                }
                if (key_slot >= 0) {
                    v3 kr = pos - r_pos, kc = sim_pos - c_pos;
                    if (!rcfg.track_root) {                             // key bodies in each character's own heading frame
                        kr = quat_rotate(calc_heading_quat_inv_alg(r_rot), kr);
                        kc = quat_rotate(calc_heading_quat_inv_alg(c_rot), kc);
                    }
                    v3 df = kr - kc;
                    key_e = dot3(df, df);
                }
                if (valid) {
                    // compute_contact_reward  mgdm_dm_util.py:555-576
                    const v3 f = sim_f;
                    float fn = fminf(fsqrt(dot3(f, f)), 1.0f);
                    float cr = -(1.0f - r_contact) * fn;
                    cr += r_contact * fn;
                    cpen = rcfg.contact_w[b] * cr;
                    // compute_done  mgdm_dm_util.py:392-460
                    if (b > 0) {
                        v3 df = (pos - r_pos) - (sim_pos - sim_root);
                        float lim = rcfg.pose_termination_dist[b - 1];
                        pose_fail = dot3(df, df) > lim * lim;
                    }
                    if (rcfg.num_contact_bodies > 0 && !rcfg.contact_body_mask[b]) {
                        fall_contact = fabsf(f.x) > 0.1f || fabsf(f.y) > 0.1f || fabsf(f.z) > 0.1f;
                        float th = hf_lookup(ter, sim_pos.x + rbuf.env_offsets[3 * e], sim_pos.y + rbuf.env_offsets[3 * e + 1]) + rcfg.termination_height;
                        fall_height = sim_pos.z < th;
                    }
                }
                pose_e = sum16(pose_e);
                vel_e = sum16(vel_e);
                key_e = sum16(key_e);
                cpen = sum16(cpen);
                pose_fail = any16(pose_fail);
                fall_contact = any16(fall_contact);
                fall_height = any16(fall_height);
                if (b == 0 && live) {
                    v3 dp = r_pos - c_pos;
                    if (!rcfg.track_root) dp.x = dp.y = 0.f;     // mgdm_dm_util.py:346-347
                    if (!rcfg.track_root_h) dp.z = 0.f;          // mgdm_dm_util.py:349-350
                    float root_pos_err = dot3(dp, dp);
                    const float rre = rot_diff;
                    float rre2 = rre * rre;
                    v3 cv = ld3(envd[le] + 12), cw = ld3(envd[le] + 15), rv = r_vel, rw = r_avel;
                    if (!rcfg.track_root) {                      // root velocities in each character's own heading frame
                        const q4 hc = calc_heading_quat_inv_alg(c_rot), hr = calc_heading_quat_inv_alg(r_rot);
                        cv = quat_rotate(hc, cv); cw = quat_rotate(hc, cw);
                        rv = quat_rotate(hr, rv); rw = quat_rotate(hr, rw);
                    }
                    v3 dv = rv - cv, dw = rw - cw;
                    float pose_r = fexp(-0.25f * pose_e);
                    float vel_r = fexp(-0.01f * vel_e);
                    float root_pose_r = fexp(-5.0f * (root_pos_err + 0.1f * rre2));
                    float root_vel_r = fexp(-1.0f * (dot3(dv, dv) + 0.1f * dot3(dw, dw)));
                    float key_r = fexp(-10.0f * key_e);
                    float cp = cpen / (float)B;
                    // ig_parkour_env.py:1317-1339,1404
                    float dm = rcfg.reward_w[0] * pose_r + rcfg.reward_w[1] * vel_r + rcfg.reward_w[2] * root_pose_r +
                               rcfg.reward_w[3] * root_vel_r + rcfg.reward_w[4] * key_r;
                    if (rcfg.use_contact_info) dm += cp;        // ig_parkour_env.py:1323-1339
                    rbuf.reward[e] = rcfg.rel_deepmimic_w * dm;
                    const int N = rbuf.reward_terms_stride > 0 ? rbuf.reward_terms_stride : rbuf.num_envs;
                    rbuf.reward_terms[0 * (size_t)N + e] = pose_r;
                    rbuf.reward_terms[1 * (size_t)N + e] = vel_r;
                    rbuf.reward_terms[2 * (size_t)N + e] = root_pose_r;
                    rbuf.reward_terms[3 * (size_t)N + e] = root_vel_r;
                    rbuf.reward_terms[4 * (size_t)N + e] = key_r;
                    rbuf.reward_terms[5 * (size_t)N + e] = cp;
                    // done
                    const float tm = qryd[0][le][7];
                    int done = PARC_DONE_NULL;
                    if (tm >= rcfg.episode_length) done = PARC_DONE_TIME;
                    if (rcfg.enable_early_termination) {
                        int failed = 0;
                        if (rcfg.num_contact_bodies > 0) failed = fall_contact && fall_height;
                        if (rcfg.pose_termination) {
                            int pf = pose_fail;
                            if (rcfg.track_root) {
                                v3 dr = sim_root - r_pos;
                                pf |= dot3(dr, dr) > rcfg.root_pos_termination_dist * rcfg.root_pos_termination_dist;
                                pf |= fabsf(rre) > rcfg.root_rot_termination_angle;
                            }
                            failed |= pf;
                        }
                        if (!(tm > 1e-5f)) failed = 0;
                        if (failed) done = PARC_DONE_FAIL;
                    }
                    // DeepMimicEnv.update_done  dm_env.py:746-783
                    const int motion_end = __float_as_int(qryd[0][le][10]);
                    int kind = 0;
                    if (done != PARC_DONE_NULL || motion_end) kind = (done == PARC_DONE_FAIL) ? 1 : 2;
                    if (motion_end) done = PARC_DONE_FAIL;
                    rbuf.done[e] = done;
                    rbuf.done_kind[e] = kind;
                }
            }
        }
        return;
    }
}

// =============================================================================================
// The reference STATE of one env: DeepMimicEnv._update_ref_motion (dm_env.py:570-595: ref_* buffers, K3 + K2 + K4 at the clip time) and,
// for a restart, the character state initialised from it (RefCharEnv._char_state_init_from_ref + add_noise_to_char_state,
// mgdm_dm_util.py:119-136), by one 16-lane group (lane b = body b).
// Until round 3 this was the first half of the reference wave of track_post_kernel, in front of the reward: the tail every launch
// waited for (full launch 16.5 us, without these stores 15.1 us).  Nothing in a step reads what it writes - the reward wave samples the
// pose itself - so it left the fused kernel: ref_state_kernel runs it alone (a restart's first launch is this small kernel instead of
// the 8-wave one), and in the rollout step it rides as extra workgroups of the fail-rate launch (step_tail_kernel), whose 64 workgroups
// leave almost the whole chip idle for the 10 us their serial walk takes.
// =============================================================================================
PARC_DEV void ref_state_group(const parc_char_model_t &m, const parc_motion_lib_t &ml, const parc_env_buffers_t &buf, const int64_t *env_ids,
                              int n_total, int what, int el, int b) {
    const bool masked = (what & PARC_POST_MASKED) != 0;
    const int elc = min(el, n_total - 1);
    const bool live = el < n_total && (!masked || buf.env_mask[elc] != 0);
    if (masked && !__any(live)) return;                         // wave-uniform: nothing flagged among this wave's 4 envs
    const int e = env_ids ? (int)env_ids[elc] : elc;
    const int B = m.num_bodies, J = B - 1, D = m.dof_size;
    const bool valid = b < B;
    const int64_t mid = buf.motion_ids[e];
    // dataset clips: env time + the clip time the episode started at; generated plans: the plan clock itself (see track_post_kernel)
    const float mtime = (what & PARC_POST_PLAN_CLOCK) ? buf.motion_time_offsets[e] : buf.time_buf[e] + buf.motion_time_offsets[e];
    const frame_query fq = make_query(ml, mid, mtime);
    q4 rq = mk4(0.f, 0.f, 0.f, 1.f);
    if (valid) rq = query_quat(fq, b);
    // root position in the reference's order: lerp, + loop shift, + tile offset (query_root_pos, dm_env.py:604-615)
    v3 r_pos = query_root_pos(ml, fq, mid);
    r_pos.x += buf.motion_xy_offset[2 * e] - buf.env_offsets[3 * e];
    r_pos.y += buf.motion_xy_offset[2 * e + 1] - buf.env_offsets[3 * e + 1];
    const q4 r_rot = shfl16(rq, 0);
    v3 pos;
    q4 rot;
    group_fk<false>(m, b, r_pos, r_rot, rq, pos, rot);
    if (!live) return;
    const float r_contact = valid ? lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend) : 0.f;
    const v3 r_vel = ld3(fq.row0 + ml.off_root_vel), r_avel = ld3(fq.row0 + ml.off_root_ang_vel);
    if (b == 0) {
        st3(buf.ref_root_pos + 3 * (size_t)e, r_pos);
        st4(buf.ref_root_rot + 4 * (size_t)e, r_rot);
        st3(buf.ref_root_vel + 3 * (size_t)e, r_vel);
        st3(buf.ref_root_ang_vel + 3 * (size_t)e, r_avel);
    } else if (valid) {
        st4(buf.ref_joint_rot + ((size_t)e * J + (b - 1)) * 4, rq);
        joint_rot_to_dof(m, b, rq, buf.ref_dof_pos + (size_t)e * D);      // K4
    }
    if (valid) {
        buf.ref_contacts[(size_t)e * B + b] = r_contact;
        st3(buf.ref_body_pos + ((size_t)e * B + b) * 3, pos);
    }
#pragma unroll 1
    for (int d = b; d < D; d += GRP) buf.ref_dof_vel[(size_t)e * D + d] = fq.row0[ml.off_dof_vel + d];
    if (what & PARC_POST_INIT_CHAR) {
        float *wrs = const_cast<float *>(buf.root_state) + (size_t)e * 13;
        float *wds = const_cast<float *>(buf.dof_state) + (size_t)e * D * 2;
        if (b == 0) {
            v3 ip = r_pos;
            if (buf.init_noise_xy) {
                ip.x += buf.init_noise_xy[2 * e];
                ip.y += buf.init_noise_xy[2 * e + 1];
            }
            st3(wrs, ip);
            st4(wrs + 3, r_rot);
            st3(wrs + 7, r_vel);
            st3(wrs + 10, r_avel);
        } else if (valid) {
            joint_rot_to_dof(m, b, rq, buf.ref_dof_pos + (size_t)e * D, wds);
        }
#pragma unroll 1
        for (int d = b; d < D; d += GRP) wds[2 * d + 1] = fq.row0[ml.off_dof_vel + d];
    }
}

#define REF_STATE_THREADS 256      // 16 envs per workgroup
__global__ __launch_bounds__(REF_STATE_THREADS) void ref_state_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_env_buffers_t buf,
                                                                      const int64_t *__restrict__ env_ids, int n_total, int what) {
    ref_state_group(m, ml, buf, env_ids, n_total, what, (int)(blockIdx.x * (REF_STATE_THREADS / GRP) + (threadIdx.x >> 4)), threadIdx.x & 15);
}

#ifdef PARC_DIAG_BUILD
// occupancy probe: bytes of dynamic LDS added to every workgroup of track_post_kernel (fewer workgroups resident per CU); diagnostics build only
static int g_post_lds_pad = 0;
extern "C" int parc_tune_post_lds_pad(int bytes) {
    if (bytes < 0 || bytes > 120 * 1024) return PARC_EINVAL;
    g_post_lds_pad = bytes;
    return PARC_OK;
}
#define POST_LDS_PAD g_post_lds_pad
#else
#define POST_LDS_PAD 0
#endif

static int track_post_step_impl(void *stream, const parc_char_model_t &model, const parc_motion_lib_t &mlib, const parc_terrain_t &terrain,
                                const parc_track_cfg_t &cfg, const parc_env_buffers_t &buf, const int64_t *env_ids, int n_sel, int what,
                                const float *ray_xy, hipEvent_t start_event, hipEvent_t stop_event) {
    if (!model_ok(model) || mlib.num_bodies != model.num_bodies || mlib.dof_size != model.dof_size) return PARC_EINVAL;
#ifndef PARC_DIAG_BUILD
    if (what & ~PARC_POST_ALL) return PARC_EINVAL;   // only the documented PARC_POST_* bits (the timing-ablation bits exist in the diagnostics build only)
#endif
    if (cfg.num_tar_steps < 0 || cfg.num_tar_steps > PARC_MAX_TAR_STEPS || cfg.num_key_bodies > PARC_MAX_KEY_BODIES) return PARC_EUNSUPPORTED;
    const int B = model.num_bodies, J = B - 1, D = model.dof_size, K = cfg.num_key_bodies, S = cfg.num_tar_steps;
    const int row_len = (12 + 6 * J + D + 3 * K) + S * (9 + 6 * J + 3 * K) + S * B + B;
    if (row_len + cfg.num_ray_points != cfg.obs_dim || cfg.obs_dim > POST_MAX_ROW || (cfg.obs_dim & 3)) return PARC_EINVAL;
    if (what & PARC_POST_HF) {
        if (!(what & PARC_POST_OBS) || !ray_xy || !terrain.hf) return PARC_EINVAL;
    }
    if (((uintptr_t)buf.obs & 15) || ((uintptr_t)mlib.frames & 15) || (mlib.row_stride & 3)) return PARC_EINVAL;
    if ((what & PARC_POST_MASKED) && (env_ids || !buf.env_mask)) return PARC_EINVAL;
    if ((what & PARC_POST_INIT_CHAR) && !(what & PARC_POST_REF)) return PARC_EINVAL;
    if ((what & PARC_POST_TARGETS) && (!buf.next_target_time || !buf.target_rand)) return PARC_EINVAL;
    int n = env_ids ? n_sel : buf.num_envs;
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    if (what & PARC_POST_REF) {
        // the reference state is its own small kernel (a caller that also updates the fail rates can have it co-scheduled with that
        // launch instead: parc_step_tail, and leave PARC_POST_REF out here)
        hipLaunchKernelGGL(ref_state_kernel, dim3((n + REF_STATE_THREADS / GRP - 1) / (REF_STATE_THREADS / GRP)), dim3(REF_STATE_THREADS), 0,
                           (hipStream_t)stream, model, mlib, buf, env_ids, n, what);
        PARC_CHECK_LAUNCH();
    }
    if (what & (PARC_POST_OBS | PARC_POST_REWARD_DONE)) {
        const dim3 grid((n + POST_EPB - 1) / POST_EPB);
        const dim3 block(64 * (2 + (cfg.num_tar_steps > 0 ? (cfg.num_tar_steps + 1) / 2 : 0) + (((what & PARC_POST_OBS) && (what & PARC_POST_HF)) ? 1 : 0)));
        if (start_event || stop_event)
            // the same launch with a pair of events bound to THIS dispatch: they carry the kernel's own begin / end time stamps (what a
            // profiler reads from the dispatch), not the time between two separate event records around it
            hipExtLaunchKernelGGL(track_post_kernel, grid, block, POST_LDS_PAD, (hipStream_t)stream, start_event, stop_event, 0, model, mlib, terrain, cfg, buf,
                                  env_ids, n, what, ray_xy);
        else
            hipLaunchKernelGGL(track_post_kernel, grid, block, POST_LDS_PAD, (hipStream_t)stream, model, mlib, terrain, cfg, buf, env_ids, n, what, ray_xy);
        PARC_CHECK_LAUNCH();
    }
    return PARC_OK;
}

extern "C" int parc_track_post_step(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_terrain_t terrain,
                                    parc_track_cfg_t cfg, parc_env_buffers_t buf, const int64_t *env_ids, int n_sel, int what,
                                    const float *ray_xy) {
    return track_post_step_impl(stream, model, mlib, terrain, cfg, buf, env_ids, n_sel, what, ray_xy, nullptr, nullptr);
}

extern "C" int parc_track_post_step_timed(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_terrain_t terrain,
                                          parc_track_cfg_t cfg, parc_env_buffers_t buf, const int64_t *env_ids, int n_sel, int what,
                                          const float *ray_xy, void *start_event, void *stop_event) {
    if (!start_event || !stop_event) return PARC_EINVAL;
    return track_post_step_impl(stream, model, mlib, terrain, cfg, buf, env_ids, n_sel, what, ray_xy, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

// =============================================================================================
// Observation rows of the non-default layouts: a column gather from [obs row | aux | scalar] (parc_hip.h, parc_assemble_obs)
// =============================================================================================
__global__ __launch_bounds__(256) void assemble_obs_kernel(const float *__restrict__ obs, int obs_dim, const float *__restrict__ aux,
                                                           const float *__restrict__ scalar, const int32_t *__restrict__ col_map,
                                                           float *__restrict__ out, int out_dim, const int64_t *__restrict__ env_ids) {
    const int e = env_ids ? (int)env_ids[blockIdx.y] : (int)blockIdx.y;
    const float sc = scalar ? scalar[0] : 0.f;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < out_dim; c += gridDim.x * blockDim.x) {
        const int k = col_map[c];
        float v;
        if (k < obs_dim) v = obs[(size_t)e * obs_dim + k];
        else if (k < obs_dim + 4) v = aux[4 * (size_t)e + (k - obs_dim)];
        else v = sc;
        out[(size_t)e * out_dim + c] = v;
    }
}

extern "C" int parc_assemble_obs(void *stream, int n_envs, const float *obs, int obs_dim, const float *aux, const float *scalar,
                                 const int32_t *col_map, float *out, int out_dim, const int64_t *env_ids, int n_sel) {
    if (n_envs < 0 || obs_dim <= 0 || out_dim <= 0 || !obs || !col_map || !out || (env_ids && n_sel < 0)) return PARC_EINVAL;
    const int rows = env_ids ? n_sel : n_envs;
    if (rows == 0) return PARC_OK;
    if (rows > 65535) return PARC_EUNSUPPORTED;          // grid.y
    const int bx = (out_dim + 255) / 256;
    hipLaunchKernelGGL(assemble_obs_kernel, dim3(bx > 2 ? 2 : bx, rows), dim3(256), 0, (hipStream_t)stream, obs, obs_dim, aux, scalar, col_map,
                       out, out_dim, env_ids);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Device-side reset bookkeeping (dm_env.py:517-568, ig_env.py:100-121,693-721), one thread per env
// =============================================================================================
__global__ __launch_bounds__(256) void reset_apply_kernel(int n, const int32_t *__restrict__ mask, const int64_t *__restrict__ new_mid,
                                                          const int64_t *__restrict__ new_tid, const float *__restrict__ new_t,
                                                          const float *__restrict__ offs, int R, int64_t *mid, int64_t *tid, float *toff,
                                                          float *xyoff, int32_t *timestep, float *time_buf, int32_t *done,
                                                          float *next_target_time, int64_t *ep_num) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || mask[e] == 0) return;
    int64_t mi = new_mid[e], ti = new_tid[e];
    mid[e] = mi;
    tid[e] = ti;
    toff[e] = new_t[e];
    xyoff[2 * e] = offs[(mi * R + ti) * 2];
    xyoff[2 * e + 1] = offs[(mi * R + ti) * 2 + 1];
    timestep[e] = 0;
    time_buf[e] = 0.f;
    done[e] = PARC_DONE_NULL;
    next_target_time[e] = 0.f;
    ep_num[e] += 1;
}

extern "C" int parc_reset_apply(void *stream, int n_envs, const int32_t *mask, const int64_t *new_motion_ids, const int64_t *new_terrain_ids,
                                const float *new_time_offsets, const float *motion_offsets, int terrains_per_motion, int64_t *motion_ids,
                                int64_t *motion_terrain_ids, float *motion_time_offsets, float *motion_xy_offset, int32_t *timestep_buf,
                                float *time_buf, int32_t *done, float *next_target_time, int64_t *ep_num) {
    if (n_envs < 0 || terrains_per_motion < 1 || !mask) return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    hipLaunchKernelGGL(reset_apply_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, mask, new_motion_ids,
                       new_terrain_ids, new_time_offsets, motion_offsets, terrains_per_motion, motion_ids, motion_terrain_ids,
                       motion_time_offsets, motion_xy_offset, timestep_buf, time_buf, done, next_target_time, ep_num);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Device-side reset, sampling included (dm_env.py:517-568 + MotionLib.sample_motions / sample_time  anim/motion_lib.py:48-63):
// which envs restart (done != NULL), on which clip (probability ~ weight * max(fail rate, floor)), on which tile copy of the
// clip's terrain (uniform), from which phase (uniform in [0, clip length)), with which xy start noise (uniform in +-scale) -
// all from five uniforms per env that the caller drew in one launch.  Kernel 1 (one workgroup) builds the cumulative weights,
// kernel 2 (one thread per env) inverts them by bisection and does the bookkeeping of reset_apply_kernel.
// =============================================================================================
__global__ __launch_bounds__(256) void reset_cdf_kernel(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w,
                                                        float *cdf);

#define RESET_CDF_LDS 4096          // clips whose cumulative weights a workgroup builds for itself in LDS (16 KB); more: reset_cdf_kernel first

// fp32 product a clip is drawn in proportion to; __fmul_rn so that it never contracts into the addition that follows it
PARC_DEV float reset_clip_product(const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w, int i) {
    return __fmul_rn(fail_rates ? fmaxf(fail_rates[i], min_w) : 1.0f, weights[i]);
}

// cumulative weights into `out` (LDS or global), by the 256 threads of one workgroup - the same steps, hence the same fp32 sums, in
// every workgroup that runs it.  table[i] = base[t] + (running sum inside chunk t), and base[t + 1] IS the last entry of chunk t:
// base[t + 1] = base[t] + (sum of chunk t), the chunk sum being the same chain of additions as the chunk's last running sum.  Rounding
// is monotonic, so the table never decreases and stays flat across clips whose product is 0, inside a chunk and over its seams, which
// the bisection below and "a clip of weight 0 is never drawn" rely on.  (Chunk bases from a parallel scan are another rounding of the
// same sums than the running sums next to them: that table stepped down at seams and up on weight-0 clips, DESIGN.md.)  The bases are a
// serial chain over the chunks, by one thread: at most 256 dependent additions.
PARC_DEV void build_reset_cdf(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w, float *out, float *part) {
    const int chunk = (M + 255) / 256;
    const int nchunks = (M + chunk - 1) / chunk;
    const int i0 = min((int)threadIdx.x * chunk, M), i1 = min(i0 + chunk, M);
    float s = 0.f;
    for (int i = i0; i < i1; ++i) s = __fadd_rn(s, reset_clip_product(weights, fail_rates, min_w, i));
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float base = 0.f;
#pragma unroll 8
        for (int t = 0; t < nchunks; ++t) {
            const float v = part[t];
            part[t] = base;
            base = __fadd_rn(base, v);
        }
    }
    __syncthreads();
    const float base = part[threadIdx.x];
    float run = 0.f;
    for (int i = i0; i < i1; ++i) {
        run = __fadd_rn(run, reset_clip_product(weights, fail_rates, min_w, i));
        out[i] = __fadd_rn(base, run);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void reset_cdf_kernel(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w,
                                                        float *cdf) {
    __shared__ float part[256];
    build_reset_cdf(M, weights, fail_rates, min_w, cdf, part);
}

template <bool CDF_IN_LDS>
__global__ __launch_bounds__(256) void reset_sample_apply_kernel(int n, const int32_t *__restrict__ done_in, int32_t *mask, const float *__restrict__ u,
                                                                 int M, const float *__restrict__ cdf_global, const float *__restrict__ weights,
                                                                 const float *__restrict__ fail_rates, float min_w,
                                                                 const float *__restrict__ lengths,
                                                                 const float *__restrict__ offs, int R, float noise_scale, int64_t *mid, int64_t *tid,
                                                                 float *toff, float *xyoff, int32_t *timestep, float *time_buf, int32_t *done,
                                                                 float *next_target_time, int64_t *ep_num, float *init_noise_xy) {
    __shared__ float s_cdf[CDF_IN_LDS ? RESET_CDF_LDS : 1];
    __shared__ float s_part[256];
    const float *cdf = cdf_global;
    if (CDF_IN_LDS) {
        // every workgroup builds the table for itself (M <= 4096 entries: a few hundred flops) instead of a one-workgroup launch in
        // front of this one; workgroup 0 also publishes it (tests read it back)
        build_reset_cdf(M, weights, fail_rates, min_w, s_cdf, s_part);
        if (blockIdx.x == 0 && cdf_global)
            for (int i = threadIdx.x; i < M; i += 256) const_cast<float *>(cdf_global)[i] = s_cdf[i];
        cdf = s_cdf;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int finished = done_in[e] != PARC_DONE_NULL;
    mask[e] = finished;
    if (!finished) return;
    // clip: first index whose cumulative weight exceeds u * total (searchsorted(..., right=True)), kept inside the table
    const float x = u[e] * cdf[M - 1];
    int lo = 0, hi = M;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (cdf[m] > x) hi = m; else lo = m + 1;
    }
    const int64_t mi = min(lo, M - 1);
    const int64_t ti = min((int)(u[n + e] * (float)R), R - 1);
    mid[e] = mi;
    tid[e] = ti;
    toff[e] = u[2 * n + e] * lengths[mi];
    xyoff[2 * e] = offs[(mi * R + ti) * 2];
    xyoff[2 * e + 1] = offs[(mi * R + ti) * 2 + 1];
    init_noise_xy[2 * e] = (2.0f * u[3 * n + e] - 1.0f) * noise_scale;
    init_noise_xy[2 * e + 1] = (2.0f * u[4 * n + e] - 1.0f) * noise_scale;
    timestep[e] = 0;
    time_buf[e] = 0.f;
    done[e] = PARC_DONE_NULL;
    next_target_time[e] = 0.f;
    ep_num[e] += 1;
}

extern "C" int parc_reset_sample_apply(void *stream, int n_envs, const int32_t *done_flags, int32_t *mask, const float *uniforms, int n_motions,
                                       const float *motion_weights, const float *fail_rates, float min_weight, const float *motion_lengths,
                                       const float *motion_offsets, int terrains_per_motion, float noise_scale, float *cdf_workspace,
                                       int64_t *motion_ids, int64_t *motion_terrain_ids, float *motion_time_offsets, float *motion_xy_offset,
                                       int32_t *timestep_buf, float *time_buf, int32_t *done, float *next_target_time, int64_t *ep_num,
                                       float *init_noise_xy) {
    if (n_envs < 0 || n_motions < 1 || terrains_per_motion < 1 || !done_flags || !mask || !uniforms || !motion_weights || !motion_lengths ||
        !cdf_workspace || !init_noise_xy)
        return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    if (n_motions <= RESET_CDF_LDS) {
        hipLaunchKernelGGL(reset_sample_apply_kernel<true>, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, done_flags, mask,
                           uniforms, n_motions, cdf_workspace, motion_weights, fail_rates, min_weight, motion_lengths, motion_offsets,
                           terrains_per_motion, noise_scale, motion_ids, motion_terrain_ids, motion_time_offsets, motion_xy_offset, timestep_buf,
                           time_buf, done, next_target_time, ep_num, init_noise_xy);
    } else {
        hipLaunchKernelGGL(reset_cdf_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_motions, motion_weights, fail_rates, min_weight, cdf_workspace);
        hipLaunchKernelGGL(reset_sample_apply_kernel<false>, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, done_flags, mask,
                           uniforms, n_motions, cdf_workspace, motion_weights, fail_rates, min_weight, motion_lengths, motion_offsets,
                           terrains_per_motion, noise_scale, motion_ids, motion_terrain_ids, motion_time_offsets, motion_xy_offset, timestep_buf,
                           time_buf, done, next_target_time, ep_num, init_noise_xy);
    }
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Fail-rate EMA (dm_env.py:758-772): for every env that finished this step, in env order,
//     fail_rate[clip] = (1 - w) fail_rate[clip] + w [episode failed]
// One 256-thread workgroup per clip.  Pass i reads the done flags of envs 256 i .. 256 i + 255 coalesced; a wave-wide ballot
// turns "finished on this clip" / "and failed" into two 64-bit masks per (pass, wave), parked in LDS.  Thread 0 then walks the
// set bits in env order and applies the updates one by one - the same fp32 operations in the same order as the reference's
// loop over done envs, so the result is bit-identical to it.  Clips nobody finished on (almost all of them, every step) cost
// the flag reads and nothing else.
// =============================================================================================
#define FR_THREADS 256
#define FR_MAX_PASSES 64          // up to 16384 envs per launch segment; larger counts loop over segments
typedef unsigned long long fr_masks_t[FR_MAX_PASSES][FR_THREADS / 64];
PARC_DEV void fail_rate_block(int mi, int n_envs, const int64_t *__restrict__ motion_ids, const int32_t *__restrict__ done_kind, float ema_w,
                              float *fail_rates, fr_masks_t &hit, fr_masks_t &fail) {
    const int wv = threadIdx.x >> 6;
    const float keep = (float)(1.0 - (double)ema_w);       // the reference multiplies by the python double (1.0 - w), cast to fp32
    float fr = 0.f;
    bool touched = false;
    if (threadIdx.x == 0) fr = fail_rates[mi];
    for (int seg = 0; seg < n_envs; seg += FR_MAX_PASSES * FR_THREADS) {
        const int passes = min(FR_MAX_PASSES, (n_envs - seg + FR_THREADS - 1) / FR_THREADS);
        for (int i0 = 0; i0 < passes; i0 += 8) {          // 8 passes at a time: their flag loads are in flight together
            int ks[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = seg + (i0 + u) * FR_THREADS + threadIdx.x;
                ks[u] = (i0 + u < passes && e < n_envs) ? done_kind[e] : 0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u >= passes) break;
                const int e = seg + (i0 + u) * FR_THREADS + threadIdx.x;
                const int k = ks[u];
                const bool h = k != 0 && motion_ids[e] == mi;
                const unsigned long long hm = __ballot(h), fm = __ballot(h && k == 1);
                if ((threadIdx.x & 63) == 0) {
                    hit[i0 + u][wv] = hm;
                    fail[i0 + u][wv] = fm;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 0; i < passes; ++i)
                for (int w = 0; w < FR_THREADS / 64; ++w) {
                    unsigned long long hm = hit[i][w];
                    const unsigned long long fm = fail[i][w];
                    while (hm) {
                        const int bit = __ffsll((long long)hm) - 1;
                        hm &= hm - 1;
                        fr = mul_add_unfused(fr, keep, ((fm >> bit) & 1ull) ? ema_w : 0.f);     // two roundings, like fr * keep + w in torch
                        touched = true;
                    }
                }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && touched) fail_rates[mi] = fr;
}

__global__ __launch_bounds__(FR_THREADS) void fail_rate_kernel(int n_envs, int n_motions, const int64_t *__restrict__ motion_ids,
                                                               const int32_t *__restrict__ done_kind, float ema_w, float *fail_rates) {
    __shared__ fr_masks_t hit, fail;
    fail_rate_block(blockIdx.x, n_envs, motion_ids, done_kind, ema_w, fail_rates, hit, fail);
}

// The tail of an env step in ONE launch of heterogeneous workgroups: blocks [0, n_motions) walk the fail-rate EMA of one clip each
// (64 workgroups that keep the chip almost idle for the ~10 us the bit-exact serial walk takes), blocks behind them publish the
// reference STATE of 16 envs each (ref_state_group) on the idle CUs.  Both only read what the fused launch and the simulator left.
static_assert(FR_THREADS == REF_STATE_THREADS, "one block size for both kinds of workgroup");
__global__ __launch_bounds__(FR_THREADS) void step_tail_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_env_buffers_t buf, int n_envs, int what,
                                                               int n_motions, const int32_t *__restrict__ done_kind, float ema_w, float *fail_rates) {
    __shared__ fr_masks_t hit, fail;
    if ((int)blockIdx.x < n_motions) {
        fail_rate_block(blockIdx.x, n_envs, buf.motion_ids, done_kind, ema_w, fail_rates, hit, fail);
        return;
    }
    const int blk = (int)blockIdx.x - n_motions;
    ref_state_group(m, ml, buf, nullptr, n_envs, what, blk * (REF_STATE_THREADS / GRP) + (int)(threadIdx.x >> 4), threadIdx.x & 15);
}

extern "C" int parc_step_tail(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_env_buffers_t buf, int what, int n_motions,
                              const int32_t *done_kind, float ema_w, float *fail_rates) {
    if (!model_ok(model) || mlib.num_bodies != model.num_bodies || mlib.dof_size != model.dof_size) return PARC_EINVAL;
    if (n_motions != mlib.num_motions || !done_kind || !fail_rates || buf.num_envs < 0) return PARC_EINVAL;
    if (what & ~(PARC_POST_REF | PARC_POST_PLAN_CLOCK)) return PARC_EINVAL;      // the per-step publication only (no restart variants)
    const int n = buf.num_envs;
    if (n == 0) return PARC_OK;
    const int state_blocks = (what & PARC_POST_REF) ? (n + REF_STATE_THREADS / GRP - 1) / (REF_STATE_THREADS / GRP) : 0;
    hipLaunchKernelGGL(step_tail_kernel, dim3(n_motions + state_blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, model, mlib, buf, n, what, n_motions,
                       done_kind, ema_w, fail_rates);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_update_fail_rates(void *stream, int n_envs, int n_motions, const int64_t *motion_ids, const int32_t *done_kind,
                                      float ema_w, float *fail_rates) {
    if (n_envs < 0 || n_motions <= 0) return PARC_EINVAL;
    hipLaunchKernelGGL(fail_rate_kernel, dim3(n_motions), dim3(FR_THREADS), 0, (hipStream_t)stream, n_envs, n_motions, motion_ids, done_kind,
                       ema_w, fail_rates);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_abi_version(void) { return 1; }
