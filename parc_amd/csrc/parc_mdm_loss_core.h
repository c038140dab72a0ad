// The motion generator's training loss for ONE sample, forward and adjoint (include/parc_mdm_loss.h), shared by the device (hipcc:
// parc_mdm_loss.hip, one workgroup per sample) and the host (g++: the CPU tests, tests/tools/mdm_loss_host.cpp).  Built with
// -ffp-contract=off on both sides: every expression is a sequence of separately rounded fp32 operations, as torch evaluates the
// reference's (diffusion/mdm.py:617-754 motion_difference).
//
// From parc_mdm_pose_core.h: the quaternion functions and their adjoints, the pose chain and its adjoint, the terrain scan, the selected
// column's gradient, the phase scheme and the folds.  Here: the scratch layout (the heightfield, a pose block for the predicted and one
// for the true side, the points' distances and columns, the per-item summands, which the backward launch's cotangents reuse), the
// fourteen terms, their totals and values, the velocity terms with their gradients, and the cotangents gathered per (frame, body).
#pragma once
#include "../../include/parc_mdm_loss.h"
#include "parc_mdm_pose_core.h"

#define PARC_ML_NOTHING PARC_MP_NOTHING      // the one code under this core's name: what its argument checks return and its launchers compare with
#define PARC_ML_LOSS_FN_TERMS 12   // terms 0..11 go through loss_fn; HF_COLLISION and TARGET do not

namespace parc_ml {

using namespace parc_mp;

// ---- Scratch layout of one sample, in floats ----
struct layout {
    int S, nb, J, P, XY, n_items;
    pose_block pose[2];          // 0 = predicted, from x; 1 = true, from the arrays
    cot_block cot;               // the backward launch's cotangents reuse the summands' block
    int o_hf, o_psdf, o_pcell, o_part, o_r1, o_sum, o_k;
    int64_t total;
};

PARC_MP_HD layout make_layout(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c) {
    layout L;
    L.S = c.seq_len, L.nb = m.num_bodies, L.J = m.num_bodies - 1, L.P = c.num_points, L.XY = c.dim_x * c.dim_y;
    L.n_items = L.S * L.nb;
    int64_t o = 0;
    L.o_hf = (int)o, o += L.XY;
    for (int s = 0; s < 2; ++s) L.pose[s] = make_pose_block(L.S, L.nb, o);
    L.o_psdf = (int)o, o += (int64_t)L.S * L.P;
    L.o_pcell = (int)o, o += (int64_t)L.S * L.P;
    L.o_part = (int)o, o += (int64_t)PARC_ML_LOSS_FN_TERMS * L.n_items;
    int64_t og = L.o_part;
    L.cot = make_cot_block(L.S, L.nb, og);          // 11 nb - 4 <= 12 nb per frame
    L.o_r1 = (int)o, o += PARC_MDM_LOSS_TERMS * PARC_MP_NSUB;
    L.o_sum = (int)o, o += PARC_MDM_LOSS_TERMS;
    L.o_k = (int)o, o += PARC_MDM_LOSS_TERMS;
    L.total = o;
    return L;
}

static inline int64_t lds_bytes(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c) { return 4 * make_layout(m, c).total; }

// What one call works on: sample b's rows of every array
struct sample {
    rows r;                                                     // x, mean, std [S, D]
    const float *root_pos, *root_rot, *joint_rot, *contacts;    // the true side
    const float *hf, *target_dir, *grid_x, *grid_y, *points;
    const int32_t *point_start;
    float *scr;
};

PARC_MP_FN bool term_on(const parc_mdm_loss_cfg_t &c, int t) { return (c.enabled >> t) & 1; }
PARC_MP_FN local_grid grid_of(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s) {
    return make_local_grid(c, s.scr + L.o_hf, s.grid_x, s.grid_y);
}

// (a - b)^2 summed over the components, + c2 per component (0 for squared_l2): the summand of loss_fn
PARC_MP_FN float sq1(float e, float c2) { return e * e + c2; }
PARC_MP_FN float sq3(v3 e, float c2) { return (sq1(e.x, c2) + sq1(e.y, c2)) + sq1(e.z, c2); }

// velocity error of the frame pair (f, f + 1) of positions stored with `stride` floats per frame: (true - pred), each side / dt
PARC_MP_FN v3 vel_err(const float *pt, const float *pp, int stride, int f, float dt) {
    const v3 dt_ = ld3(pt + (size_t)(f + 1) * stride) - ld3(pt + (size_t)f * stride), dp = ld3(pp + (size_t)(f + 1) * stride) - ld3(pp + (size_t)f * stride);
    return mk3(dt_.x / dt - dp.x / dt, dt_.y / dt - dp.y / dt, dt_.z / dt - dp.z / dt);
}
// angular velocity of the pair (q0 = frame f, q1 = frame f + 1): quat_to_exp_map(q1 (x) conj(q0)) / dt
PARC_MP_FN v3 ang_vel(q4 q0, q4 q1, float dt) {
    const v3 e = quat_to_em(qmul(q1, qconj(q0)));
    return mk3(e.x / dt, e.y / dt, e.z / dt);
}

// ---- Forward phases ----
// The chain of one frame of one side into its pose block.  The lanes of one wave work on either side, so both sides go through ONE
// chain_walk whose joint source branches per joint (chain_from_feat or chain_from_true by side would put two walks into the kernel, run
// one after the other by a wave that holds both sides).  The block is selected by value: indexing pose[side] would keep L in memory.
PARC_MP_FN void chain_item(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int side, int f) {
    const pose_block pb = side == 0 ? L.pose[0] : L.pose[1];
    const feat_layout fl = make_feat_layout(c);
    if (side == 0) root_from_feat(pb, s.scr, s.r, fl, f);
    else root_from_true(pb, s.scr, s.root_pos, s.root_rot, f);
    chain_walk(m, pb, s.scr, f, [&](int b) { return side == 0 ? joint_quat(m, s.r, fl, f, b) : joint_true(s.joint_rot, pb.J, f, b); });
}

PARC_MP_FN void point_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int p) {
    int cell;
    s.scr[L.o_psdf + f * L.P + p] = point_sdf(grid_of(c, L, s), L.pose[0], s.scr, s.points, s.point_start, f, p, cell);
    reinterpret_cast<int32_t *>(s.scr + L.o_pcell)[f * L.P + p] = cell;
}

// the summands of (frame f, body b) for the twelve loss_fn terms
PARC_MP_FN void terms_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int b) {
    const float c2 = c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER ? 0.0009f : 0.f;
    const pose_block &pred = L.pose[0], &real = L.pose[1];
    const float *bpT = s.scr + real.o_bpos, *bpP = s.scr + pred.o_bpos, *brT = s.scr + real.o_brot, *brP = s.scr + pred.o_brot;
    const float *jqT = s.scr + real.o_jq, *jqP = s.scr + pred.o_jq;
    const size_t i = (size_t)f * L.nb + b;
    const bool pair = f < L.S - 1;
    float t[PARC_ML_LOSS_FN_TERMS];
    for (int k = 0; k < PARC_ML_LOSS_FN_TERMS; ++k) t[k] = 0.f;
    if (b == 0) {
        t[PARC_MDM_LOSS_SIMPLE_ROOT_POS] = sq3(ld3(bpT + i * 3) - ld3(bpP + i * 3), c2);
        t[PARC_MDM_LOSS_SIMPLE_ROOT_ROT] = sq1(qdiff_angle(ld4(brT + i * 4), ld4(brP + i * 4)), c2);
        if (pair) {
            t[PARC_MDM_LOSS_VEL_ROOT_POS] = sq3(vel_err(bpT, bpP, L.nb * 3, f, c.dt), c2);
            t[PARC_MDM_LOSS_VEL_ROOT_ROT] = sq3(ang_vel(ld4(brT + i * 4), ld4(brT + (i + L.nb) * 4), c.dt) - ang_vel(ld4(brP + i * 4), ld4(brP + (i + L.nb) * 4), c.dt), c2);
        }
    } else {
        const size_t j = (size_t)f * L.J + (b - 1);
        t[PARC_MDM_LOSS_SIMPLE_JOINT_ROT] = sq1(qdiff_angle(ld4(jqT + j * 4), ld4(jqP + j * 4)), c2);
        if (pair)
            t[PARC_MDM_LOSS_VEL_JOINT_ROT] = sq3(ang_vel(ld4(jqT + j * 4), ld4(jqT + (j + L.J) * 4), c.dt) - ang_vel(ld4(jqP + j * 4), ld4(jqP + (j + L.J) * 4), c.dt), c2);
        if (c.off_joint_pos >= 0) {
            const v3 jp = feat3(s.r, c.feat_dim, f, c.off_joint_pos + 3 * (b - 1));
            t[PARC_MDM_LOSS_SIMPLE_BODY_POS] = sq3(ld3(bpT + i * 3) - jp, c2);
            t[PARC_MDM_LOSS_BODY_POS_CONSISTENCY] = sq3(ld3(bpP + i * 3) - jp, c2);
        }
    }
    if (c.off_contacts >= 0) t[PARC_MDM_LOSS_SIMPLE_CONTACT] = sq1(s.contacts[i] - feat(s.r, c.feat_dim, f, c.off_contacts + b), c2);
    t[PARC_MDM_LOSS_FK_BODY_POS] = sq3(ld3(bpT + i * 3) - ld3(bpP + i * 3), c2);
    t[PARC_MDM_LOSS_FK_BODY_ROT] = sq1(qdiff_angle(ld4(brT + i * 4), ld4(brP + i * 4)), c2);
    if (pair) t[PARC_MDM_LOSS_VEL_FK_BODY_POS] = sq3(vel_err(bpT + b * 3, bpP + b * 3, L.nb * 3, f, c.dt), c2);
    for (int k = 0; k < PARC_ML_LOSS_FN_TERMS; ++k) s.scr[L.o_part + (size_t)k * L.n_items + i] = t[k];
}

// sub-sum `sub` of term t: summands sub, sub + 16, ... in ascending order
PARC_MP_FN void subsum_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t, int sub) {
    float acc = 0.f;
    if (t < PARC_ML_LOSS_FN_TERMS) acc = row_subsum(s.scr + L.o_part + (size_t)t * L.n_items, L.n_items, sub);      // 0 where the term has no element
    else if (t == PARC_MDM_LOSS_HF_COLLISION && term_on(c, t)) acc = penetration_subsum(s.scr + L.o_psdf, L.S * L.P, sub);
    s.scr[L.o_r1 + t * PARC_MP_NSUB + sub] = acc;
}

// the raw total of term t (before weight, square root and clamp)
PARC_MP_FN void total_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t) {
    float acc = 0.f;
    if (t == PARC_MDM_LOSS_TARGET) {
        const float *last = s.scr + L.pose[0].o_bpos + (size_t)(L.S - 1) * L.nb * 3, *ref = s.scr + L.pose[0].o_bpos + (size_t)c.ref_idx * L.nb * 3;
        acc = -s.target_dir[0] * (last[0] - ref[0]) + -s.target_dir[1] * (last[1] - ref[1]);
    } else {
        acc = fold_subsums(s.scr + L.o_r1 + t * PARC_MP_NSUB);
    }
    s.scr[L.o_sum + t] = acc;
}

PARC_MP_FN float term_value(const parc_mdm_loss_cfg_t &c, int t, float total) {
    if (!term_on(c, t)) return 0.f;
    if (t == PARC_MDM_LOSS_TARGET) return (total >= -c.target_eps ? total : (total == total ? -c.target_eps : total)) * c.w[t];
    if (t == PARC_MDM_LOSS_HF_COLLISION) return c.w[t] * (0.5f * total);
    return c.w[t] * (c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER ? sqrtf(total) - 0.03f : total);
}

// Everything up to the raw totals.  Ends with a barrier.
PARC_MP_FN void forward_phases(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int lane, int nlanes) {
    for (int i = lane; i < L.XY; i += nlanes) s.scr[L.o_hf + i] = s.hf[i] * c.max_h;
    for (int i = lane; i < 2 * L.S; i += nlanes) chain_item(m, c, L, s, i / L.S, i % L.S);
    PARC_MP_SYNC();
    if (term_on(c, PARC_MDM_LOSS_HF_COLLISION))
        for (int i = lane; i < L.S * L.P; i += nlanes) point_item(c, L, s, i / L.P, i % L.P);
    for (int i = lane; i < L.n_items; i += nlanes) terms_item(c, L, s, i / L.nb, i % L.nb);
    PARC_MP_SYNC();
    for (int i = lane; i < PARC_MDM_LOSS_TERMS * PARC_MP_NSUB; i += nlanes) subsum_item(c, L, s, i / PARC_MP_NSUB, i % PARC_MP_NSUB);
    PARC_MP_SYNC();
    for (int i = lane; i < PARC_MDM_LOSS_TERMS; i += nlanes) total_item(c, L, s, i);
    PARC_MP_SYNC();
}

// sample b of a batch of B: losses [TERMS, B]
PARC_MP_FN void forward_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const sample &s, int b, int B, float *losses, int lane, int nlanes) {
    const layout L = make_layout(m, c);
    forward_phases(m, c, L, s, lane, nlanes);
    for (int t = lane; t < PARC_MDM_LOSS_TERMS; t += nlanes) losses[(size_t)t * B + b] = term_value(c, t, s.scr[L.o_sum + t]);
}

// ---- Backward phases ----
// k[t]: cotangent of term t's raw total (loss_fn terms: of the sum of squares; HF: of sum(min(sdf, 0)^2) / 2 ... see grad_item)
PARC_MP_FN void scale_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t, float g) {
    float k = 0.f;
    if (term_on(c, t)) {
        const float total = s.scr[L.o_sum + t];
        k = g * c.w[t];
        if (t == PARC_MDM_LOSS_TARGET) k = total >= -c.target_eps ? k : 0.f;
        else if (t < PARC_ML_LOSS_FN_TERMS && c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER) k = k / (2.0f * sqrtf(total));
    }
    s.scr[L.o_k + t] = k;
}

// cotangent that the angular-velocity term (weight k on the sum of squared errors) sends to the quaternion of frame f, from the
// pairs (f - 1, f) and (f, f + 1); qT / qP: the frame-0 quaternion of this root / joint on either side, stride floats per frame
PARC_MP_FN q4 ang_vel_grad(const float *qT, const float *qP, int stride, int S, int f, float dt, float k) {
    q4 g = q4{0.f, 0.f, 0.f, 0.f};
    for (int side = 0; side < 2; ++side) {          // 0: f is the later frame of its pair, 1: the earlier
        const int f0 = f - 1 + side;
        if (f0 < 0 || f0 >= S - 1) continue;
        const q4 a = ld4(qP + (size_t)f0 * stride), b = ld4(qP + (size_t)(f0 + 1) * stride);
        const v3 e = ang_vel(ld4(qT + (size_t)f0 * stride), ld4(qT + (size_t)(f0 + 1) * stride), dt) - ang_vel(a, b, dt);
        const float sc = -2.0f * k / dt;            // d/d(pred exp map) of k (true - pred)^2, through the division by dt
        const q4 gd = quat_to_em_bwd(qmul(b, qconj(a)), mk3(sc * e.x, sc * e.y, sc * e.z));
        g = qadd(g, side == 0 ? qdiff_bwd_b(a, gd) : qdiff_bwd_a(b, gd));
    }
    return g;
}
PARC_MP_FN v3 vel_grad(const float *pt, const float *pp, int stride, int S, int f, float dt, float k) {
    v3 g = mk3(0.f, 0.f, 0.f);
    if (f >= 1) g = g + (-2.0f * k / dt) * vel_err(pt, pp, stride, f - 1, dt);
    if (f < S - 1) g = g + (2.0f * k / dt) * vel_err(pt, pp, stride, f, dt);
    return g;
}

// cotangents of the predicted body transform and joint rotation of (frame f, body b); the feature columns that no chain reaches
// (joint positions, contacts) get their g_x here
PARC_MP_FN void grad_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int b, float *g_x) {
    const float *k = s.scr + L.o_k;
    const pose_block &pred = L.pose[0], &real = L.pose[1];
    const float *bpT = s.scr + real.o_bpos, *bpP = s.scr + pred.o_bpos, *brT = s.scr + real.o_brot, *brP = s.scr + pred.o_brot;
    const float *jqT = s.scr + real.o_jq, *jqP = s.scr + pred.o_jq;
    const size_t i = (size_t)f * L.nb + b;
    const v3 pT = ld3(bpT + i * 3), pP = ld3(bpP + i * 3);
    const q4 rT = ld4(brT + i * 4), rP = ld4(brP + i * 4);
    const size_t row = (size_t)f * c.feat_dim;
    // FK_BODY_POS, VEL_FK_BODY_POS
    v3 gp = (-2.0f * k[PARC_MDM_LOSS_FK_BODY_POS]) * (pT - pP) + vel_grad(bpT + b * 3, bpP + b * 3, L.nb * 3, L.S, f, c.dt, k[PARC_MDM_LOSS_VEL_FK_BODY_POS]);
    // FK_BODY_ROT
    const q4 d = qmul(rP, qconj(rT));
    q4 gq = qdiff_bwd_b(rT, qangle_bwd(d, 2.0f * k[PARC_MDM_LOSS_FK_BODY_ROT] * qangle(d)));
    if (b == 0) {
        gp = gp + (-2.0f * k[PARC_MDM_LOSS_SIMPLE_ROOT_POS]) * (pT - pP) + vel_grad(bpT, bpP, L.nb * 3, L.S, f, c.dt, k[PARC_MDM_LOSS_VEL_ROOT_POS]);
        const float kt = k[PARC_MDM_LOSS_TARGET];
        if (f == L.S - 1) gp.x += kt * -s.target_dir[0], gp.y += kt * -s.target_dir[1];
        if (f == c.ref_idx) gp.x += kt * s.target_dir[0], gp.y += kt * s.target_dir[1];
        gq = qadd(gq, qdiff_bwd_b(rT, qangle_bwd(d, 2.0f * k[PARC_MDM_LOSS_SIMPLE_ROOT_ROT] * qangle(d))));
        gq = qadd(gq, ang_vel_grad(brT, brP, L.nb * 4, L.S, f, c.dt, k[PARC_MDM_LOSS_VEL_ROOT_ROT]));
    } else {
        const size_t j = (size_t)f * L.J + (b - 1);
        const q4 jT = ld4(jqT + j * 4), jP = ld4(jqP + j * 4);
        const q4 dj = qmul(jP, qconj(jT));
        q4 gj = qdiff_bwd_b(jT, qangle_bwd(dj, 2.0f * k[PARC_MDM_LOSS_SIMPLE_JOINT_ROT] * qangle(dj)));
        gj = qadd(gj, ang_vel_grad(jqT + (b - 1) * 4, jqP + (b - 1) * 4, L.J * 4, L.S, f, c.dt, k[PARC_MDM_LOSS_VEL_JOINT_ROT]));
        st4(s.scr + L.cot.o_gjq + j * 4, gj);
        if (c.off_joint_pos >= 0) {
            const int d0 = c.off_joint_pos + 3 * (b - 1);
            const v3 jp = feat3(s.r, c.feat_dim, f, d0);
            const v3 ec = (2.0f * k[PARC_MDM_LOSS_BODY_POS_CONSISTENCY]) * (pP - jp);
            gp = gp + ec;
            const v3 gjp = (-2.0f * k[PARC_MDM_LOSS_SIMPLE_BODY_POS]) * (pT - jp) - ec;
            g_x[row + d0] = gjp.x * s.r.std[row + d0];
            g_x[row + d0 + 1] = gjp.y * s.r.std[row + d0 + 1];
            g_x[row + d0 + 2] = gjp.z * s.r.std[row + d0 + 2];
        }
    }
    if (c.off_contacts >= 0) {
        const int d0 = c.off_contacts + b;
        g_x[row + d0] = -2.0f * k[PARC_MDM_LOSS_SIMPLE_CONTACT] * (s.contacts[i] - feat(s.r, c.feat_dim, f, d0)) * s.r.std[row + d0];
    }
    if (term_on(c, PARC_MDM_LOSS_HF_COLLISION)) {
        const int32_t *cells = reinterpret_cast<const int32_t *>(s.scr + L.o_pcell);
        const local_grid grid = grid_of(c, L, s);
        const int p0 = s.point_start[b] > 0 ? s.point_start[b] : 0, p1 = s.point_start[b + 1] < L.P ? s.point_start[b + 1] : L.P;      // the table is trusted for nothing
        for (int p = p0; p < p1; ++p) {
            const float sdf = s.scr[L.o_psdf + f * L.P + p];
            if (!(sdf < 0.f)) continue;
            const v3 loc = ld3(s.points + (size_t)p * 3);
            const v3 cg = column_grad(grid, pP + qrot(rP, loc), cells[f * L.P + p]);
            const v3 g = (-(k[PARC_MDM_LOSS_HF_COLLISION] * sdf)) * cg;          // sdf = -distance; d(sdf^2 / 2) = sdf
            gp = gp + g;
            gq = qadd(gq, qrot_bwd_q(rP, loc, g));
        }
    }
    st3(s.scr + L.cot.o_gpos + i * 3, gp);
    st4(s.scr + L.cot.o_grot + i * 4, gq);
}

// sample b of a batch of B: g_losses [TERMS, B] -> g_x (this sample's [S, D] rows)
PARC_MP_FN void backward_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const sample &s, int b, int B, const float *g_losses, float *g_x,
                                int lane, int nlanes) {
    const layout L = make_layout(m, c);
    forward_phases(m, c, L, s, lane, nlanes);
    for (int t = lane; t < PARC_MDM_LOSS_TERMS; t += nlanes) scale_item(c, L, s, t, g_losses[(size_t)t * B + b]);
    PARC_MP_SYNC();
    for (int i = lane; i < L.n_items; i += nlanes) grad_item(c, L, s, i / L.nb, i % L.nb, g_x);
    PARC_MP_SYNC();
    for (int f = lane; f < L.S; f += nlanes) chain_grad_item(m, L.pose[0], L.cot, s.scr, s.r, make_feat_layout(c), f, g_x);
}

// sample b's rows
PARC_MP_FN sample make_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int b, const float *x, const float *mean, const float *std,
                              const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts, const float *hfs,
                              const float *target_dir, const float *grid_x, const float *grid_y, const float *points, const int32_t *point_start,
                              float *scr) {
    const size_t S = (size_t)c.seq_len, nb = (size_t)m.num_bodies;
    sample s;
    s.r = rows{x + b * S * c.feat_dim, mean, std};
    s.root_pos = root_pos + b * S * 3, s.root_rot = root_rot + b * S * 4, s.joint_rot = joint_rot + b * S * (nb - 1) * 4;
    s.contacts = contacts ? contacts + b * S * nb : contacts;
    s.hf = hfs + (size_t)b * c.dim_x * c.dim_y, s.target_dir = target_dir + (size_t)b * 2;
    s.grid_x = grid_x, s.grid_y = grid_y, s.points = points, s.point_start = point_start, s.scr = scr;
    return s;
}

// ---- Argument rules of the entry points (include/parc_mdm_loss.h), answered before any HIP call ----
static inline int check_cfg(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int B) {
    if (check_window(m, c, B) != PARC_OK) return PARC_EINVAL;          // the slices tile [0, D): every column of g_x is written
    if (c.ref_idx < 0 || c.ref_idx >= c.seq_len) return PARC_EINVAL;
    if (c.loss_fn != PARC_MDM_LOSS_SQUARED_L2 && c.loss_fn != PARC_MDM_LOSS_PSEUDO_HUBER) return PARC_EINVAL;
    if (c.off_joint_pos < 0 && (c.enabled & ((1 << PARC_MDM_LOSS_SIMPLE_BODY_POS) | (1 << PARC_MDM_LOSS_BODY_POS_CONSISTENCY)))) return PARC_EINVAL;
    if (c.off_contacts < 0 && (c.enabled & (1 << PARC_MDM_LOSS_SIMPLE_CONTACT))) return PARC_EINVAL;
    // sizes in 64 bits before the layout multiplies them as int
    if ((int64_t)c.dim_x * c.dim_y > PARC_MDM_LOSS_MAX_LDS / 4) return PARC_EUNSUPPORTED;
    if ((int64_t)c.seq_len * (m.num_bodies * 12 + (int64_t)c.num_points) > 0x7fffff) return PARC_EUNSUPPORTED;
    if (lds_bytes(m, c) > PARC_MDM_LOSS_MAX_LDS) return PARC_EUNSUPPORTED;
    return PARC_OK;
}

static inline int check_args(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int B, const void *x, const void *mean, const void *std,
                             const void *root_pos, const void *root_rot, const void *joint_rot, const void *contacts, const void *hfs,
                             const void *target_dir, const void *grid_x, const void *grid_y, const void *points, const void *point_start,
                             const void *out, const void *extra) {
    const int rc = check_cfg(m, c, B);
    if (rc != PARC_OK) return rc;
    if (B == 0) return PARC_ML_NOTHING;
    if (!x || !mean || !std || !root_pos || !root_rot || !joint_rot || !hfs || !target_dir || !grid_x || !grid_y || !point_start || !out || !extra)
        return PARC_EINVAL;
    if (c.off_contacts >= 0 && !contacts) return PARC_EINVAL;
    if (c.num_points > 0 && !points) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_ml
