// The motion generator's guidance step for ONE sample: the guidance loss, its gradient and the update in place
// (include/parc_mdm_guide.h), shared by the device (hipcc: parc_mdm_guide.hip, one workgroup per sample) and the host (g++: the CPU
// tests, tests/tools/mdm_guide_host.cpp).  Built with -ffp-contract=off on both sides.  Reference: diffusion/mdm.py:1444-1542.
//
// From parc_mdm_pose_core.h: the pose chain from standardised features (chain_from_feat), its adjoint (chain_grad_item), the terrain
// scan (point_sdf), the selected column's gradient (column_grad), the phase scheme and the folds.  Here: the scratch layout, the
// difference hinges along the body axis with their gathered cotangents, the 16-bit column record, and the update, which keeps every
// read of x in front of a barrier and every write of x_out behind it.
#pragma once
#include "../../include/parc_mdm_guide.h"
#include "parc_mdm_pose_core.h"

#define PARC_MG_NOTHING PARC_MP_NOTHING      // the one code under this core's name: what its argument checks return and its launchers compare with

namespace parc_mg {

using namespace parc_mp;

// Scratch layout of one sample, in floats.  The summands of TARGET, SPEED, ACC, JERK [4, n_items] live in the first 4 n_items floats
// of the cotangent block (o_part == cot.o_gpos): they are folded before a cotangent is written.
struct layout {
    int S, nb, J, P, XY, D, n_items;
    pose_block pose;
    cot_block cot;
    int o_hf, o_part, o_gx, o_r1, o_psdf, o_pcol;      // o_gx: [S, D] gradient, then the updated sample; o_pcol: [S, P] columns, 16 bits each
    int64_t total;
};

PARC_MP_HD layout make_layout(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c) {
    layout L;
    L.S = c.seq_len, L.nb = m.num_bodies, L.J = m.num_bodies - 1, L.P = c.num_points, L.XY = c.dim_x * c.dim_y, L.D = c.feat_dim;
    L.n_items = L.S * L.nb;
    int64_t o = 0;
    L.o_hf = (int)o, o += L.XY;
    L.pose = make_pose_block(L.S, L.nb, o);
    L.cot = make_cot_block(L.S, L.nb, o);
    L.o_part = L.cot.o_gpos;
    L.o_gx = (int)o, o += (int64_t)L.S * L.D;
    L.o_r1 = (int)o, o += PARC_MDM_GUIDE_TERMS * PARC_MP_NSUB;
    L.o_psdf = (int)o, o += (int64_t)L.S * L.P;
    L.o_pcol = (int)o, o += ((int64_t)L.S * L.P + 1) / 2;
    L.total = o;
    return L;
}

static inline int64_t lds_bytes(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c) { return 4 * make_layout(m, c).total; }

// What one call works on: sample b's rows of every array
struct gsample {
    rows r;                                                     // x, mean, std [S, D]
    const float *hf, *target_xy, *grid_x, *grid_y, *points;      // target_xy [2]
    const int32_t *point_start;
    float *scr;
};

PARC_MP_HD bool on(const parc_mdm_guide_cfg_t &c, int t) { return (c.enabled >> t) & 1; }
PARC_MP_FN local_grid grid_of(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g) {
    return make_local_grid(c, g.scr + L.o_hf, g.grid_x, g.grid_y);
}

// max_rate[k - 1] * dt^k: a double product rounded once, as the reference's Python scalar is when torch subtracts it from a tensor
PARC_MP_FN float threshold(const parc_mdm_guide_cfg_t &c, int k) {
    double p = c.dt;
    for (int i = 1; i < k; ++i) p *= c.dt;
    return (float)(c.max_rate[k - 1] * p);
}

// element e of the k-th difference of n positions stored `stride` floats apart: torch's vel = p[1:] - p[:-1], acc = vel[1:] - vel[:-1], ...
PARC_MP_FN v3 diff_k(const float *p, int stride, int e, int k) {
    v3 d[4];
    for (int i = 0; i <= k; ++i) d[i] = ld3(p + (size_t)(e + i) * stride);
    for (int o = 0; o < k; ++o)
        for (int i = 0; i < k - o; ++i) d[i] = d[i + 1] - d[i];
    return d[0];
}
// clamp(min=0) keeps a NaN
PARC_MP_FN float hinge(float v) { return v > 0.f ? v : (v == v ? 0.f : v); }

// the summands of (frame f, body b) for TARGET, SPEED, ACC, JERK: body b owns element b of each difference order
PARC_MP_FN void terms_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int f, int b) {
    const float *pos = g.scr + L.pose.o_bpos + (size_t)f * L.nb * 3;
    const size_t i = (size_t)f * L.nb + b;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (b == 0 && on(c, PARC_MDM_GUIDE_TARGET)) {
        const float dx = g.target_xy[0] - pos[0], dy = g.target_xy[1] - pos[1];
        t[0] = dx * dx + dy * dy;
    }
    for (int k = 1; k <= 3; ++k)
        if (on(c, PARC_MDM_GUIDE_SPEED + k - 1) && b < L.nb - k) {
            const v3 d = diff_k(pos, 3, b, k);
            t[k] = hinge(sqrtf(dot3(d, d)) - threshold(c, k));
        }
    for (int k = 0; k < 4; ++k) g.scr[L.o_part + (size_t)k * L.n_items + i] = t[k];
}

PARC_MP_FN void point_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int f, int p) {
    int cell;
    g.scr[L.o_psdf + f * L.P + p] = point_sdf(grid_of(c, L, g), L.pose, g.scr, g.points, g.point_start, f, p, cell);
    reinterpret_cast<uint16_t *>(g.scr + L.o_pcol)[f * L.P + p] = (uint16_t)cell;
}

// sub-sum `sub` of term t: summands sub, sub + 16, ... in ascending order
PARC_MP_FN void subsum_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int t, int sub) {
    float acc = 0.f;
    if (t == PARC_MDM_GUIDE_HF) {
        if (on(c, t)) acc = penetration_subsum(g.scr + L.o_psdf, L.S * L.P, sub);
    } else {
        const int k = t == PARC_MDM_GUIDE_TARGET ? 0 : t - PARC_MDM_GUIDE_SPEED + 1;
        acc = row_subsum(g.scr + L.o_part + (size_t)k * L.n_items, L.n_items, sub);
    }
    g.scr[L.o_r1 + t * PARC_MP_NSUB + sub] = acc;
}

PARC_MP_FN float term_value(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int t) {
    if (!on(c, t)) return 0.f;
    const float acc = fold_subsums(g.scr + L.o_r1 + t * PARC_MP_NSUB);
    return t <= PARC_MDM_GUIDE_HF ? 0.5f * acc : acc;
}

// cotangents of the body transform of (frame f, body b), gathered from every term that reads it
PARC_MP_FN void grad_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int f, int b) {
    const float *pos = g.scr + L.pose.o_bpos + (size_t)f * L.nb * 3;
    const size_t i = (size_t)f * L.nb + b;
    const v3 pP = ld3(pos + b * 3);
    const q4 rP = ld4(g.scr + L.pose.o_brot + i * 4);
    v3 gp = mk3(0.f, 0.f, 0.f);
    q4 gq = q4{0.f, 0.f, 0.f, 0.f};
    if (b == 0 && on(c, PARC_MDM_GUIDE_TARGET)) {
        gp.x = -(c.w[PARC_MDM_GUIDE_TARGET] * (g.target_xy[0] - pP.x));
        gp.y = -(c.w[PARC_MDM_GUIDE_TARGET] * (g.target_xy[1] - pP.y));
    }
    for (int k = 1; k <= 3; ++k) {
        const int t = PARC_MDM_GUIDE_SPEED + k - 1;
        if (!on(c, t)) continue;
        const float thr = threshold(c, k);
        // element e = b - j reads body b with the coefficient of p[e + j] in the k-th difference: (-1)^(k - j) binomial(k, j)
        for (int j = 0; j <= k; ++j) {
            const int e = b - j;
            if (e < 0 || e >= L.nb - k) continue;
            const float binom = (j == 0 || j == k) ? 1.f : (float)k, coef = ((k - j) & 1) ? -binom : binom;
            const v3 d = diff_k(pos, 3, e, k);
            const float n = sqrtf(dot3(d, d)), h = n - thr;
            if (h > 0.f) gp = gp + (c.w[t] * coef / n) * d;
            else if (h != h) gp = gp + mk3(h, h, h);
        }
    }
    if (on(c, PARC_MDM_GUIDE_HF)) {
        const uint16_t *cols = reinterpret_cast<const uint16_t *>(g.scr + L.o_pcol);
        const local_grid grid = grid_of(c, L, g);
        const int p0 = g.point_start[b] > 0 ? g.point_start[b] : 0, p1 = g.point_start[b + 1] < L.P ? g.point_start[b + 1] : L.P;
        for (int p = p0; p < p1; ++p) {
            const float sdf = g.scr[L.o_psdf + f * L.P + p];
            if (sdf != sdf) gp = gp + mk3(sdf, sdf, sdf);
            if (!(sdf < 0.f)) continue;
            const v3 loc = ld3(g.points + (size_t)p * 3);
            const v3 cg = column_grad(grid, pP + qrot(rP, loc), (int)cols[f * L.P + p]);
            const v3 gg = (-(c.w[PARC_MDM_GUIDE_HF] * sdf)) * cg;          // sdf = -distance; d(sdf^2 / 2) = sdf
            gp = gp + gg;
            gq = qadd(gq, qrot_bwd_q(rP, loc, gg));
        }
    }
    st3(g.scr + L.cot.o_gpos + i * 3, gp);
    st4(g.scr + L.cot.o_grot + i * 4, gq);
}

// does the guidance loss read feature column d?  (root position, root rotation and the joint dofs; JOINT_POS and CONTACTS never)
PARC_MP_FN bool column_read(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, int d) {
    return (d >= c.off_root_pos && d < c.off_root_pos + 3) || (d >= c.off_root_rot && d < c.off_root_rot + 3) ||
           (d >= c.off_joint_rot && d < c.off_joint_rot + m.dof_size);
}

// sample b of a batch of B: x_out (this sample's [S, D] rows; may be g.r.x) and terms [TERMS, B]
PARC_MP_FN void step_sample(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, const gsample &g, int b, int B, float *x_out, float *terms,
                            int lane, int nlanes) {
    const layout L = make_layout(m, c);
    const feat_layout fl = make_feat_layout(c);
    float *scr = g.scr;
    const int SD = L.S * L.D;
    if (on(c, PARC_MDM_GUIDE_HF))
        for (int i = lane; i < L.XY; i += nlanes) scr[L.o_hf + i] = g.hf[i] * c.max_h;
    for (int i = lane; i < SD; i += nlanes) scr[L.o_gx + i] = 0.f;          // columns of joints without dofs stay 0
    for (int i = lane; i < L.S * L.J * 4; i += nlanes) scr[L.cot.o_gjq + i] = 0.f;          // no term reads a joint rotation directly
    for (int f = lane; f < L.S; f += nlanes) chain_from_feat(m, L.pose, scr, g.r, fl, f);
    PARC_MP_SYNC();
    if (on(c, PARC_MDM_GUIDE_HF))
        for (int i = lane; i < L.S * L.P; i += nlanes) point_item(c, L, g, i / L.P, i % L.P);
    for (int i = lane; i < L.n_items; i += nlanes) terms_item(c, L, g, i / L.nb, i % L.nb);
    PARC_MP_SYNC();
    for (int i = lane; i < PARC_MDM_GUIDE_TERMS * PARC_MP_NSUB; i += nlanes) subsum_item(c, L, g, i / PARC_MP_NSUB, i % PARC_MP_NSUB);
    PARC_MP_SYNC();
    for (int t = lane; t < PARC_MDM_GUIDE_TERMS; t += nlanes) terms[(size_t)t * B + b] = term_value(c, L, g, t);
    for (int i = lane; i < L.n_items; i += nlanes) grad_item(c, L, g, i / L.nb, i % L.nb);
    PARC_MP_SYNC();
    for (int f = lane; f < L.S; f += nlanes) chain_grad_item(m, L.pose, L.cot, scr, g.r, fl, f, scr + L.o_gx);
    PARC_MP_SYNC();
    // the updated sample, still in the scratch: the last reads of x
    for (int i = lane; i < SD; i += nlanes) {
        const float xi = g.r.x[i];
        scr[L.o_gx + i] = column_read(m, c, i % L.D) ? xi - scr[L.o_gx + i] * c.guidance_str : xi;
    }
    PARC_MP_SYNC();
    for (int i = lane; i < SD; i += nlanes) x_out[i] = scr[L.o_gx + i];
}

PARC_MP_FN gsample make_gsample(const parc_mdm_guide_cfg_t &c, int b, const float *x, const float *mean, const float *std, const float *hfs,
                                const float *target_xy, const float *grid_x, const float *grid_y, const float *points,
                                const int32_t *point_start, float *scr) {
    gsample g;
    g.r = rows{x + (size_t)b * c.seq_len * c.feat_dim, mean, std};
    g.hf = hfs ? hfs + (size_t)b * c.dim_x * c.dim_y : hfs;
    g.grid_x = grid_x, g.grid_y = grid_y, g.points = points, g.point_start = point_start, g.scr = scr;
    g.target_xy = target_xy ? target_xy + (size_t)b * 2 : target_xy;
    return g;
}

// ---- Argument rules of the entry point (include/parc_mdm_guide.h), answered before any HIP call ----
static inline int check_cfg(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, int B) {
    if (check_window(m, c, B) != PARC_OK) return PARC_EINVAL;
    if (c.enabled & ~((1 << PARC_MDM_GUIDE_TERMS) - 1)) return PARC_EINVAL;
    if (on(c, PARC_MDM_GUIDE_HF) && c.num_points < 1) return PARC_EINVAL;
    // sizes in 64 bits before the layout multiplies them as int; a column index is stored in 16 bits
    if ((int64_t)c.dim_x * c.dim_y > PARC_MDM_GUIDE_MAX_LDS / 4) return PARC_EUNSUPPORTED;
    if ((int64_t)c.seq_len * (m.num_bodies * 22 + (int64_t)c.feat_dim + 2 * (int64_t)c.num_points) > 0x7fffff) return PARC_EUNSUPPORTED;
    if (lds_bytes(m, c) > PARC_MDM_GUIDE_MAX_LDS) return PARC_EUNSUPPORTED;
    return PARC_OK;
}

static inline int check_args(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, int B, const void *x, const void *mean, const void *std,
                             const void *hfs, const void *target_xy, const void *grid_x, const void *grid_y, const void *points,
                             const void *point_start, const void *x_out, const void *terms) {
    const int rc = check_cfg(m, c, B);
    if (rc != PARC_OK) return rc;
    if (B == 0 || c.enabled == 0) return PARC_MG_NOTHING;
    if (!x || !mean || !std || !x_out || !terms) return PARC_EINVAL;
    if (on(c, PARC_MDM_GUIDE_TARGET) && !target_xy) return PARC_EINVAL;
    if (on(c, PARC_MDM_GUIDE_HF) && (!hfs || !grid_x || !grid_y || !points || !point_start)) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_mg
