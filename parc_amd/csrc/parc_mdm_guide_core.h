// The motion generator's guidance step for ONE sample: the guidance loss, its gradient and the update in place
// (include/parc_mdm_guide.h), shared by the device (hipcc: parc_mdm_guide.hip, one workgroup per sample) and the host (g++: the CPU
// tests, tests/tools/mdm_guide_host.cpp).  Built with -ffp-contract=off on both sides.  Reference: diffusion/mdm.py:1444-1542.
//
// The pose chain from standardised features (chain_item), its adjoint (chain_grad_item), the terrain scan (point_sdf) and the selected
// column's gradient (column_grad) are those of parc_mdm_loss_core.h, called on a parc_ml::layout whose offsets are this file's; so are
// the phase scheme (loops `for (i = lane; i < n; i += nlanes)` separated by PARC_ML_SYNC()) and the fold (summand i to sub-sum i % 16,
// the 16 sub-sums added in ascending order).  New here: the difference hinges along the body axis with their gathered cotangents, the
// 16-bit column record, and the update, which keeps every read of x in front of a barrier and every write of x_out behind it.
#pragma once
#include "../../include/parc_mdm_guide.h"
#include "parc_mdm_loss_core.h"

#define PARC_MG_NOTHING 1      // argument check: valid, and nothing to do

namespace parc_mg {

using namespace parc_ml;

// Scratch layout of one sample, in floats: parc_ml::layout for the shared pieces, and this file's own blocks
struct glayout {
    layout L;
    int o_gx, o_pcol;      // [S, D] gradient, then the updated sample; [S, P] columns, 16 bits each
    int64_t total;
};

PARC_ML_HD glayout make_glayout(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c) {
    glayout G;
    layout &L = G.L;
    L.S = c.seq_len, L.nb = m.num_bodies, L.J = m.num_bodies - 1, L.P = c.num_points, L.XY = c.dim_x * c.dim_y, L.D = c.feat_dim;
    L.n_items = L.S * L.nb;
    int64_t o = 0;
    L.o_hf = (int)o, o += L.XY;
    L.o_bpos[0] = L.o_bpos[1] = (int)o, o += (int64_t)L.n_items * 3;
    L.o_brot[0] = L.o_brot[1] = (int)o, o += (int64_t)L.n_items * 4;
    L.o_jq[0] = L.o_jq[1] = (int)o, o += (int64_t)L.S * L.J * 4;
    L.o_gpos = (int)o, o += (int64_t)L.n_items * 3;
    L.o_grot = (int)o, o += (int64_t)L.n_items * 4;
    L.o_part = L.o_gpos;          // the summands of TARGET, SPEED, ACC, JERK [4, n_items] are folded before a cotangent is written
    L.o_gjq = (int)o, o += (int64_t)L.S * L.J * 4;
    G.o_gx = (int)o, o += (int64_t)L.S * L.D;
    L.o_r1 = (int)o, o += PARC_MDM_GUIDE_TERMS * PARC_ML_NSUB;
    L.o_sum = L.o_k = L.o_r1;     // not used
    L.o_psdf = (int)o, o += (int64_t)L.S * L.P;
    L.o_pcell = L.o_psdf;         // not used: the columns are G.o_pcol
    G.o_pcol = (int)o, o += ((int64_t)L.S * L.P + 1) / 2;
    L.total = G.total = o;
    return G;
}

static inline int64_t lds_bytes(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c) { return 4 * make_glayout(m, c).total; }

// the part of the configuration that the loss's primitives read
PARC_ML_HD parc_mdm_loss_cfg_t loss_cfg(const parc_mdm_guide_cfg_t &c) {
    parc_mdm_loss_cfg_t l = {};
    l.seq_len = c.seq_len, l.feat_dim = c.feat_dim;
    l.off_root_pos = c.off_root_pos, l.off_root_rot = c.off_root_rot, l.off_joint_pos = c.off_joint_pos, l.off_joint_rot = c.off_joint_rot;
    l.off_contacts = c.off_contacts;
    l.dim_x = c.dim_x, l.dim_y = c.dim_y, l.num_points = c.num_points;
    l.ox = c.ox, l.oy = c.oy, l.half_x = c.half_x, l.half_y = c.half_y, l.max_h = c.max_h, l.base_z = c.base_z;
    l.dt = (float)c.dt;
    return l;
}

struct gsample {
    sample s;
    const float *target_xy;      // [2]
};

PARC_ML_HD bool on(const parc_mdm_guide_cfg_t &c, int t) { return (c.enabled >> t) & 1; }

// max_rate[k - 1] * dt^k: a double product rounded once, as the reference's Python scalar is when torch subtracts it from a tensor
PARC_ML_FN float threshold(const parc_mdm_guide_cfg_t &c, int k) {
    double p = c.dt;
    for (int i = 1; i < k; ++i) p *= c.dt;
    return (float)(c.max_rate[k - 1] * p);
}

// element e of the k-th difference of n positions stored `stride` floats apart: torch's vel = p[1:] - p[:-1], acc = vel[1:] - vel[:-1], ...
PARC_ML_FN v3 diff_k(const float *p, int stride, int e, int k) {
    v3 d[4];
    for (int i = 0; i <= k; ++i) d[i] = ld3(p + (size_t)(e + i) * stride);
    for (int o = 0; o < k; ++o)
        for (int i = 0; i < k - o; ++i) d[i] = d[i + 1] - d[i];
    return d[0];
}
// clamp(min=0) keeps a NaN
PARC_ML_FN float hinge(float v) { return v > 0.f ? v : (v == v ? 0.f : v); }

// the summands of (frame f, body b) for TARGET, SPEED, ACC, JERK: body b owns element b of each difference order
PARC_ML_FN void terms_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int f, int b) {
    const float *pos = g.s.scr + L.o_bpos[0] + (size_t)f * L.nb * 3;
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
    for (int k = 0; k < 4; ++k) g.s.scr[L.o_part + (size_t)k * L.n_items + i] = t[k];
}

PARC_ML_FN void point_item(const parc_mdm_loss_cfg_t &lc, const glayout &G, const gsample &g, int f, int p) {
    int cell;
    g.s.scr[G.L.o_psdf + f * G.L.P + p] = point_sdf(lc, G.L, g.s, f, p, cell);
    reinterpret_cast<uint16_t *>(g.s.scr + G.o_pcol)[f * G.L.P + p] = (uint16_t)cell;
}

// sub-sum `sub` of term t: summands sub, sub + 16, ... in ascending order
PARC_ML_FN void subsum_item(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int t, int sub) {
    float acc = 0.f;
    if (t == PARC_MDM_GUIDE_HF) {
        if (on(c, t))
            for (int i = sub; i < L.S * L.P; i += PARC_ML_NSUB) {
                const float d = g.s.scr[L.o_psdf + i];
                const float mn = d < 0.f ? d : (d == d ? 0.f : d);          // clamp(max=0) keeps a NaN
                acc += mn * mn;
            }
    } else {
        const int k = t == PARC_MDM_GUIDE_TARGET ? 0 : t - PARC_MDM_GUIDE_SPEED + 1;
        for (int i = sub; i < L.n_items; i += PARC_ML_NSUB) acc += g.s.scr[L.o_part + (size_t)k * L.n_items + i];
    }
    g.s.scr[L.o_r1 + t * PARC_ML_NSUB + sub] = acc;
}

PARC_ML_FN float term_value(const parc_mdm_guide_cfg_t &c, const layout &L, const gsample &g, int t) {
    if (!on(c, t)) return 0.f;
    float acc = 0.f;
    for (int k = 0; k < PARC_ML_NSUB; ++k) acc += g.s.scr[L.o_r1 + t * PARC_ML_NSUB + k];
    return t <= PARC_MDM_GUIDE_HF ? 0.5f * acc : acc;
}

// cotangents of the body transform of (frame f, body b), gathered from every term that reads it
PARC_ML_FN void grad_item(const parc_mdm_guide_cfg_t &c, const parc_mdm_loss_cfg_t &lc, const glayout &G, const gsample &g, int f, int b) {
    const layout &L = G.L;
    const float *pos = g.s.scr + L.o_bpos[0] + (size_t)f * L.nb * 3;
    const size_t i = (size_t)f * L.nb + b;
    const v3 pP = ld3(pos + b * 3);
    const q4 rP = ld4(g.s.scr + L.o_brot[0] + i * 4);
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
        const uint16_t *cols = reinterpret_cast<const uint16_t *>(g.s.scr + G.o_pcol);
        const int p0 = g.s.point_start[b] > 0 ? g.s.point_start[b] : 0, p1 = g.s.point_start[b + 1] < L.P ? g.s.point_start[b + 1] : L.P;
        for (int p = p0; p < p1; ++p) {
            const float sdf = g.s.scr[L.o_psdf + f * L.P + p];
            if (sdf != sdf) gp = gp + mk3(sdf, sdf, sdf);
            if (!(sdf < 0.f)) continue;
            const v3 loc = ld3(g.s.points + (size_t)p * 3);
            const v3 cg = column_grad(lc, L, g.s, pP + qrot(rP, loc), (int)cols[f * L.P + p]);
            const v3 gg = (-(c.w[PARC_MDM_GUIDE_HF] * sdf)) * cg;          // sdf = -distance; d(sdf^2 / 2) = sdf
            gp = gp + gg;
            gq = qadd(gq, qrot_bwd_q(rP, loc, gg));
        }
    }
    st3(g.s.scr + L.o_gpos + i * 3, gp);
    st4(g.s.scr + L.o_grot + i * 4, gq);
}

// does the guidance loss read feature column d?  (root position, root rotation and the joint dofs; JOINT_POS and CONTACTS never)
PARC_ML_FN bool column_read(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, int d) {
    return (d >= c.off_root_pos && d < c.off_root_pos + 3) || (d >= c.off_root_rot && d < c.off_root_rot + 3) ||
           (d >= c.off_joint_rot && d < c.off_joint_rot + m.dof_size);
}

// sample b of a batch of B: x_out (this sample's [S, D] rows; may be g.s.x) and terms [TERMS, B]
PARC_ML_FN void step_sample(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, const gsample &g, int b, int B, float *x_out, float *terms,
                            int lane, int nlanes) {
    const glayout G = make_glayout(m, c);
    const layout &L = G.L;
    const parc_mdm_loss_cfg_t lc = loss_cfg(c);
    float *scr = g.s.scr;
    const int SD = L.S * L.D;
    if (on(c, PARC_MDM_GUIDE_HF))
        for (int i = lane; i < L.XY; i += nlanes) scr[L.o_hf + i] = g.s.hf[i] * c.max_h;
    for (int i = lane; i < SD; i += nlanes) scr[G.o_gx + i] = 0.f;          // columns of joints without dofs stay 0
    for (int i = lane; i < L.S * L.J * 4; i += nlanes) scr[L.o_gjq + i] = 0.f;          // no term reads a joint rotation directly
    for (int f = lane; f < L.S; f += nlanes) chain_item(m, lc, L, g.s, 0, f);
    PARC_ML_SYNC();
    if (on(c, PARC_MDM_GUIDE_HF))
        for (int i = lane; i < L.S * L.P; i += nlanes) point_item(lc, G, g, i / L.P, i % L.P);
    for (int i = lane; i < L.n_items; i += nlanes) terms_item(c, L, g, i / L.nb, i % L.nb);
    PARC_ML_SYNC();
    for (int i = lane; i < PARC_MDM_GUIDE_TERMS * PARC_ML_NSUB; i += nlanes) subsum_item(c, L, g, i / PARC_ML_NSUB, i % PARC_ML_NSUB);
    PARC_ML_SYNC();
    for (int t = lane; t < PARC_MDM_GUIDE_TERMS; t += nlanes) terms[(size_t)t * B + b] = term_value(c, L, g, t);
    for (int i = lane; i < L.n_items; i += nlanes) grad_item(c, lc, G, g, i / L.nb, i % L.nb);
    PARC_ML_SYNC();
    for (int f = lane; f < L.S; f += nlanes) chain_grad_item(m, lc, L, g.s, f, scr + G.o_gx);
    PARC_ML_SYNC();
    // the updated sample, still in the scratch: the last reads of x
    for (int i = lane; i < SD; i += nlanes) {
        const float xi = g.s.x[i];
        scr[G.o_gx + i] = column_read(m, c, i % L.D) ? xi - scr[G.o_gx + i] * c.guidance_str : xi;
    }
    PARC_ML_SYNC();
    for (int i = lane; i < SD; i += nlanes) x_out[i] = scr[G.o_gx + i];
}

PARC_ML_FN gsample make_gsample(const parc_mdm_guide_cfg_t &c, int b, const float *x, const float *mean, const float *std, const float *hfs,
                                const float *target_xy, const float *grid_x, const float *grid_y, const float *points,
                                const int32_t *point_start, float *scr) {
    gsample g;
    g.s.x = x + (size_t)b * c.seq_len * c.feat_dim, g.s.mean = mean, g.s.std = std;
    g.s.root_pos = g.s.root_rot = g.s.joint_rot = g.s.contacts = g.s.target_dir = nullptr;
    g.s.hf = hfs ? hfs + (size_t)b * c.dim_x * c.dim_y : hfs;
    g.s.grid_x = grid_x, g.s.grid_y = grid_y, g.s.points = points, g.s.point_start = point_start, g.s.scr = scr;
    g.target_xy = target_xy ? target_xy + (size_t)b * 2 : target_xy;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Argument rules of the entry point (include/parc_mdm_guide.h), answered before any HIP call
// ---------------------------------------------------------------------------------------------------------------------------------
static inline int check_cfg(const parc_char_model_t &m, const parc_mdm_guide_cfg_t &c, int B) {
    if (check_layout(m, loss_cfg(c), B) != PARC_OK) return PARC_EINVAL;
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
