// The motion generator's training loss for ONE sample, forward and adjoint (include/parc_mdm_loss.h), shared by the device (hipcc:
// parc_mdm_loss.hip, one workgroup per sample) and the host (g++: the CPU tests, tests/tools/mdm_loss_host.cpp).  Built with
// -ffp-contract=off on both sides: every expression is a sequence of separately rounded fp32 operations, as torch evaluates the
// reference's (diffusion/mdm.py:434-478 extract_motion_features, :617-754 motion_difference, :978-1028 compute_point_hf_sdf).
//
// A sample is worked on by `nlanes` lanes in phases; a phase is a loop `for (i = lane; i < n; i += nlanes)` over its work items and
// phases are separated by PARC_ML_SYNC() (a barrier on the device, nothing on the host, which calls with lane 0 of 1).  Everything a
// later phase needs sits in the sample's scratch (LDS on the device): the heightfield, both sides' body transforms and joint rotations,
// the points' distances and columns, the per-item summands.  Sums are folded in an order that does not depend on nlanes: summand i goes
// to sub-sum i % 16, the 16 sub-sums are added in ascending order.
//
// Adjoint formulas (those of parc_pose_opt.hip, restated here because that file is device-only):
//   q = a (x) b bilinear               =>  g_a = g (x) conj(b),  g_b = conj(a) (x) g
//   r = v + w t + u x t, t = 2 u x v   =>  g_w = g.t,  g_t = w g + g x u,  g_u = t x g + 2 v x g_t
//   angle = 2 atan2(|v|, w) of the w >= 0 representative; e = angle v / |v|
// and the singular-input rule of the header: a rotation in the reference's "below 1e-5" branch has gradient 0.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/parc_mdm_loss.h"
#include "parc_sdf_core.h"

#if defined(__HIPCC__)
#define PARC_ML_FN __device__ __forceinline__
#define PARC_ML_HD __host__ __device__ inline
#else
#define PARC_ML_FN static inline
#define PARC_ML_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PARC_ML_SYNC() __syncthreads()
#else
#define PARC_ML_SYNC() ((void)0)
#endif

#define PARC_ML_NOTHING 1      // argument check: valid, and nothing to do
#define PARC_ML_NSUB 16        // sub-sums per term
#define PARC_ML_LOSS_FN_TERMS 12   // terms 0..11 go through loss_fn; HF_COLLISION and TARGET do not

namespace parc_ml {

struct v3 { float x, y, z; };
struct q4 { float x, y, z, w; };

PARC_ML_FN v3 mk3(float x, float y, float z) { return v3{x, y, z}; }
PARC_ML_FN v3 operator+(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PARC_ML_FN v3 operator-(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PARC_ML_FN v3 operator*(float s, v3 a) { return v3{s * a.x, s * a.y, s * a.z}; }
PARC_ML_FN float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PARC_ML_FN v3 cross3(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PARC_ML_FN q4 qadd(q4 a, q4 b) { return q4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
PARC_ML_FN q4 qscale(float s, q4 a) { return q4{s * a.x, s * a.y, s * a.z, s * a.w}; }
PARC_ML_FN q4 qconj(q4 q) { return q4{-q.x, -q.y, -q.z, q.w}; }
PARC_ML_FN v3 ld3(const float *p) { return v3{p[0], p[1], p[2]}; }
PARC_ML_FN q4 ld4(const float *p) { return q4{p[0], p[1], p[2], p[3]}; }
PARC_ML_FN void st3(float *p, v3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
PARC_ML_FN void st4(float *p, q4 q) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }

PARC_ML_FN q4 qmul(q4 a, q4 b) {
    return q4{((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y, ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x,
              ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w, ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z};
}
// util/torch_util.py:60-66
PARC_ML_FN v3 qrot(q4 q, v3 v) {
    const v3 u = mk3(q.x, q.y, q.z);
    const v3 t = 2.f * cross3(u, v);
    const v3 c = cross3(u, t);
    return v3{(v.x + q.w * t.x) + c.x, (v.y + q.w * t.y) + c.y, (v.z + q.w * t.z) + c.z};
}
PARC_ML_FN q4 qunit(q4 q) {
    const float n = fmaxf(sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w), 1e-9f);
    return q4{q.x / n, q.y / n, q.z / n, q.w / n};
}
// util/torch_util.py:311-317
PARC_ML_FN q4 aa_to_quat(v3 axis, float angle) {
    const float th = angle / 2.f;
    const float n = fmaxf(sqrtf(dot3(axis, axis)), 1e-9f);
    const float s = sinf(th);
    return qunit(q4{axis.x / n * s, axis.y / n * s, axis.z / n * s, cosf(th)});
}
// util/torch_util.py:394-419
PARC_ML_FN q4 em_to_quat(v3 em) {
    float a = sqrtf(dot3(em, em));
    v3 ax = v3{em.x / a, em.y / a, em.z / a};
    a = atan2f(sinf(a), cosf(a));
    if (!(fabsf(a) > 1e-5f)) {
        ax = mk3(0.f, 0.f, 1.f);
        a = 0.f;
    }
    return aa_to_quat(ax, a);
}
// util/torch_util.py:68-88 and :346-351: the w >= 0 representative's angle and exponential map
PARC_ML_FN float qangle(q4 d) {
    const float s = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    return s > 1e-5f ? 2.0f * atan2f(s, fabsf(d.w)) : 0.f;
}
PARC_ML_FN v3 quat_to_em(q4 d) {
    const float sg = d.w < 0.f ? -1.f : 1.f;
    const v3 v = mk3(sg * d.x, sg * d.y, sg * d.z);
    const float s = sqrtf(dot3(v, v));
    if (!(s > 1e-5f)) return mk3(0.f, 0.f, 0.f);          // angle 0 times the z axis
    const float a = 2.0f * atan2f(s, sg * d.w);
    return mk3(v.x / s * a, v.y / s * a, v.z / s * a);
}
PARC_ML_FN float qdiff_angle(q4 q0, q4 q1) { return qangle(qmul(q1, qconj(q0))); }

// ---- adjoints ----
// cotangent of d for angle = qangle(d)
PARC_ML_FN q4 qangle_bwd(q4 d, float g) {
    const float s = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    if (!(s > 1e-5f)) return q4{0.f, 0.f, 0.f, 0.f};
    const float sg = d.w < 0.f ? -1.0f : 1.0f;
    const float w = sg * d.w, den = s * s + w * w;
    const float gs = 2.0f * w / den * g / s;
    return q4{gs * d.x, gs * d.y, gs * d.z, sg * (-2.0f * s / den * g)};
}
// cotangent of d for e = quat_to_em(d)
PARC_ML_FN q4 quat_to_em_bwd(q4 d, v3 g) {
    const float sg = d.w < 0.f ? -1.f : 1.f;
    const v3 v = mk3(sg * d.x, sg * d.y, sg * d.z);
    const float w = sg * d.w;
    const float s = sqrtf(dot3(v, v));
    if (!(s > 1e-5f)) return q4{0.f, 0.f, 0.f, 0.f};
    const float a = 2.0f * atan2f(s, w), den = s * s + w * w;
    const v3 u = mk3(v.x / s, v.y / s, v.z / s);
    const float gu = dot3(g, u);
    const float c0 = a / s, c1 = 2.0f * w / den * gu;
    const v3 gv = mk3(c0 * (g.x - gu * u.x) + c1 * u.x, c0 * (g.y - gu * u.y) + c1 * u.y, c0 * (g.z - gu * u.z) + c1 * u.z);
    return q4{sg * gv.x, sg * gv.y, sg * gv.z, sg * (-2.0f * s / den * gu)};
}
// d = b (x) conj(a): cotangents of a and b from the cotangent of d
PARC_ML_FN q4 qdiff_bwd_a(q4 b, q4 gd) {
    const q4 gc = qmul(qconj(b), gd);
    return q4{-gc.x, -gc.y, -gc.z, gc.w};
}
PARC_ML_FN q4 qdiff_bwd_b(q4 a, q4 gd) { return qmul(gd, a); }

PARC_ML_FN q4 qrot_bwd_q(q4 q, v3 v, v3 g) {
    const v3 u = mk3(q.x, q.y, q.z);
    const v3 t = 2.f * cross3(u, v);
    const v3 gxu = cross3(g, u);
    const v3 gt = mk3(q.w * g.x + gxu.x, q.w * g.y + gxu.y, q.w * g.z + gxu.z);
    const v3 gu = cross3(t, g) + 2.f * cross3(v, gt);
    return q4{gu.x, gu.y, gu.z, dot3(g, t)};
}
struct aa_grad { v3 g_axis; float g_angle; };
PARC_ML_FN aa_grad aa_to_quat_bwd(v3 axis, float angle, q4 q, q4 g) {
    const float gq = ((g.x * q.x + g.y * q.y) + g.z * q.z) + g.w * q.w;          // through qunit at unit length: a projection
    const q4 gr = q4{g.x - gq * q.x, g.y - gq * q.y, g.z - gq * q.z, g.w - gq * q.w};
    const float h = 0.5f * angle;
    const float sh = sinf(h), ch = cosf(h);
    const float na = fmaxf(sqrtf(dot3(axis, axis)), 1e-9f);
    const v3 a = mk3(axis.x / na, axis.y / na, axis.z / na);
    const v3 grv = mk3(gr.x, gr.y, gr.z);
    aa_grad o;
    o.g_angle = 0.5f * (ch * dot3(a, grv) - sh * gr.w);
    const v3 ga = mk3(sh * grv.x, sh * grv.y, sh * grv.z);
    const float gaa = dot3(ga, a);
    o.g_axis = mk3((ga.x - gaa * a.x) / na, (ga.y - gaa * a.y) / na, (ga.z - gaa * a.z) / na);
    return o;
}
PARC_ML_FN v3 em_to_quat_bwd(v3 em, q4 q, q4 g) {
    const float raw = sqrtf(dot3(em, em));
    const float ang = atan2f(sinf(raw), cosf(raw));
    if (!(fabsf(ang) > 1e-5f)) return mk3(0.f, 0.f, 0.f);
    const v3 a = mk3(em.x / raw, em.y / raw, em.z / raw);
    const aa_grad ag = aa_to_quat_bwd(a, ang, q, g);
    const float ga = dot3(ag.g_axis, a);
    return mk3((ag.g_axis.x - ga * a.x) / raw + ag.g_angle * a.x, (ag.g_axis.y - ga * a.y) / raw + ag.g_angle * a.y,
               (ag.g_axis.z - ga * a.z) / raw + ag.g_angle * a.z);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Scratch layout of one sample, in floats
// ---------------------------------------------------------------------------------------------------------------------------------
struct layout {
    int S, nb, J, P, XY, D, n_items;
    int o_hf, o_bpos[2], o_brot[2], o_jq[2], o_psdf, o_pcell, o_part, o_r1, o_sum, o_k;
    int o_gpos, o_grot, o_gjq;          // the backward launch's cotangents reuse the summands' block
    int64_t total;
};

PARC_ML_HD layout make_layout(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c) {
    layout L;
    L.S = c.seq_len, L.nb = m.num_bodies, L.J = m.num_bodies - 1, L.P = c.num_points, L.XY = c.dim_x * c.dim_y, L.D = c.feat_dim;
    L.n_items = L.S * L.nb;
    int64_t o = 0;
    L.o_hf = (int)o, o += L.XY;
    for (int s = 0; s < 2; ++s) {
        L.o_bpos[s] = (int)o, o += (int64_t)L.n_items * 3;
        L.o_brot[s] = (int)o, o += (int64_t)L.n_items * 4;
        L.o_jq[s] = (int)o, o += (int64_t)L.S * L.J * 4;
    }
    L.o_psdf = (int)o, o += (int64_t)L.S * L.P;
    L.o_pcell = (int)o, o += (int64_t)L.S * L.P;
    L.o_part = (int)o, o += (int64_t)PARC_ML_LOSS_FN_TERMS * L.n_items;
    L.o_gpos = L.o_part, L.o_grot = L.o_gpos + L.n_items * 3, L.o_gjq = L.o_grot + L.n_items * 4;        // 11 nb - 4 <= 12 nb per frame
    L.o_r1 = (int)o, o += PARC_MDM_LOSS_TERMS * PARC_ML_NSUB;
    L.o_sum = (int)o, o += PARC_MDM_LOSS_TERMS;
    L.o_k = (int)o, o += PARC_MDM_LOSS_TERMS;
    L.total = o;
    return L;
}

static inline int64_t lds_bytes(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c) { return 4 * make_layout(m, c).total; }

// What one call works on: sample b's rows of every array
struct sample {
    const float *x, *mean, *std;                                // [S, D]
    const float *root_pos, *root_rot, *joint_rot, *contacts;    // the true side
    const float *hf, *target_dir, *grid_x, *grid_y, *points;
    const int32_t *point_start;
    float *scr;
};

PARC_ML_FN bool term_on(const parc_mdm_loss_cfg_t &c, int t) { return (c.enabled >> t) & 1; }
PARC_ML_FN float feat(const sample &s, const parc_mdm_loss_cfg_t &c, int f, int d) {
    const int i = f * c.feat_dim + d;
    return s.x[i] * s.std[i] + s.mean[i];
}
PARC_ML_FN v3 feat3(const sample &s, const parc_mdm_loss_cfg_t &c, int f, int d) { return mk3(feat(s, c, f, d), feat(s, c, f, d + 1), feat(s, c, f, d + 2)); }
PARC_ML_FN v3 local_t(const parc_char_model_t &m, int b) { return mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]); }
PARC_ML_FN q4 local_r(const parc_char_model_t &m, int b) {
    return q4{m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]};
}
PARC_ML_FN v3 joint_axis(const parc_char_model_t &m, int b) { return mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]); }

// (a - b)^2 summed over the components, + c2 per component (0 for squared_l2): the summand of loss_fn
PARC_ML_FN float sq1(float e, float c2) { return e * e + c2; }
PARC_ML_FN float sq3(v3 e, float c2) { return (sq1(e.x, c2) + sq1(e.y, c2)) + sq1(e.z, c2); }

// velocity error of the frame pair (f, f + 1) of positions stored with `stride` floats per frame: (true - pred), each side / dt
PARC_ML_FN v3 vel_err(const float *pt, const float *pp, int stride, int f, float dt) {
    const v3 dt_ = ld3(pt + (size_t)(f + 1) * stride) - ld3(pt + (size_t)f * stride), dp = ld3(pp + (size_t)(f + 1) * stride) - ld3(pp + (size_t)f * stride);
    return mk3(dt_.x / dt - dp.x / dt, dt_.y / dt - dp.y / dt, dt_.z / dt - dp.z / dt);
}
// angular velocity of the pair (q0 = frame f, q1 = frame f + 1): quat_to_exp_map(q1 (x) conj(q0)) / dt
PARC_ML_FN v3 ang_vel(q4 q0, q4 q1, float dt) {
    const v3 e = quat_to_em(qmul(q1, qconj(q0)));
    return mk3(e.x / dt, e.y / dt, e.z / dt);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Forward phases
// ---------------------------------------------------------------------------------------------------------------------------------
// The rotation of joint b >= 1 of J in frame f of one side (0 = predicted, from the dofs in x; 1 = true, from the quaternions)
PARC_ML_FN q4 joint_quat(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const sample &s, int side, int f, int b, int J) {
    if (side != 0) return ld4(s.joint_rot + ((size_t)f * J + (b - 1)) * 4);
    const int jt = m.joint_type[b], d0 = c.off_joint_rot + m.dof_idx[b];
    if (jt == PARC_JOINT_HINGE) return aa_to_quat(joint_axis(m, b), feat(s, c, f, d0));
    if (jt == PARC_JOINT_SPHERICAL) return em_to_quat(feat3(s, c, f, d0));
    return q4{0.f, 0.f, 0.f, 1.f};
}

// The chain of one frame of one side (0 = predicted, from x; 1 = true, from the quaternions) into the scratch
PARC_ML_FN void chain_item(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int side, int f) {
    float *bpos = s.scr + L.o_bpos[side] + (size_t)f * L.nb * 3, *brot = s.scr + L.o_brot[side] + (size_t)f * L.nb * 4;
    float *jq = s.scr + L.o_jq[side] + (size_t)f * L.J * 4;
    if (side == 0) {
        st3(bpos, feat3(s, c, f, c.off_root_pos));
        st4(brot, em_to_quat(feat3(s, c, f, c.off_root_rot)));
    } else {
        st3(bpos, ld3(s.root_pos + (size_t)f * 3));
        st4(brot, ld4(s.root_rot + (size_t)f * 4));
    }
    for (int b = 1; b < L.nb; ++b) {
        const q4 j = joint_quat(m, c, s, side, f, b, L.J);
        st4(jq + (b - 1) * 4, j);
        const int p = m.parent[b];
        const q4 rp = ld4(brot + p * 4);
        st4(brot + b * 4, qmul(rp, qmul(local_r(m, b), j)));
        st3(bpos + b * 3, ld3(bpos + p * 3) + qrot(rp, local_t(m, b)));
    }
}

PARC_ML_FN int point_owner(const layout &L, const int32_t *start, int p) {
    int b = 0;
    while (b + 1 < L.nb && p >= start[b + 1]) ++b;
    return b;
}

// signed distance of sample point p of frame f to the sample's terrain (negative inside the ground) and the column that attains it
PARC_ML_FN float point_sdf(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int p, int &cell) {
    const int b = point_owner(L, s.point_start, p);
    const v3 w = ld3(s.scr + L.o_bpos[0] + ((size_t)f * L.nb + b) * 3) + qrot(ld4(s.scr + L.o_brot[0] + ((size_t)f * L.nb + b) * 4), ld3(s.points + (size_t)p * 3));
    cell = 0;
    float sd = hf_window_min(w.x, w.y, w.z, s.scr + L.o_hf, c.dim_x, c.dim_y, c.ox, c.oy, s.grid_x, s.grid_y, c.half_x, c.half_y, c.base_z, 1, cell);
    if (!(w.x == w.x && w.y == w.y && w.z == w.z)) sd = __builtin_nanf("");      // torch's abs / clamp / min propagate a NaN coordinate
    return -sd;
}
PARC_ML_FN void point_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int p) {
    int cell;
    s.scr[L.o_psdf + f * L.P + p] = point_sdf(c, L, s, f, p, cell);
    reinterpret_cast<int32_t *>(s.scr + L.o_pcell)[f * L.P + p] = cell;
}

// the summands of (frame f, body b) for the twelve loss_fn terms
PARC_ML_FN void terms_item(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int b) {
    const float c2 = c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER ? 0.0009f : 0.f;
    const float *bpT = s.scr + L.o_bpos[1], *bpP = s.scr + L.o_bpos[0], *brT = s.scr + L.o_brot[1], *brP = s.scr + L.o_brot[0];
    const float *jqT = s.scr + L.o_jq[1], *jqP = s.scr + L.o_jq[0];
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
            const v3 jp = feat3(s, c, f, c.off_joint_pos + 3 * (b - 1));
            t[PARC_MDM_LOSS_SIMPLE_BODY_POS] = sq3(ld3(bpT + i * 3) - jp, c2);
            t[PARC_MDM_LOSS_BODY_POS_CONSISTENCY] = sq3(ld3(bpP + i * 3) - jp, c2);
        }
    }
    if (c.off_contacts >= 0) t[PARC_MDM_LOSS_SIMPLE_CONTACT] = sq1(s.contacts[i] - feat(s, c, f, c.off_contacts + b), c2);
    t[PARC_MDM_LOSS_FK_BODY_POS] = sq3(ld3(bpT + i * 3) - ld3(bpP + i * 3), c2);
    t[PARC_MDM_LOSS_FK_BODY_ROT] = sq1(qdiff_angle(ld4(brT + i * 4), ld4(brP + i * 4)), c2);
    if (pair) t[PARC_MDM_LOSS_VEL_FK_BODY_POS] = sq3(vel_err(bpT + b * 3, bpP + b * 3, L.nb * 3, f, c.dt), c2);
    for (int k = 0; k < PARC_ML_LOSS_FN_TERMS; ++k) s.scr[L.o_part + (size_t)k * L.n_items + i] = t[k];
}

// sub-sum `sub` of term t: summands sub, sub + 16, ... in ascending order
PARC_ML_FN void subsum_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t, int sub) {
    float acc = 0.f;
    if (t < PARC_ML_LOSS_FN_TERMS) {
        for (int i = sub; i < L.n_items; i += PARC_ML_NSUB) acc += s.scr[L.o_part + (size_t)t * L.n_items + i];      // 0 where the term has no element
    } else if (t == PARC_MDM_LOSS_HF_COLLISION && term_on(c, t)) {
        for (int i = sub; i < L.S * L.P; i += PARC_ML_NSUB) {
            const float d = s.scr[L.o_psdf + i];
            const float mn = d < 0.f ? d : (d == d ? 0.f : d);          // clamp(max=0) keeps a NaN
            acc += mn * mn;
        }
    }
    s.scr[L.o_r1 + t * PARC_ML_NSUB + sub] = acc;
}

// the raw total of term t (before weight, square root and clamp)
PARC_ML_FN void total_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t) {
    float acc = 0.f;
    if (t == PARC_MDM_LOSS_TARGET) {
        const float *last = s.scr + L.o_bpos[0] + (size_t)(L.S - 1) * L.nb * 3, *ref = s.scr + L.o_bpos[0] + (size_t)c.ref_idx * L.nb * 3;
        acc = -s.target_dir[0] * (last[0] - ref[0]) + -s.target_dir[1] * (last[1] - ref[1]);
    } else {
        for (int k = 0; k < PARC_ML_NSUB; ++k) acc += s.scr[L.o_r1 + t * PARC_ML_NSUB + k];
    }
    s.scr[L.o_sum + t] = acc;
}

PARC_ML_FN float term_value(const parc_mdm_loss_cfg_t &c, int t, float total) {
    if (!term_on(c, t)) return 0.f;
    if (t == PARC_MDM_LOSS_TARGET) return (total >= -c.target_eps ? total : (total == total ? -c.target_eps : total)) * c.w[t];
    if (t == PARC_MDM_LOSS_HF_COLLISION) return c.w[t] * (0.5f * total);
    return c.w[t] * (c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER ? sqrtf(total) - 0.03f : total);
}

// Everything up to the raw totals.  Ends with a barrier.
PARC_ML_FN void forward_phases(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int lane, int nlanes) {
    for (int i = lane; i < L.XY; i += nlanes) s.scr[L.o_hf + i] = s.hf[i] * c.max_h;
    for (int i = lane; i < 2 * L.S; i += nlanes) chain_item(m, c, L, s, i / L.S, i % L.S);
    PARC_ML_SYNC();
    if (term_on(c, PARC_MDM_LOSS_HF_COLLISION))
        for (int i = lane; i < L.S * L.P; i += nlanes) point_item(c, L, s, i / L.P, i % L.P);
    for (int i = lane; i < L.n_items; i += nlanes) terms_item(m, c, L, s, i / L.nb, i % L.nb);
    PARC_ML_SYNC();
    for (int i = lane; i < PARC_MDM_LOSS_TERMS * PARC_ML_NSUB; i += nlanes) subsum_item(c, L, s, i / PARC_ML_NSUB, i % PARC_ML_NSUB);
    PARC_ML_SYNC();
    for (int i = lane; i < PARC_MDM_LOSS_TERMS; i += nlanes) total_item(c, L, s, i);
    PARC_ML_SYNC();
}

// sample b of a batch of B: losses [TERMS, B]
PARC_ML_FN void forward_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const sample &s, int b, int B, float *losses, int lane, int nlanes) {
    const layout L = make_layout(m, c);
    forward_phases(m, c, L, s, lane, nlanes);
    for (int t = lane; t < PARC_MDM_LOSS_TERMS; t += nlanes) losses[(size_t)t * B + b] = term_value(c, t, s.scr[L.o_sum + t]);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward phases
// ---------------------------------------------------------------------------------------------------------------------------------
// k[t]: cotangent of term t's raw total (loss_fn terms: of the sum of squares; HF: of sum(min(sdf, 0)^2) / 2 ... see grad_item)
PARC_ML_FN void scale_item(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int t, float g) {
    float k = 0.f;
    if (term_on(c, t)) {
        const float total = s.scr[L.o_sum + t];
        k = g * c.w[t];
        if (t == PARC_MDM_LOSS_TARGET) k = total >= -c.target_eps ? k : 0.f;
        else if (t < PARC_ML_LOSS_FN_TERMS && c.loss_fn == PARC_MDM_LOSS_PSEUDO_HUBER) k = k / (2.0f * sqrtf(total));
    }
    s.scr[L.o_k + t] = k;
}

// d(column distance)/d(point) of the column the forward pass selected: the piecewise expression of ragged_grad_thread (parc_moopt_core.h)
PARC_ML_FN v3 column_grad(const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, v3 pt, int cell) {
    if (cell < 0 || cell >= L.XY) return mk3(0.f, 0.f, 0.f);
    const int i = cell / c.dim_y, j = cell - i * c.dim_y;
    const float h = s.scr[L.o_hf + cell], top_z = -c.base_z;
    const float cz = (h + top_z) / 2.0f, hz = (top_z - h) / 2.0f;
    const float d[3] = {pt.x - (s.grid_x[i] + c.ox), pt.y - (s.grid_y[j] + c.oy), pt.z - cz};
    const float q[3] = {fabsf(d[0]) - c.half_x, fabsf(d[1]) - c.half_y, fabsf(d[2]) - hz};
    const float a[3] = {fmaxf(q[0], 0.f), fmaxf(q[1], 0.f), fmaxf(q[2], 0.f)};
    const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    float g[3] = {0.f, 0.f, 0.f};
    if (n > 0.f) g[0] = a[0] / n, g[1] = a[1] / n, g[2] = a[2] / n;
    int km = 0;
    if (q[1] > q[km]) km = 1;
    if (q[2] > q[km]) km = 2;
    if (q[km] <= 0.f) g[km] += 1.0f;
    float o[3];
    for (int k = 0; k < 3; ++k) o[k] = g[k] * (d[k] > 0.f ? 1.0f : (d[k] < 0.f ? -1.0f : 0.0f));
    return mk3(o[0], o[1], o[2]);
}

// cotangent that the angular-velocity term (weight k on the sum of squared errors) sends to the quaternion of frame f, from the
// pairs (f - 1, f) and (f, f + 1); qT / qP: the frame-0 quaternion of this root / joint on either side, stride floats per frame
PARC_ML_FN q4 ang_vel_grad(const float *qT, const float *qP, int stride, int S, int f, float dt, float k) {
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
PARC_ML_FN v3 vel_grad(const float *pt, const float *pp, int stride, int S, int f, float dt, float k) {
    v3 g = mk3(0.f, 0.f, 0.f);
    if (f >= 1) g = g + (-2.0f * k / dt) * vel_err(pt, pp, stride, f - 1, dt);
    if (f < S - 1) g = g + (2.0f * k / dt) * vel_err(pt, pp, stride, f, dt);
    return g;
}

// cotangents of the predicted body transform and joint rotation of (frame f, body b); the feature columns that no chain reaches
// (joint positions, contacts) get their g_x here
PARC_ML_FN void grad_item(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, int b, float *g_x) {
    const float *k = s.scr + L.o_k;
    const float *bpT = s.scr + L.o_bpos[1], *bpP = s.scr + L.o_bpos[0], *brT = s.scr + L.o_brot[1], *brP = s.scr + L.o_brot[0];
    const float *jqT = s.scr + L.o_jq[1], *jqP = s.scr + L.o_jq[0];
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
        st4(s.scr + L.o_gjq + j * 4, gj);
        if (c.off_joint_pos >= 0) {
            const int d0 = c.off_joint_pos + 3 * (b - 1);
            const v3 jp = feat3(s, c, f, d0);
            const v3 ec = (2.0f * k[PARC_MDM_LOSS_BODY_POS_CONSISTENCY]) * (pP - jp);
            gp = gp + ec;
            const v3 gjp = (-2.0f * k[PARC_MDM_LOSS_SIMPLE_BODY_POS]) * (pT - jp) - ec;
            g_x[row + d0] = gjp.x * s.std[row + d0];
            g_x[row + d0 + 1] = gjp.y * s.std[row + d0 + 1];
            g_x[row + d0 + 2] = gjp.z * s.std[row + d0 + 2];
        }
    }
    if (c.off_contacts >= 0) {
        const int d0 = c.off_contacts + b;
        g_x[row + d0] = -2.0f * k[PARC_MDM_LOSS_SIMPLE_CONTACT] * (s.contacts[i] - feat(s, c, f, d0)) * s.std[row + d0];
    }
    if (term_on(c, PARC_MDM_LOSS_HF_COLLISION)) {
        const int32_t *cells = reinterpret_cast<const int32_t *>(s.scr + L.o_pcell);
        const int p0 = s.point_start[b] > 0 ? s.point_start[b] : 0, p1 = s.point_start[b + 1] < L.P ? s.point_start[b + 1] : L.P;      // the table is trusted for nothing
        for (int p = p0; p < p1; ++p) {
            const float sdf = s.scr[L.o_psdf + f * L.P + p];
            if (!(sdf < 0.f)) continue;
            const v3 loc = ld3(s.points + (size_t)p * 3);
            const v3 cg = column_grad(c, L, s, pP + qrot(rP, loc), cells[f * L.P + p]);
            const v3 g = (-(k[PARC_MDM_LOSS_HF_COLLISION] * sdf)) * cg;          // sdf = -distance; d(sdf^2 / 2) = sdf
            gp = gp + g;
            gq = qadd(gq, qrot_bwd_q(rP, loc, g));
        }
    }
    st3(s.scr + L.o_gpos + i * 3, gp);
    st4(s.scr + L.o_grot + i * 4, gq);
}

// the chain's adjoint for frame f: body cotangents -> root position, root exponential map, joint dofs -> g_x (times std)
PARC_ML_FN void chain_grad_item(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const layout &L, const sample &s, int f, float *g_x) {
    float *gpos = s.scr + L.o_gpos + (size_t)f * L.nb * 3, *grot = s.scr + L.o_grot + (size_t)f * L.nb * 4;
    const float *gjq = s.scr + L.o_gjq + (size_t)f * L.J * 4;
    const float *brot = s.scr + L.o_brot[0] + (size_t)f * L.nb * 4, *jq = s.scr + L.o_jq[0] + (size_t)f * L.J * 4;
    const size_t row = (size_t)f * c.feat_dim;
    for (int b = L.nb - 1; b >= 1; --b) {          // children before parents: a body's index exceeds its parent's
        const int p = m.parent[b];
        const q4 rp = ld4(brot + p * 4), j = ld4(jq + (b - 1) * 4), lr = local_r(m, b);
        const q4 loc = qmul(lr, j);
        const v3 gpb = ld3(gpos + b * 3);
        const q4 grb = ld4(grot + b * 4);
        st3(gpos + p * 3, ld3(gpos + p * 3) + gpb);
        st4(grot + p * 4, qadd(qadd(ld4(grot + p * 4), qrot_bwd_q(rp, local_t(m, b), gpb)), qmul(grb, qconj(loc))));
        const q4 gj = qadd(qmul(qconj(lr), qmul(qconj(rp), grb)), ld4(gjq + (b - 1) * 4));
        const int jt = m.joint_type[b], d0 = c.off_joint_rot + m.dof_idx[b];
        if (jt == PARC_JOINT_HINGE) {
            g_x[row + d0] = aa_to_quat_bwd(joint_axis(m, b), feat(s, c, f, d0), j, gj).g_angle * s.std[row + d0];
        } else if (jt == PARC_JOINT_SPHERICAL) {
            const v3 ge = em_to_quat_bwd(feat3(s, c, f, d0), j, gj);
            g_x[row + d0] = ge.x * s.std[row + d0];
            g_x[row + d0 + 1] = ge.y * s.std[row + d0 + 1];
            g_x[row + d0 + 2] = ge.z * s.std[row + d0 + 2];
        }
    }
    const v3 g0 = ld3(gpos);
    const v3 ge = em_to_quat_bwd(feat3(s, c, f, c.off_root_rot), ld4(brot), ld4(grot));
    const float gr[6] = {g0.x, g0.y, g0.z, ge.x, ge.y, ge.z};
    for (int k = 0; k < 3; ++k) {
        g_x[row + c.off_root_pos + k] = gr[k] * s.std[row + c.off_root_pos + k];
        g_x[row + c.off_root_rot + k] = gr[3 + k] * s.std[row + c.off_root_rot + k];
    }
}

// sample b of a batch of B: g_losses [TERMS, B] -> g_x (this sample's [S, D] rows)
PARC_ML_FN void backward_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, const sample &s, int b, int B, const float *g_losses, float *g_x,
                                int lane, int nlanes) {
    const layout L = make_layout(m, c);
    forward_phases(m, c, L, s, lane, nlanes);
    for (int t = lane; t < PARC_MDM_LOSS_TERMS; t += nlanes) scale_item(c, L, s, t, g_losses[(size_t)t * B + b]);
    PARC_ML_SYNC();
    for (int i = lane; i < L.n_items; i += nlanes) grad_item(m, c, L, s, i / L.nb, i % L.nb, g_x);
    PARC_ML_SYNC();
    for (int f = lane; f < L.S; f += nlanes) chain_grad_item(m, c, L, s, f, g_x);
}

// sample b's rows
PARC_ML_FN sample make_sample(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int b, const float *x, const float *mean, const float *std,
                              const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts, const float *hfs,
                              const float *target_dir, const float *grid_x, const float *grid_y, const float *points, const int32_t *point_start,
                              float *scr) {
    const size_t S = (size_t)c.seq_len, nb = (size_t)m.num_bodies;
    sample s;
    s.x = x + b * S * c.feat_dim, s.mean = mean, s.std = std;
    s.root_pos = root_pos + b * S * 3, s.root_rot = root_rot + b * S * 4, s.joint_rot = joint_rot + b * S * (nb - 1) * 4;
    s.contacts = contacts ? contacts + b * S * nb : contacts;
    s.hf = hfs + (size_t)b * c.dim_x * c.dim_y, s.target_dir = target_dir + (size_t)b * 2;
    s.grid_x = grid_x, s.grid_y = grid_y, s.points = points, s.point_start = point_start, s.scr = scr;
    return s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Argument rules of the entry points (include/parc_mdm_loss.h), answered before any HIP call
// ---------------------------------------------------------------------------------------------------------------------------------
// the counts, the model and the feature layout (shared with the guidance step, parc_mdm_guide_core.h)
// a model the chain can walk: bodies stored parents-first, every joint's dofs inside [0, dof_size)
static inline int check_model(const parc_char_model_t &m) {
    if (m.num_bodies < 1 || m.num_bodies > PARC_MAX_BODIES || m.dof_size < 0 || m.dof_size > PARC_MAX_DOFS) return PARC_EINVAL;
    for (int b = 1; b < m.num_bodies; ++b) {
        if (m.parent[b] < 0 || m.parent[b] >= b) return PARC_EINVAL;
        const int n = m.joint_type[b] == PARC_JOINT_HINGE ? 1 : m.joint_type[b] == PARC_JOINT_SPHERICAL ? 3 : 0;
        if (n && (m.dof_idx[b] < 0 || m.dof_idx[b] + n > m.dof_size)) return PARC_EINVAL;
    }
    return PARC_OK;
}

// the slices {root_pos, root_rot, joint_rot, joint_pos, contacts} of lengths len[] tile [0, feat_dim); the last two may be absent (< 0)
static inline int check_tiling(int feat_dim, const int off[5], const int len[5]) {
    int want = len[0] + len[1] + len[2] + (off[3] >= 0 ? len[3] : 0) + (off[4] >= 0 ? len[4] : 0);
    if (feat_dim != want) return PARC_EINVAL;
    for (int k = 0; k < 5; ++k) {
        if (k >= 3 && off[k] < 0) continue;
        if (off[k] < 0 || off[k] + len[k] > feat_dim) return PARC_EINVAL;
        for (int i = 0; i < k; ++i)          // disjoint, and their lengths add up to D: a tiling
            if (off[i] >= 0 && len[i] > 0 && len[k] > 0 && off[i] < off[k] + len[k] && off[k] < off[i] + len[i]) return PARC_EINVAL;
    }
    return PARC_OK;
}

static inline int check_layout(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int B) {
    if (B < 0 || check_model(m) != PARC_OK) return PARC_EINVAL;
    if (c.seq_len < 1 || c.dim_x < 1 || c.dim_y < 1 || c.num_points < 0) return PARC_EINVAL;
    // the slices tile [0, D): every column of g_x is written
    const int J = m.num_bodies - 1;
    const int off[5] = {c.off_root_pos, c.off_root_rot, c.off_joint_rot, c.off_joint_pos, c.off_contacts};
    const int len[5] = {3, 3, m.dof_size, 3 * J, m.num_bodies};
    return check_tiling(c.feat_dim, off, len);
}

static inline int check_cfg(const parc_char_model_t &m, const parc_mdm_loss_cfg_t &c, int B) {
    if (check_layout(m, c, B) != PARC_OK) return PARC_EINVAL;
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
