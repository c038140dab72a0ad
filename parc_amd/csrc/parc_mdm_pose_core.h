// What the motion generator's per-sample cores share (parc_mdm_loss_core.h, parc_mdm_guide_core.h, parc_mdm_gen_core.h), for the device
// (hipcc) and the host (g++: the CPU tests).  Built with -ffp-contract=off on both sides: every expression is a sequence of separately
// rounded fp32 operations, as torch evaluates the reference's (diffusion/mdm.py:434-478 extract_motion_features, :978-1028
// compute_point_hf_sdf; util/torch_util.py).
//
// The quaternion and exponential-map functions and their adjoints are those of parc_rot.h (the singular-input rule included: a rotation
// in the reference's "below 1e-5" branch has gradient 0).  Here: the model accessors and checks, and the values the cores hand to the
// primitives - the feature layout (feat_layout), a sample's standardised rows (rows), one side's pose block in the scratch
// (pose_block) with the pose chain, the cotangent block (cot_block) with the chain's adjoint, the local grid (local_grid) with the
// terrain scan and the selected column's gradient, and the two folds.  Whatever only one core uses stays in that core.
//
// The rule: a primitive's parameter list is exactly what it reads.  No core fills another core's configuration, layout or sample to
// call one; a new read inside a primitive is a new parameter, which every caller then has to supply.
//
// A sample is worked on by `nlanes` lanes in phases; a phase is a loop `for (i = lane; i < n; i += nlanes)` over its work items and
// phases are separated by PARC_MP_SYNC() (a barrier on the device, nothing on the host, which calls with lane 0 of 1).  Everything a
// later phase needs sits in the sample's scratch (LDS on the device).  Sums are folded in an order that does not depend on nlanes:
// summand i goes to sub-sum i % 16, the 16 sub-sums are added in ascending order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_rot.h"
#include "parc_sdf_core.h"

#if defined(__HIPCC__)
#define PARC_MP_FN __device__ __forceinline__
#define PARC_MP_HD __host__ __device__ inline
#else
#define PARC_MP_FN static inline
#define PARC_MP_HD static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PARC_MP_SYNC() __syncthreads()
#else
#define PARC_MP_SYNC() ((void)0)
#endif

#define PARC_MP_NOTHING 1      // argument check: valid, and nothing to do
#define PARC_MP_NSUB 16        // sub-sums per term

namespace parc_mp {

// ---- the model ----
PARC_MP_FN v3 local_t(const parc_char_model_t &m, int b) { return mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]); }
PARC_MP_FN q4 local_r(const parc_char_model_t &m, int b) {
    return q4{m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]};
}
PARC_MP_FN v3 joint_axis(const parc_char_model_t &m, int b) { return mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]); }

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

// ---- the feature layout: where a row of D features keeps its slices; JOINT_POS and CONTACTS may be absent (< 0) ----
struct feat_layout { int feat_dim, off_root_pos, off_root_rot, off_joint_pos, off_joint_rot, off_contacts; };

// from parc_mdm_loss_cfg_t, parc_mdm_guide_cfg_t or parc_mdm_gen_cfg_t: they name these fields alike
template <class Cfg>
PARC_MP_HD feat_layout make_feat_layout(const Cfg &c) {
    return feat_layout{c.feat_dim, c.off_root_pos, c.off_root_rot, c.off_joint_pos, c.off_joint_rot, c.off_contacts};
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

// the layout of rot type DEFAULT (root exponential map, joint dofs) tiles [0, D): every column belongs to one slice
static inline int check_feat_layout(const parc_char_model_t &m, const feat_layout &fl) {
    const int off[5] = {fl.off_root_pos, fl.off_root_rot, fl.off_joint_rot, fl.off_joint_pos, fl.off_contacts};
    const int len[5] = {3, 3, m.dof_size, 3 * (m.num_bodies - 1), m.num_bodies};
    return check_tiling(fl.feat_dim, off, len);
}

// the batch, the model, the counts and the feature layout of a configuration with a window and a local grid (loss, guidance step)
template <class Cfg>
static inline int check_window(const parc_char_model_t &m, const Cfg &c, int B) {
    if (B < 0 || check_model(m) != PARC_OK) return PARC_EINVAL;
    if (c.seq_len < 1 || c.dim_x < 1 || c.dim_y < 1 || c.num_points < 0) return PARC_EINVAL;
    return check_feat_layout(m, make_feat_layout(c));
}

// ---- a sample's standardised rows ----
struct rows { const float *x, *mean, *std; };      // [S, D]: D is the feature layout's feat_dim

PARC_MP_FN float feat(const rows &r, int D, int f, int d) {
    const int i = f * D + d;
    return r.x[i] * r.std[i] + r.mean[i];
}
PARC_MP_FN v3 feat3(const rows &r, int D, int f, int d) { return mk3(feat(r, D, f, d), feat(r, D, f, d + 1), feat(r, D, f, d + 2)); }

// The rotation of joint b >= 1 in frame f from its dofs
PARC_MP_FN q4 joint_quat(const parc_char_model_t &m, const rows &r, const feat_layout &fl, int f, int b) {
    const int jt = m.joint_type[b], d0 = fl.off_joint_rot + m.dof_idx[b];
    if (jt == PARC_JOINT_HINGE) return aa_to_quat(joint_axis(m, b), feat(r, fl.feat_dim, f, d0));
    if (jt == PARC_JOINT_SPHERICAL) return em_to_quat(feat3(r, fl.feat_dim, f, d0));
    return q4{0.f, 0.f, 0.f, 1.f};
}

// ---- one side's pose in the scratch, at float offsets: body positions [S, nb, 3], body rotations [S, nb, 4], joint rotations [S, J, 4] ----
struct pose_block { int S, nb, J, o_bpos, o_brot, o_jq; };

// the next S (11 nb - 4) floats at o
PARC_MP_HD pose_block make_pose_block(int S, int nb, int64_t &o) {
    const int n = S * nb, o_bpos = (int)o, o_brot = (int)(o += (int64_t)n * 3), o_jq = (int)(o += (int64_t)n * 4);
    o += (int64_t)S * (nb - 1) * 4;
    return pose_block{S, nb, nb - 1, o_bpos, o_brot, o_jq};
}

// frame f's body positions [nb, 3] and rotations [nb, 4]; element 0 is the root's
PARC_MP_FN float *body_pos(const pose_block &pb, float *scr, int f) { return scr + pb.o_bpos + (size_t)f * pb.nb * 3; }
PARC_MP_FN float *body_rot(const pose_block &pb, float *scr, int f) { return scr + pb.o_brot + (size_t)f * pb.nb * 4; }

// The walk of frame f behind its root, whose transform is in the block: joint(b) is the rotation of joint b >= 1
template <class JointRot>
PARC_MP_FN void chain_walk(const parc_char_model_t &m, const pose_block &pb, float *scr, int f, JointRot joint) {
    float *bpos = body_pos(pb, scr, f), *brot = body_rot(pb, scr, f), *jq = scr + pb.o_jq + (size_t)f * pb.J * 4;
    for (int b = 1; b < pb.nb; ++b) {
        const q4 j = joint(b);
        st4(jq + (b - 1) * 4, j);
        const int p = m.parent[b];
        const q4 rp = ld4(brot + p * 4);
        st4(brot + b * 4, qmul(rp, qmul(local_r(m, b), j)));
        st3(bpos + b * 3, ld3(bpos + p * 3) + qrot(rp, local_t(m, b)));
    }
}

// The root of frame f and the chain behind it from the features: root position, root exponential map, joint dofs
PARC_MP_FN void root_from_feat(const pose_block &pb, float *scr, const rows &r, const feat_layout &fl, int f) {
    st3(body_pos(pb, scr, f), feat3(r, fl.feat_dim, f, fl.off_root_pos));          // stored before the rotation is worked out, not behind it
    st4(body_rot(pb, scr, f), em_to_quat(feat3(r, fl.feat_dim, f, fl.off_root_rot)));
}
PARC_MP_FN void chain_from_feat(const parc_char_model_t &m, const pose_block &pb, float *scr, const rows &r, const feat_layout &fl, int f) {
    root_from_feat(pb, scr, r, fl, f);
    chain_walk(m, pb, scr, f, [&](int b) { return joint_quat(m, r, fl, f, b); });
}

// The same from true arrays: root_pos [S, 3], root_rot [S, 4], joint_rot [S, J, 4]
PARC_MP_FN void root_from_true(const pose_block &pb, float *scr, const float *root_pos, const float *root_rot, int f) {
    st3(body_pos(pb, scr, f), ld3(root_pos + (size_t)f * 3));
    st4(body_rot(pb, scr, f), ld4(root_rot + (size_t)f * 4));
}
PARC_MP_FN q4 joint_true(const float *joint_rot, int J, int f, int b) { return ld4(joint_rot + ((size_t)f * J + (b - 1)) * 4); }
PARC_MP_FN void chain_from_true(const parc_char_model_t &m, const pose_block &pb, float *scr, const float *root_pos, const float *root_rot,
                                const float *joint_rot, int f) {
    root_from_true(pb, scr, root_pos, root_rot, f);
    chain_walk(m, pb, scr, f, [&](int b) { return joint_true(joint_rot, pb.J, f, b); });
}

// ---- the cotangents of a pose block, shaped like it, and the chain's adjoint ----
struct cot_block { int o_gpos, o_grot, o_gjq; };

PARC_MP_HD cot_block make_cot_block(int S, int nb, int64_t &o) {
    const pose_block like = make_pose_block(S, nb, o);
    return cot_block{like.o_bpos, like.o_brot, like.o_jq};
}

// the chain's adjoint for frame f: body cotangents -> root position, root exponential map, joint dofs -> g_x (times std)
PARC_MP_FN void chain_grad_item(const parc_char_model_t &m, const pose_block &pb, const cot_block &cb, float *scr, const rows &r,
                                const feat_layout &fl, int f, float *g_x) {
    float *gpos = scr + cb.o_gpos + (size_t)f * pb.nb * 3, *grot = scr + cb.o_grot + (size_t)f * pb.nb * 4;
    const float *gjq = scr + cb.o_gjq + (size_t)f * pb.J * 4;
    const float *brot = scr + pb.o_brot + (size_t)f * pb.nb * 4, *jq = scr + pb.o_jq + (size_t)f * pb.J * 4;
    const size_t row = (size_t)f * fl.feat_dim;
    for (int b = pb.nb - 1; b >= 1; --b) {          // children before parents: a body's index exceeds its parent's
        const int p = m.parent[b];
        const q4 rp = ld4(brot + p * 4), j = ld4(jq + (b - 1) * 4), lr = local_r(m, b);
        const q4 loc = qmul(lr, j);
        const v3 gpb = ld3(gpos + b * 3);
        const q4 grb = ld4(grot + b * 4);
        st3(gpos + p * 3, ld3(gpos + p * 3) + gpb);
        st4(grot + p * 4, qadd(qadd(ld4(grot + p * 4), qrot_bwd_q(rp, local_t(m, b), gpb)), qmul(grb, qconj(loc))));
        const q4 gj = qadd(qmul(qconj(lr), qmul(qconj(rp), grb)), ld4(gjq + (b - 1) * 4));
        const int jt = m.joint_type[b], d0 = fl.off_joint_rot + m.dof_idx[b];
        if (jt == PARC_JOINT_HINGE) {
            g_x[row + d0] = aa_to_quat_bwd(joint_axis(m, b), feat(r, fl.feat_dim, f, d0), j, gj).g_angle * r.std[row + d0];
        } else if (jt == PARC_JOINT_SPHERICAL) {
            const v3 ge = em_to_quat_bwd(feat3(r, fl.feat_dim, f, d0), j, gj);
            g_x[row + d0] = ge.x * r.std[row + d0];
            g_x[row + d0 + 1] = ge.y * r.std[row + d0 + 1];
            g_x[row + d0 + 2] = ge.z * r.std[row + d0 + 2];
        }
    }
    const v3 g0 = ld3(gpos);
    const v3 ge = em_to_quat_bwd(feat3(r, fl.feat_dim, f, fl.off_root_rot), ld4(brot), ld4(grot));
    const float gr[6] = {g0.x, g0.y, g0.z, ge.x, ge.y, ge.z};
    for (int k = 0; k < 3; ++k) {
        g_x[row + fl.off_root_pos + k] = gr[k] * r.std[row + fl.off_root_pos + k];
        g_x[row + fl.off_root_rot + k] = gr[3 + k] * r.std[row + fl.off_root_rot + k];
    }
}

// ---- the local grid of the loss and the guidance step ----
// columns of half size (half_x, half_y) about (grid_x[i] + ox, grid_y[j] + oy), from base_z up to the heightfield (times max_h, in the scratch)
struct local_grid { int dim_x, dim_y; float ox, oy, half_x, half_y, base_z; const float *hf, *grid_x, *grid_y; };

// from parc_mdm_loss_cfg_t or parc_mdm_guide_cfg_t
template <class Cfg>
PARC_MP_FN local_grid make_local_grid(const Cfg &c, const float *hf, const float *grid_x, const float *grid_y) {
    return local_grid{c.dim_x, c.dim_y, c.ox, c.oy, c.half_x, c.half_y, c.base_z, hf, grid_x, grid_y};
}

// the body that owns sample point p: body b owns [start[b], start[b + 1])
PARC_MP_FN int point_owner(int nb, const int32_t *start, int p) {
    int b = 0;
    while (b + 1 < nb && p >= start[b + 1]) ++b;
    return b;
}

// signed distance of sample point p of frame f to the sample's terrain (negative inside the ground) and the column that attains it
PARC_MP_FN float point_sdf(const local_grid &g, const pose_block &pb, const float *scr, const float *points, const int32_t *point_start, int f,
                           int p, int &cell) {
    const int b = point_owner(pb.nb, point_start, p);
    const v3 w = ld3(scr + pb.o_bpos + ((size_t)f * pb.nb + b) * 3) + qrot(ld4(scr + pb.o_brot + ((size_t)f * pb.nb + b) * 4), ld3(points + (size_t)p * 3));
    cell = 0;
    float sd = hf_window_min(w.x, w.y, w.z, g.hf, g.dim_x, g.dim_y, g.ox, g.oy, g.grid_x, g.grid_y, g.half_x, g.half_y, g.base_z, 1, cell);
    if (!(w.x == w.x && w.y == w.y && w.z == w.z)) sd = __builtin_nanf("");      // torch's abs / clamp / min propagate a NaN coordinate
    return -sd;
}

// d(column distance)/d(point) of the column the forward pass selected: the piecewise expression of ragged_grad_thread (parc_moopt_core.h)
PARC_MP_FN v3 column_grad(const local_grid &g, v3 pt, int cell) {
    if (cell < 0 || cell >= g.dim_x * g.dim_y) return mk3(0.f, 0.f, 0.f);
    const int i = cell / g.dim_y, j = cell - i * g.dim_y;
    const float h = g.hf[cell], top_z = -g.base_z;
    const float cz = (h + top_z) / 2.0f, hz = (top_z - h) / 2.0f;
    const float d[3] = {pt.x - (g.grid_x[i] + g.ox), pt.y - (g.grid_y[j] + g.oy), pt.z - cz};
    const float q[3] = {fabsf(d[0]) - g.half_x, fabsf(d[1]) - g.half_y, fabsf(d[2]) - hz};
    const float a[3] = {fmaxf(q[0], 0.f), fmaxf(q[1], 0.f), fmaxf(q[2], 0.f)};
    const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    float o[3] = {0.f, 0.f, 0.f};
    if (n > 0.f) o[0] = a[0] / n, o[1] = a[1] / n, o[2] = a[2] / n;
    int km = 0;
    if (q[1] > q[km]) km = 1;
    if (q[2] > q[km]) km = 2;
    if (q[km] <= 0.f) o[km] += 1.0f;
    for (int k = 0; k < 3; ++k) o[k] = o[k] * (d[k] > 0.f ? 1.0f : (d[k] < 0.f ? -1.0f : 0.0f));
    return mk3(o[0], o[1], o[2]);
}

// ---- folds ----
// sub-sum `sub` of n summands: elements sub, sub + 16, ... in ascending order
PARC_MP_FN float row_subsum(const float *v, int n, int sub) {
    float acc = 0.f;
    for (int i = sub; i < n; i += PARC_MP_NSUB) acc += v[i];
    return acc;
}

// sub-sum `sub` of the terrain term over n distances: the summand of a distance is min(sdf, 0)^2
PARC_MP_FN float penetration_subsum(const float *sdf, int n, int sub) {
    float acc = 0.f;
    for (int i = sub; i < n; i += PARC_MP_NSUB) {
        const float d = sdf[i];
        const float mn = d < 0.f ? d : (d == d ? 0.f : d);          // clamp(max=0) keeps a NaN
        acc += mn * mn;
    }
    return acc;
}

// the 16 sub-sums of a term, added in ascending order
PARC_MP_FN float fold_subsums(const float *sub) {
    float acc = 0.f;
    for (int k = 0; k < PARC_MP_NSUB; ++k) acc += sub[k];
    return acc;
}

}  // namespace parc_mp
