// The motion generator's call for ONE sample: the conditions gen_mdm_motion builds in front of the sampling loop (encode) and the motion
// frames it builds behind it (decode) (include/parc_mdm_gen.h), shared by the device (hipcc: parc_mdm_gen.hip) and the host (g++: the
// CPU tests, tests/tools/mdm_gen_host.cpp).  Built with -ffp-contract=off on both sides: every expression is a sequence of separately
// rounded fp32 operations, as torch evaluates the reference's (diffusion/gen_util.py:81-134, :211-218; diffusion/mdm.py:1341-1364,
// :1392-1396; util/terrain_util.py:2049-2082 sample_hf_z_on_terrain; util/torch_util.py:619-631 rotate_2d_vec).
//
// From parc_mdm_pose_core.h: the quaternion and exponential-map functions, joint_quat (dofs -> a joint's rotation), chain_from_true (the
// pose chain of a frame into the sample's scratch) and the phase scheme `for (i = lane; i < n; i += nlanes)`.  From parc_hf_cell.h:
// hf_lookup, which rounds half to even and clamps both indices before the load.  Here: the heading frame, the rotated grid, the
// target direction, quaternion -> dofs of one joint (library precision; the tracker's joint_rot_to_dof of parc_pose_lane.h is built
// on the device's short polynomials and cannot be compiled for the host), and the feature rows.
#pragma once
#include "../../include/parc_mdm_gen.h"
#include "parc_hf_cell.h"
#include "parc_mdm_pose_core.h"

#define PARC_MGN_NOTHING PARC_MP_NOTHING      // the one code under this core's name: what its argument checks return and its launchers compare with

namespace parc_mgn {

using namespace parc_mp;

// Scratch of one encode sample: the pose block of the T previous frames, `floats` long
PARC_MP_HD pose_block encode_pose(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, int64_t &floats) {
    floats = 0;
    return make_pose_block(c.num_frames, m.num_bodies, floats);
}

static inline int64_t lds_bytes(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c) {
    int64_t floats;
    encode_pose(m, c, floats);
    return 4 * floats;
}

// util/torch_util.py:619-631
PARC_MP_FN void rotate_2d(float x, float y, float cs, float sn, float &ox, float &oy) {
    ox = x * cs - y * sn;
    oy = x * sn + y * cs;
}

// util/torch_util.py:68-88: axis and angle of the w >= 0 representative; the z axis and 0 at or below 1e-5 (a NaN length included)
PARC_MP_FN void quat_to_aa(q4 d, v3 &axis, float &angle) {
    const float sg = d.w < 0.f ? -1.f : 1.f;
    const v3 v = mk3(sg * d.x, sg * d.y, sg * d.z);
    const float s = sqrtf(dot3(v, v));
    if (!(s > 1e-5f)) {
        axis = mk3(0.f, 0.f, 1.f), angle = 0.f;
        return;
    }
    angle = 2.0f * atan2f(s, sg * d.w);
    axis = mk3(v.x / s, v.y / s, v.z / s);
}

// anim/kin_char_model.py:79-100: the rotation of joint b >= 1 -> its dofs, into dof[dof_idx[b] ...]
PARC_MP_FN void joint_to_dof(const parc_char_model_t &m, int b, q4 q, float *dof) {
    const int jt = m.joint_type[b], d = m.dof_idx[b];
    if (jt == PARC_JOINT_HINGE) {
        v3 ax;
        float an;
        quat_to_aa(q, ax, an);
        if (dot3(joint_axis(m, b), ax) < 0.f) an *= -1.f;
        dof[d] = an;
    } else if (jt == PARC_JOINT_SPHERICAL) {
        const v3 e = quat_to_em(q);
        dof[d] = e.x, dof[d + 1] = e.y, dof[d + 2] = e.z;
    }
}

// The heading frame of a sample: frame[PARC_MDM_GEN_FRAME] as stored
struct gframe {
    float cx, cy;
    q4 h;
    float z_ref, heading;
};

PARC_MP_FN gframe load_frame(const float *f) { return gframe{f[0], f[1], ld4(f + 2), f[6], f[7]}; }
PARC_MP_FN void store_frame(float *f, const gframe &g) {
    f[0] = g.cx, f[1] = g.cy;
    st4(f + 2, g.h);
    f[6] = g.z_ref, f[7] = g.heading;
}

// gen_util.py:81-86, :104-116 on the reference frame (root position p, root rotation q)
PARC_MP_FN gframe make_frame(const parc_mdm_gen_cfg_t &c, const parc_terrain_t &ter, v3 p, q4 q) {
    gframe g;
    const v3 d = qrot(q, mk3(1.f, 0.f, 0.f));
    g.heading = atan2f(d.y, d.x);
    g.h = aa_to_quat(mk3(0.f, 0.f, 1.f), g.heading);
    g.cx = p.x, g.cy = p.y;
    g.z_ref = c.z_style == PARC_MDM_GEN_Z_ROOT_FLOOR ? hf_lookup(ter, p.x, p.y) : p.z;
    return g;
}

// torch.clamp keeps a NaN
PARC_MP_FN float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// What one encode call works on: sample b's rows of every array
struct enc_sample {
    const float *root_pos, *root_rot, *joint_rot, *contacts, *target_world;          // [T, 3], [T, 4], [T, J, 4], [T, nb], [2]
    const float *grid_x, *grid_y, *mean, *std;
    float *frame, *out_root_pos, *out_root_rot, *out_body_pos, *hf_z, *target, *target_dir, *prev_state, *obs;
    float *scr;
};

// the standardised feature row of previous frame t (mdm.py:382-432 with rot_type DEFAULT, :366-369)
PARC_MP_FN void feature_row(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, const pose_block &L, const enc_sample &e, int t, v3 rp, q4 rr) {
    float *row = e.prev_state + (size_t)t * c.feat_dim;
    const float *mean = e.mean + (size_t)t * c.feat_dim, *std = e.std + (size_t)t * c.feat_dim;
    float dof[PARC_MAX_DOFS];
    for (int d = 0; d < m.dof_size; ++d) dof[d] = 0.f;
    for (int b = 1; b < L.nb; ++b) joint_to_dof(m, b, ld4(e.scr + L.o_jq + ((size_t)t * L.J + (b - 1)) * 4), dof);
    const v3 em = quat_to_em(rr);
    const float r6[6] = {rp.x, rp.y, rp.z, em.x, em.y, em.z};
    for (int k = 0; k < 3; ++k) {
        const int d0 = c.off_root_pos + k, d1 = c.off_root_rot + k;
        row[d0] = (r6[k] - mean[d0]) / std[d0];
        row[d1] = (r6[3 + k] - mean[d1]) / std[d1];
    }
    for (int k = 0; k < m.dof_size; ++k) {
        const int d = c.off_joint_rot + k;
        row[d] = (dof[k] - mean[d]) / std[d];
    }
    if (c.off_joint_pos >= 0)
        for (int k = 0; k < 3 * L.J; ++k) {
            const int d = c.off_joint_pos + k;
            row[d] = (e.scr[L.o_bpos + ((size_t)t * L.nb + 1) * 3 + k] - mean[d]) / std[d];
        }
    if (c.off_contacts >= 0)
        for (int k = 0; k < L.nb; ++k) {
            const int d = c.off_contacts + k;
            row[d] = (e.contacts[(size_t)t * L.nb + k] - mean[d]) / std[d];
        }
}

// one previous frame: canonical root, the pose chain, the body positions, and its feature row when t < P
PARC_MP_FN void encode_frame(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, const pose_block &L, const enc_sample &e, const gframe &g, int t) {
    const q4 hinv = aa_to_quat(mk3(0.f, 0.f, 1.f), -g.heading);
    v3 p = ld3(e.root_pos + (size_t)t * 3);
    p.x -= g.cx, p.y -= g.cy;
    v3 rp = qrot(hinv, p);
    rp.z -= g.z_ref;
    const q4 rr = qmul(hinv, ld4(e.root_rot + (size_t)t * 4));
    st3(e.out_root_pos + (size_t)t * 3, rp);
    st4(e.out_root_rot + (size_t)t * 4, rr);
    // the chain reads the root from the arrays just written and the joints from the input
    chain_from_true(m, L, e.scr, e.out_root_pos, e.out_root_rot, e.joint_rot, t);
    for (int k = 0; k < 3 * L.J; ++k) e.out_body_pos[(size_t)t * L.J * 3 + k] = e.scr[L.o_bpos + ((size_t)t * L.nb + 1) * 3 + k];
    if (e.prev_state && t < c.num_prev_states) feature_row(m, c, L, e, t, rp, rr);
}

// sample b of an encode call, worked on by `nlanes` lanes.  No lane reads what another wrote: no barrier.
PARC_MP_FN void encode_sample(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, const parc_terrain_t &ter, const enc_sample &e, int lane,
                              int nlanes) {
    int64_t floats;
    const pose_block L = encode_pose(m, c, floats);
    const int XY = c.dim_x * c.dim_y, ci = c.num_prev_states - 1;
    // every lane evaluates the frame for itself: the same operations on the same values
    const gframe g = make_frame(c, ter, ld3(e.root_pos + (size_t)ci * 3), ld4(e.root_rot + (size_t)ci * 4));
    if (lane == 0) {
        store_frame(e.frame, g);
        // gen_util.py:124-134: the target in the canonical frame, and F.normalize (eps 1e-12) of it
        float tx, ty;
        rotate_2d(e.target_world[0] - g.cx, e.target_world[1] - g.cy, cosf(-g.heading), sinf(-g.heading), tx, ty);
        e.target[0] = tx, e.target[1] = ty;
        const float n = fmaxf(sqrtf(tx * tx + ty * ty), 1e-12f);
        e.target_dir[0] = tx / n, e.target_dir[1] = ty / n;
    }
    const float cs = cosf(g.heading), sn = sinf(g.heading);
    for (int i = lane; i < XY; i += nlanes) {
        float rx, ry;
        rotate_2d(e.grid_x[i / c.dim_y], e.grid_y[i % c.dim_y], cs, sn, rx, ry);
        const float z = hf_lookup(ter, rx + g.cx, ry + g.cy) - g.z_ref;
        e.hf_z[i] = z;
        if (e.obs) e.obs[i] = clampf(z, c.min_h, c.max_h) / c.max_h;
    }
    for (int t = lane; t < c.num_frames; t += nlanes) encode_frame(m, c, L, e, g, t);
}

PARC_MP_FN enc_sample make_enc_sample(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, int b, const float *root_pos, const float *root_rot,
                                      const float *joint_rot, const float *contacts, const float *target_world, const float *grid_x,
                                      const float *grid_y, const float *mean, const float *std, float *frame, float *out_root_pos,
                                      float *out_root_rot, float *out_body_pos, float *hf_z, float *target, float *target_dir, float *prev_state,
                                      float *obs, float *scr) {
    const size_t T = c.num_frames, J = m.num_bodies - 1, nb = m.num_bodies, XY = (size_t)c.dim_x * c.dim_y;
    enc_sample e;
    e.root_pos = root_pos + b * T * 3, e.root_rot = root_rot + b * T * 4;
    e.joint_rot = joint_rot ? joint_rot + b * T * J * 4 : joint_rot;
    e.contacts = contacts ? contacts + b * T * nb : contacts;
    e.target_world = target_world + (size_t)b * 2;
    e.grid_x = grid_x, e.grid_y = grid_y, e.mean = mean, e.std = std;
    e.frame = frame + (size_t)b * PARC_MDM_GEN_FRAME;
    e.out_root_pos = out_root_pos + b * T * 3, e.out_root_rot = out_root_rot + b * T * 4;
    e.out_body_pos = out_body_pos ? out_body_pos + b * T * J * 3 : out_body_pos;
    e.hf_z = hf_z + b * XY, e.target = target + (size_t)b * 2, e.target_dir = target_dir + (size_t)b * 2;
    e.prev_state = prev_state ? prev_state + (size_t)b * c.num_prev_states * c.feat_dim : prev_state;
    e.obs = obs ? obs + b * XY : obs;
    e.scr = scr;
    return e;
}

// ---- Decode: frame s of sample b (mdm.py:1392-1396, :434-478; gen_util.py:211-218) ----
PARC_MP_FN void decode_item(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, int b, int s, const float *x, const float *prev_state,
                            const uint8_t *no_noise, const float *mean, const float *std, const float *frame, float *root_pos, float *root_rot,
                            float *joint_rot, float *contacts, float *frames) {
    const size_t S = c.seq_len, D = c.feat_dim, J = m.num_bodies - 1, nb = m.num_bodies, i = (size_t)b * S + s;
    const bool keep = prev_state && s < c.num_prev_states && no_noise[b];
    const rows smp = {keep ? prev_state + (size_t)b * c.num_prev_states * D : x + (size_t)b * S * D, mean, std};
    const feat_layout fl = make_feat_layout(c);
    const gframe g = load_frame(frame + (size_t)b * PARC_MDM_GEN_FRAME);
    v3 p = qrot(g.h, feat3(smp, c.feat_dim, s, c.off_root_pos));
    p.x += g.cx, p.y += g.cy, p.z += g.z_ref;
    const q4 r = qmul(g.h, em_to_quat(feat3(smp, c.feat_dim, s, c.off_root_rot)));
    st3(root_pos + i * 3, p);
    st4(root_rot + i * 4, r);
    float dof[PARC_MAX_DOFS];
    for (int d = 0; d < m.dof_size; ++d) dof[d] = 0.f;
    for (int jb = 1; jb < m.num_bodies; ++jb) {
        const q4 j = joint_quat(m, smp, fl, s, jb);
        st4(joint_rot + (i * J + (jb - 1)) * 4, j);
        if (frames) joint_to_dof(m, jb, j, dof);
    }
    if (c.off_contacts >= 0)
        for (int k = 0; k < m.num_bodies; ++k) contacts[i * nb + k] = feat(smp, c.feat_dim, s, c.off_contacts + k);
    if (frames) {
        float *row = frames + i * (6 + (size_t)m.dof_size);
        st3(row, p);
        st3(row + 3, quat_to_em(r));
        for (int d = 0; d < m.dof_size; ++d) row[6 + d] = dof[d];
    }
}

// ---- Argument rules of the entry points (include/parc_mdm_gen.h), answered before any HIP call ----
static inline int check_cfg(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, int B, bool decode) {
    if (B < 0 || check_model(m) != PARC_OK) return PARC_EINVAL;
    if (c.num_prev_states < 1 || c.dim_x < 1 || c.dim_y < 1 || c.feat_dim < 1) return PARC_EINVAL;
    if (decode ? c.seq_len < c.num_prev_states : c.num_prev_states > c.num_frames) return PARC_EINVAL;
    if (c.z_style != PARC_MDM_GEN_Z_ROOT && c.z_style != PARC_MDM_GEN_Z_ROOT_FLOOR) return PARC_EINVAL;
    if (c.rot_type != PARC_MDM_GEN_ROT_DEFAULT && c.rot_type != PARC_MDM_GEN_ROT_EXP_MAP && c.rot_type != PARC_MDM_GEN_ROT_QUAT) return PARC_EINVAL;
    if (c.rot_type != PARC_MDM_GEN_ROT_DEFAULT) {          // a layout of a rot type the kernels do not take is still checked: EINVAL first
        const int J = m.num_bodies - 1, root = c.rot_type == PARC_MDM_GEN_ROT_QUAT ? 4 : 3;
        const int off[5] = {c.off_root_pos, c.off_root_rot, c.off_joint_rot, c.off_joint_pos, c.off_contacts};
        const int len[5] = {3, root, root * J, 3 * J, m.num_bodies};
        return check_tiling(c.feat_dim, off, len) != PARC_OK ? PARC_EINVAL : PARC_EUNSUPPORTED;
    }
    if (check_feat_layout(m, make_feat_layout(c)) != PARC_OK) return PARC_EINVAL;
    // sizes in 64 bits before the layout multiplies them as int
    if (!decode && (int64_t)c.num_frames * (11 * m.num_bodies - 4) * 4 > PARC_MDM_GEN_MAX_LDS) return PARC_EUNSUPPORTED;
    if ((int64_t)c.dim_x * c.dim_y > 0x7fffff || (int64_t)(decode ? c.seq_len : c.num_frames) * c.feat_dim > 0x7fffff) return PARC_EUNSUPPORTED;
    return PARC_OK;
}

static inline bool terrain_ok(const parc_terrain_t &t) { return t.hf && t.dim_x >= 1 && t.dim_y >= 1; }

static inline int check_encode(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, const parc_terrain_t &ter, int B, const void *root_pos,
                               const void *root_rot, const void *joint_rot, const void *contacts, const void *target_world, const void *grid_x,
                               const void *grid_y, const void *mean, const void *std, const void *frame, const void *out_root_pos,
                               const void *out_root_rot, const void *out_body_pos, const void *hf_z, const void *target, const void *target_dir,
                               const void *prev_state) {
    const int rc = check_cfg(m, c, B, false);
    if (rc != PARC_OK) return rc;
    if (B == 0) return PARC_MGN_NOTHING;
    if (!terrain_ok(ter) || !root_pos || !root_rot || !target_world || !grid_x || !grid_y || !frame || !out_root_pos || !out_root_rot || !hf_z ||
        !target || !target_dir)
        return PARC_EINVAL;
    if (m.num_bodies > 1 && (!joint_rot || !out_body_pos)) return PARC_EINVAL;
    if (prev_state && (!mean || !std || (c.off_contacts >= 0 && !contacts))) return PARC_EINVAL;
    return PARC_OK;
}

static inline int check_decode(const parc_char_model_t &m, const parc_mdm_gen_cfg_t &c, int B, const void *x, const void *prev_state,
                               const void *no_noise, const void *mean, const void *std, const void *frame, const void *root_pos,
                               const void *root_rot, const void *joint_rot, const void *contacts) {
    const int rc = check_cfg(m, c, B, true);
    if (rc != PARC_OK) return rc;
    if (B == 0) return PARC_MGN_NOTHING;
    if (!x || !mean || !std || !frame || !root_pos || !root_rot) return PARC_EINVAL;
    if (m.num_bodies > 1 && !joint_rot) return PARC_EINVAL;
    if ((prev_state == nullptr) != (no_noise == nullptr)) return PARC_EINVAL;
    if ((c.off_contacts >= 0) != (contacts != nullptr)) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_mgn
