// Body-per-lane helpers: a pose is handled by a 16-lane group, lane b = body b (b = 0 root).  One joint's dofs <-> quaternion and the
// launchers' model check, shared by parc_kin.hip, parc_motion.hip and parc_pose_opt.hip.  Device only (model_ok: host).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/parc_hip.h"
#include "parc_math.h"

static bool model_ok(const parc_char_model_t &m) { return m.num_bodies >= 1 && m.num_bodies <= PARC_MAX_BODIES && m.dof_size <= PARC_MAX_DOFS; }

// anim/kin_char_model.py:57-77: one joint's dofs -> quaternion (lane b >= 1)
template <bool LIB = false>
PARC_DEV q4 joint_dof_to_rot(const parc_char_model_t &m, int b, const float *dof, int stride) {
    int jt = m.joint_type[b];
    if (jt == PARC_JOINT_HINGE) {
        v3 ax = mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]);
        float an = dof[m.dof_idx[b] * stride];
        return LIB ? aa_to_quat(ax, an) : axis_angle_to_quat(ax, an);
    } else if (jt == PARC_JOINT_SPHERICAL) {
        int d = m.dof_idx[b];
        v3 em = mk3(dof[d * stride], dof[(d + 1) * stride], dof[(d + 2) * stride]);
        return LIB ? em_to_quat(em) : exp_map_to_quat(em);
    }
    return mk4(0.f, 0.f, 0.f, 1.f);
}

// anim/kin_char_model.py:79-100: one joint's quaternion -> dofs
// (dof2, when given, receives the same values at stride 2: the position slots of an interleaved dof_state row)
PARC_DEV void joint_rot_to_dof(const parc_char_model_t &m, int b, q4 q, float *dof, float *dof2 = nullptr) {
    int jt = m.joint_type[b];
    if (jt == PARC_JOINT_HINGE) {
        v3 ax;
        float an;
        quat_to_axis_angle(q, ax, an);
        float d = m.joint_axis[b][0] * ax.x + m.joint_axis[b][1] * ax.y + m.joint_axis[b][2] * ax.z;
        if (d < 0.f) an *= -1.f;
        dof[m.dof_idx[b]] = an;
        if (dof2) dof2[2 * m.dof_idx[b]] = an;
    } else if (jt == PARC_JOINT_SPHERICAL) {
        v3 e = quat_to_exp_map(q);
        int d = m.dof_idx[b];
        dof[d] = e.x;
        dof[d + 1] = e.y;
        dof[d + 2] = e.z;
        if (dof2) {
            dof2[2 * d] = e.x;
            dof2[2 * d + 2] = e.y;
            dof2[2 * d + 4] = e.z;
        }
    }
}
