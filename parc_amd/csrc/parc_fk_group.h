// Body-per-lane forward kinematics: a pose is handled by a 16-lane group, lane b = body b (b = 0 root).  Shared by the tracker step
// (parc_kin.hip), the stand-alone kinematics (parc_motion.hip) and the motion scorer (parc_score.hip).  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/parc_hip.h"
#include "parc_math.h"

#define GRP 16

PARC_DEV float shfl16(float v, int src) { return __shfl(v, src, GRP); }
PARC_DEV q4 shfl16(q4 q, int src) { return q4{shfl16(q.x, src), shfl16(q.y, src), shfl16(q.z, src), shfl16(q.w, src)}; }
PARC_DEV v3 shfl16(v3 v, int src) { return v3{shfl16(v.x, src), shfl16(v.y, src), shfl16(v.z, src)}; }

// all-reduce over the 16 lanes of a group = one DPP row: rotate-and-add with row_ror 8, 4, 2, 1 (dpp_ctrl 0x120 + n).  DPP
// operands ride on the VALU instruction itself - no ds_bpermute round trip per step as with __shfl_xor.
template <int CTRL>
PARC_DEV float row_ror_f(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
PARC_DEV float sum16(float v) {
    v += row_ror_f<0x128>(v);
    v += row_ror_f<0x124>(v);
    v += row_ror_f<0x122>(v);
    v += row_ror_f<0x121>(v);
    return v;
}
PARC_DEV int any16(int v) {
    v |= __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x124, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x122, 0xf, 0xf, false);
    v |= __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false);
    return v;
}

// anim/kin_char_model.py:509-541, level-synchronous over the tree: lane b ends with body b's world
// position/rotation.  jq = joint rotation of lane's body (ignored for the root lane).
// LEAF_ROT = false: the rotations of the deepest level are not produced (callers that only use positions)
// what the walk needs to know about a lane's body (fk_consts reads it from the model struct; the post-step kernel keeps one copy per
// workgroup in LDS instead of having every wave load the four tables)
struct fk_consts {
    int par, dep;         // parent lane (0 for the root and for lanes without a body), depth (-1 without a body)
    q4 lrot;              // local_rotation
    v3 lt;                // local_translation
};
PARC_DEV fk_consts fk_consts_of(const parc_char_model_t &m, int b) {
    fk_consts k;
    const bool valid = b < m.num_bodies;
    k.par = (valid && b > 0) ? m.parent[b] : 0;
    k.dep = valid ? m.depth[b] : -1;
    k.lrot = mk4(0.f, 0.f, 0.f, 1.f);
    k.lt = mk3(0.f, 0.f, 0.f);
    if (valid && b > 0) {
        k.lrot = ld4(m.local_rotation[b]);
        k.lt = ld3(m.local_translation[b]);
    }
    return k;
}
template <bool LEAF_ROT = true>
PARC_DEV void group_fk(const fk_consts &k, int max_depth, v3 root_pos, q4 root_rot, q4 jq, v3 &pos, q4 &rot) {
    q4 lq = mk4(0.f, 0.f, 0.f, 1.f);
    if (k.dep > 0) lq = quat_mul(k.lrot, jq);
    pos = root_pos;
    rot = root_rot;
    for (int lev = 1; lev <= max_depth; ++lev) {
        v3 pp = shfl16(pos, k.par);
        q4 pr = shfl16(rot, k.par);
        if (k.dep == lev) {
            pos = pp + quat_rotate(pr, k.lt);
            if (LEAF_ROT || lev < max_depth) rot = quat_mul(pr, lq);
        }
    }
}
template <bool LEAF_ROT = true>
PARC_DEV void group_fk(const parc_char_model_t &m, int b, v3 root_pos, q4 root_rot, q4 jq, v3 &pos, q4 &rot) {
    group_fk<LEAF_ROT>(fk_consts_of(m, b), m.max_depth, root_pos, root_rot, jq, pos, rot);
}
