// Primitives of stage 2's motion optimiser on one motion, each with its adjoint: pose chain, rotation angle, frame-to-frame terms,
// body sample points (their packed-motions twins are in parc_moopt.hip).  C-ABI in include/parc_hip.h.  Reference citations are
// relative to the reference root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_math.h"
#include "parc_pose_lane.h"    // model_ok, joint_dof_to_rot
#include "parc_moopt_core.h"   // tt_args, tt_forward_body, tt_backward_body

// =============================================================================================
// Pose chain with its adjoint, one thread per frame: (root position, root exponential map, joint dofs) -> root quaternion, joint
// rotations, body positions / rotations, and the vector-Jacobian product back.  This is what stage 2's motion optimiser
// differentiates thousands of times per clip (tools/motion_opt/motion_optimization.py:203-213: exp_map_to_quat, KinCharModel.dof_to_rot,
// forward_kinematics and their autograd); as torch ops it is ~190 autograd nodes per evaluation, here two launches.
// Forward uses the torch-exact maps (the values torch computes); the adjoint is exact for those formulas.  Maps and adjoints are those of
// parc_rot.h, so the same lines run on the host under the generator cores' CPU tests.
// =============================================================================================
__global__ __launch_bounds__(64) void pose_chain_fwd_kernel(parc_char_model_t m, int n, const float *__restrict__ root_pos,
                                                            const float *__restrict__ root_exp, const float *__restrict__ dof,
                                                            float *root_quat, float *joint_rot, float *body_pos, float *body_rot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int B = m.num_bodies;
    q4 rot[PARC_MAX_BODIES];
    v3 pos[PARC_MAX_BODIES];
    rot[0] = em_to_quat(ld3(root_exp + 3 * (size_t)i));
    pos[0] = ld3(root_pos + 3 * (size_t)i);
    st4(root_quat + 4 * (size_t)i, rot[0]);
    const float *d = dof + (size_t)i * m.dof_size;
    for (int b = 1; b < B; ++b) {
        const int p = m.parent[b];
        const q4 jq = joint_dof_to_rot<true>(m, b, d, 1);
        st4(joint_rot + ((size_t)i * (B - 1) + (b - 1)) * 4, jq);
        const q4 loc = quat_mul(mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]), jq);
        rot[b] = quat_mul(rot[p], loc);
        pos[b] = pos[p] + quat_rotate(rot[p], mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]));
    }
    for (int b = 0; b < B; ++b) {
        st3(body_pos + ((size_t)i * B + b) * 3, pos[b]);
        st4(body_rot + ((size_t)i * B + b) * 4, rot[b]);
    }
}

__global__ __launch_bounds__(64) void pose_chain_bwd_kernel(parc_char_model_t m, int n, const float *__restrict__ root_exp,
                                                            const float *__restrict__ dof, const float *__restrict__ g_root_quat,
                                                            const float *__restrict__ g_joint_rot, const float *__restrict__ g_body_pos,
                                                            const float *__restrict__ g_body_rot, float *g_root_pos, float *g_root_exp,
                                                            float *g_dof) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int B = m.num_bodies;
    q4 rot[PARC_MAX_BODIES], jq[PARC_MAX_BODIES], loc[PARC_MAX_BODIES], grot[PARC_MAX_BODIES];
    v3 gpos[PARC_MAX_BODIES];
    const v3 em = ld3(root_exp + 3 * (size_t)i);
    const float *d = dof + (size_t)i * m.dof_size;
    float *gd = g_dof + (size_t)i * m.dof_size;
    for (int k = 0; k < m.dof_size; ++k) gd[k] = 0.f;
    rot[0] = em_to_quat(em);
    for (int b = 1; b < B; ++b) {
        jq[b] = joint_dof_to_rot<true>(m, b, d, 1);
        loc[b] = quat_mul(mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]), jq[b]);
        rot[b] = quat_mul(rot[m.parent[b]], loc[b]);
    }
    for (int b = 0; b < B; ++b) {
        gpos[b] = ld3(g_body_pos + ((size_t)i * B + b) * 3);
        grot[b] = ld4(g_body_rot + ((size_t)i * B + b) * 4);
    }
    for (int b = B - 1; b >= 1; --b) {          // children before parents: a body's index exceeds its parent's
        const int p = m.parent[b];
        // pos[b] = pos[p] + rotate(rot[p], t_b)
        gpos[p] = gpos[p] + gpos[b];
        grot[p] = qadd(grot[p], qrot_bwd_q(rot[p], mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]), gpos[b]));
        // rot[b] = rot[p] (x) loc[b]
        grot[p] = qadd(grot[p], quat_mul(grot[b], quat_conj(loc[b])));
        const q4 gloc = quat_mul(quat_conj(rot[p]), grot[b]);
        // loc[b] = lrot (x) jq[b], + the cotangent handed in for the joint rotation itself
        const q4 lr = mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]);
        const q4 gj = qadd(quat_mul(quat_conj(lr), gloc), ld4(g_joint_rot + ((size_t)i * (B - 1) + (b - 1)) * 4));
        const int jt = m.joint_type[b], d0 = m.dof_idx[b];
        if (jt == PARC_JOINT_HINGE) {
            const v3 ax = mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]);
            gd[d0] = aa_to_quat_bwd(ax, d[d0], jq[b], gj).g_angle;
        } else if (jt == PARC_JOINT_SPHERICAL) {
            const v3 ge = em_to_quat_bwd(mk3(d[d0], d[d0 + 1], d[d0 + 2]), jq[b], gj);
            gd[d0] = ge.x;
            gd[d0 + 1] = ge.y;
            gd[d0 + 2] = ge.z;
        }
    }
    st3(g_root_pos + 3 * (size_t)i, gpos[0]);
    st3(g_root_exp + 3 * (size_t)i, em_to_quat_bwd(em, rot[0], qadd(grot[0], ld4(g_root_quat + 4 * (size_t)i))));
}

// Angle between two rotations, torch_util.quat_diff_angle(q0, q1) = angle of q1 (x) conj(q0) (util/torch_util.py:421-431,68-88: the
// w >= 0 representative, 2 atan2(|v|, w), 0 below |v| = 1e-5), and its adjoint; one thread per pair.  The optimiser evaluates it for
// the root, every joint and every body-to-next-frame pair of every frame.
__global__ __launch_bounds__(256) void quat_diff_angle_kernel(size_t n, const float *__restrict__ q0, const float *__restrict__ q1, float *angle) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    angle[i] = qangle(quat_mul(ld4(q1 + 4 * i), quat_conj(ld4(q0 + 4 * i))));      // qdiff_angle on the FMA-grouped product
}

__global__ __launch_bounds__(256) void quat_diff_angle_grad_kernel(size_t n, const float *__restrict__ q0, const float *__restrict__ q1,
                                                                   const float *__restrict__ g_angle, float *g_q0, float *g_q1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const q4 a = ld4(q0 + 4 * i), b = ld4(q1 + 4 * i);
    const q4 d = quat_mul(b, quat_conj(a));
    q4 ga = mk4(0.f, 0.f, 0.f, 0.f), gb = ga;
    if (sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z) > 1e-5f) {      // in qangle's zero branch both stay exact zeros, not products with 0
        // qangle_bwd has gs * d.x for the flip, scale, flip back sg * gs * (sg * d.x): multiplying by sg = +-1 is exact, the bits are the same
        const q4 gd = qangle_bwd(d, g_angle[i]);
        gb = quat_mul(gd, a);                                   // qdiff_bwd_b and qdiff_bwd_a on the FMA-grouped product, as d above
        const q4 gc = quat_mul(quat_conj(b), gd);
        ga = q4{-gc.x, -gc.y, -gc.z, gc.w};
    }
    st4(g_q0 + 4 * i, ga);
    st4(g_q1 + 4 * i, gb);
}

extern "C" int parc_quat_diff_angle(void *stream, int64_t n, const float *q0, const float *q1, float *angle) {
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(quat_diff_angle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (size_t)n, q0, q1, angle);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_quat_diff_angle_grad(void *stream, int64_t n, const float *q0, const float *q1, const float *g_angle, float *g_q0, float *g_q1) {
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(quat_diff_angle_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (size_t)n, q0, q1, g_angle,
                       g_q0, g_q1);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// The frame-to-frame terms of stage 2's motion loss and their adjoint: the bodies live in parc_moopt_core.h (tt_forward_body /
// tt_backward_body), shared with the packed-motions pair of parc_moopt.hip.  One thread per (frame, body).
__global__ __launch_bounds__(256) void temporal_terms_kernel(int T, int B, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                                                             const float *__restrict__ src_vel, const float *__restrict__ keep,
                                                             const float *__restrict__ pair_contact, tt_args a, float *partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int t = i / B, b = i - t * B;
    float sm, sl, jl;
    tt_forward_body(T, B, t, b, i, pos, rot_err_sq, src_vel, keep, pair_contact, a, sm, sl, jl);
    const size_t n = (size_t)T * B;
    partial[i] = sm;
    partial[n + i] = sl;
    partial[2 * n + i] = jl;
}

__global__ __launch_bounds__(256) void temporal_terms_grad_kernel(int T, int B, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                                                                  const float *__restrict__ src_vel, const float *__restrict__ keep,
                                                                  const float *__restrict__ pair_contact, tt_args a,
                                                                  const float *__restrict__ w /* cotangents of the 3 sums */, float *g_pos,
                                                                  float *g_rot_err_sq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int t = i / B, b = i - t * B;
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    float g_r;
    bool has_r;
    const v3 g = tt_backward_body(T, B, t, b, i, pos, rot_err_sq, src_vel, keep, pair_contact, a, w0, w1, w2, g_r, has_r);
    st3(g_pos + (size_t)i * 3, g);
    if (has_r) g_rot_err_sq[i] = g_r;
}

extern "C" int parc_temporal_terms(void *stream, int n_frames, int num_bodies, const float *body_pos, const float *rot_err_sq, const float *src_vel,
                                   const float *keep, const float *pair_contact, float c, float c2, float jerk_limit, float *partial) {
    if (n_frames < 0 || num_bodies <= 0) return PARC_EINVAL;
    const int n = n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(temporal_terms_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, body_pos, rot_err_sq,
                       src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, partial);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_temporal_terms_grad(void *stream, int n_frames, int num_bodies, const float *body_pos, const float *rot_err_sq,
                                        const float *src_vel, const float *keep, const float *pair_contact, float c, float c2, float jerk_limit,
                                        const float *cotangents, float *g_body_pos, float *g_rot_err_sq) {
    if (n_frames < 0 || num_bodies <= 0) return PARC_EINVAL;
    const int n = n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(temporal_terms_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, body_pos,
                       rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, cotangents, g_body_pos, g_rot_err_sq);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// Sample points of the bodies in the world frame, x[t, p] = pos[t, owner(p)] + rotate(rot[t, owner(p)], local[p]), and the adjoint
// (the points of a body are contiguous: body b owns [start[b], start[b + 1])), one thread per point / per (frame, body).
__global__ __launch_bounds__(256) void body_points_world_kernel(int n_frames, int B, int P, const float *__restrict__ body_pos,
                                                                const float *__restrict__ body_rot, const float *__restrict__ local,
                                                                const int32_t *__restrict__ owner, float *world) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * P) return;
    const int t = (int)(i / P), p = (int)(i - (size_t)t * P), b = owner[p];
    const v3 x = ld3(body_pos + ((size_t)t * B + b) * 3) + quat_rotate(ld4(body_rot + ((size_t)t * B + b) * 4), ld3(local + 3 * (size_t)p));
    st3(world + i * 3, x);
}

__global__ __launch_bounds__(256) void body_points_world_grad_kernel(int n_frames, int B, int P, const float *__restrict__ body_rot,
                                                                     const float *__restrict__ local, const int32_t *__restrict__ start,
                                                                     const float *__restrict__ g_world, float *g_body_pos, float *g_body_rot) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * B) return;
    const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
    const q4 q = ld4(body_rot + i * 4);
    v3 gp = mk3(0.f, 0.f, 0.f);
    q4 gq = mk4(0.f, 0.f, 0.f, 0.f);
    for (int p = start[b]; p < start[b + 1]; ++p) {
        const v3 g = ld3(g_world + ((size_t)t * P + p) * 3);
        gp = gp + g;
        gq = qadd(gq, qrot_bwd_q(q, ld3(local + 3 * (size_t)p), g));
    }
    st3(g_body_pos + i * 3, gp);
    st4(g_body_rot + i * 4, gq);
}

extern "C" int parc_body_points_world(void *stream, int n_frames, int num_bodies, int num_points, const float *body_pos, const float *body_rot,
                                      const float *local, const int32_t *owner, float *world) {
    if (n_frames < 0 || num_bodies <= 0 || num_points < 0) return PARC_EINVAL;
    const size_t n = (size_t)n_frames * num_points;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(body_points_world_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, num_points,
                       body_pos, body_rot, local, owner, world);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_body_points_world_grad(void *stream, int n_frames, int num_bodies, int num_points, const float *body_rot, const float *local,
                                           const int32_t *start, const float *g_world, float *g_body_pos, float *g_body_rot) {
    if (n_frames < 0 || num_bodies <= 0 || num_points < 0) return PARC_EINVAL;
    const size_t n = (size_t)n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(body_points_world_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies,
                       num_points, body_rot, local, start, g_world, g_body_pos, g_body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_pose_chain_forward(void *stream, parc_char_model_t model, int n, const float *root_pos, const float *root_exp,
                                       const float *dof, float *root_quat, float *joint_rot, float *body_pos, float *body_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    for (int b = 1; b < model.num_bodies; ++b)
        if (model.parent[b] < 0 || model.parent[b] >= b) return PARC_EUNSUPPORTED;      // the sweeps rely on parents-first order
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(pose_chain_fwd_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, model, n, root_pos, root_exp, dof, root_quat,
                       joint_rot, body_pos, body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_pose_chain_backward(void *stream, parc_char_model_t model, int n, const float *root_exp, const float *dof,
                                        const float *g_root_quat, const float *g_joint_rot, const float *g_body_pos, const float *g_body_rot,
                                        float *g_root_pos, float *g_root_exp, float *g_dof) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    for (int b = 1; b < model.num_bodies; ++b)
        if (model.parent[b] < 0 || model.parent[b] >= b) return PARC_EUNSUPPORTED;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(pose_chain_bwd_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, model, n, root_exp, dof, g_root_quat,
                       g_joint_rot, g_body_pos, g_body_rot, g_root_pos, g_root_exp, g_dof);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}
