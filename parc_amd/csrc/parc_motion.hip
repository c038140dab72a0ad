// Stand-alone kernels of MotionLib and KinCharModel: the frame query, the clip database build, dofs <-> joint rotations and forward
// kinematics, 16 lanes per pose.  C-ABI in include/parc_hip.h.  Reference citations are relative to the reference root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_math.h"
#include "parc_fk_group.h"      // GRP, group_fk
#include "parc_pose_lane.h"     // model_ok, joint_dof_to_rot, joint_rot_to_dof
#include "parc_motion_query.h"  // make_query, query_quat, lerp_ref, query_root_pos

// =============================================================================================
// K3 standalone (16 lanes per query, 4 queries per wave)
// =============================================================================================
__global__ __launch_bounds__(256) void motion_frame_kernel(parc_motion_lib_t ml, int nq, const int64_t *__restrict__ ids,
                                                           const float *__restrict__ times, float *root_pos, float *root_rot,
                                                           float *root_vel, float *root_ang_vel, float *joint_rot,
                                                           float *dof_vel, float *contacts) {
    int q = (blockIdx.x * blockDim.x + threadIdx.x) / GRP;
    int b = threadIdx.x % GRP;
    if (q >= nq) return;
    const int B = ml.num_bodies, J = B - 1, D = ml.dof_size;
    int64_t id = ids[q];
    frame_query fq = make_query(ml, id, times[q]);
    if (b < B) {
        q4 r = query_quat(fq, b);
        if (b == 0) st4(root_rot + 4 * (size_t)q, r);
        else st4(joint_rot + ((size_t)q * J + (b - 1)) * 4, r);
        contacts[(size_t)q * B + b] = lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend);
    }
    if (b == 0) {
        st3(root_pos + 3 * (size_t)q, query_root_pos(ml, fq, id));
        st3(root_vel + 3 * (size_t)q, ld3(fq.row0 + ml.off_root_vel));
        st3(root_ang_vel + 3 * (size_t)q, ld3(fq.row0 + ml.off_root_ang_vel));
    }
    for (int d = b; d < D; d += GRP) dof_vel[(size_t)q * D + d] = fq.row0[ml.off_dof_vel + d];
}

extern "C" int parc_calc_motion_frame(void *stream, parc_motion_lib_t mlib, int nq, const int64_t *ids, const float *times,
                                      float *root_pos, float *root_rot, float *root_vel, float *root_ang_vel, float *joint_rot,
                                      float *dof_vel, float *contacts) {
    if (nq < 0 || mlib.num_bodies > PARC_MAX_BODIES || (mlib.row_stride & 3)) return PARC_EINVAL;
    if (nq == 0) return PARC_OK;
    int threads = 256, per = threads / GRP;
    hipLaunchKernelGGL(motion_frame_kernel, dim3((nq + per - 1) / per), dim3(threads), 0, (hipStream_t)stream, mlib, nq, ids, times,
                       root_pos, root_rot, root_vel, root_ang_vel, joint_rot, dof_vel, contacts);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}


// =============================================================================================
// Clip database build: MotionLib._load_motions  anim/motion_lib.py:264-290,405-423 and
// KinCharModel.compute_frame_dof_vel  anim/kin_char_model.py:543-581, for ALL clips in one launch.
// pass 1: pose rows (quaternions, root position, contacts); pass 2: finite-difference velocities.
// =============================================================================================
__global__ __launch_bounds__(256) void motion_rows_kernel(parc_char_model_t m, parc_motion_lib_t ml, int total_frames,
                                                          const float *__restrict__ frames, const float *__restrict__ contacts,
                                                          float *rows) {
    int f = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (f >= total_frames || b >= m.num_bodies) return;
    const float *fr = frames + (size_t)f * (6 + m.dof_size);
    float *row = rows + (size_t)f * ml.row_stride;
    q4 q;
    if (b == 0) {
        q = em_to_quat(mk3(fr[3], fr[4], fr[5]));        // motion_lib.py:418
        st3(row + ml.off_pos, ld3(fr));
    } else {
        q = quat_pos(joint_dof_to_rot<true>(m, b, fr + 6, 1));     // motion_lib.py:420-421
    }
    st4(row + 4 * b, q);
    row[ml.off_contacts + b] = contacts ? contacts[(size_t)f * m.num_bodies + b] : 0.f;
}

__global__ __launch_bounds__(256) void motion_vel_kernel(parc_char_model_t m, parc_motion_lib_t ml, int total_frames,
                                                         const int32_t *__restrict__ frame_clip, const float *__restrict__ clip_fps,
                                                         float *rows) {
    int f = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (f >= total_frames || b >= m.num_bodies) return;
    int c = frame_clip[f];
    int nf = ml.num_frames[c], st = ml.start_idx[c];
    float *row = rows + (size_t)f * ml.row_stride;
    if (nf < 2) {
        if (b == 0) {
            st3(row + ml.off_root_vel, mk3(0.f, 0.f, 0.f));
            st3(row + ml.off_root_ang_vel, mk3(0.f, 0.f, 0.f));
        }
        for (int d = b; d < m.dof_size; d += GRP) row[ml.off_dof_vel + d] = 0.f;
        return;
    }
    int f0 = min(f - st, nf - 2) + st;  // the last frame repeats the previous difference (motion_lib.py:283,288)
    const float *r0 = rows + (size_t)f0 * ml.row_stride, *r1 = r0 + ml.row_stride;
    float fps = clip_fps[c];
    float dt = 1.0f / fps;
    if (b == 0) {
        v3 p0 = ld3(r0 + ml.off_pos), p1 = ld3(r1 + ml.off_pos);
        st3(row + ml.off_root_vel, fps * (p1 - p0));                                        // :281-283
        v3 em = quat_to_exp_map(quat_mul(ld4(r1), quat_conj(ld4(r0))));                     // quat_diff :286-287
        st3(row + ml.off_root_ang_vel, fps * em);
    } else {
        q4 dr = quat_unit(quat_pos(quat_mul(quat_conj(ld4(r0 + 4 * b)), ld4(r1 + 4 * b))));  // kin_char_model.py:558-559
        int jt = m.joint_type[b];
        if (jt == PARC_JOINT_HINGE) {
            v3 e = quat_to_exp_map(dr);
            row[ml.off_dof_vel + m.dof_idx[b]] = m.joint_axis[b][0] * (e.x / dt) + m.joint_axis[b][1] * (e.y / dt) + m.joint_axis[b][2] * (e.z / dt);
        } else if (jt == PARC_JOINT_SPHERICAL) {
            v3 e = quat_to_exp_map(dr);
            float *o = row + ml.off_dof_vel + m.dof_idx[b];
            o[0] = e.x / dt;
            o[1] = e.y / dt;
            o[2] = e.z / dt;
        }
    }
}

extern "C" int parc_motion_lib_build(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, int total_frames,
                                     const float *frames, const float *contacts, const int32_t *frame_clip, const float *clip_fps,
                                     float *rows) {
    if (!model_ok(model) || total_frames < 0 || mlib.num_bodies != model.num_bodies || (mlib.row_stride & 3)) return PARC_EINVAL;
    if (total_frames == 0) return PARC_OK;
    dim3 grid((total_frames + 15) / 16), block(256);
    (void)hipMemsetAsync(rows, 0, sizeof(float) * (size_t)total_frames * mlib.row_stride, (hipStream_t)stream);
    hipLaunchKernelGGL(motion_rows_kernel, grid, block, 0, (hipStream_t)stream, model, mlib, total_frames, frames, contacts, rows);
    hipLaunchKernelGGL(motion_vel_kernel, grid, block, 0, (hipStream_t)stream, model, mlib, total_frames, frame_clip, clip_fps, rows);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K1 / K4 / K2 standalone (16 lanes per pose)
// =============================================================================================
__global__ __launch_bounds__(256) void dof_to_rot_kernel(parc_char_model_t m, int n, const float *__restrict__ dof, float *jrot) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (i >= n || b == 0 || b >= m.num_bodies) return;
    st4(jrot + ((size_t)i * (m.num_bodies - 1) + (b - 1)) * 4, joint_dof_to_rot(m, b, dof + (size_t)i * m.dof_size, 1));
}

__global__ __launch_bounds__(256) void rot_to_dof_kernel(parc_char_model_t m, int n, const float *__restrict__ jrot, float *dof) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (i >= n || b == 0 || b >= m.num_bodies) return;
    joint_rot_to_dof(m, b, ld4(jrot + ((size_t)i * (m.num_bodies - 1) + (b - 1)) * 4), dof + (size_t)i * m.dof_size);
}

__global__ __launch_bounds__(256) void fk_kernel(parc_char_model_t m, int n, const float *__restrict__ root_pos,
                                                 const float *__restrict__ root_rot, const float *__restrict__ jrot,
                                                 float *body_pos, float *body_rot) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    bool live = i < n;
    int ii = live ? i : 0;
    q4 jq = mk4(0.f, 0.f, 0.f, 1.f);
    if (b >= 1 && b < m.num_bodies) jq = ld4(jrot + ((size_t)ii * (m.num_bodies - 1) + (b - 1)) * 4);
    v3 pos;
    q4 rot;
    group_fk(m, b, ld3(root_pos + 3 * (size_t)ii), ld4(root_rot + 4 * (size_t)ii), jq, pos, rot);
    if (live && b < m.num_bodies) {
        st3(body_pos + ((size_t)i * m.num_bodies + b) * 3, pos);
        st4(body_rot + ((size_t)i * m.num_bodies + b) * 4, rot);
    }
}

extern "C" int parc_dof_to_rot(void *stream, parc_char_model_t model, int n, const float *dof, float *joint_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(dof_to_rot_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, dof, joint_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_rot_to_dof(void *stream, parc_char_model_t model, int n, const float *joint_rot, float *dof) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    (void)hipMemsetAsync(dof, 0, sizeof(float) * (size_t)n * model.dof_size, (hipStream_t)stream);
    hipLaunchKernelGGL(rot_to_dof_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, joint_rot, dof);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_forward_kinematics(void *stream, parc_char_model_t model, int n, const float *root_pos, const float *root_rot,
                                       const float *joint_rot, float *body_pos, float *body_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(fk_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, root_pos, root_rot, joint_rot,
                       body_pos, body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}
