// parc_motion_score: rank candidate motions against the terrain (include/parc_score.h).  Two launches in a linear chain.
//
// motion_score_frames_kernel  grid = frame tiles x candidates, 256 threads = 16 frames.  A 16-lane group owns one frame: lane b runs
//   body b through group_fk (parc_fk_group.h), then the group walks the bodies in order - body b's pose is broadcast from lane b and the
//   16 lanes stripe its sample points, each lane adding its penetrations in a register in point order and keeping its smallest outside
//   distance.  The per-body minimum is a DPP row reduction (the values are >= 0: order-free), the frame's two sums are sum16 rotation
//   trees.  No atomics, no [B,F,P] array: a frame leaves two floats (and its body positions, when the jerk figures are asked for).
//   Heights come from L2 as in points_hf_sdf_kernel.
// motion_score_fold_kernel    one 64-thread workgroup per candidate: strided partial sums over the counted frames and over the jerk
//   items, a halving tree in LDS, the weights.
// All arithmetic from the body poses on is parc_score_core.h, shared with the host build of the tests.
#include <hip/hip_runtime.h>

#include "parc_fk_group.h"
#include "parc_launch.h"
#include "parc_score_core.h"

using namespace parc_sc;

#define SCORE_THREADS (PARC_SCORE_TILE * GRP)

PARC_DEV float min16(float v) {
    v = fminf(v, row_ror_f<0x128>(v));
    v = fminf(v, row_ror_f<0x124>(v));
    v = fminf(v, row_ror_f<0x122>(v));
    v = fminf(v, row_ror_f<0x121>(v));
    return v;
}

__global__ __launch_bounds__(SCORE_THREADS) void motion_score_frames_kernel(
    parc_char_model_t m, int F, const int32_t *__restrict__ num_frames, const float *__restrict__ root_pos, const float *__restrict__ root_rot,
    const float *__restrict__ joint_rot, const float *__restrict__ contacts, int n_points, const float *__restrict__ local,
    const int32_t *__restrict__ start, parc_score_terrain_t ter, float base_z, float *__restrict__ body_pos_ws, float *__restrict__ frame_terms) {
    const int cand = blockIdx.y;
    const int lane = threadIdx.x % GRP;
    const int f = blockIdx.x * PARC_SCORE_TILE + threadIdx.x / GRP;
    if (f >= counted_frames(num_frames, cand, F)) return;        // whole groups leave: the shuffles below stay inside a group
    const int Bd = m.num_bodies;
    const size_t row = (size_t)cand * F + f;
    q4 jq = mk4(0.f, 0.f, 0.f, 1.f);
    if (lane >= 1 && lane < Bd) jq = ld4(joint_rot + (row * (Bd - 1) + (lane - 1)) * 4);
    v3 pos;
    q4 rot;
    group_fk(m, lane, ld3(root_pos + 3 * row), ld4(root_rot + 4 * row), jq, pos, rot);
    int bad = lane < Bd && !finite_pose(pos, rot);
    if (body_pos_ws && lane < Bd) st3(body_pos_ws + (row * Bd + lane) * 3, pos);

    const Field fld = make_field(ter, base_z);
    float pen_acc = 0.f, con = 0.f;
    for (int b = 0; b < Bd; ++b) {
        const v3 bp = shfl16(pos, b);
        const q4 br = shfl16(rot, b);
        int p0, p1;
        body_range(start, b, n_points, p0, p1);
        const float mn = min16(body_lane_terms(fld, bp, br, local, p0, p1, lane, pen_acc, bad));
        if (lane == b && p1 > p0) con = contacts[row * Bd + b] * mn;
    }
    const float pen_f = sum16(pen_acc), con_f = sum16(con);
    bad = any16(bad);
    if (lane == 0) {
        const float nanv = __builtin_nanf("");
        frame_terms[2 * row] = bad ? nanv : pen_f;
        frame_terms[2 * row + 1] = bad ? nanv : con_f;
    }
}

__global__ __launch_bounds__(kFoldThreads) void motion_score_fold_kernel(int F, int num_bodies, const int32_t *__restrict__ num_frames,
                                                                         const float *__restrict__ frame_terms,
                                                                         const float *__restrict__ body_pos_ws, float w_contact, float w_pen,
                                                                         float dt, float max_jerk, float *__restrict__ losses,
                                                                         float *__restrict__ jerk) {
    __shared__ FoldPartial part[kFoldThreads];
    const int cand = blockIdx.x, t = threadIdx.x;
    const int n = counted_frames(num_frames, cand, F);
    part[t] = fold_partial(t, n, num_bodies, frame_terms + 2 * (size_t)cand * F,
                           jerk ? body_pos_ws + (size_t)cand * F * num_bodies * 3 : nullptr, dt, max_jerk);
    __syncthreads();
    for (int s = kFoldThreads / 2; s >= 1; s >>= 1) {
        if (t < s) fold_add(part[t], part[t + s]);
        __syncthreads();
    }
    if (t == 0) fold_finish(part[0], n, num_bodies, w_contact, w_pen, losses + 3 * (size_t)cand, jerk ? jerk + 2 * (size_t)cand : nullptr);
}

extern "C" int parc_motion_score(void *stream, parc_char_model_t model, int B, int F, const int32_t *num_frames, const float *root_pos,
                                 const float *root_rot, const float *joint_rot, const float *contacts, int n_points, const float *local,
                                 const int32_t *start, parc_score_terrain_t terrain, float base_z, float w_contact, float w_pen, float dt,
                                 float max_jerk, float *body_pos_ws, float *frame_terms, float *losses, float *jerk) {
    const int rc = check_args(model, B, F, root_pos, root_rot, joint_rot, contacts, n_points, local, start, terrain, body_pos_ws, frame_terms, losses, jerk);
    if (rc != PARC_OK) return rc;
    if (B == 0 || F == 0) return PARC_OK;
    hipLaunchKernelGGL(motion_score_frames_kernel, dim3((F + PARC_SCORE_TILE - 1) / PARC_SCORE_TILE, B), dim3(SCORE_THREADS), 0, (hipStream_t)stream,
                       model, F, num_frames, root_pos, root_rot, joint_rot, contacts, n_points, local, start, terrain, base_z,
                       jerk ? body_pos_ws : nullptr, frame_terms);
    PARC_CHECK_LAUNCH();
    hipLaunchKernelGGL(motion_score_fold_kernel, dim3(B), dim3(kFoldThreads), 0, (hipStream_t)stream, F, model.num_bodies, num_frames, frame_terms,
                       body_pos_ws, w_contact, w_pen, dt, max_jerk, losses, jerk);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_score_abi(void) { return 1; }
