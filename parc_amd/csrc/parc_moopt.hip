// Kernels of the batched motion optimiser (include/parc_moopt.h): M motions packed along the frame axis descend together, so the
// terrain query takes a terrain per row, the frame-to-frame terms are cut at motion seams and per-frame partials are folded per motion.
// The bodies are in parc_moopt_core.h (shared with parc_pose_opt.hip and with the host build of the CPU tests); here are the thread maps.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_moopt.h"
#include "parc_launch.h"
#include "parc_moopt_core.h"

#define RAGGED_THREADS 64       // as points_hf_sdf_kernel: the window scan diverges per point, a workgroup of one wave retires early

// One thread per point of the flat [n_rows * points_per_row] grid; the row's table entry names the heightfield inside the pool.
__global__ __launch_bounds__(RAGGED_THREADS) void points_hf_sdf_ragged_kernel(size_t n_total, int points_per_row, const float *__restrict__ points,
                                                                              const int32_t *__restrict__ row_terrain, int n_terrains,
                                                                              const parc_moopt_terrain_t *__restrict__ table,
                                                                              const float *__restrict__ pool, int inverted, float radius,
                                                                              float *__restrict__ out, int32_t *__restrict__ out_cell) {
    const size_t idx = (size_t)blockIdx.x * RAGGED_THREADS + threadIdx.x;
    if (idx >= n_total) return;
    ragged_thread(idx, points_per_row, points, row_terrain, n_terrains, table, pool, inverted, radius, out, out_cell);
}

__global__ __launch_bounds__(RAGGED_THREADS) void points_hf_sdf_ragged_grad_kernel(size_t n_total, int points_per_row, const float *__restrict__ points,
                                                                                   const int32_t *__restrict__ row_terrain, int n_terrains,
                                                                                   const parc_moopt_terrain_t *__restrict__ table,
                                                                                   const float *__restrict__ pool, int inverted,
                                                                                   const int32_t *__restrict__ cell, const float *__restrict__ g_out,
                                                                                   float *__restrict__ g_points) {
    const size_t idx = (size_t)blockIdx.x * RAGGED_THREADS + threadIdx.x;
    if (idx >= n_total) return;
    ragged_grad_thread(idx, points_per_row, points, row_terrain, n_terrains, table, pool, inverted, cell, g_out, g_points);
}

// One thread per (packed frame, body).
__global__ __launch_bounds__(256) void temporal_terms_seg_kernel(int N, int B, int M, const int32_t *__restrict__ seg_start,
                                                                 const int32_t *__restrict__ seg_of_frame, const float *__restrict__ pos,
                                                                 const float *__restrict__ rot_err_sq, const float *__restrict__ src_vel,
                                                                 const float *__restrict__ keep, const float *__restrict__ pair_contact, tt_args a,
                                                                 float *partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * B) return;
    tt_seg_thread(i, N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, a, partial);
}

__global__ __launch_bounds__(256) void temporal_terms_seg_grad_kernel(int N, int B, int M, const int32_t *__restrict__ seg_start,
                                                                      const int32_t *__restrict__ seg_of_frame, const float *__restrict__ pos,
                                                                      const float *__restrict__ rot_err_sq, const float *__restrict__ src_vel,
                                                                      const float *__restrict__ keep, const float *__restrict__ pair_contact,
                                                                      tt_args a, const float *__restrict__ w, float *g_pos, float *g_rot_err_sq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * B) return;
    tt_seg_grad_thread(i, N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, a, w, g_pos, g_rot_err_sq);
}

// One workgroup per (motion, plane): lane k adds the motion's elements k, k + 256, ... in ascending order, then the 256 partials are
// folded pairwise through LDS.  The order is a function of the motion's own block only.
__global__ __launch_bounds__(PARC_MOOPT_SUM_LANES) void segment_sums_kernel(int n_rows, int width, int M, const int32_t *__restrict__ seg_start,
                                                                            const float *__restrict__ values, float *__restrict__ out) {
    __shared__ float lanes[PARC_MOOPT_SUM_LANES];
    const int m = blockIdx.x, plane = blockIdx.y, lane = threadIdx.x;
    size_t e0 = 0, e1 = 0;
    const bool any = segsum_block(plane, m, n_rows, width, seg_start, e0, e1);      // uniform over the workgroup
    lanes[lane] = any ? segsum_lane(values, e0, e1, lane) : 0.f;
    __syncthreads();
    for (int off = PARC_MOOPT_SUM_LANES / 2; off > 0; off >>= 1) {
        if (lane < off) lanes[lane] += lanes[lane + off];
        __syncthreads();
    }
    if (lane == 0) out[(size_t)plane * M + m] = lanes[0];
}

static inline bool ragged_grid(int64_t n_rows, int points_per_row, size_t &n_total, unsigned &blocks) {
    n_total = (size_t)n_rows * (size_t)points_per_row;
    const size_t nb = (n_total + RAGGED_THREADS - 1) / RAGGED_THREADS;
    blocks = (unsigned)nb;
    return nb <= 0x7fffffffu;
}

extern "C" int parc_points_hf_sdf_ragged(void *stream, int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain,
                                         int n_terrains, const parc_moopt_terrain_t *table, const float *pool, int inverted, float radius,
                                         float *out, int32_t *out_cell) {
    const int rc = moopt_check_ragged(n_rows, points_per_row, points, row_terrain, n_terrains, table, pool, out);
    if (rc != PARC_OK) return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc;
    size_t n_total;
    unsigned blocks;
    if (!ragged_grid(n_rows, points_per_row, n_total, blocks)) return PARC_EUNSUPPORTED;
    hipLaunchKernelGGL(points_hf_sdf_ragged_kernel, dim3(blocks), dim3(RAGGED_THREADS), 0, (hipStream_t)stream, n_total, points_per_row, points,
                       row_terrain, n_terrains, table, pool, inverted, radius, out, out_cell);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_points_hf_sdf_ragged_grad(void *stream, int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain,
                                              int n_terrains, const parc_moopt_terrain_t *table, const float *pool, int inverted,
                                              const int32_t *cell, const float *g_out, float *g_points) {
    const int rc = moopt_check_ragged(n_rows, points_per_row, points, row_terrain, n_terrains, table, pool, g_points);
    if (rc != PARC_OK) return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc;
    if (!cell || !g_out) return PARC_EINVAL;
    size_t n_total;
    unsigned blocks;
    if (!ragged_grid(n_rows, points_per_row, n_total, blocks)) return PARC_EUNSUPPORTED;
    hipLaunchKernelGGL(points_hf_sdf_ragged_grad_kernel, dim3(blocks), dim3(RAGGED_THREADS), 0, (hipStream_t)stream, n_total, points_per_row, points,
                       row_terrain, n_terrains, table, pool, inverted, cell, g_out, g_points);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_temporal_terms_seg(void *stream, int n_frames, int num_bodies, int n_motions, const int32_t *seg_start,
                                       const int32_t *seg_of_frame, const float *body_pos, const float *rot_err_sq, const float *src_vel,
                                       const float *keep, const float *pair_contact, float c, float c2, float jerk_limit, float *partial) {
    const int rc = moopt_check_tt_seg(n_frames, num_bodies, n_motions, seg_start, seg_of_frame, body_pos, rot_err_sq, src_vel, keep, pair_contact, partial);
    if (rc != PARC_OK) return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc;
    const int n = n_frames * num_bodies;
    hipLaunchKernelGGL(temporal_terms_seg_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, n_motions, seg_start,
                       seg_of_frame, body_pos, rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, partial);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_temporal_terms_seg_grad(void *stream, int n_frames, int num_bodies, int n_motions, const int32_t *seg_start,
                                            const int32_t *seg_of_frame, const float *body_pos, const float *rot_err_sq, const float *src_vel,
                                            const float *keep, const float *pair_contact, float c, float c2, float jerk_limit,
                                            const float *cotangents, float *g_body_pos, float *g_rot_err_sq) {
    const int rc = moopt_check_tt_seg(n_frames, num_bodies, n_motions, seg_start, seg_of_frame, body_pos, rot_err_sq, src_vel, keep, pair_contact,
                                      g_body_pos);
    if (rc != PARC_OK) return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc;
    if (!cotangents || !g_rot_err_sq) return PARC_EINVAL;
    const int n = n_frames * num_bodies;
    hipLaunchKernelGGL(temporal_terms_seg_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, n_motions,
                       seg_start, seg_of_frame, body_pos, rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, cotangents, g_body_pos,
                       g_rot_err_sq);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_segment_sums(void *stream, int n_planes, int n_rows, int width, int n_motions, const int32_t *seg_start, const float *values,
                                 float *out) {
    const int rc = moopt_check_segment_sums(n_planes, n_rows, width, n_motions, seg_start, values, out);
    if (rc != PARC_OK) return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(segment_sums_kernel, dim3(n_motions, n_planes), dim3(PARC_MOOPT_SUM_LANES), 0, (hipStream_t)stream, n_rows, width, n_motions,
                       seg_start, values, out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_moopt_abi(void) { return 1; }
