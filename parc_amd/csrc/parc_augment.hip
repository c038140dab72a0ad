// Kernels of the dataset augmentation (include/parc_augment.h): V variants of a few seed clips - frames turned and stretched, the
// terrain under them cut out, re-centred and scaled or stamped with boxes - built in three launches.  The arithmetic is in
// parc_augment_core.h (shared with the host build of the CPU tests); here are the thread maps.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_augment.h"
#include "parc_augment_core.h"
#include "parc_launch.h"

using namespace parc_aug;

#define AUG_CELL_THREADS 256

// One workgroup per variant, its threads stride over the variant's frames; the 256 partial bounds are folded pairwise through LDS
// (min and max are exact in any order).
__global__ __launch_bounds__(PARC_AUG_THREADS) void augment_frames_kernel(int n_src_rows, int contact_width, const float *__restrict__ src_frames,
                                                                          const float *__restrict__ src_contacts,
                                                                          const parc_augment_frames_t *__restrict__ vars, int n_out_rows,
                                                                          float *__restrict__ out_frames, float *__restrict__ out_contacts,
                                                                          float *__restrict__ bounds) {
    __shared__ float lo_x[PARC_AUG_THREADS], lo_y[PARC_AUG_THREADS], hi_x[PARC_AUG_THREADS], hi_y[PARC_AUG_THREADS];
    __shared__ int nan_flag[PARC_AUG_THREADS];
    const int v = blockIdx.x, lane = threadIdx.x;
    const parc_augment_frames_t a = vars[v];
    const Bounds b = frames_lane(a, lane, PARC_AUG_THREADS, n_src_rows, contact_width, src_frames, src_contacts, n_out_rows, out_frames, out_contacts);
    lo_x[lane] = b.lo_x, lo_y[lane] = b.lo_y, hi_x[lane] = b.hi_x, hi_y[lane] = b.hi_y, nan_flag[lane] = b.nan;
    __syncthreads();
    for (int off = PARC_AUG_THREADS / 2; off > 0; off >>= 1) {
        if (lane < off) {
            lo_x[lane] = fminf(lo_x[lane], lo_x[lane + off]);
            lo_y[lane] = fminf(lo_y[lane], lo_y[lane + off]);
            hi_x[lane] = fmaxf(hi_x[lane], hi_x[lane + off]);
            hi_y[lane] = fmaxf(hi_y[lane], hi_y[lane + off]);
            nan_flag[lane] |= nan_flag[lane + off];
        }
        __syncthreads();
    }
    if (lane == 0) bounds_store(Bounds{lo_x[0], lo_y[0], hi_x[0], hi_y[0], nan_flag[0]}, bounds + (size_t)v * 4);
}

// One thread per output cell of the flat [n_cells] index over all variants.
__global__ __launch_bounds__(AUG_CELL_THREADS) void augment_terrains_kernel(int n_variants, int64_t n_cells, const int64_t *__restrict__ cell_start,
                                                                            const parc_augment_variant_t *__restrict__ vars, int n_sources,
                                                                            const parc_augment_terrain_t *__restrict__ src_table,
                                                                            const float *__restrict__ src_pool, int64_t src_pool_floats,
                                                                            const parc_augment_terrain_t *__restrict__ out_table,
                                                                            const float *__restrict__ points, int64_t points_floats,
                                                                            const parc_augment_box_t *__restrict__ boxes, int n_boxes,
                                                                            const float *__restrict__ frames, int n_rows, float *__restrict__ out_pool,
                                                                            int64_t out_pool_floats, float *__restrict__ canon) {
    const int64_t cell = (int64_t)blockIdx.x * AUG_CELL_THREADS + threadIdx.x;
    if (cell >= n_cells) return;
    terrain_thread(cell, n_variants, cell_start, vars, n_sources, src_table, src_pool, src_pool_floats, out_table, points, points_floats, boxes, n_boxes,
                   frames, n_rows, out_pool, out_pool_floats, canon);
}

// One workgroup per variant, its threads stride over the variant's frames.
__global__ __launch_bounds__(PARC_AUG_THREADS) void augment_localize_kernel(const parc_augment_variant_t *__restrict__ vars,
                                                                            const float *__restrict__ canon, float *__restrict__ frames, int n_rows,
                                                                            parc_moopt_terrain_t *hf_table) {
    const int v = blockIdx.x;
    localize_lane(vars[v], v, threadIdx.x, PARC_AUG_THREADS, canon, frames, n_rows, hf_table);
}

extern "C" int parc_augment_frames(void *stream, int n_variants, int n_src_rows, int contact_width, const float *src_frames, const float *src_contacts,
                                   const parc_augment_frames_t *vars, int n_out_rows, float *out_frames, float *out_contacts, float *bounds) {
    const int rc = check_frames(n_variants, n_src_rows, contact_width, src_frames, src_contacts, vars, n_out_rows, out_frames, out_contacts, bounds);
    if (rc != PARC_OK) return rc == PARC_AUG_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(augment_frames_kernel, dim3((unsigned)n_variants), dim3(PARC_AUG_THREADS), 0, (hipStream_t)stream, n_src_rows, contact_width,
                       src_frames, src_contacts, vars, n_out_rows, out_frames, out_contacts, bounds);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_augment_terrains(void *stream, int n_variants, int64_t n_cells, const int64_t *cell_start, const parc_augment_variant_t *vars,
                                     int n_sources, const parc_augment_terrain_t *src_table, const float *src_pool, int64_t src_pool_floats,
                                     const parc_augment_terrain_t *out_table, const float *points, int64_t points_floats,
                                     const parc_augment_box_t *boxes, int n_boxes, const float *frames, int n_rows, float *out_pool,
                                     int64_t out_pool_floats, float *canon) {
    const int rc = check_terrains(n_variants, n_cells, cell_start, vars, n_sources, src_table, src_pool, src_pool_floats, out_table, points,
                                  points_floats, boxes, n_boxes, frames, n_rows, out_pool, out_pool_floats, canon);
    if (rc != PARC_OK) return rc == PARC_AUG_NOTHING ? PARC_OK : rc;
    if (n_cells == 0) return PARC_OK;
    const int64_t nb = (n_cells + AUG_CELL_THREADS - 1) / AUG_CELL_THREADS;
    if (nb > 0x7fffffffLL) return PARC_EUNSUPPORTED;
    hipLaunchKernelGGL(augment_terrains_kernel, dim3((unsigned)nb), dim3(AUG_CELL_THREADS), 0, (hipStream_t)stream, n_variants, n_cells, cell_start, vars,
                       n_sources, src_table, src_pool, src_pool_floats, out_table, points, points_floats, boxes, n_boxes, frames, n_rows, out_pool,
                       out_pool_floats, canon);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_augment_localize(void *stream, int n_variants, const parc_augment_variant_t *vars, const float *canon, float *frames, int n_rows,
                                     void *hf_table) {
    const int rc = check_localize(n_variants, vars, canon, frames, n_rows);
    if (rc != PARC_OK) return rc == PARC_AUG_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(augment_localize_kernel, dim3((unsigned)n_variants), dim3(PARC_AUG_THREADS), 0, (hipStream_t)stream, vars, canon, frames, n_rows,
                       (parc_moopt_terrain_t *)hf_table);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_augment_abi(void) { return 1; }
