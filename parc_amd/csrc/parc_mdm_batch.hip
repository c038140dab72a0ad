// Kernels of the motion generator's training-batch sampler (include/parc_mdm_batch.h): the local heightfields of a batch with their
// motion-aware augmentation, and the canonicalised motion windows with their targets - two launches per batch.  The arithmetic is in
// parc_mdm_batch_core.h (shared with the host build of the CPU tests); here are the thread maps.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_mdm_batch.h"
#include "parc_launch.h"
#include "parc_mdm_batch_core.h"

using namespace parc_mdm;

// One workgroup per sample; the local grid's four planes and the terrain's mask bitmap live in dynamic LDS.
__global__ __launch_bounds__(PARC_MDM_HF_THREADS) void mdm_heightfields_kernel(
    parc_motion_lib_t ml, parc_mdm_cfg_t cfg, const int64_t *__restrict__ motion_ids, const float *__restrict__ start_times,
    const float *__restrict__ motion_times, const float *__restrict__ grid_x, const float *__restrict__ grid_y, int n_clips,
    const parc_mdm_clip_t *__restrict__ clips, const float *__restrict__ pool, int64_t pool_floats, const int32_t *__restrict__ cell_start,
    int64_t n_cell_start, const int32_t *__restrict__ cells, int64_t n_cells, int mask_cells, const parc_mdm_draw_t *__restrict__ draws,
    const parc_mdm_box_t *__restrict__ boxes, const float *__restrict__ noise, float *__restrict__ hfs, float *__restrict__ center_h,
    float *__restrict__ pre, int32_t *__restrict__ cell_code) {
    extern __shared__ float lds[];
    const int XY = cfg.dim_x * cfg.dim_y;
    float *hf = lds, *bmax = lds + XY, *bmin = lds + 2 * XY, *tmp = lds + 3 * XY;
    uint32_t *bits = reinterpret_cast<uint32_t *>(lds + 4 * XY);
    hf_sample(ml, cfg, (int)blockIdx.x, motion_ids, start_times, motion_times, grid_x, grid_y, n_clips, clips, pool, pool_floats, cell_start,
              n_cell_start, cells, n_cells, mask_cells, draws, boxes, noise, hfs, center_h, pre, cell_code, (int)threadIdx.x, PARC_MDM_HF_THREADS, hf,
              bmax, bmin, tmp, bits);
}

// One lane per (sample, frame); a lane's FK workspace is its column of the LDS array.
__global__ __launch_bounds__(PARC_MDM_WIN_THREADS) void mdm_windows_kernel(
    parc_char_model_t model, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *__restrict__ motion_ids,
    const float *__restrict__ start_times, const float *__restrict__ motion_times, const float *__restrict__ center_h,
    const float *__restrict__ future_time, const float *__restrict__ future_noise, float *__restrict__ root_pos, float *__restrict__ root_rot,
    float *__restrict__ body_pos, float *__restrict__ joint_rot, float *__restrict__ contacts, float *__restrict__ future_pos,
    float *__restrict__ future_rot) {
    __shared__ float ws[PARC_MAX_BODIES * PARC_MDM_FK_FLOATS * PARC_MDM_WIN_THREADS];
    const int64_t at = (int64_t)blockIdx.x * PARC_MDM_WIN_THREADS + threadIdx.x;
    if (at >= (int64_t)n * cfg.seq_len) return;
    window_lane(model, ml, cfg, (int)(at / cfg.seq_len), (int)(at % cfg.seq_len), motion_ids, start_times, motion_times, center_h, future_time,
                future_noise, root_pos, root_rot, body_pos, joint_rot, contacts, future_pos, future_rot, ws + threadIdx.x, PARC_MDM_WIN_THREADS);
}

extern "C" int parc_mdm_heightfields(void *stream, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids,
                                     const float *start_times, const float *motion_times, const float *grid_x, const float *grid_y, int n_clips,
                                     const parc_mdm_clip_t *clips, const float *pool, int64_t pool_floats, const int32_t *cell_start,
                                     int64_t n_cell_start, const int32_t *cells, int64_t n_cells, int mask_cells, const parc_mdm_draw_t *draws,
                                     const parc_mdm_box_t *boxes, const float *noise, float *hfs, float *center_h, float *pre, int32_t *cell_code) {
    const int rc = check_heightfields(ml, cfg, n, motion_ids, start_times, motion_times, grid_x, grid_y, n_clips, clips, pool, pool_floats,
                                      cell_start, n_cell_start, cells, n_cells, mask_cells, draws, boxes, noise, hfs, center_h);
    if (rc != PARC_OK) return rc == PARC_MDM_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(mdm_heightfields_kernel, dim3((unsigned)n), dim3(PARC_MDM_HF_THREADS), hf_lds_bytes(cfg, mask_cells), (hipStream_t)stream, ml,
                       cfg, motion_ids, start_times, motion_times, grid_x, grid_y, n_clips, clips, pool, pool_floats, cell_start, n_cell_start, cells,
                       n_cells, mask_cells, draws, boxes, noise, hfs, center_h, pre, cell_code);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_windows(void *stream, parc_char_model_t model, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids,
                                const float *start_times, const float *motion_times, const float *center_h, const float *future_time,
                                const float *future_noise, float *root_pos, float *root_rot, float *body_pos, float *joint_rot, float *contacts,
                                float *future_pos, float *future_rot) {
    const int rc = check_windows(model, ml, cfg, n, motion_ids, start_times, motion_times, future_time, future_noise, root_pos, root_rot, body_pos,
                                 joint_rot, contacts, future_pos, future_rot);
    if (rc != PARC_OK) return rc == PARC_MDM_NOTHING ? PARC_OK : rc;
    const int64_t lanes = (int64_t)n * cfg.seq_len;
    const unsigned nb = (unsigned)((lanes + PARC_MDM_WIN_THREADS - 1) / PARC_MDM_WIN_THREADS);
    hipLaunchKernelGGL(mdm_windows_kernel, dim3(nb), dim3(PARC_MDM_WIN_THREADS), 0, (hipStream_t)stream, model, ml, cfg, n, motion_ids, start_times,
                       motion_times, center_h, future_time, future_noise, root_pos, root_rot, body_pos, joint_rot, contacts, future_pos, future_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_batch_abi(void) { return 1; }
