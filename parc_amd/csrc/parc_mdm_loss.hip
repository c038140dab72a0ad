// Kernels of the motion generator's training loss (include/parc_mdm_loss.h): the 14 per-sample terms of MDM.motion_difference from the
// denoiser's output in one launch, and their adjoint in one more.  The arithmetic is in parc_mdm_loss_core.h (shared with the host
// build of the CPU tests); here are the thread maps.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_mdm_loss.h"
#include "parc_launch.h"
#include "parc_mdm_loss_core.h"

using namespace parc_ml;

// One workgroup per sample; the sample's scratch (parc_ml::layout) is the dynamic LDS.
__global__ __launch_bounds__(PARC_MDM_LOSS_THREADS) void mdm_loss_fwd_kernel(
    parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *__restrict__ x, const float *__restrict__ mean,
    const float *__restrict__ std, const float *__restrict__ root_pos, const float *__restrict__ root_rot, const float *__restrict__ joint_rot,
    const float *__restrict__ contacts, const float *__restrict__ hfs, const float *__restrict__ target_dir, const float *__restrict__ grid_x,
    const float *__restrict__ grid_y, const float *__restrict__ points, const int32_t *__restrict__ point_start, float *__restrict__ losses) {
    extern __shared__ float lds[];
    const int b = (int)blockIdx.x;
    const sample s = make_sample(model, cfg, b, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                                 point_start, lds);
    forward_sample(model, cfg, s, b, B, losses, (int)threadIdx.x, PARC_MDM_LOSS_THREADS);
}

__global__ __launch_bounds__(PARC_MDM_LOSS_THREADS) void mdm_loss_bwd_kernel(
    parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *__restrict__ x, const float *__restrict__ mean,
    const float *__restrict__ std, const float *__restrict__ root_pos, const float *__restrict__ root_rot, const float *__restrict__ joint_rot,
    const float *__restrict__ contacts, const float *__restrict__ hfs, const float *__restrict__ target_dir, const float *__restrict__ grid_x,
    const float *__restrict__ grid_y, const float *__restrict__ points, const int32_t *__restrict__ point_start,
    const float *__restrict__ g_losses, float *__restrict__ g_x) {
    extern __shared__ float lds[];
    const int b = (int)blockIdx.x;
    const sample s = make_sample(model, cfg, b, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                                 point_start, lds);
    backward_sample(model, cfg, s, b, B, g_losses, g_x + (size_t)b * cfg.seq_len * cfg.feat_dim, (int)threadIdx.x, PARC_MDM_LOSS_THREADS);
}

extern "C" int64_t parc_mdm_loss_lds_bytes(parc_char_model_t model, parc_mdm_loss_cfg_t cfg) { return lds_bytes(model, cfg); }

extern "C" int parc_mdm_loss_forward(void *stream, parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean,
                                     const float *std, const float *root_pos, const float *root_rot, const float *joint_rot,
                                     const float *contacts, const float *hfs, const float *target_dir, const float *grid_x, const float *grid_y,
                                     const float *points, const int32_t *point_start, float *losses) {
    const int rc = check_args(model, cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                              point_start, losses, losses);
    if (rc != PARC_OK) return rc == PARC_ML_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(mdm_loss_fwd_kernel, dim3((unsigned)B), dim3(PARC_MDM_LOSS_THREADS), (size_t)lds_bytes(model, cfg), (hipStream_t)stream, model,
                       cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points, point_start, losses);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_loss_backward(void *stream, parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean,
                                      const float *std, const float *root_pos, const float *root_rot, const float *joint_rot,
                                      const float *contacts, const float *hfs, const float *target_dir, const float *grid_x, const float *grid_y,
                                      const float *points, const int32_t *point_start, const float *g_losses, float *g_x) {
    const int rc = check_args(model, cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                              point_start, g_x, g_losses);
    if (rc != PARC_OK) return rc == PARC_ML_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(mdm_loss_bwd_kernel, dim3((unsigned)B), dim3(PARC_MDM_LOSS_THREADS), (size_t)lds_bytes(model, cfg), (hipStream_t)stream, model,
                       cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points, point_start, g_losses,
                       g_x);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_loss_abi(void) { return 1; }
