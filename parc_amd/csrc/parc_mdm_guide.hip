// Kernel of the motion generator's guidance step (include/parc_mdm_guide.h): the guidance loss of MDM.apply_guidance, its gradient and
// the update x <- x - guidance_str * gradient for every sample of a batch in one launch.  The arithmetic is in parc_mdm_guide_core.h
// (shared with the host build of the CPU tests); here is the thread map.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_mdm_guide.h"
#include "parc_launch.h"
#include "parc_mdm_guide_core.h"

using namespace parc_mg;

// One workgroup per sample; the sample's scratch (parc_mg::layout) is the dynamic LDS.  x and x_out may be the same array: no
// __restrict__ on either.
__global__ __launch_bounds__(PARC_MDM_GUIDE_THREADS) void mdm_guide_step_kernel(
    parc_char_model_t model, parc_mdm_guide_cfg_t cfg, int B, const float *x, const float *__restrict__ mean, const float *__restrict__ std,
    const float *__restrict__ hfs, const float *__restrict__ target_xy, const float *__restrict__ grid_x, const float *__restrict__ grid_y,
    const float *__restrict__ points, const int32_t *__restrict__ point_start, float *x_out, float *__restrict__ terms) {
    extern __shared__ float lds[];
    const int b = (int)blockIdx.x;
    const gsample g = make_gsample(cfg, b, x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, lds);
    step_sample(model, cfg, g, b, B, x_out + (size_t)b * cfg.seq_len * cfg.feat_dim, terms, (int)threadIdx.x, PARC_MDM_GUIDE_THREADS);
}

extern "C" int64_t parc_mdm_guide_lds_bytes(parc_char_model_t model, parc_mdm_guide_cfg_t cfg) { return lds_bytes(model, cfg); }

extern "C" int parc_mdm_guide_step(void *stream, parc_char_model_t model, parc_mdm_guide_cfg_t cfg, int B, const float *x, const float *mean,
                                   const float *std, const float *hfs, const float *target_xy, const float *grid_x, const float *grid_y,
                                   const float *points, const int32_t *point_start, float *x_out, float *terms) {
    const int rc = check_args(model, cfg, B, x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, x_out, terms);
    if (rc != PARC_OK) return rc == PARC_MG_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(mdm_guide_step_kernel, dim3((unsigned)B), dim3(PARC_MDM_GUIDE_THREADS), (size_t)lds_bytes(model, cfg), (hipStream_t)stream,
                       model, cfg, B, x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, x_out, terms);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_guide_abi(void) { return 1; }
