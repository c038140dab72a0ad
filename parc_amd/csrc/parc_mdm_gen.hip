// Kernels of the motion generator's call (include/parc_mdm_gen.h): the conditions of a whole batch in one launch, and the motion frames
// of a whole batch in one more.  The arithmetic is in parc_mdm_gen_core.h (shared with the host build of the CPU tests); here are the
// thread maps.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_mdm_gen.h"
#include "parc_launch.h"
#include "parc_mdm_gen_core.h"

using namespace parc_mgn;

// One workgroup per sample; the pose chain's scratch (parc_mgn::encode_pose) is the dynamic LDS.  The chain reads the canonical root
// back from out_root_pos / out_root_rot: no __restrict__ on the outputs.
__global__ __launch_bounds__(PARC_MDM_GEN_THREADS) void mdm_gen_encode_kernel(
    parc_char_model_t model, parc_mdm_gen_cfg_t cfg, parc_terrain_t terrain, const float *root_pos, const float *root_rot, const float *joint_rot,
    const float *contacts, const float *target_world, const float *grid_x, const float *grid_y, const float *mean, const float *std, float *frame,
    float *out_root_pos, float *out_root_rot, float *out_body_pos, float *hf_z, float *target, float *target_dir, float *prev_state, float *obs) {
    extern __shared__ float lds[];
    const enc_sample e = make_enc_sample(model, cfg, (int)blockIdx.x, root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std,
                                         frame, out_root_pos, out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state, obs, lds);
    encode_sample(model, cfg, terrain, e, (int)threadIdx.x, PARC_MDM_GEN_THREADS);
}

// One lane per (sample, frame)
__global__ __launch_bounds__(PARC_MDM_GEN_DECODE_THREADS) void mdm_gen_decode_kernel(
    parc_char_model_t model, parc_mdm_gen_cfg_t cfg, int B, const float *__restrict__ x, const float *__restrict__ prev_state,
    const uint8_t *__restrict__ no_noise, const float *__restrict__ mean, const float *__restrict__ std, const float *__restrict__ frame,
    float *__restrict__ root_pos, float *__restrict__ root_rot, float *__restrict__ joint_rot, float *__restrict__ contacts,
    float *__restrict__ frames) {
    const int64_t i = (int64_t)blockIdx.x * PARC_MDM_GEN_DECODE_THREADS + threadIdx.x;
    if (i >= (int64_t)B * cfg.seq_len) return;
    decode_item(model, cfg, (int)(i / cfg.seq_len), (int)(i % cfg.seq_len), x, prev_state, no_noise, mean, std, frame, root_pos, root_rot, joint_rot,
                contacts, frames);
}

extern "C" int parc_mdm_gen_encode(void *stream, parc_char_model_t model, parc_mdm_gen_cfg_t cfg, parc_terrain_t terrain, int B, const float *root_pos,
                                   const float *root_rot, const float *joint_rot, const float *contacts, const float *target_world,
                                   const float *grid_x, const float *grid_y, const float *mean, const float *std, float *frame, float *out_root_pos,
                                   float *out_root_rot, float *out_body_pos, float *hf_z, float *target, float *target_dir, float *prev_state,
                                   float *obs) {
    const int rc = check_encode(model, cfg, terrain, B, root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std, frame,
                                out_root_pos, out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state);
    if (rc != PARC_OK) return rc == PARC_MGN_NOTHING ? PARC_OK : rc;
    hipLaunchKernelGGL(mdm_gen_encode_kernel, dim3((unsigned)B), dim3(PARC_MDM_GEN_THREADS), (size_t)lds_bytes(model, cfg), (hipStream_t)stream, model,
                       cfg, terrain, root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std, frame, out_root_pos,
                       out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state, obs);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_gen_decode(void *stream, parc_char_model_t model, parc_mdm_gen_cfg_t cfg, int B, const float *x, const float *prev_state,
                                   const uint8_t *no_noise, const float *mean, const float *std, const float *frame, float *root_pos,
                                   float *root_rot, float *joint_rot, float *contacts, float *frames) {
    const int rc = check_decode(model, cfg, B, x, prev_state, no_noise, mean, std, frame, root_pos, root_rot, joint_rot, contacts);
    if (rc != PARC_OK) return rc == PARC_MGN_NOTHING ? PARC_OK : rc;
    const int64_t n = (int64_t)B * cfg.seq_len;
    hipLaunchKernelGGL(mdm_gen_decode_kernel, dim3((unsigned)((n + PARC_MDM_GEN_DECODE_THREADS - 1) / PARC_MDM_GEN_DECODE_THREADS)),
                       dim3(PARC_MDM_GEN_DECODE_THREADS), 0, (hipStream_t)stream, model, cfg, B, x, prev_state, no_noise, mean, std, frame, root_pos,
                       root_rot, joint_rot, contacts, frames);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_mdm_gen_abi(void) { return 1; }
