/*
 * parc_mdm_guide.h -- C-ABI of the motion generator's guidance step inside libparc_hip.so.
 *
 * MDM.apply_guidance (diffusion/mdm.py:1444-1542 of the reference): after a denoising step the predicted clean motion x [B, S, D] is moved
 * down the gradient of a guidance loss, x <- x - guidance_str * d(sum_t w_t term_t)/dx.  The reference does this through autograd for a
 * batch of one; the loss is a sum over the batch, so sample b's gradient depends on sample b alone and parc_mdm_guide_step does the whole
 * step for B samples in one launch, one workgroup of PARC_MDM_GUIDE_THREADS per sample, each giving what the reference gives for that
 * sample by itself.  The sample's heightfield (times max_h), body transforms and cotangents live in dynamic LDS; no [points, columns]
 * tensor exists; cotangents are gathered per (frame, body), not scattered: no float atomics; vector stores only; every sum is folded in
 * a fixed order that does not depend on the launch shape, so two runs give the same bits.  The arithmetic is in
 * parc_amd/csrc/parc_mdm_guide_core.h (pose chain, its adjoint and the terrain scan are those of parc_mdm_pose_core.h), compiled with
 * floating-point contraction off for the device and for the host.
 *
 * Terms (rows of terms [PARC_MDM_GUIDE_TERMS, B], unweighted, in the order the reference adds them; a term switched off is written 0).
 * root, body_pos, body_rot: the pose chain of x * std + mean.
 *   TARGET  0.5 * sum_frames |target_xy - root_xy|^2
 *   HF      0.5 * sum_(frame, point) min(sdf, 0)^2         sdf: signed distance of a body's sample point to the local heightfield,
 *                                                          negative inside the ground (compute_point_hf_sdf with its default base_z)
 *   SPEED   sum max(|D1 pos| - max_speed dt,   0)
 *   ACC     sum max(|D2 pos| - max_acc   dt^2, 0)
 *   JERK    sum max(|D3 pos| - max_jerk  dt^3, 0)
 * D1 is the reference's `body_pos[..., 1:, :] - body_pos[..., :-1, :]` on body_pos [B, S, num_bodies, 3]: that slice runs over the
 * second-to-last axis, the BODIES of one frame in model order, not over frames; D2 and D3 are its repeated differences.  The sums run
 * over every frame and every element of that order (num_bodies - k elements per frame for Dk).  An order with no element
 * (num_bodies <= k) is an empty sum: 0 with gradient 0.  The thresholds are formed in double and rounded once, as the reference's Python
 * scalars are.
 *
 * Update.  x_out = x - guidance_str * gradient; every element of x_out is written.  x_out may be the same pointer as x (nothing else may
 * alias): a workgroup finishes its last read of x, passes a barrier, and only then writes; the in-place result equals the out-of-place
 * one bit for bit.  Columns that the loss never reads (JOINT_POS, CONTACTS) are copied bit for bit; fixed joints have no column.
 *
 * Singular points.  A rotation in the reference's "substitute the z axis" branch (vector part or exponential-map angle <= 1e-5) has
 * gradient 0; a point with sdf == 0 has gradient 0; a hinge at or below its threshold (a zero difference vector included) has gradient 0.
 * A NaN or Inf in a sample's x reaches that sample's x_out and terms only.
 *
 * parc_mdm_guide_step answers in this order, before any HIP call: PARC_EINVAL for a negative count or a configuration that names no
 * layout (seq_len < 1, a grid dimension < 1, num_points < 0, slices that do not tile [0, D), unknown bits in `enabled`, the terrain term
 * switched on with num_points < 1, a model whose bodies are not stored parents-first); PARC_EUNSUPPORTED when
 * parc_mdm_guide_lds_bytes > PARC_MDM_GUIDE_MAX_LDS; PARC_OK with nothing launched and x_out untouched for B == 0 or no term enabled;
 * PARC_EINVAL for a NULL required pointer.
 *
 * LDS bytes of one workgroup, with n = S * num_bodies, J = num_bodies - 1, XY = dim_x * dim_y, P = num_points:
 *   4 * (XY + 7 n + 4 S J          heightfield; body positions and rotations, joint rotations
 *        + 7 n + 4 S J             their cotangents (the per-item summands of the four per-body terms reuse the first 4 n)
 *        + S D                     the gradient, then the updated sample
 *        + 5 * 16                  sub-sums
 *        + S P + ceil(S P / 2))    per (frame, point): the distance as a float and the column that attains it as 16 bits
 * The shipped generation configuration (S 16, 31 x 31 grid, 304 points, D 91) needs 59780 bytes.
 */
#ifndef PARC_MDM_GUIDE_H
#define PARC_MDM_GUIDE_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_MDM_GUIDE_TARGET 0
#define PARC_MDM_GUIDE_HF 1
#define PARC_MDM_GUIDE_SPEED 2
#define PARC_MDM_GUIDE_ACC 3
#define PARC_MDM_GUIDE_JERK 4
#define PARC_MDM_GUIDE_TERMS 5

#define PARC_MDM_GUIDE_THREADS 256
#define PARC_MDM_GUIDE_MAX_LDS 65536 /* bytes of dynamic LDS one workgroup may ask for */

/* The feature layout and the local grid are those of parc_mdm_loss_cfg_t (include/parc_mdm_loss.h).  enabled: bit t set = term t is part
 * of the guidance loss; w[t] its weight; max_rate = {max_speed, max_acc, max_jerk}; dt = 1 / sequence_fps. */
typedef struct {
    int32_t seq_len, feat_dim;
    int32_t off_root_pos, off_root_rot, off_joint_pos, off_joint_rot, off_contacts;
    int32_t dim_x, dim_y;
    int32_t enabled, num_points;
    float ox, oy, half_x, half_y, max_h, base_z;
    float guidance_str;
    float w[PARC_MDM_GUIDE_TERMS];
    double dt, max_rate[3];
} parc_mdm_guide_cfg_t;

/* Bytes of dynamic LDS a workgroup needs for this configuration (the formula above). */
int64_t parc_mdm_guide_lds_bytes(parc_char_model_t model, parc_mdm_guide_cfg_t cfg);

/*   x [B, S, D], mean / std [S, D]                          the predicted clean motion and the feature statistics
 *   hfs [B, dim_x, dim_y]                                   divided by max_h; NULL iff the terrain term is off
 *   target_xy [B, 2]                                        NULL iff the target term is off
 *   grid_x [dim_x], grid_y [dim_y], points [num_points, 3], point_start [num_bodies + 1]
 *                                                           read by the terrain term alone; body b owns points [start[b], start[b + 1])
 *   x_out [B, S, D], terms [PARC_MDM_GUIDE_TERMS, B]        written */
int parc_mdm_guide_step(void *stream, parc_char_model_t model, parc_mdm_guide_cfg_t cfg, int B, const float *x, const float *mean,
                        const float *std, const float *hfs, const float *target_xy, const float *grid_x, const float *grid_y,
                        const float *points, const int32_t *point_start, float *x_out, float *terms);

int parc_mdm_guide_abi(void);

#ifdef __cplusplus
}
#endif
#endif
