/*
 * parc_mdm_loss.h -- C-ABI of the motion generator's training loss inside libparc_hip.so.
 *
 * MDM.extract_motion_features followed by MDM.motion_difference (diffusion/mdm.py:434-478, 617-754, compute_point_hf_sdf :978-1028 of
 * the reference): the denoiser's output x [B, S, D] becomes PARC_MDM_LOSS_TERMS per-sample loss terms in one launch
 * (parc_mdm_loss_forward) and their cotangents become g_x in one more (parc_mdm_loss_backward).  One workgroup per sample; the sample's
 * heightfield, the body transforms of both sides and every partial sum live in LDS, so no [points, columns] tensor exists and nothing is
 * saved between the two launches: the backward launch evaluates the chain again.  The arithmetic is in
 * parc_amd/csrc/parc_mdm_loss_core.h, compiled with floating-point contraction off for the device and for the host.  Nothing is
 * allocated, read back or waited for; no float atomics; vector stores only; sums are folded in a fixed order, so two runs give the same
 * bits.
 *
 * Every entry point answers in this order, before any HIP call: PARC_EINVAL for a negative count or a configuration that names no
 * layout (seq_len < 1, ref_idx outside [0, seq_len), a grid dimension < 1, slices that do not tile [0, D), an unknown loss_fn, a model
 * whose bodies are not stored parents-first); PARC_EUNSUPPORTED when the sample does not fit the
 * workgroup's LDS (parc_mdm_loss_lds_bytes > PARC_MDM_LOSS_MAX_LDS); PARC_OK with nothing launched for B == 0; PARC_EINVAL for a NULL
 * required pointer.
 *
 * Gradients at singular inputs.  torch differentiates norm() and atan2 at a zero vector part to NaN; here every rotation whose vector
 * part (or exponential-map angle) is at most 1e-5 - the branch where the reference substitutes the constant z axis and angle 0 - has
 * gradient 0.  Fixed joints (no dofs; the hands) are constants on both sides and never reach g_x.  A sample point exactly on the
 * surface (sdf == 0) has gradient 0, as clamp(max=0) followed by square gives.
 *
 * Non-finite values in a sample's x reach that sample's terms and gradient only: a workgroup reads and writes its own sample.
 */
#ifndef PARC_MDM_LOSS_H
#define PARC_MDM_LOSS_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of losses [PARC_MDM_LOSS_TERMS, B], in the order motion_difference inserts its keys.  A term that the configuration switches off
 * (enabled bit clear) is written as 0 and takes no cotangent. */
#define PARC_MDM_LOSS_VEL_ROOT_POS 0
#define PARC_MDM_LOSS_VEL_ROOT_ROT 1
#define PARC_MDM_LOSS_VEL_JOINT_ROT 2
#define PARC_MDM_LOSS_SIMPLE_ROOT_POS 3
#define PARC_MDM_LOSS_SIMPLE_ROOT_ROT 4
#define PARC_MDM_LOSS_SIMPLE_JOINT_ROT 5
#define PARC_MDM_LOSS_SIMPLE_CONTACT 6
#define PARC_MDM_LOSS_SIMPLE_BODY_POS 7
#define PARC_MDM_LOSS_FK_BODY_POS 8
#define PARC_MDM_LOSS_FK_BODY_ROT 9
#define PARC_MDM_LOSS_BODY_POS_CONSISTENCY 10
#define PARC_MDM_LOSS_VEL_FK_BODY_POS 11
#define PARC_MDM_LOSS_HF_COLLISION 12
#define PARC_MDM_LOSS_TARGET 13
#define PARC_MDM_LOSS_TERMS 14

#define PARC_MDM_LOSS_SQUARED_L2 0
#define PARC_MDM_LOSS_PSEUDO_HUBER 1 /* sqrt(sum((a - b)^2 + 0.0009)) - 0.03 */

#define PARC_MDM_LOSS_THREADS 256
#define PARC_MDM_LOSS_MAX_LDS 65536 /* bytes of dynamic LDS one workgroup may ask for */

/* What the samples of a batch share.  Feature row d of x: off_root_pos (3), off_root_rot (3, exponential map), off_joint_rot
 * (model.dof_size), off_joint_pos (3 per non-root body; -1 = absent), off_contacts (1 per body; -1 = absent).  The local grid has
 * dim_x * dim_y columns, column (i, j) centred at (ox + grid_x[i], oy + grid_y[j]) with half extents (half_x, half_y); hfs arrive
 * divided by max_h.  enabled: bit t set = term t is computed. */
typedef struct {
    int32_t seq_len, feat_dim, ref_idx;
    int32_t off_root_pos, off_root_rot, off_joint_pos, off_joint_rot, off_contacts;
    int32_t dim_x, dim_y;
    int32_t loss_fn, enabled;
    int32_t num_points;
    float ox, oy, half_x, half_y, max_h, base_z;
    float dt, target_eps;
    float w[PARC_MDM_LOSS_TERMS];
} parc_mdm_loss_cfg_t;

/* Bytes of dynamic LDS a workgroup needs for this configuration. */
int64_t parc_mdm_loss_lds_bytes(parc_char_model_t model, parc_mdm_loss_cfg_t cfg);

/*   x [B, S, D], mean / std [S, D]                          the denoiser's output and the feature statistics
 *   root_pos [B, S, 3], root_rot [B, S, 4], joint_rot [B, S, J, 4], contacts [B, S, num_bodies] (NULL when off_contacts < 0)
 *                                                           the true side as the sampler returns it (quaternions xyzw)
 *   hfs [B, dim_x, dim_y], target_dir [B, 2], grid_x [dim_x], grid_y [dim_y]
 *   points [num_points, 3], point_start [num_bodies + 1]    sample points in body frames; body b owns [start[b], start[b + 1])
 *   losses [PARC_MDM_LOSS_TERMS, B]                         written */
int parc_mdm_loss_forward(void *stream, parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean,
                          const float *std, const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts,
                          const float *hfs, const float *target_dir, const float *grid_x, const float *grid_y, const float *points,
                          const int32_t *point_start, float *losses);

/* The same inputs and the cotangent g_losses [PARC_MDM_LOSS_TERMS, B] -> g_x [B, S, D], every element overwritten.  The per-sample
 * totals the pseudo-Huber gradient needs are evaluated again, not read from the forward launch's output. */
int parc_mdm_loss_backward(void *stream, parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean,
                           const float *std, const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts,
                           const float *hfs, const float *target_dir, const float *grid_x, const float *grid_y, const float *points,
                           const int32_t *point_start, const float *g_losses, float *g_x);

int parc_mdm_loss_abi(void);

#ifdef __cplusplus
}
#endif
#endif
