/*
 * parc_mdm_gen.h -- C-ABI of the motion generator's call inside libparc_hip.so: what gen_mdm_motion does around the sampling loop.
 *
 * diffusion/gen_util.py:81-134, :211-218 and the head and tail of MDM.gen_sequence_with_contacts (diffusion/mdm.py:1341-1364, :1392-1396)
 * of the reference.  Before the sampling loop the previous frames of every sample are canonicalised about frame c = num_prev_states - 1
 * (its root over the origin, its heading along +x), the rotated local heightfield is read off the terrain, forward kinematics gives the
 * body positions, the target becomes a direction and the previous-state features are assembled and standardised: parc_mdm_gen_encode,
 * one launch for B samples, one workgroup of PARC_MDM_GEN_THREADS per sample (lanes stride over the grid cells and over the frames).
 * After it the standardised sample becomes world-frame motion frames: parc_mdm_gen_decode, one launch, one lane per (sample, frame).
 * The arithmetic is in parc_amd/csrc/parc_mdm_gen_core.h (quaternion functions, joint rotations and the pose chain are those of
 * parc_mdm_pose_core.h; the cell lookup is parc_hf_cell.h), compiled with floating-point contraction off for the device and the host.
 * Vector stores only; no atomics; nothing is allocated, read back or waited for.  Sample b's outputs depend on sample b alone (and on
 * the terrain, mean and std, which all samples share): a NaN or Inf in its inputs reaches its outputs only.  Every terrain index is
 * clamped to the grid before its load, whatever the bits of the inputs (a NaN coordinate reads row or column 0).
 *
 * Encode, per sample (frame c: root position p_c, root rotation q_c):
 *   heading = atan2 of the rotated x axis of q_c; h = rotation by heading about z; canon_xy = p_c.xy
 *   z_ref: PARC_MDM_GEN_Z_ROOT        p_c.z (RELATIVE_TO_ROOT, the shipped style)
 *          PARC_MDM_GEN_Z_ROOT_FLOOR  the height of the terrain cell under canon_xy (RELATIVE_TO_ROOT_FLOOR).  The reference's branch
 *                                     (gen_util.py:104-111) indexes the batch axis in get_hf_val and raises for B != 2; this is its
 *                                     evident per-sample meaning, checked against the float64 restatement alone.
 *   frame [8] = canon_xy (2), h (4, xyzw), z_ref, heading
 *   root_pos[t] = conj(h) rotate (p_t - (canon_xy, 0)), then z - z_ref;  root_rot[t] = conj(h) (x) q_t
 *   body_pos[t] = forward kinematics of (root_pos[t], root_rot[t], joint_rot[t]), bodies 1 .. num_bodies - 1
 *   hf_z[i][j] = terrain height at round((rotate_2d((grid_x[i], grid_y[j]), heading) + canon_xy - min) / dxdy), clamped, minus z_ref
 *   obs = clamp(hf_z, min_h, max_h) / max_h                                                     (optional)
 *   target = rotate_2d(target_world - canon_xy, -heading);  target_dir = target / max(|target|, 1e-12)   (a zero target stays zero)
 *   prev_state[t < P] = (features - mean[t]) / std[t]: root_pos, exponential map of root_rot, body_pos (JOINT_POS), joint dofs,
 *                       contacts, each where the layout has it                                  (optional)
 *
 * Decode, per (sample, frame s): row = prev_state[b][s] where s < P and no_noise[b], else x[b][s];  u = row * std[s] + mean[s];
 *   root_pos = h rotate u_root_pos, + (canon_xy, z_ref);  root_rot = h (x) exp_map_to_quat(u_root_rot);  joint_rot = dof_to_rot(u);
 *   contacts = u_contacts;  frames = root_pos, quat_to_exp_map(root_rot), rot_to_dof(joint_rot)  (optional: the clip rows a MotionLib
 *   takes, from the registers that hold the quaternions)
 *
 * Both entry points answer in this order, before any HIP call: PARC_EINVAL for a negative count or a configuration that names no
 * layout (num_prev_states < 1 or > num_frames, a grid dimension < 1, an unknown rot_type or z_style, slices that do not tile
 * [0, feat_dim) for the rot_type, seq_len < num_prev_states in decode, a model whose bodies are not stored parents-first);
 * PARC_EUNSUPPORTED for a rot_type other than PARC_MDM_GEN_ROT_DEFAULT (the kernels take root exponential map + joint dofs) or previous
 * frames that do not fit a workgroup's LDS; PARC_OK with nothing launched for B == 0; PARC_EINVAL for a NULL required pointer.
 */
#ifndef PARC_MDM_GEN_H
#define PARC_MDM_GEN_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_MDM_GEN_THREADS 256
#define PARC_MDM_GEN_DECODE_THREADS 64
#define PARC_MDM_GEN_MAX_LDS 65536 /* bytes of dynamic LDS an encode workgroup may ask for: 4 * num_frames * (11 num_bodies - 4) */

#define PARC_MDM_GEN_Z_ROOT 0
#define PARC_MDM_GEN_Z_ROOT_FLOOR 1

#define PARC_MDM_GEN_ROT_DEFAULT 0 /* root exponential map (3), joint dofs (model.dof_size) */
#define PARC_MDM_GEN_ROT_EXP_MAP 1 /* exponential maps throughout (3, 3 per joint): not taken */
#define PARC_MDM_GEN_ROT_QUAT 2    /* quaternions throughout (4, 4 per joint): not taken */

#define PARC_MDM_GEN_FRAME 8 /* floats of a sample's frame record */

/* The feature offsets are those of parc_mdm_loss_cfg_t (-1 = JOINT_POS / CONTACTS absent).  num_frames T: frames of the previous
 * motion (encode); seq_len S: frames of the sample (decode); num_prev_states P.  The local grid has dim_x * dim_y cells at
 * (grid_x[i], grid_y[j]) in the canonical frame: the host's linspace(-dx num_x_neg, dx num_x_pos, dim_x), so the counts on the negative
 * side are in the coordinates and not in this struct. */
typedef struct {
    int32_t num_frames, seq_len, num_prev_states, feat_dim;
    int32_t off_root_pos, off_root_rot, off_joint_pos, off_joint_rot, off_contacts;
    int32_t dim_x, dim_y;
    int32_t z_style, rot_type;
    float min_h, max_h;
} parc_mdm_gen_cfg_t;

/*   root_pos [B, T, 3], root_rot [B, T, 4], joint_rot [B, T, J, 4]   the previous frames (J = num_bodies - 1; NULL allowed iff J == 0)
 *   contacts [B, T, num_bodies]                                      read for prev_state when the layout has CONTACTS; else may be NULL
 *   target_world [B, 2], grid_x [dim_x], grid_y [dim_y], mean / std [>= P, D] (read with prev_state alone)
 *   written: frame [B, 8], out_root_pos [B, T, 3], out_root_rot [B, T, 4], out_body_pos [B, T, J, 3], hf_z [B, dim_x, dim_y],
 *            target [B, 2], target_dir [B, 2];  prev_state [B, P, D] and obs [B, dim_x, dim_y] when not NULL
 *   No output may alias an input. */
int parc_mdm_gen_encode(void *stream, parc_char_model_t model, parc_mdm_gen_cfg_t cfg, parc_terrain_t terrain, int B, const float *root_pos,
                        const float *root_rot, const float *joint_rot, const float *contacts, const float *target_world, const float *grid_x,
                        const float *grid_y, const float *mean, const float *std, float *frame, float *out_root_pos, float *out_root_rot,
                        float *out_body_pos, float *hf_z, float *target, float *target_dir, float *prev_state, float *obs);

/*   x [B, S, D], mean / std [S, D], frame [B, 8] (encode's);  prev_state [B, P, D] and no_noise [B] (bytes, 0 = keep the sample's rows):
 *   both or neither
 *   written: root_pos [B, S, 3], root_rot [B, S, 4], joint_rot [B, S, J, 4]; contacts [B, S, num_bodies] (NULL iff the layout has
 *            none); frames [B, S, 6 + dof_size] when not NULL */
int parc_mdm_gen_decode(void *stream, parc_char_model_t model, parc_mdm_gen_cfg_t cfg, int B, const float *x, const float *prev_state,
                        const uint8_t *no_noise, const float *mean, const float *std, const float *frame, float *root_pos, float *root_rot,
                        float *joint_rot, float *contacts, float *frames);

int parc_mdm_gen_abi(void);

#ifdef __cplusplus
}
#endif
#endif
