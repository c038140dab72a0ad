/*
 * parc_score.h -- C-ABI of the motion scorer inside libparc_hip.so.
 *
 * Ranks a batch of candidate motions against a terrain: tools/procgen/mdm_path.compute_motion_loss (mdm_path.py:31-127) of the
 * reference for every candidate at once, plus the jerk figures of tools/motion_tests/compute_losses.py:158-169.  Two launches in a
 * linear chain; no allocation, host read or wait, so the call can sit in a captured step.
 */
#ifndef PARC_SCORE_H
#define PARC_SCORE_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Frames per workgroup of the frame kernel (a 16-lane group owns one frame). */
#define PARC_SCORE_TILE 16

/* The heightfield as points_hf_sdf sees it: cell (i, j) is the column with centre (x_points[i] + min_x, y_points[j] + min_y) and half
 * extents (dx / 2, dy / 2).  x_points / y_points are the grid the Python side computes once (linspace(0, (dim - 1) * d, dim)). */
typedef struct {
    const float *hf;                     /* DEVICE [dim_x, dim_y] */
    int32_t dim_x, dim_y;
    float min_x, min_y;
    float dx, dy;
    const float *x_points, *y_points;    /* DEVICE [dim_x], [dim_y] */
} parc_score_terrain_t;

/* Score B candidates of F frames each.
 *   num_frames [B] int32 or NULL (= F for all): frames f < clamp(num_frames[b], 0, F) count; the others are never read
 *   root_pos [B,F,3], root_rot [B,F,4] (x y z w), joint_rot [B,F,Bd-1,4], contacts [B,F,Bd]          (Bd = model.num_bodies <= 16)
 *   local [n_points,3]: sample points in their body's frame, body-major; start [Bd+1] int32: body b owns points start[b] .. start[b+1]-1
 *     (the kernel clamps them into [0, n_points]); a body without points contributes no contact term
 *   base_z: floor of the columns, min(hf) - 10 in the reference
 * Per sample point p of body b: world = body_pos[b] + rotate(body_rot[b], local[p]); d_out = max(sdf(world), 0) and
 * d_in = min(sdf_inverted(world), 0) with the column distance of parc_points_hf_sdf.  Per frame pen_f = sum_p -d_in and
 * contact_f = sum_b contacts[b] * min_{p in b} d_out.
 *   frame_terms [B,F,2]: (pen_f, contact_f) of the counted frames (other rows are left untouched)
 *   losses [B,3]: total, contact = w_contact * sum_f contact_f, pen = w_pen * sum_f pen_f;  total = pen + contact
 *   jerk [B,2] or NULL: the mean over (n - 3) x Bd of |third difference of body_pos| / dt^3, and the count of those above max_jerk
 *     divided by n - 3 (n = counted frames); both NaN when n < 4.  body_pos_ws [B,F,Bd,3] is the workspace the body positions go
 *     through; it is required (and written) only when jerk is given.
 * A non-finite pose in a counted frame makes all five outputs of that candidate NaN; other candidates are not affected.
 * PARC_EINVAL (before any HIP call): B < 0, F < 0, n_points <= 0, a model with no or more than 16 bodies, a NULL required pointer, a
 * terrain with non-positive dims or dx / dy.  PARC_EUNSUPPORTED: B > 65535.  B == 0 or F == 0: PARC_OK, nothing launched. */
int parc_motion_score(void *stream, parc_char_model_t model, int B, int F, const int32_t *num_frames, const float *root_pos,
                      const float *root_rot, const float *joint_rot, const float *contacts, int n_points, const float *local,
                      const int32_t *start, parc_score_terrain_t terrain, float base_z, float w_contact, float w_pen, float dt,
                      float max_jerk, float *body_pos_ws, float *frame_terms, float *losses, float *jerk);

int parc_score_abi(void);

#ifdef __cplusplus
}
#endif
#endif
