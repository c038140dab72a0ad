/*
 * parc_moopt.h -- C-ABI of the batched motion optimiser's kernels inside libparc_hip.so.
 *
 * M motions packed along the frame axis descend together (tools/motion_opt/motion_optimization.motion_contact_optimization_batch):
 * the terrain query takes a terrain per row, the frame-to-frame terms are cut at the seams between motions, and per-frame partials
 * are folded into per-motion sums.  One launch per call; no allocation, host read, wait or float atomic, so every call can sit in a
 * captured iteration.
 */
#ifndef PARC_MOOPT_H
#define PARC_MOOPT_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One heightfield of a ragged batch, as points_hf_sdf sees it: cell (i, j) is the column with centre
 * (pool[off_x + i] + ox, pool[off_y + j] + oy), half extents (half_x, half_y) and height pool[off_hf + i * dim_y + j]; vertically it
 * spans [base_z, height], or inverted [height, -base_z].  All offsets count floats of ONE pool shared by the table. */
typedef struct {
    int32_t off_hf, off_x, off_y;
    int32_t dim_x, dim_y;
    float ox, oy;
    float half_x, half_y;
    float base_z;
} parc_moopt_terrain_t;

/* parc_points_hf_sdf with a terrain per row.
 *   points [n_rows, points_per_row, 3], row_terrain [n_rows] int32, table [n_terrains] (DEVICE), pool (DEVICE floats)
 *   out [n_rows, points_per_row]; out_cell (may be NULL) int32, same shape: the column i * dim_y + j that attains the minimum
 * The value, the NaN rule (a NaN coordinate gives NaN), the radius rule (radius > 0 is subtracted) and the sign rule (inverted flips
 * the sign) are those of parc_points_hf_sdf.  A row whose terrain id lies outside [0, n_terrains) gives NaN and cell -1 for its points
 * and reads neither table nor pool.  Points are indexed flat (row = index / points_per_row): any n_rows is accepted.
 * PARC_EINVAL (before any HIP call): n_rows < 0, n_terrains < 0, points_per_row <= 0; then n_rows == 0: PARC_OK, nothing launched;
 * then PARC_EINVAL for a NULL required pointer (every entry point here answers in this order). */
int parc_points_hf_sdf_ragged(void *stream, int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain, int n_terrains,
                              const parc_moopt_terrain_t *table, const float *pool, int inverted, float radius, float *out, int32_t *out_cell);

/* Adjoint of the query with respect to the points: g_points = g_out * d(distance to column cell)/d(point), the expression of
 * parc_points_hf_sdf_grad with the row's table entry.  A cell of -1 (or outside the row's field, or an invalid terrain id) gives a
 * zero gradient.  Argument rules as above; cell, g_out and g_points are required. */
int parc_points_hf_sdf_ragged_grad(void *stream, int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain,
                                   int n_terrains, const parc_moopt_terrain_t *table, const float *pool, int inverted, const int32_t *cell,
                                   const float *g_out, float *g_points);

/* parc_temporal_terms over packed frames: motion m owns frames seg_start[m] .. seg_start[m + 1] - 1 (seg_start [n_motions + 1] int32,
 * ascending, seg_start[n_motions] <= n_frames), seg_of_frame [n_frames] int32 names each frame's motion.  Within a motion of T_m frames
 * the arithmetic is parc_temporal_terms' with T = T_m: velocity pairs for local t < T_m - 1, third differences for local t < T_m - 3;
 * nothing is read across a seam.  body_pos / src_vel [n_frames, num_bodies, 3]; rot_err_sq, keep, pair_contact [n_frames, num_bodies]
 * (the last row of every motion is present and never read).  partial [3, n_frames, num_bodies] (smoothness, sliding, jerk).
 * A frame whose motion id or segment lies outside the tables gets zeros.
 * PARC_EINVAL: n_frames < 0, n_motions < 0, num_bodies <= 0, a NULL required pointer.  n_frames == 0: PARC_OK, nothing launched. */
int parc_temporal_terms_seg(void *stream, int n_frames, int num_bodies, int n_motions, const int32_t *seg_start, const int32_t *seg_of_frame,
                            const float *body_pos, const float *rot_err_sq, const float *src_vel, const float *keep, const float *pair_contact,
                            float c, float c2, float jerk_limit, float *partial);

/* Adjoint: cotangents [3, n_motions] of the three per-motion sums; g_body_pos [n_frames, num_bodies, 3], g_rot_err_sq
 * [n_frames, num_bodies] (0 in the last row of every motion). */
int parc_temporal_terms_seg_grad(void *stream, int n_frames, int num_bodies, int n_motions, const int32_t *seg_start, const int32_t *seg_of_frame,
                                 const float *body_pos, const float *rot_err_sq, const float *src_vel, const float *keep,
                                 const float *pair_contact, float c, float c2, float jerk_limit, const float *cotangents, float *g_body_pos,
                                 float *g_rot_err_sq);

/* Number of partial sums a motion's elements are dealt into before they are folded pairwise. */
#define PARC_MOOPT_SUM_LANES 256

/* out[p, m] = sum of values[p, seg_start[m] .. seg_start[m + 1] - 1, :]   (values [n_planes, n_rows, width], out [n_planes, n_motions]).
 * Element e of the motion's contiguous block goes to partial e mod 256, in ascending e; the 256 partials are folded pairwise
 * (k with k + 128, then k + 64, ...).  The order depends on the motion's own length and width only: the result does not depend on
 * n_motions, on the motion's place or on the other motions.  An empty (or out-of-range) segment gives exactly 0.
 * PARC_EINVAL: n_planes < 0, n_rows < 0, n_motions < 0, width <= 0, a NULL required pointer.  n_planes == 0 or n_motions == 0:
 * PARC_OK, nothing launched.  PARC_EUNSUPPORTED: n_planes > 65535. */
int parc_segment_sums(void *stream, int n_planes, int n_rows, int width, int n_motions, const int32_t *seg_start, const float *values,
                      float *out);

int parc_moopt_abi(void);

#ifdef __cplusplus
}
#endif
#endif
