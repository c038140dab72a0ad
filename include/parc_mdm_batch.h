/*
 * parc_mdm_batch.h -- C-ABI of the motion generator's training-batch sampler inside libparc_hip.so.
 *
 * A batch of n samples (clip id, start time) of diffusion/mdm_heightfield_contact_motion_sampler.py is built in two launches: the local
 * heightfield under each sample with its motion-aware augmentation (parc_mdm_heightfields, one workgroup per sample, the grid in LDS) and
 * the canonicalised motion window with its target (parc_mdm_windows, one lane per sample and frame).  The arithmetic is in
 * parc_amd/csrc/parc_mdm_batch_core.h, compiled with floating-point contraction off for the device and for the host.  Nothing is
 * allocated, read back or waited for; vector stores only.  Every random number arrives in the draw tables: both entry points are
 * deterministic.
 *
 * Every entry point answers in this order, before any HIP call: PARC_EINVAL for a negative count or a configuration that names no grid
 * (seq_len < 1, ref_idx outside [0, seq_len), a grid dimension < 1, the centre cell outside the grid, an unknown mode or z style);
 * PARC_EUNSUPPORTED for a size over the caps below; PARC_OK with nothing launched for n == 0; PARC_EINVAL for a NULL required pointer.
 * The tables are trusted for nothing: a sample whose clip id, clip table row or cell lists point outside their arrays gets NaN outputs
 * (it alone), and every index derived from a table is checked before its load.
 */
#ifndef PARC_MDM_BATCH_H
#define PARC_MDM_BATCH_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caps, bounded by LDS (160 KiB per CU): a workgroup of parc_mdm_heightfields holds four fp32 planes of the local grid (heights, band
 * maximum, band minimum, pool scratch) and one bit per cell of the clip's terrain.  At the caps that is 32 KiB + 16 KiB; at the shipped
 * 31 x 31 grid 15.0 KiB + the bitmap, so three or more workgroups share a CU. */
#define PARC_MDM_MAX_LOCAL_CELLS 2048     /* dim_x * dim_y of the local grid */
#define PARC_MDM_MAX_TERRAIN_CELLS 131072 /* cells of one clip's terrain (the mask bitmap) */
#define PARC_MDM_MAX_BOXES 64             /* boxes per sample */
#define PARC_MDM_MAX_SEQ_LEN 1024         /* frames per window */

/* z styles (RelativeZStyle) and augmentation modes (HFAugmentationMode; OFF = use_hf_augmentation false) */
#define PARC_MDM_Z_ROOT 0
#define PARC_MDM_Z_ROOT_FLOOR 1
#define PARC_MDM_AUG_NOISE 0
#define PARC_MDM_AUG_MAXPOOL_AND_BOXES 1
#define PARC_MDM_AUG_NONE 2

/* pool kinds of a draw: the 2-D pool, the 1-D pool along the first index, the 1-D pool along the second index */
#define PARC_MDM_POOL_UNUSED (-1)
#define PARC_MDM_POOL_2D 0
#define PARC_MDM_POOL_X 1
#define PARC_MDM_POOL_Y 2

/* What the samples of a batch share.  The window's frame k is looked up at start + motion_times[k]; the reference frame is ref_idx
 * (num_prev_states - 1).  The local grid has dim_x * dim_y cells of size dx, the character over cell (num_x_neg, num_y_neg).  dt is
 * 1 / sequence_fps as fp32: the mask window starts at frame rint(start / dt) of the clip, whatever the clip's own fps. */
typedef struct {
    int32_t seq_len, ref_idx;
    int32_t num_x_neg, num_y_neg, dim_x, dim_y;
    int32_t z_style, mode;
    int32_t max_boxes; /* row width of the box table */
    float dt;
    float min_h, max_h;
} parc_mdm_cfg_t;

/* One clip's terrain and cell lists.  Heights at pool[off_hf + i * dim_y + j]; the band at pool[off_band + 2 * (i * dim_y + j)]:
 * [0] the MAXIMUM, [1] the minimum (hf_maxmin).  Cell (0, 0) has its centre at (min_x, min_y).  Frame f of the clip (0 <= f <
 * num_frames) masks the cells cells[cell_start[frame_off + f] .. cell_start[frame_off + f + 1]), each i * dim_y + j. */
typedef struct {
    int32_t off_hf, off_band;
    int32_t dim_x, dim_y;
    float min_x, min_y, dx, dy;
    int32_t frame_off, num_frames;
} parc_mdm_clip_t;

/* One sample's draws of _box_hf_augmentation, in the order they are applied: the height change, then pool[0..2] (kind UNUSED: the
 * roll failed), then boxes [0, num_boxes) of the sample's row of the box table. */
typedef struct {
    int32_t change_height;
    float new_height;
    int32_t pool_kind[3];
    int32_t pool_radius[3];
    int32_t num_boxes;
} parc_mdm_draw_t;

/* A box in cell units of the local grid: centre, side lengths, angle, height (add_boxes_to_hf2). */
typedef struct {
    float cx, cy, lx, ly, angle, h;
} parc_mdm_box_t;

/* Heightfields.  motion_ids [n] int64, start_times [n], motion_times [seq_len], grid_x [dim_x], grid_y [dim_y] (the generic grid's
 * coordinates), clips [n_clips] over pool [pool_floats], cell_start [n_cell_start] int32 over cells [n_cells] int32, all DEVICE.
 * mask_cells >= the largest dim_x * dim_y of a clip terrain a sample of this batch uses (sizes the bitmap; a sample on a larger terrain
 * gets NaN).  draws [n] and boxes [n, cfg.max_boxes] are read in mode MAXPOOL_AND_BOXES, noise [n, dim_x, dim_y] (rand * (max_h -
 * min_h) + min_h) in mode NOISE; NULL otherwise.
 *   -> hfs [n, dim_x, dim_y], center_h [n] (the height under the character before anything is subtracted).
 * Optional outputs (NULL: not written): pre [n, 3, dim_x, dim_y] = heights, band maximum, band minimum after the z style is
 * subtracted and before the augmentation; cell_code [n, dim_x, dim_y] int32 = the terrain cell i * dim_y + j each local point reads,
 * + 2^30 where the mask holds.  One workgroup of 256 threads per sample. */
int parc_mdm_heightfields(void *stream, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids, const float *start_times,
                          const float *motion_times, const float *grid_x, const float *grid_y, int n_clips, const parc_mdm_clip_t *clips,
                          const float *pool, int64_t pool_floats, const int32_t *cell_start, int64_t n_cell_start, const int32_t *cells,
                          int64_t n_cells, int mask_cells, const parc_mdm_draw_t *draws, const parc_mdm_box_t *boxes, const float *noise,
                          float *hfs, float *center_h, float *pre, int32_t *cell_code);

/* Windows.  center_h [n] (may be NULL) is subtracted from every frame's root z before the reference position is (RELATIVE_TO_ROOT_FLOOR
 * with heightfields).  future_time [n], future_noise [n, 3] (already scaled), future_pos [n, 3], future_rot [n, 4]: all four or none.
 *   -> root_pos [n, S, 3], root_rot [n, S, 4], body_pos [n, S, B - 1, 3] (without the root body), joint_rot [n, S, B - 1, 4],
 *      contacts [n, S, B].
 * One lane per (sample, frame), 64 lanes per workgroup; the lane of frame 0 also writes the sample's target. */
int parc_mdm_windows(void *stream, parc_char_model_t model, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids,
                     const float *start_times, const float *motion_times, const float *center_h, const float *future_time,
                     const float *future_noise, float *root_pos, float *root_rot, float *body_pos, float *joint_rot, float *contacts,
                     float *future_pos, float *future_rot);

int parc_mdm_batch_abi(void);

#ifdef __cplusplus
}
#endif
#endif
