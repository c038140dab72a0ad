/*
 * parc_augment.h -- C-ABI of the motion-dataset augmentation kernels inside libparc_hip.so.
 *
 * V variants of a few seed clips are built on the device (tools/motion_opt/augment_motions.prepare_variants): a window of a clip is
 * turned by a heading and stretched in x and y, the terrain under it is cut out of the (virtually padded) source terrain, re-centred
 * on the first frame, and its heights are scaled or stamped with rotated boxes along the path.  The arithmetic is in
 * parc_amd/csrc/parc_augment_core.h.  No allocation, host read, wait or atomic inside; vector stores only.
 *
 * Every entry point answers in this order: PARC_EINVAL (before any HIP call) for a negative count; PARC_OK with nothing launched for
 * zero variants; PARC_EINVAL for a NULL required pointer.  The tables are trusted for nothing: every index derived from them is
 * clamped before its load, and a variant whose table row points outside its arrays gets NaN outputs (it alone).
 */
#ifndef PARC_AUGMENT_H
#define PARC_AUGMENT_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_AUG_FRAME_DIM 34 /* root pos 3 | root exp-map 3 | dofs 28 */

/* terrain modes (c) of a variant */
#define PARC_AUG_NONE 0
#define PARC_AUG_HEIGHT_SCALE 1
#define PARC_AUG_BOXES_ALONG_PATH 2

/* One variant's frames: rows src_off + start .. + length - 1 of the packed source (the clip owns rows src_off .. src_off + src_len - 1)
 * become rows out_off .. out_off + length - 1 of the packed output.  (cos_h, sin_h) turn xy; (qz, qw) is the heading quaternion
 * axis_angle_to_quat(z, heading) that multiplies the root rotation from the left; then x *= sx, y *= sy. */
typedef struct {
    int32_t src_off, src_len;
    int32_t start, length;
    int32_t out_off;
    float cos_h, sin_h;
    float qz, qw;
    float sx, sy;
} parc_augment_frames_t;

/* One heightfield over float pools: heights at pool[off_hf + i * dim_y + j]; cell (i, j) of an OUTPUT grid is looked up at
 * (points[off_x + i], points[off_y + j]); (min_x, min_y) is the centre of cell (0, 0), (dx, dy) the cell size. */
typedef struct {
    int32_t off_hf, off_x, off_y;
    int32_t dim_x, dim_y;
    float min_x, min_y;
    float dx, dy;
} parc_augment_terrain_t;

/* One variant's terrain: source id, `pad` cells of height 0 around the source, mode and its scale or boxes
 * (boxes[box_off .. box_off + box_count - 1], in order: the last box that contains a cell sets its height), and the variant's rows
 * frame_off .. frame_off + frame_len - 1 of the packed transformed frames.  slice = 0: the output grid IS the padded source grid
 * (cell (i, j) is padded cell (i, j)), nothing is re-centred and canon is 0. */
typedef struct {
    int32_t src, pad, mode, slice;
    int32_t box_off, box_count;
    int32_t frame_off, frame_len;
    float scale;
} parc_augment_variant_t;

/* A box in grid-index space of the variant's output grid, centred under frame frame_ind of the variant. */
typedef struct {
    int32_t frame_ind;
    float len_x, len_y;
    float angle, cos_a, sin_a; /* cos_a, sin_a: cos / sin of angle as the caller's reference evaluates them */
    float h;
} parc_augment_box_t;

/* Frames.  src_frames [n_src_rows, 34], src_contacts [n_src_rows, contact_width], vars [n_variants] (DEVICE)
 *   -> out_frames [n_out_rows, 34], out_contacts [n_out_rows, contact_width], bounds [n_variants, 4] = min x, min y, max x, max y of the
 * transformed frames.  z and the dofs (and the contacts) are copied bit for bit.  A NaN x or y makes the variant's bounds NaN.  A
 * variant whose window leaves its clip or the source (or with length <= 0) gets NaN frames, contacts and bounds; rows outside
 * [0, n_out_rows) are never written.  One workgroup per variant. */
int parc_augment_frames(void *stream, int n_variants, int n_src_rows, int contact_width, const float *src_frames, const float *src_contacts,
                        const parc_augment_frames_t *vars, int n_out_rows, float *out_frames, float *out_contacts, float *bounds);

/* Terrains.  One value per output cell; cell_start [n_variants + 1] int64 (DEVICE) is the running sum of the variants' dim_x * dim_y and
 * n_cells = cell_start[n_variants] is given by the caller.  src_table [n_sources] over src_pool [src_pool_floats]; out_table [n_variants]:
 * heights go to out_pool [out_pool_floats] at off_hf, the grid's x and y points are read from points [points_floats] at off_x / off_y.
 * frames [n_rows, 34] are the transformed frames BEFORE parc_augment_localize.  canon [n_variants, 3] = first frame's x, y and the height
 * under it (0, 0, 0 for slice = 0).  A source id outside [0, n_sources), a frame range or box range outside its array, or a box whose
 * frame index lies outside the variant gives NaN heights and NaN canon for that variant only.  One thread per cell, flat index. */
int parc_augment_terrains(void *stream, int n_variants, int64_t n_cells, const int64_t *cell_start, const parc_augment_variant_t *vars,
                          int n_sources, const parc_augment_terrain_t *src_table, const float *src_pool, int64_t src_pool_floats,
                          const parc_augment_terrain_t *out_table, const float *points, int64_t points_floats, const parc_augment_box_t *boxes,
                          int n_boxes, const float *frames, int n_rows, float *out_pool, int64_t out_pool_floats, float *canon);

/* Localise (slice_terrain_around_motion, localize=True): for every variant with slice != 0, xy of each of its frames -= canon xy,
 * z -= canon z, and (when hf_table is not NULL) hf_table[v].ox / .oy -= canon xy: hf_table is the parc_moopt_terrain_t table
 * (include/parc_moopt.h) the batched optimiser reads.  One workgroup per variant. */
int parc_augment_localize(void *stream, int n_variants, const parc_augment_variant_t *vars, const float *canon, float *frames, int n_rows,
                          void *hf_table);

int parc_augment_abi(void);

#ifdef __cplusplus
}
#endif
#endif
