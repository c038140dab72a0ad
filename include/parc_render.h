/*
 * parc_render.h -- C-ABI of the offscreen ray-cast renderer inside libparc_hip.so.
 *
 * Stands in for the viewer of the reference (envs/ig_env.py `_render`, envs/ig_char_env.py:512-541 `_init_camera` /
 * `_update_camera`): the simulated character, the reference character (drawn at `ref_char_offset`,
 * envs/ig_parkour/ig_parkour_env.py:577) and the terrain, as image sequences instead of a window.  One launch draws
 * n_views images of width x height pixels straight from the state tensors of the simulator; nothing is read back.
 */
#ifndef PARC_RENDER_H
#define PARC_RENDER_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Primitives per character.  A workgroup stages both characters of its view in LDS: 2 x PARC_RENDER_MAX_PRIMS rows of 64 bytes. */
#define PARC_RENDER_MAX_PRIMS 32

#define PARC_RENDER_SPHERE 0
#define PARC_RENDER_CAPSULE 1
#define PARC_RENDER_BOX 2

/* One collision geom of the MJCF in the frame of its body (64 bytes).
 *   sphere:  a = centre, radius
 *   capsule: a, b = the two ends of the segment, radius
 *   box:     a = centre, b = half extents, q = orientation in the body frame (x y z w) */
typedef struct {
    int32_t body, type;
    float a[3], b[3], radius, q[4];
    float _pad[3];
} parc_render_prim_t;

typedef struct {
    const parc_render_prim_t *prims;   /* DEVICE [n_prims] */
    int32_t n_prims, num_bodies;       /* n_prims <= PARC_RENDER_MAX_PRIMS, 1 <= num_bodies */
    float light_dir[3];                /* direction TOWARD the light (normalised by the kernel) */
    float ambient;                     /* colour = albedo * (ambient + (1 - ambient) * max(n.l, 0) * lit) */
    float sim_color[3], ref_color[3];  /* albedo of the simulated / the reference character, 0..1 */
    float ref_char_offset[3];          /* added to the reference character's body positions */
    int32_t shadows, show_contacts;
    float contact_eps;                 /* show_contacts: bodies with |contact force| > contact_eps are tinted */
} parc_render_scene_t;

#define PARC_RENDER_CAM_STILL 0        /* vec = eye (world), target as given */
#define PARC_RENDER_CAM_TRACK 1        /* vec = (dx, dy, height): eye = (root.xy + env_offset.xy + (dx, dy), height),
                                          target = (root.xy + env_offset.xy, 1.0) -- envs/ig_char_env.py:522-541 */

/* One view (64 bytes).  env outside [0, n_envs) is clamped by the kernel. */
typedef struct {
    int32_t env, mode;
    float fov_y;                       /* vertical field of view, radians */
    float vec[3];
    float target[3];
    float _pad[7];
} parc_render_view_t;

/* Draw n_views images.  One thread per pixel in 16 x 16 workgroups.  The terrain is the column field of hf_lookup: cell (i, j) is
 * centred at min + (i, j) * dx, owns rint((p - min) / dx), has its top at hf[i, j] and vertical walls.  Body poses are in the env
 * frame (env_offsets is added), cameras and the terrain in world coordinates.
 *   rgba  [V,H,W] packed R | G << 8 | B << 16 | 255 << 24
 *   depth [V,H,W] distance along the normalised ray, +inf on a miss (optional)
 *   ids   [V,H,W] -1 miss, b = body b of the simulated character, B + b = of the reference character,
 *                 2B + i * dim_y + j = terrain cell (i, j) (optional)
 * PARC_EINVAL (before any launch): width or height <= 0, n_views < 0 or > 65535 (a view is one z-slice of the grid), n_envs <= 0, NULL scene / views / rgba / rigid_body_state /
 * root_state / env_offsets / scene->prims (with n_prims > 0), only one of ref_body_pos / ref_body_rot, n_prims outside
 * [0, PARC_RENDER_MAX_PRIMS], num_bodies < 1, contact_forces NULL with show_contacts, a terrain with NULL hf or non-positive dx, dy
 * or dims.  n_views == 0: PARC_OK, no launch. */
int parc_render(void *stream, parc_terrain_t terrain, const parc_render_scene_t *scene, int n_views,
                const parc_render_view_t *views, int width, int height, const float *root_state, const float *rigid_body_state,
                const float *ref_body_pos, const float *ref_body_rot, const float *contact_forces, const float *env_offsets,
                int n_envs, uint32_t *rgba, float *depth, int32_t *ids);

int parc_render_abi(void);

#ifdef __cplusplus
}
#endif
#endif
