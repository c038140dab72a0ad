// parc_render: the offscreen ray caster (include/parc_render.h).  One thread per pixel, 16 x 16 pixels per workgroup, so a 64-lane
// wave covers a compact 16 x 4 tile and its lanes mostly take the same branches.  Per workgroup the view's frame is staged once in
// LDS: camera basis, both characters' primitives in world space (2 x PARC_RENDER_MAX_PRIMS rows of 64 bytes) and one bounding sphere
// per character.  All ray arithmetic is parc_render_core.h, shared with the host build of the tests.
#include <hip/hip_runtime.h>

#include "parc_launch.h"
#include "parc_render_core.h"

using namespace parc_rc;

#define RENDER_TILE 16

__global__ __launch_bounds__(RENDER_TILE * RENDER_TILE) void render_kernel(
    parc_terrain_t ter, parc_render_scene_t sc, const parc_render_view_t *__restrict__ views, int width, int height,
    const float *__restrict__ root_state, const float *__restrict__ rigid_body_state, const float *__restrict__ ref_body_pos,
    const float *__restrict__ ref_body_rot, const float *__restrict__ contact_forces, const float *__restrict__ env_offsets, int n_envs,
    uint32_t *__restrict__ rgba, float *__restrict__ depth, int32_t *__restrict__ ids) {
    __shared__ Frame fr;
    __shared__ WPrim wp[2 * PARC_RENDER_MAX_PRIMS];
    const int tid = threadIdx.y * RENDER_TILE + threadIdx.x;
    const int v = blockIdx.z;
    const parc_render_view_t view = views[v];
    const int e = view_env(view, n_envs);
    const Inputs in = {root_state, rigid_body_state, ref_body_pos, ref_body_rot, contact_forces, env_offsets, n_envs};
    if (tid < n_staged_prims(sc, in)) stage_prim(tid, sc, in, e, wp);
    if (tid == RENDER_TILE * RENDER_TILE - 1) stage_frame(view, ter, sc, in, width, height, wp, fr);
    __syncthreads();
    if (tid < 2) stage_bound(tid, sc, in, e, wp, fr);
    __syncthreads();

    const int px = blockIdx.x * RENDER_TILE + threadIdx.x, py = blockIdx.y * RENDER_TILE + threadIdx.y;
    if (px >= width || py >= height) return;
    uint32_t c;
    float dep;
    int32_t id;
    shade_pixel(fr, px, py, width, height, c, dep, id, nullptr);
    const size_t idx = ((size_t)v * height + py) * width + px;
    rgba[idx] = c;
    if (depth) depth[idx] = dep;
    if (ids) ids[idx] = id;
}

extern "C" int parc_render(void *stream, parc_terrain_t terrain, const parc_render_scene_t *scene, int n_views,
                           const parc_render_view_t *views, int width, int height, const float *root_state, const float *rigid_body_state,
                           const float *ref_body_pos, const float *ref_body_rot, const float *contact_forces, const float *env_offsets,
                           int n_envs, uint32_t *rgba, float *depth, int32_t *ids) {
    const int rc = check_args(terrain, scene, n_views, views, width, height, root_state, rigid_body_state, ref_body_pos, ref_body_rot, contact_forces,
                              env_offsets, n_envs, rgba);
    if (rc != PARC_OK) return rc;
    if (n_views == 0) return PARC_OK;
    const dim3 grid((width + RENDER_TILE - 1) / RENDER_TILE, (height + RENDER_TILE - 1) / RENDER_TILE, n_views);
    hipLaunchKernelGGL(render_kernel, grid, dim3(RENDER_TILE, RENDER_TILE), 0, (hipStream_t)stream, terrain, *scene, views, width, height,
                       root_state, rigid_body_state, ref_body_pos, ref_body_rot, contact_forces, env_offsets, n_envs, rgba, depth, ids);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_render_abi(void) { return 1; }
