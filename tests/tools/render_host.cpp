// HOST build of the ray caster (parc_amd/csrc/parc_render_core.h) -- TEST INFRASTRUCTURE ONLY (tests/test_render.py builds it into a
// temporary directory with the host compiler).  render_host() is parc_render with host pointers everywhere: the same argument check, the
// kernel's own staging pieces (stage_prim / stage_frame / stage_bound) run once per view, then the core's shade_pixel per pixel.  `normals` [V,H,W,3] (optional) receives
// the shading normal.  With -DRENDER_HOST_MAIN this is a stand-alone program that renders a scene file written by
// tests/tools/render_host.py (dump_scene) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_render_core.h"

using namespace parc_rc;

extern "C" int render_host(parc_terrain_t ter, const parc_render_scene_t *scene, int n_views, const parc_render_view_t *views, int width,
                           int height, const float *root_state, const float *rigid_body_state, const float *ref_body_pos,
                           const float *ref_body_rot, const float *contact_forces, const float *env_offsets, int n_envs, uint32_t *rgba,
                           float *depth, int32_t *ids, float *normals) {
    const int rc = check_args(ter, scene, n_views, views, width, height, root_state, rigid_body_state, ref_body_pos, ref_body_rot, contact_forces,
                              env_offsets, n_envs, rgba);
    if (rc != PARC_OK) return rc;
    const parc_render_scene_t &sc = *scene;
    const Inputs in = {root_state, rigid_body_state, ref_body_pos, ref_body_rot, contact_forces, env_offsets, n_envs};
    for (int v = 0; v < n_views; ++v) {
        WPrim wp[2 * PARC_RENDER_MAX_PRIMS];
        Frame fr;
        const parc_render_view_t view = views[v];
        const int e = view_env(view, n_envs);
        for (int k = 0; k < n_staged_prims(sc, in); ++k) stage_prim(k, sc, in, e, wp);
        stage_frame(view, ter, sc, in, width, height, wp, fr);
        for (int c = 0; c < 2; ++c) stage_bound(c, sc, in, e, wp, fr);
        for (int py = 0; py < height; ++py)
            for (int px = 0; px < width; ++px) {
                const size_t idx = ((size_t)v * height + py) * width + px;
                uint32_t col;
                float dep;
                int32_t id;
                shade_pixel(fr, px, py, width, height, col, dep, id, normals ? normals + 3 * idx : nullptr);
                rgba[idx] = col;
                if (depth) depth[idx] = dep;
                if (ids) ids[idx] = id;
            }
    }
    return PARC_OK;
}

#ifdef RENDER_HOST_MAIN
// scene file: int32 header {width, height, n_views, n_envs, has_ref, has_cf, dim_x, dim_y}, float {min_x, min_y, dx, dy}, the scene struct
// (its pointer field is ignored), then prims, views, hf, root_state, rigid_body_state, [ref_body_pos, ref_body_rot], [contact_forces], env_offsets
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short scene file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 8);
    const std::vector<float> g = rd<float>(f, 4);
    std::vector<parc_render_scene_t> sc = rd<parc_render_scene_t>(f, 1);
    const int W = h[0], H = h[1], V = h[2], N = h[3], B = sc[0].num_bodies;
    if (W <= 0 || H <= 0 || V < 0 || N <= 0 || B <= 0 || W > 4096 || H > 4096 || V > 64 || sc[0].n_prims < 0 || sc[0].n_prims > PARC_RENDER_MAX_PRIMS ||
        h[6] <= 0 || h[7] <= 0)
        return 2;
    const std::vector<parc_render_prim_t> prims = rd<parc_render_prim_t>(f, sc[0].n_prims);
    const std::vector<parc_render_view_t> views = rd<parc_render_view_t>(f, V);
    const std::vector<float> hf = rd<float>(f, (size_t)h[6] * h[7]);
    const std::vector<float> root = rd<float>(f, (size_t)N * 13), rbs = rd<float>(f, (size_t)N * B * 13);
    const std::vector<float> rpos = rd<float>(f, h[4] ? (size_t)N * B * 3 : 0), rrot = rd<float>(f, h[4] ? (size_t)N * B * 4 : 0);
    const std::vector<float> cf = rd<float>(f, h[5] ? (size_t)N * B * 3 : 0), off = rd<float>(f, (size_t)N * 3);
    fclose(f);
    sc[0].prims = prims.data();
    const parc_terrain_t ter = {hf.data(), h[6], h[7], g[0], g[1], g[2], g[3]};
    std::vector<uint32_t> rgba((size_t)V * H * W);
    std::vector<float> depth((size_t)V * H * W), normals((size_t)V * H * W * 3);
    std::vector<int32_t> ids((size_t)V * H * W);
    const int rc = render_host(ter, &sc[0], V, views.data(), W, H, root.data(), rbs.data(), h[4] ? rpos.data() : nullptr, h[4] ? rrot.data() : nullptr,
                               h[5] ? cf.data() : nullptr, off.data(), N, rgba.data(), depth.data(), ids.data(), normals.data());
    if (rc != PARC_OK) return 3;
    uint64_t sum = 0;
    for (size_t k = 0; k < rgba.size(); ++k) sum = sum * 1099511628211ull + rgba[k] + (uint32_t)ids[k];
    if (argc > 2) {       // the images, for the caller to compare with the plain build's
        FILE *o = fopen(argv[2], "wb");
        if (!o) return 2;
        fwrite(rgba.data(), 4, rgba.size(), o);
        fwrite(ids.data(), 4, ids.size(), o);
        fwrite(depth.data(), 4, depth.size(), o);
        fclose(o);
    }
    printf("render ok %llu\n", (unsigned long long)sum);
    return 0;
}
#endif
