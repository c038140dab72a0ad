// HOST build of the dataset augmentation's kernel bodies (parc_amd/csrc/parc_augment_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_augment.py builds it into a temporary directory with the host compiler, -ffp-contract=off).  Every augment_*_host() is the
// entry point of include/parc_augment.h with host pointers: the same argument check, then the core's per-lane / per-thread body for
// every index.  With -DAUGMENT_HOST_MAIN this is a stand-alone program that runs a case file written by tests/tools/augment_host.py
// (dump) through all three entry points - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_augment_core.h"

using namespace parc_aug;

static int done(int rc) { return rc == PARC_AUG_NOTHING ? PARC_OK : rc; }

extern "C" int augment_frames_host(int n_variants, int n_src_rows, int contact_width, const float *src_frames, const float *src_contacts,
                                   const parc_augment_frames_t *vars, int n_out_rows, float *out_frames, float *out_contacts, float *bounds) {
    const int rc = check_frames(n_variants, n_src_rows, contact_width, src_frames, src_contacts, vars, n_out_rows, out_frames, out_contacts, bounds);
    if (rc != PARC_OK) return done(rc);
    for (int v = 0; v < n_variants; ++v) {
        Bounds b = bounds_empty();
        for (int lane = 0; lane < PARC_AUG_THREADS; ++lane)
            bounds_merge(b, frames_lane(vars[v], lane, PARC_AUG_THREADS, n_src_rows, contact_width, src_frames, src_contacts, n_out_rows, out_frames,
                                        out_contacts));
        bounds_store(b, bounds + (size_t)v * 4);
    }
    return PARC_OK;
}

extern "C" int augment_terrains_host(int n_variants, int64_t n_cells, const int64_t *cell_start, const parc_augment_variant_t *vars, int n_sources,
                                     const parc_augment_terrain_t *src_table, const float *src_pool, int64_t src_pool_floats,
                                     const parc_augment_terrain_t *out_table, const float *points, int64_t points_floats,
                                     const parc_augment_box_t *boxes, int n_boxes, const float *frames, int n_rows, float *out_pool,
                                     int64_t out_pool_floats, float *canon) {
    const int rc = check_terrains(n_variants, n_cells, cell_start, vars, n_sources, src_table, src_pool, src_pool_floats, out_table, points,
                                  points_floats, boxes, n_boxes, frames, n_rows, out_pool, out_pool_floats, canon);
    if (rc != PARC_OK) return done(rc);
    for (int64_t cell = 0; cell < n_cells; ++cell)
        terrain_thread(cell, n_variants, cell_start, vars, n_sources, src_table, src_pool, src_pool_floats, out_table, points, points_floats, boxes,
                       n_boxes, frames, n_rows, out_pool, out_pool_floats, canon);
    return PARC_OK;
}

extern "C" int augment_localize_host(int n_variants, const parc_augment_variant_t *vars, const float *canon, float *frames, int n_rows, void *hf_table) {
    const int rc = check_localize(n_variants, vars, canon, frames, n_rows);
    if (rc != PARC_OK) return done(rc);
    for (int v = 0; v < n_variants; ++v)
        for (int lane = 0; lane < PARC_AUG_THREADS; ++lane)
            localize_lane(vars[v], v, lane, PARC_AUG_THREADS, canon, frames, n_rows, (parc_moopt_terrain_t *)hf_table);
    return PARC_OK;
}

#ifdef AUGMENT_HOST_MAIN
// case file (tests/tools/augment_host.py: dump): int64 header h[12] = {V, n_src_rows, contact_width, n_out_rows, n_sources, src_pool_floats,
// out_floats, points_floats, n_boxes, n_cells, 0, 0}, then src_frames, src_contacts, frames table [V], src_table [n_sources], src_pool,
// out_table [V], variant table [V], boxes [n_boxes], cell_start [V + 1], pool [out_floats + points_floats], hf table [V].
// output: out_frames, out_contacts, bounds, pool[:out_floats], canon, hf table.
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

template <class T>
static void wr(FILE *o, const std::vector<T> &v, size_t n) {
    if (o && n) fwrite(v.data(), sizeof(T), n, o);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !o) return 2;
    const std::vector<int64_t> h = rd<int64_t>(f, 12);
    const int64_t lim = 1 << 24;
    for (int k = 0; k < 10; ++k)
        if (h[k] < 0 || h[k] > lim) return 2;
    const int V = (int)h[0], n_src = (int)h[1], C = (int)h[2], n_out = (int)h[3], S = (int)h[4], n_boxes = (int)h[8];
    const int64_t src_pool_n = h[5], out_n = h[6], pts_n = h[7], n_cells = h[9];
    if (C > 64) return 2;
    const std::vector<float> src_frames = rd<float>(f, (size_t)n_src * PARC_AUG_FRAME_DIM), src_contacts = rd<float>(f, (size_t)n_src * C);
    const std::vector<parc_augment_frames_t> ft = rd<parc_augment_frames_t>(f, V);
    const std::vector<parc_augment_terrain_t> st = rd<parc_augment_terrain_t>(f, S);
    const std::vector<float> src_pool = rd<float>(f, src_pool_n);
    const std::vector<parc_augment_terrain_t> ot = rd<parc_augment_terrain_t>(f, V);
    const std::vector<parc_augment_variant_t> vt = rd<parc_augment_variant_t>(f, V);
    const std::vector<parc_augment_box_t> boxes = rd<parc_augment_box_t>(f, n_boxes);
    const std::vector<int64_t> cell_start = rd<int64_t>(f, (size_t)V + 1);
    std::vector<float> pool = rd<float>(f, (size_t)(out_n + pts_n));
    std::vector<parc_moopt_terrain_t> hft = rd<parc_moopt_terrain_t>(f, V);
    if (V > 0 && cell_start[V] != n_cells) return 2;
    for (int v = 0; v < V; ++v)
        if (cell_start[v] < 0 || cell_start[v] > cell_start[v + 1]) return 2;        // the running sum is trusted to ascend
    // exactly-sized vectors: an access one element too far is an error under the sanitizer
    std::vector<float> frames((size_t)n_out * PARC_AUG_FRAME_DIM), contacts((size_t)n_out * C), bounds((size_t)V * 4), canon((size_t)V * 3);
    std::vector<float> points(pool.begin() + out_n, pool.end());
    pool.resize(out_n);
    pool.shrink_to_fit();
    int rc = augment_frames_host(V, n_src, C, src_frames.data(), src_contacts.data(), ft.data(), n_out, frames.data(), contacts.data(), bounds.data());
    if (rc == PARC_OK)
        rc = augment_terrains_host(V, n_cells, cell_start.data(), vt.data(), S, st.data(), src_pool.data(), src_pool_n, ot.data(), points.data(), pts_n,
                                   boxes.data(), n_boxes, frames.data(), n_out, pool.data(), out_n, canon.data());
    if (rc == PARC_OK) rc = augment_localize_host(V, vt.data(), canon.data(), frames.data(), n_out, hft.data());
    wr(o, frames, frames.size());
    wr(o, contacts, contacts.size());
    wr(o, bounds, bounds.size());
    wr(o, pool, pool.size());
    wr(o, canon, canon.size());
    wr(o, hft, hft.size());
    fclose(f);
    if (o) fclose(o);
    if (rc != PARC_OK) return 3;
    printf("augment ok %d\n", V);
    return 0;
}
#endif
