// HOST build of the batched motion optimiser's kernel bodies (parc_amd/csrc/parc_moopt_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_motion_opt_batch.py builds it into a temporary directory with the host compiler).  Every moopt_*_host() is the entry point
// of include/parc_moopt.h with host pointers: the same argument check, then the core's per-thread body for every index, in index order;
// the segment sums add in the kernel's order.  With -DMOOPT_HOST_MAIN this is a stand-alone program that runs a case file written by
// tests/tools/moopt_host.py (dump) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_moopt_core.h"

static int done(int rc) { return rc == PARC_MOOPT_NOTHING ? PARC_OK : rc; }

extern "C" int moopt_ragged_host(int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain, int n_terrains,
                                 const parc_moopt_terrain_t *table, const float *pool, int inverted, float radius, float *out, int32_t *out_cell) {
    const int rc = moopt_check_ragged(n_rows, points_per_row, points, row_terrain, n_terrains, table, pool, out);
    if (rc != PARC_OK) return done(rc);
    const size_t n = (size_t)n_rows * points_per_row;
    for (size_t i = 0; i < n; ++i) ragged_thread(i, points_per_row, points, row_terrain, n_terrains, table, pool, inverted, radius, out, out_cell);
    return PARC_OK;
}

extern "C" int moopt_ragged_grad_host(int64_t n_rows, int points_per_row, const float *points, const int32_t *row_terrain, int n_terrains,
                                      const parc_moopt_terrain_t *table, const float *pool, int inverted, const int32_t *cell, const float *g_out,
                                      float *g_points) {
    const int rc = moopt_check_ragged(n_rows, points_per_row, points, row_terrain, n_terrains, table, pool, g_points);
    if (rc != PARC_OK) return done(rc);
    if (!cell || !g_out) return PARC_EINVAL;
    const size_t n = (size_t)n_rows * points_per_row;
    for (size_t i = 0; i < n; ++i) ragged_grad_thread(i, points_per_row, points, row_terrain, n_terrains, table, pool, inverted, cell, g_out, g_points);
    return PARC_OK;
}

extern "C" int moopt_tt_seg_host(int N, int B, int M, const int32_t *seg_start, const int32_t *seg_of_frame, const float *pos, const float *rot_err_sq,
                                 const float *src_vel, const float *keep, const float *pair_contact, float c, float c2, float jerk_limit,
                                 float *partial) {
    const int rc = moopt_check_tt_seg(N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, partial);
    if (rc != PARC_OK) return done(rc);
    for (int i = 0; i < N * B; ++i)
        tt_seg_thread(i, N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, partial);
    return PARC_OK;
}

extern "C" int moopt_tt_seg_grad_host(int N, int B, int M, const int32_t *seg_start, const int32_t *seg_of_frame, const float *pos,
                                      const float *rot_err_sq, const float *src_vel, const float *keep, const float *pair_contact, float c, float c2,
                                      float jerk_limit, const float *cotangents, float *g_pos, float *g_rot_err_sq) {
    const int rc = moopt_check_tt_seg(N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, g_pos);
    if (rc != PARC_OK) return done(rc);
    if (!cotangents || !g_rot_err_sq) return PARC_EINVAL;
    for (int i = 0; i < N * B; ++i)
        tt_seg_grad_thread(i, N, B, M, seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, cotangents,
                           g_pos, g_rot_err_sq);
    return PARC_OK;
}

extern "C" int moopt_segment_sums_host(int n_planes, int n_rows, int width, int n_motions, const int32_t *seg_start, const float *values, float *out) {
    const int rc = moopt_check_segment_sums(n_planes, n_rows, width, n_motions, seg_start, values, out);
    if (rc != PARC_OK) return done(rc);
    for (int p = 0; p < n_planes; ++p)
        for (int m = 0; m < n_motions; ++m) {
            float lanes[PARC_MOOPT_SUM_LANES];
            size_t e0 = 0, e1 = 0;
            const bool any = segsum_block(p, m, n_rows, width, seg_start, e0, e1);
            for (int k = 0; k < PARC_MOOPT_SUM_LANES; ++k) lanes[k] = any ? segsum_lane(values, e0, e1, k) : 0.f;
            out[(size_t)p * n_motions + m] = segsum_fold_host(lanes);
        }
    return PARC_OK;
}

#ifdef MOOPT_HOST_MAIN
// case file: int32 header h[8], float header g[4], then the arrays of the case (tests/tools/moopt_host.py: dump_*):
//   h[0] = 1  temporal terms: h = {1, N, B, M}, g = {c, c2, jerk_limit}; seg_start, seg_of_frame, pos, rot_err_sq, src_vel, keep,
//             pair_contact, cotangents [3, M]                        -> partial, g_pos, g_rot_err_sq
//   h[0] = 2  ragged query:   h = {2, n_rows, points_per_row, n_terrains, inverted, pool floats}, g = {radius}; points, row_terrain, table, pool,
//             g_out                                                   -> out, cell, g_points
//   h[0] = 3  segment sums:   h = {3, n_planes, n_rows, width, n_motions}; seg_start, values   -> out
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
    const std::vector<int32_t> h = rd<int32_t>(f, 8);
    const std::vector<float> g = rd<float>(f, 4);
    const int lim = 1 << 20;
    int rc = 0;
    if (h[0] == 1) {
        const int N = h[1], B = h[2], M = h[3];
        if (N < 0 || N > lim || B <= 0 || B > 64 || M < 0 || M > lim) return 2;
        const size_t n = (size_t)N * B;
        const std::vector<int32_t> ss = rd<int32_t>(f, M + 1), sf = rd<int32_t>(f, N);
        const std::vector<float> pos = rd<float>(f, n * 3), r = rd<float>(f, n), sv = rd<float>(f, n * 3), keep = rd<float>(f, n), pc = rd<float>(f, n),
                                 w = rd<float>(f, (size_t)3 * M);
        std::vector<float> partial(3 * n + 1), g_pos(3 * n + 1), g_r(n + 1);
        rc = moopt_tt_seg_host(N, B, M, ss.data(), sf.data(), pos.data(), r.data(), sv.data(), keep.data(), pc.data(), g[0], g[1], g[2], partial.data());
        if (rc == PARC_OK)
            rc = moopt_tt_seg_grad_host(N, B, M, ss.data(), sf.data(), pos.data(), r.data(), sv.data(), keep.data(), pc.data(), g[0], g[1], g[2], w.data(),
                                        g_pos.data(), g_r.data());
        wr(o, partial, 3 * n);
        wr(o, g_pos, 3 * n);
        wr(o, g_r, n);
    } else if (h[0] == 2) {
        const int R = h[1], K = h[2], nt = h[3], inverted = h[4], pool_n = h[5];
        if (R < 0 || R > lim || K <= 0 || K > lim || nt < 0 || nt > 4096 || pool_n < 0 || pool_n > (1 << 26)) return 2;
        const size_t n = (size_t)R * K;
        const std::vector<float> pts = rd<float>(f, n * 3);
        const std::vector<int32_t> rt = rd<int32_t>(f, R);
        std::vector<parc_moopt_terrain_t> table = rd<parc_moopt_terrain_t>(f, nt);
        const std::vector<float> pool = rd<float>(f, pool_n), g_out = rd<float>(f, n);
        for (const parc_moopt_terrain_t &e : table) {       // the entry points trust the table: a case file must stay inside its pool
            if (e.dim_x <= 0 || e.dim_y <= 0 || e.off_hf < 0 || e.off_x < 0 || e.off_y < 0 || (int64_t)e.off_hf + (int64_t)e.dim_x * e.dim_y > pool_n ||
                (int64_t)e.off_x + e.dim_x > pool_n || (int64_t)e.off_y + e.dim_y > pool_n)
                return 2;
        }
        table.resize(nt + 1);
        std::vector<float> out(n + 1), g_pts(3 * n + 1);
        std::vector<int32_t> cell(n + 1);
        rc = moopt_ragged_host(R, K, pts.data(), rt.data(), nt, table.data(), pool.data(), inverted, g[0], out.data(), cell.data());
        if (rc == PARC_OK)
            rc = moopt_ragged_grad_host(R, K, pts.data(), rt.data(), nt, table.data(), pool.data(), inverted, cell.data(), g_out.data(), g_pts.data());
        wr(o, out, n);
        wr(o, cell, n);
        wr(o, g_pts, 3 * n);
    } else if (h[0] == 3) {
        const int P = h[1], R = h[2], W = h[3], M = h[4];
        if (P < 0 || P > 64 || R < 0 || R > lim || W <= 0 || W > 4096 || M < 0 || M > lim) return 2;
        const std::vector<int32_t> ss = rd<int32_t>(f, M + 1);
        const std::vector<float> values = rd<float>(f, (size_t)P * R * W);
        std::vector<float> out((size_t)P * M + 1);
        rc = moopt_segment_sums_host(P, R, W, M, ss.data(), values.data(), out.data());
        wr(o, out, (size_t)P * M);
    } else {
        return 2;
    }
    fclose(f);
    if (o) fclose(o);
    if (rc != PARC_OK) return 3;
    printf("moopt ok %d\n", h[0]);
    return 0;
}
#endif
