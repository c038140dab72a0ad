// Signed distance of one point to a heightfield seen as a grid of axis-aligned columns: the column distance and the window scan of
// points_hf_sdf_kernel (parc_terrain.hip), shared with the motion scorer (parc_score_core.h).  Compiles for the device (hipcc) and for
// the host (g++: the CPU tests of the scorer).
//
// terrain_util.points_hf_sdf  util/terrain_util.py:1835-1893 of the reference: every heightfield cell (i, j) is a box with centre
// (x_i + cx, y_j + cy) and half extents (dx/2, dy/2); vertically it spans [base_z, hf] - or, "inverted", the AIR column [hf, -base_z].
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PARC_SDF_FN __device__ __forceinline__
#define PARC_SDF_SQRT(x) __fsqrt_rn(x)
#define PARC_SDF_IMAX(a, b) max(a, b)
#define PARC_SDF_IMIN(a, b) min(a, b)
#else
#define PARC_SDF_FN static inline
#define PARC_SDF_SQRT(x) sqrtf(x)
#define PARC_SDF_IMAX(a, b) ((a) > (b) ? (a) : (b))
#define PARC_SDF_IMIN(a, b) ((a) < (b) ? (a) : (b))
#endif

// sdBox of one column: q = |p - centre| - half extents; |max(q, 0)| + min(max(q.x, q.y, q.z), 0), same fp32 operations as the
// reference (:1862-1871)
PARC_SDF_FN float column_sd(float px, float py, float pz, float cx, float cy, float h, float half_x, float half_y, float base_z,
                            float top_z, int inverted) {
    const float cz = inverted ? (h + top_z) / 2.0f : (h + base_z) / 2.0f;
    const float hz = inverted ? (top_z - h) / 2.0f : (h - base_z) / 2.0f;
    const float qx = fabsf(px - cx) - half_x, qy = fabsf(py - cy) - half_y, qz = fabsf(pz - cz) - hz;
    const float ax = fmaxf(qx, 0.f), ay = fmaxf(qy, 0.f), az = fmaxf(qz, 0.f);
    return PARC_SDF_SQRT(ax * ax + ay * ay + az * az) + fminf(fmaxf(qx, fmaxf(qy, qz)), 0.f);
}

// The minimum over ALL columns of one heightfield hfb [dim_x, dim_y], found exactly without visiting all of them: the distance d0 to the
// column under the point bounds the answer, and a column more than R = floor(d0 / cell) + 2 cells away in x or in y is further than d0
// in that coordinate alone (columns do not overlap in xy), so only the (2R+1)^2 window is scanned - in the same cell order as a full
// scan, so "first column that attains the minimum" is the same column.  Every index is clamped to the grid before a load.  NaN
// coordinates: fmaxf / fminf drop them, the result is then some finite number - the caller flags such points itself.
PARC_SDF_FN float hf_window_min(float px, float py, float pz, const float *__restrict__ hfb, int dim_x, int dim_y, float ox, float oy,
                                const float *__restrict__ x_points, const float *__restrict__ y_points, float half_x, float half_y,
                                float base_z, int inverted, int &best_cell) {
    const float top_z = -base_z;
    const float cell_x = 2.0f * half_x, cell_y = 2.0f * half_y;
    // NaN / inf coordinates: the comparisons below are all false for NaN, so the window degenerates to the whole field
    const float fi = rintf((px - ox) / cell_x), fj = rintf((py - oy) / cell_y);
    const int i0 = (int)fminf(fmaxf(fi, 0.f), (float)(dim_x - 1)), j0 = (int)fminf(fmaxf(fj, 0.f), (float)(dim_y - 1));
    const float d0 = column_sd(px, py, pz, x_points[i0] + ox, y_points[j0] + oy, hfb[i0 * dim_y + j0], half_x, half_y, base_z, top_z, inverted);
    int i_lo = 0, i_hi = dim_x - 1, j_lo = 0, j_hi = dim_y - 1;
    if (d0 < 3.0e8f) {              // also false for NaN
        const float bound = fmaxf(d0, 0.f);
        const int rx = (int)(bound / cell_x) + 2, ry = (int)(bound / cell_y) + 2;
        i_lo = PARC_SDF_IMAX(i0 - rx, 0);
        i_hi = PARC_SDF_IMIN(i0 + rx, dim_x - 1);
        j_lo = PARC_SDF_IMAX(j0 - ry, 0);
        j_hi = PARC_SDF_IMIN(j0 + ry, dim_y - 1);
    }
    float best = INFINITY;
    best_cell = 0;
    for (int i = i_lo; i <= i_hi; ++i) {
        const float cx = x_points[i] + ox;
        const float *row = hfb + (size_t)i * dim_y;
        for (int j = j_lo; j <= j_hi; ++j) {
            const float sd = column_sd(px, py, pz, cx, y_points[j] + oy, row[j], half_x, half_y, base_z, top_z, inverted);
            if (sd < best) {             // first column that attains the minimum
                best = sd;
                best_cell = i * dim_y + j;
            }
        }
    }
    return best;
}
