// Terrain-geometry kernels either side of the tracker ("next" rows of the scope table): signed distance of point sets to a
// heightfield seen as a grid of axis-aligned columns.
//
// terrain_util.points_hf_sdf  util/terrain_util.py:1835-1893 of the reference (+ points_boxes_sdf :1774-1804,
// geom_util.sdBox / sdRoundBox  util/geom_util.py:113-143): every heightfield cell (i, j) is a box with centre
// (x_i + cx, y_j + cy) and half extents (dx/2, dy/2); vertically it spans [base_z, hf] - or, "inverted", the AIR column
// [hf, -base_z] above the cell, so that after the final sign flip a point inside the ground gets its (negative) depth to the
// nearest free surface.  The reference materialises [B, N, M, 3] tensors and takes the min over M; here every thread owns one point
// and scans only the window of columns that can hold the minimum (see the kernel): no temporaries, exact result.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_sdf_core.h"      // column_sd, hf_window_min

#define SDF_THREADS 64

// One thread per point.  The minimum over ALL columns is found exactly without visiting all of them: hf_window_min (parc_sdf_core.h) scans
// only the window of columns that can hold it.  Heights come straight from L2 (a heightfield is a few hundred KB).
__global__ __launch_bounds__(SDF_THREADS) void points_hf_sdf_kernel(int n_points, int dim_x, int dim_y, const float *__restrict__ points,
                                                                    const float *__restrict__ hf, const float *__restrict__ min_box_center,
                                                                    const float *__restrict__ x_points, const float *__restrict__ y_points,
                                                                    float half_x, float half_y, float base_z, int inverted, float radius,
                                                                    float *__restrict__ out, int32_t *__restrict__ out_cell) {
    const int bi = blockIdx.y;
    const int p = blockIdx.x * SDF_THREADS + threadIdx.x;
    if (p >= n_points) return;
    const float *pt = points + ((size_t)bi * n_points + p) * 3;
    const float px = pt[0], py = pt[1], pz = pt[2];
    const float *hfb = hf + (size_t)bi * dim_x * dim_y;
    const float ox = min_box_center[2 * bi], oy = min_box_center[2 * bi + 1];
    int best_cell;
    float best = hf_window_min(px, py, pz, hfb, dim_x, dim_y, ox, oy, x_points, y_points, half_x, half_y, base_z, inverted, best_cell);
    if (!(px == px && py == py && pz == pz)) best = __builtin_nanf("");   // a NaN coordinate: torch's abs / clamp / min propagate it, fmaxf / fminf above do not
    if (radius > 0.f) best -= radius;           // sdRoundBox: x - r is monotone, so it commutes with the min
    if (inverted) best = -best;
    out[(size_t)bi * n_points + p] = best;
    if (out_cell) out_cell[(size_t)bi * n_points + p] = best_cell;
}

// Adjoint of the query above with respect to the points: g_points = g_out * d(sd)/dp for the column the forward pass selected
// (out_cell).  The same piecewise expression torch's autograd differentiates in the reference (abs -> sign, clamp(min=0) + norm ->
// unit vector of the positive part, max -> its first arg-max, clamp(max=0) -> passes at <= 0), evaluated once per point.
__global__ __launch_bounds__(SDF_THREADS) void points_hf_sdf_grad_kernel(int n_points, int dim_x, int dim_y, const float *__restrict__ points,
                                                                         const float *__restrict__ hf, const float *__restrict__ min_box_center,
                                                                         const float *__restrict__ x_points, const float *__restrict__ y_points,
                                                                         float half_x, float half_y, float base_z, int inverted,
                                                                         const int32_t *__restrict__ cell, const float *__restrict__ g_out,
                                                                         float *__restrict__ g_points) {
    const int bi = blockIdx.y;
    const int p = blockIdx.x * SDF_THREADS + threadIdx.x;
    if (p >= n_points) return;
    const size_t ip = (size_t)bi * n_points + p;
    const float *pt = points + ip * 3;
    const int ci = cell[ip], i = ci / dim_y, j = ci - i * dim_y;
    const float h = hf[(size_t)bi * dim_x * dim_y + ci];
    const float top_z = -base_z;
    const float cx = x_points[i] + min_box_center[2 * bi], cy = y_points[j] + min_box_center[2 * bi + 1];
    const float cz = inverted ? (h + top_z) / 2.0f : (h + base_z) / 2.0f;
    const float hz = inverted ? (top_z - h) / 2.0f : (h - base_z) / 2.0f;
    const float d[3] = {pt[0] - cx, pt[1] - cy, pt[2] - cz};
    const float q[3] = {fabsf(d[0]) - half_x, fabsf(d[1]) - half_y, fabsf(d[2]) - hz};
    const float a[3] = {fmaxf(q[0], 0.f), fmaxf(q[1], 0.f), fmaxf(q[2], 0.f)};
    const float n = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    float g[3] = {0.f, 0.f, 0.f};
    if (n > 0.f) {
        g[0] = a[0] / n;
        g[1] = a[1] / n;
        g[2] = a[2] / n;
    }
    int km = 0;
    if (q[1] > q[km]) km = 1;
    if (q[2] > q[km]) km = 2;
    if (q[km] <= 0.f) g[km] += 1.0f;
    const float s = (inverted ? -1.0f : 1.0f) * g_out[ip];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float sg = d[k] > 0.f ? 1.0f : (d[k] < 0.f ? -1.0f : 0.0f);
        g_points[ip * 3 + k] = s * g[k] * sg;
    }
}

extern "C" int parc_points_hf_sdf_grad(void *stream, int batch, int n_points, int dim_x, int dim_y, const float *points, const float *hf,
                                       const float *min_box_center, const float *x_points, const float *y_points, float half_x, float half_y,
                                       float base_z, int inverted, const int32_t *cell, const float *g_out, float *g_points) {
    if (batch < 0 || n_points < 0 || dim_x <= 0 || dim_y <= 0) return PARC_EINVAL;
    if (batch == 0 || n_points == 0) return PARC_OK;
    if (batch > 65535) return PARC_EUNSUPPORTED;
    if (!points || !hf || !min_box_center || !x_points || !y_points || !cell || !g_out || !g_points) return PARC_EINVAL;
    hipLaunchKernelGGL(points_hf_sdf_grad_kernel, dim3((n_points + SDF_THREADS - 1) / SDF_THREADS, batch), dim3(SDF_THREADS), 0, (hipStream_t)stream,
                       n_points, dim_x, dim_y, points, hf, min_box_center, x_points, y_points, half_x, half_y, base_z, inverted, cell, g_out, g_points);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_points_hf_sdf(void *stream, int batch, int n_points, int dim_x, int dim_y, const float *points, const float *hf,
                                  const float *min_box_center, const float *x_points, const float *y_points, float half_x, float half_y,
                                  float base_z, int inverted, float radius, float *out, int32_t *out_cell) {
    if (batch < 0 || n_points < 0 || dim_x <= 0 || dim_y <= 0 || (int64_t)dim_x * dim_y > (int64_t)1 << 30) return PARC_EINVAL;
    if (batch == 0 || n_points == 0) return PARC_OK;
    if (batch > 65535) return PARC_EUNSUPPORTED;
    if (!points || !hf || !min_box_center || !x_points || !y_points || !out) return PARC_EINVAL;
    hipLaunchKernelGGL(points_hf_sdf_kernel, dim3((n_points + SDF_THREADS - 1) / SDF_THREADS, batch), dim3(SDF_THREADS), 0, (hipStream_t)stream,
                       n_points, dim_x, dim_y, points, hf, min_box_center, x_points, y_points, half_x, half_y, base_z, inverted, radius, out, out_cell);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}
