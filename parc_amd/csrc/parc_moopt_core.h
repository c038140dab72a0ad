// Bodies of the motion optimiser's kernels, shared by the device (hipcc: parc_pose_opt.hip, parc_moopt.hip) and the host (g++: the CPU
// tests, tests/tools/moopt_host.cpp):
//   * the frame-to-frame terms of stage 2's motion loss and their adjoint (tt_*), for one motion (parc_temporal_terms) and for motions
//     packed along the frame axis (parc_temporal_terms_seg);
//   * the terrain query with a terrain per row (ragged_*), on hf_window_min of parc_sdf_core.h;
//   * the per-motion fold of per-frame partials (segsum_*).
// Every "thread" function is what one device thread does for one index; the host build calls it in a loop.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/parc_moopt.h"
#include "parc_sdf_core.h"

#include "parc_rot.h"       // v3, ld3, st3, mk3, dot3

#if defined(__HIPCC__)
#define PARC_MO_FN __device__ __forceinline__
#else
#define PARC_MO_FN static inline
#endif

// ---------------------------------------------------------------------------------------------------------------------------------
// The frame-to-frame terms of stage 2's motion loss (tools/motion_opt/motion_optimization.py:215-224,346-362) per (frame, body), and
// their adjoint: smoothness |v - v_src|^2 + r, sliding (pseudo-Huber of the same errors where the constraint mask keeps them, times the
// contact of the frame pair), jerk max(|third difference| - limit, 0); v = p[t+1] - p[t], r = squared rotation-speed error (an input).
// Forward gives the three partial terms per (t, b) (summed by one reduction afterwards); backward gathers, per (t, b), the
// contributions of the (at most) two velocity errors and four third differences that contain p[t, b] - no atomics.
// ---------------------------------------------------------------------------------------------------------------------------------
struct tt_args { float c, c2, jerk_limit; };

PARC_MO_FN v3 tt_vel_err(const float *__restrict__ pos, const float *__restrict__ src_vel, int B, int t, int b) {
    return (ld3(pos + ((size_t)(t + 1) * B + b) * 3) - ld3(pos + ((size_t)t * B + b) * 3)) - ld3(src_vel + ((size_t)t * B + b) * 3);
}
PARC_MO_FN v3 tt_third_diff(const float *__restrict__ pos, int B, int t, int b) {
    const v3 p0 = ld3(pos + ((size_t)t * B + b) * 3), p1 = ld3(pos + ((size_t)(t + 1) * B + b) * 3), p2 = ld3(pos + ((size_t)(t + 2) * B + b) * 3),
             p3 = ld3(pos + ((size_t)(t + 3) * B + b) * 3);
    return ((p3 - p2) - (p2 - p1)) - ((p2 - p1) - (p1 - p0));      // (a[t+1] - a[t]) of the velocities' differences, like the torch expression
}

// the three partial terms of (t, b) of ONE motion of T frames; every pointer is the motion's first row, i = t * B + b
PARC_MO_FN void tt_forward_body(int T, int B, int t, int b, int i, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                              const float *__restrict__ src_vel, const float *__restrict__ keep, const float *__restrict__ pair_contact, tt_args a,
                              float &sm, float &sl, float &jl) {
    sm = 0.f, sl = 0.f, jl = 0.f;
    if (t < T - 1) {
        const v3 e = tt_vel_err(pos, src_vel, B, t, b);
        const float e2 = (e.x * e.x + e.y * e.y) + e.z * e.z, r = rot_err_sq[i], k = keep[i], pc = pair_contact[i];
        sm = e2 + r;
        sl = (sqrtf(k * e2 + a.c2) - a.c) * pc + (sqrtf(k * r + a.c2) - a.c) * pc;
    }
    if (t < T - 3) {
        const v3 j = tt_third_diff(pos, B, t, b);
        jl = fmaxf(sqrtf(dot3(j, j)) - a.jerk_limit, 0.f);
    }
}

// adjoint at (t, b) of ONE motion of T frames for the cotangents (w0, w1, w2) of its three sums: returns the gradient of p[t, b];
// g_r is written for t < T - 1 only (has_r tells)
PARC_MO_FN v3 tt_backward_body(int T, int B, int t, int b, int i, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                             const float *__restrict__ src_vel, const float *__restrict__ keep, const float *__restrict__ pair_contact, tt_args a,
                             float w0, float w1, float w2, float &g_r, bool &has_r) {
    v3 g = mk3(0.f, 0.f, 0.f);
    // velocity errors of the pairs (t-1, t) [+] and (t, t+1) [-]
    for (int k = 0; k < 2; ++k) {
        const int tp = t - 1 + k;
        if (tp < 0 || tp >= T - 1) continue;
        const v3 e = tt_vel_err(pos, src_vel, B, tp, b);
        const float e2 = (e.x * e.x + e.y * e.y) + e.z * e.z;
        const size_t ip = (size_t)tp * B + b;
        const float f = (k == 0 ? 1.f : -1.f) * (2.f * w0 + w1 * pair_contact[ip] * keep[ip] / sqrtf(keep[ip] * e2 + a.c2));
        g = g + f * e;
    }
    // third differences j[t-3] (+1), j[t-2] (-3), j[t-1] (+3), j[t] (-1)
    const float coef[4] = {1.f, -3.f, 3.f, -1.f};
    for (int k = 0; k < 4; ++k) {
        const int tj = t - 3 + k;
        if (tj < 0 || tj >= T - 3) continue;
        const v3 j = tt_third_diff(pos, B, tj, b);
        const float jn = sqrtf(dot3(j, j));
        if (jn - a.jerk_limit >= 0.f && jn > 0.f) g = g + (w2 * coef[k] / jn) * j;
    }
    has_r = t < T - 1;
    if (has_r) g_r = w0 + w1 * pair_contact[i] * keep[i] / (2.f * sqrtf(keep[i] * rot_err_sq[i] + a.c2));
    return g;
}

// The motion of packed frame f: its id m, first frame s and length T, checked against the tables (a frame the tables do not cover
// reads nothing).
PARC_MO_FN bool tt_seg_of(int f, int N, int M, const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_of_frame, int &m, int &s,
                        int &T) {
    m = seg_of_frame[f];
    if (m < 0 || m >= M) return false;
    s = seg_start[m];
    const int e = seg_start[m + 1];
    T = e - s;
    return s >= 0 && e <= N && f >= s && f < e;
}

// thread i of parc_temporal_terms_seg: (frame, body) i of the packed [N, B] grid
PARC_MO_FN void tt_seg_thread(int i, int N, int B, int M, const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_of_frame,
                            const float *__restrict__ pos, const float *__restrict__ rot_err_sq, const float *__restrict__ src_vel,
                            const float *__restrict__ keep, const float *__restrict__ pair_contact, tt_args a, float *partial) {
    const int f = i / B, b = i - f * B;
    float sm = 0.f, sl = 0.f, jl = 0.f;
    int m, s, T;
    if (tt_seg_of(f, N, M, seg_start, seg_of_frame, m, s, T)) {
        const size_t o = (size_t)s * B;
        const int t = f - s;
        tt_forward_body(T, B, t, b, t * B + b, pos + o * 3, rot_err_sq + o, src_vel + o * 3, keep + o, pair_contact + o, a, sm, sl, jl);
    }
    const size_t n = (size_t)N * B;
    partial[i] = sm;
    partial[n + i] = sl;
    partial[2 * n + i] = jl;
}

// thread i of parc_temporal_terms_seg_grad; w [3, M]: cotangents of the three sums of every motion
PARC_MO_FN void tt_seg_grad_thread(int i, int N, int B, int M, const int32_t *__restrict__ seg_start, const int32_t *__restrict__ seg_of_frame,
                                 const float *__restrict__ pos, const float *__restrict__ rot_err_sq, const float *__restrict__ src_vel,
                                 const float *__restrict__ keep, const float *__restrict__ pair_contact, tt_args a, const float *__restrict__ w,
                                 float *g_pos, float *g_rot_err_sq) {
    const int f = i / B, b = i - f * B;
    v3 g = mk3(0.f, 0.f, 0.f);
    float g_r = 0.f;
    int m, s, T;
    if (tt_seg_of(f, N, M, seg_start, seg_of_frame, m, s, T)) {
        const size_t o = (size_t)s * B;
        const int t = f - s;
        bool has_r;
        float r = 0.f;
        g = tt_backward_body(T, B, t, b, t * B + b, pos + o * 3, rot_err_sq + o, src_vel + o * 3, keep + o, pair_contact + o, a, w[m], w[M + m],
                             w[2 * M + m], r, has_r);
        if (has_r) g_r = r;
    }
    st3(g_pos + (size_t)i * 3, g);
    g_rot_err_sq[i] = g_r;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Terrain query with a terrain per row
// ---------------------------------------------------------------------------------------------------------------------------------
// point idx of the flat [n_rows * points_per_row] grid: value and arg-min column by the rules of points_hf_sdf_kernel
PARC_MO_FN void ragged_thread(size_t idx, int points_per_row, const float *__restrict__ points, const int32_t *__restrict__ row_terrain,
                            int n_terrains, const parc_moopt_terrain_t *__restrict__ table, const float *__restrict__ pool, int inverted,
                            float radius, float *__restrict__ out, int32_t *__restrict__ out_cell) {
    const size_t row = idx / (size_t)points_per_row;
    const int ti = row_terrain[row];
    float best = __builtin_nanf("");
    int best_cell = -1;
    if (ti >= 0 && ti < n_terrains) {
        const parc_moopt_terrain_t e = table[ti];
        const float *pt = points + idx * 3;
        const float px = pt[0], py = pt[1], pz = pt[2];
        best = hf_window_min(px, py, pz, pool + e.off_hf, e.dim_x, e.dim_y, e.ox, e.oy, pool + e.off_x, pool + e.off_y, e.half_x, e.half_y, e.base_z,
                             inverted, best_cell);
        if (!(px == px && py == py && pz == pz)) best = __builtin_nanf("");   // a NaN coordinate: torch's abs / clamp / min propagate it, fmaxf / fminf do not
        if (radius > 0.f) best -= radius;           // sdRoundBox: x - r is monotone, so it commutes with the min
        if (inverted) best = -best;
    }
    out[idx] = best;
    if (out_cell) out_cell[idx] = best_cell;
}

// Adjoint at point idx: the piecewise expression of points_hf_sdf_grad_kernel (abs -> sign, clamp(min=0) + norm -> unit vector of the
// positive part, max -> its first arg-max, clamp(max=0) -> passes at <= 0) for the column the forward pass selected.
PARC_MO_FN void ragged_grad_thread(size_t idx, int points_per_row, const float *__restrict__ points, const int32_t *__restrict__ row_terrain,
                                 int n_terrains, const parc_moopt_terrain_t *__restrict__ table, const float *__restrict__ pool, int inverted,
                                 const int32_t *__restrict__ cell, const float *__restrict__ g_out, float *__restrict__ g_points) {
    const size_t row = idx / (size_t)points_per_row;
    const int ti = row_terrain[row];
    const int ci = cell[idx];
    float o[3] = {0.f, 0.f, 0.f};
    if (ti >= 0 && ti < n_terrains) {
        const parc_moopt_terrain_t e = table[ti];
        if (ci >= 0 && ci < e.dim_x * e.dim_y) {
            const float *pt = points + idx * 3;
            const int i = ci / e.dim_y, j = ci - i * e.dim_y;
            const float h = pool[e.off_hf + ci];
            const float base_z = e.base_z, top_z = -base_z, half_x = e.half_x, half_y = e.half_y;
            const float cx = pool[e.off_x + i] + e.ox, cy = pool[e.off_y + j] + e.oy;
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
            const float s = (inverted ? -1.0f : 1.0f) * g_out[idx];
            for (int k = 0; k < 3; ++k) {
                const float sg = d[k] > 0.f ? 1.0f : (d[k] < 0.f ? -1.0f : 0.0f);
                o[k] = s * g[k] * sg;
            }
        }
    }
    g_points[idx * 3 + 0] = o[0];
    g_points[idx * 3 + 1] = o[1];
    g_points[idx * 3 + 2] = o[2];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Per-motion sums of per-frame partials
// ---------------------------------------------------------------------------------------------------------------------------------
// The block of plane `plane` that motion m owns: elements [e0, e1) of values; false (an empty block) when the segment is empty or does
// not lie inside [0, n_rows].
PARC_MO_FN bool segsum_block(int plane, int m, int n_rows, int width, const int32_t *__restrict__ seg_start, size_t &e0, size_t &e1) {
    const int s = seg_start[m], e = seg_start[m + 1];
    if (s < 0 || e > n_rows || e <= s) return false;
    e0 = ((size_t)plane * n_rows + s) * width;
    e1 = ((size_t)plane * n_rows + e) * width;
    return true;
}

// partial sum `lane` of the block: elements e0 + lane, e0 + lane + 256, ... in ascending order
PARC_MO_FN float segsum_lane(const float *__restrict__ values, size_t e0, size_t e1, int lane) {
    float acc = 0.f;
    for (size_t e = e0 + lane; e < e1; e += PARC_MOOPT_SUM_LANES) acc += values[e];
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Argument rules of the entry points (include/parc_moopt.h), answered before any HIP call (counts, then
// "nothing to do", then pointers): PARC_OK = go on, 1 = nothing to do
// ---------------------------------------------------------------------------------------------------------------------------------
#define PARC_MOOPT_NOTHING 1

static inline int moopt_check_ragged(int64_t n_rows, int points_per_row, const void *points, const void *row_terrain, int n_terrains,
                                     const void *table, const void *pool, const void *out) {
    if (n_rows < 0 || n_terrains < 0 || points_per_row <= 0) return PARC_EINVAL;
    if (n_rows == 0) return PARC_MOOPT_NOTHING;
    return !points || !row_terrain || !table || !pool || !out ? PARC_EINVAL : PARC_OK;
}

static inline int moopt_check_tt_seg(int n_frames, int num_bodies, int n_motions, const void *seg_start, const void *seg_of_frame, const void *pos,
                                     const void *rot_err_sq, const void *src_vel, const void *keep, const void *pair_contact, const void *out) {
    if (n_frames < 0 || n_motions < 0 || num_bodies <= 0) return PARC_EINVAL;
    if ((int64_t)n_frames * num_bodies > (int64_t)0x7fffffff / 3) return PARC_EINVAL;
    if (n_frames == 0) return PARC_MOOPT_NOTHING;
    return !seg_start || !seg_of_frame || !pos || !rot_err_sq || !src_vel || !keep || !pair_contact || !out ? PARC_EINVAL : PARC_OK;
}

static inline int moopt_check_segment_sums(int n_planes, int n_rows, int width, int n_motions, const void *seg_start, const void *values,
                                           const void *out) {
    if (n_planes < 0 || n_rows < 0 || n_motions < 0 || width <= 0) return PARC_EINVAL;
    if (n_planes == 0 || n_motions == 0) return PARC_MOOPT_NOTHING;
    if (!seg_start || !values || !out) return PARC_EINVAL;
    return n_planes > 65535 ? PARC_EUNSUPPORTED : PARC_OK;
}

#if !defined(__HIPCC__)
// The device's fold of the 256 partials (k with k + 128, then k + 64, ...) in the same order.
static inline float segsum_fold_host(float *lanes) {
    for (int off = PARC_MOOPT_SUM_LANES / 2; off > 0; off >>= 1)
        for (int k = 0; k < off; ++k) lanes[k] += lanes[k + off];
    return lanes[0];
}
#endif
