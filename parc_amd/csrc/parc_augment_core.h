// Dataset augmentation: all arithmetic of include/parc_augment.h.
//
// The same source compiles for the device (parc_augment.hip) and for the host (g++: tests/tools/augment_host.cpp, the CPU tests and
// the sanitizer program), where the threads of a launch are loops.  Both are compiled with floating-point contraction OFF: the
// products and sums below are the separately rounded fp32 operations of the torch code they restate (on the device the ones that
// decide a grid index or a height are spelled __fmul_rn / __fadd_rn / __fsub_rn as well).
//
// Reference: tools/motion_opt/augment_motions.py:155-205, util/terrain_util.py:117-130 (grid index), :223-240 (pad), :930-969 (boxes),
// :1675-1740 (slice and localise); quaternion rules of util/torch_util.py.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/parc_augment.h"
#include "../../include/parc_moopt.h"

#if defined(__HIPCC__)
#define PARC_AUG_FN __device__ __forceinline__
#define PARC_AUG_HOST_FN static inline
#else
#define PARC_AUG_FN static inline
#define PARC_AUG_HOST_FN static inline
#endif

#define PARC_AUG_NOTHING 1      // argument check: valid, and nothing to do
#define PARC_AUG_THREADS 256    // workgroup of the per-variant kernels

namespace parc_aug {

#if defined(__HIP_DEVICE_COMPILE__)
PARC_AUG_FN float mul_rn(float a, float b) { return __fmul_rn(a, b); }
PARC_AUG_FN float add_rn(float a, float b) { return __fadd_rn(a, b); }
PARC_AUG_FN float sub_rn(float a, float b) { return __fsub_rn(a, b); }
#else
PARC_AUG_FN float mul_rn(float a, float b) { return a * b; }
PARC_AUG_FN float add_rn(float a, float b) { return a + b; }
PARC_AUG_FN float sub_rn(float a, float b) { return a - b; }
#endif

PARC_AUG_FN float quiet_nan() { return __builtin_nanf(""); }
PARC_AUG_FN bool is_nan(float x) { return x != x; }

// ---------------------------------------------------------------------------------------------------------------------------------
// frames
// ---------------------------------------------------------------------------------------------------------------------------------
// the window lies inside its clip and the clip inside the source
PARC_AUG_FN bool frames_valid(const parc_augment_frames_t &v, int n_src_rows) {
    return v.length > 0 && v.start >= 0 && v.src_len >= 0 && v.src_off >= 0 && (int64_t)v.start + v.length <= (int64_t)v.src_len &&
           (int64_t)v.src_off + v.src_len <= (int64_t)n_src_rows;
}

// util/torch_util.py: exp_map_to_quat (min_theta 1e-5, normalize_angle, +z below it), quat_mul by the heading quaternion (0, 0, qz, qw)
// from the left, quat_to_exp_map (w >= 0 representative, eps 1e-5, +z below it)
PARC_AUG_FN void turn_exp_map(float qz, float qw, const float *r, float *out) {
    const float raw = sqrtf((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    float ang = atan2f(sinf(raw), cosf(raw));
    const bool ok = fabsf(ang) > 1e-5f;
    float ax = 0.f, ay = 0.f, az = 1.f;
    if (ok) {
        ax = r[0] / raw;
        ay = r[1] / raw;
        az = r[2] / raw;
    } else {
        ang = 0.f;
    }
    // axis_angle_to_quat: normalize(axis) * sin(angle / 2), cos(angle / 2), then quat_unit
    const float an = fmaxf(sqrtf((ax * ax + ay * ay) + az * az), 1e-9f);
    const float h = 0.5f * ang, sh = sinf(h), ch = cosf(h);
    float x2 = (ax / an) * sh, y2 = (ay / an) * sh, z2 = (az / an) * sh, w2 = ch;
    const float qn = fmaxf(sqrtf(((x2 * x2 + y2 * y2) + z2 * z2) + w2 * w2), 1e-9f);
    x2 /= qn, y2 /= qn, z2 /= qn, w2 /= qn;
    // (x1, y1, z1, w1) = (0, 0, qz, qw)
    const float x1 = 0.f, y1 = 0.f, z1 = qz, w1 = qw;
    float x = ((w1 * x2 + x1 * w2) + y1 * z2) - z1 * y2;
    float y = ((w1 * y2 - x1 * z2) + y1 * w2) + z1 * x2;
    float z = ((w1 * z2 + x1 * y2) - y1 * x2) + z1 * w2;
    float w = ((w1 * w2 - x1 * x2) - y1 * y2) - z1 * z2;
    if (w < 0.f) x = -x, y = -y, z = -z, w = -w;
    const float s = sqrtf((x * x + y * y) + z * z);
    if (s > 1e-5f) {
        const float angle = 2.0f * atan2f(s, w);
        out[0] = angle * (x / s);
        out[1] = angle * (y / s);
        out[2] = angle * (z / s);
    } else {
        out[0] = 0.f * 0.f, out[1] = 0.f * 0.f, out[2] = 0.f * 1.f;      // angle 0 times the +z axis
    }
}

// one frame of a valid variant: src -> dst (34 floats each); returns the transformed x and y
PARC_AUG_FN void transform_frame(const parc_augment_frames_t &v, const float *__restrict__ src, float *__restrict__ dst, float &ox, float &oy) {
    const float x = src[0], y = src[1];
    const float rx = sub_rn(mul_rn(x, v.cos_h), mul_rn(y, v.sin_h));
    const float ry = add_rn(mul_rn(x, v.sin_h), mul_rn(y, v.cos_h));
    ox = mul_rn(rx, v.sx);
    oy = mul_rn(ry, v.sy);
    dst[0] = ox;
    dst[1] = oy;
    dst[2] = src[2];
    float e[3];
    turn_exp_map(v.qz, v.qw, src + 3, e);
    dst[3] = e[0], dst[4] = e[1], dst[5] = e[2];
    for (int k = 6; k < PARC_AUG_FRAME_DIM; ++k) dst[k] = src[k];
}

// running min / max of a variant's xy; min and max are exact in any order, a NaN raises the flag instead (fminf drops it)
struct Bounds {
    float lo_x, lo_y, hi_x, hi_y;
    int nan;
};
PARC_AUG_FN Bounds bounds_empty() { return Bounds{INFINITY, INFINITY, -INFINITY, -INFINITY, 0}; }
PARC_AUG_FN void bounds_add(Bounds &b, float x, float y) {
    b.nan |= (is_nan(x) || is_nan(y)) ? 1 : 0;
    b.lo_x = fminf(b.lo_x, x), b.lo_y = fminf(b.lo_y, y);
    b.hi_x = fmaxf(b.hi_x, x), b.hi_y = fmaxf(b.hi_y, y);
}
PARC_AUG_FN void bounds_merge(Bounds &b, const Bounds &o) {
    b.nan |= o.nan;
    b.lo_x = fminf(b.lo_x, o.lo_x), b.lo_y = fminf(b.lo_y, o.lo_y);
    b.hi_x = fmaxf(b.hi_x, o.hi_x), b.hi_y = fmaxf(b.hi_y, o.hi_y);
}
PARC_AUG_FN void bounds_store(const Bounds &b, float *out) {
    const float n = quiet_nan();
    out[0] = b.nan ? n : b.lo_x, out[1] = b.nan ? n : b.lo_y, out[2] = b.nan ? n : b.hi_x, out[3] = b.nan ? n : b.hi_y;
}

// What lane `lane` of `lanes` does for variant v: its share of the frames and of the contact elements; returns its share of the bounds.
// Rows outside [0, n_out_rows) are not written.
PARC_AUG_FN Bounds frames_lane(const parc_augment_frames_t &v, int lane, int lanes, int n_src_rows, int contact_width,
                               const float *__restrict__ src_frames, const float *__restrict__ src_contacts, int n_out_rows,
                               float *__restrict__ out_frames, float *__restrict__ out_contacts) {
    Bounds b = bounds_empty();
    const bool valid = frames_valid(v, n_src_rows);
    const int len = v.length > 0 ? v.length : 0;
    if (!valid) b.nan = 1;
    for (int t = lane; t < len; t += lanes) {
        const int64_t orow = (int64_t)v.out_off + t;
        if (orow < 0 || orow >= n_out_rows) {
            b.nan = 1;
            continue;
        }
        float *dst = out_frames + (size_t)orow * PARC_AUG_FRAME_DIM;
        if (!valid) {
            for (int k = 0; k < PARC_AUG_FRAME_DIM; ++k) dst[k] = quiet_nan();
            continue;
        }
        const size_t srow = (size_t)v.src_off + v.start + t;        // inside the source: frames_valid
        float x, y;
        transform_frame(v, src_frames + srow * PARC_AUG_FRAME_DIM, dst, x, y);
        bounds_add(b, x, y);
    }
    const int64_t n_el = (int64_t)len * contact_width;
    for (int64_t e = lane; e < n_el; e += lanes) {
        const int t = (int)(e / contact_width), c = (int)(e % contact_width);
        const int64_t orow = (int64_t)v.out_off + t;
        if (orow < 0 || orow >= n_out_rows) continue;
        out_contacts[(size_t)orow * contact_width + c] =
            valid ? src_contacts[((size_t)v.src_off + v.start + t) * contact_width + c] : quiet_nan();
    }
    return b;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// terrains
// ---------------------------------------------------------------------------------------------------------------------------------
// clamp(round(f), 0, n - 1) of SubTerrain.get_grid_index; a NaN lands on 0 (n >= 1)
PARC_AUG_FN int grid_index(float f, int n) {
    const float r = rintf(f);
    if (!(r >= 0.f)) return 0;
    if (r >= (float)(n - 1)) return n - 1;
    return (int)r;
}

// height of the source terrain padded by `pad` cells of height 0 at point (px, py): the padded min point is min - dxdy * pad, the
// index a true divide then rintf; nothing is materialised
PARC_AUG_FN float padded_height(const parc_augment_terrain_t &s, const float *__restrict__ src_pool, int64_t src_pool_floats, int pad, float px,
                                float py) {
    const float mx = sub_rn(s.min_x, mul_rn(s.dx, (float)pad)), my = sub_rn(s.min_y, mul_rn(s.dy, (float)pad));
    const int i = grid_index(sub_rn(px, mx) / s.dx, s.dim_x + 2 * pad) - pad, j = grid_index(sub_rn(py, my) / s.dy, s.dim_y + 2 * pad) - pad;
    if (i < 0 || i >= s.dim_x || j < 0 || j >= s.dim_y) return 0.f;
    const int64_t at = (int64_t)s.off_hf + (int64_t)i * s.dim_y + j;
    if (at < 0 || at >= src_pool_floats) return quiet_nan();
    return src_pool[at];
}

PARC_AUG_FN float point_at(const float *__restrict__ points, int64_t points_floats, int64_t at) {
    return (at < 0 || at >= points_floats) ? quiet_nan() : points[at];
}

// What the cells of one variant share.  ok = 0: the variant's table rows point outside their arrays - NaN outputs.
struct Variant {
    int ok;
    float cx, cy, cz;       // canon: the first frame's xy and the height under it (0 when nothing is localised)
    float lmx, lmy;         // the output grid's min point, localised
};

PARC_AUG_FN Variant variant_setup(const parc_augment_variant_t &a, int n_sources, const parc_augment_terrain_t *__restrict__ src_table,
                                  const float *__restrict__ src_pool, int64_t src_pool_floats, const parc_augment_terrain_t &o,
                                  const float *__restrict__ points, int64_t points_floats, int n_boxes, const float *__restrict__ frames,
                                  int n_rows) {
    Variant r = Variant{0, 0.f, 0.f, 0.f, o.min_x, o.min_y};
    if (a.src < 0 || a.src >= n_sources || a.pad < 0 || o.dim_x <= 0 || o.dim_y <= 0) return r;
    if (a.frame_len <= 0 || a.frame_off < 0 || (int64_t)a.frame_off + a.frame_len > (int64_t)n_rows) return r;
    if (a.mode == PARC_AUG_BOXES_ALONG_PATH && (a.box_count < 0 || a.box_off < 0 || (int64_t)a.box_off + a.box_count > (int64_t)n_boxes)) return r;
    r.ok = 1;
    if (!a.slice) return r;
    const parc_augment_terrain_t s = src_table[a.src];
    const float *f0 = frames + (size_t)a.frame_off * PARC_AUG_FRAME_DIM;
    r.cx = f0[0], r.cy = f0[1];
    r.lmx = sub_rn(o.min_x, r.cx), r.lmy = sub_rn(o.min_y, r.cy);
    // the height under the localised first frame, looked up in the sliced grid (get_hf_val_from_points of the sliced terrain)
    const int ci = grid_index(sub_rn(sub_rn(r.cx, r.cx), r.lmx) / o.dx, o.dim_x), cj = grid_index(sub_rn(sub_rn(r.cy, r.cy), r.lmy) / o.dy, o.dim_y);
    r.cz = padded_height(s, src_pool, src_pool_floats, a.pad, point_at(points, points_floats, (int64_t)o.off_x + ci),
                         point_at(points, points_floats, (int64_t)o.off_y + cj));
    return r;
}

// add_boxes_to_hf_at_xy_points in grid-index space: is cell (i, j) inside box b whose centre is (bcx, bcy)?  strict < and >
PARC_AUG_FN bool in_box(const parc_augment_box_t &b, float bcx, float bcy, int i, int j) {
    const float px = sub_rn((float)i, bcx), py = sub_rn((float)j, bcy);
    const float tx = add_rn(sub_rn(mul_rn(px, b.cos_a), mul_rn(py, b.sin_a)), bcx);
    const float ty = add_rn(add_rn(mul_rn(px, b.sin_a), mul_rn(py, b.cos_a)), bcy);
    const float hx = b.len_x / 2.0f, hy = b.len_y / 2.0f;
    return tx < add_rn(bcx, hx) && tx > sub_rn(bcx, hx) && ty < add_rn(bcy, hy) && ty > sub_rn(bcy, hy);
}

// the height of output cell (i, j) of a variant
PARC_AUG_FN float cell_height(const parc_augment_variant_t &a, const Variant &r, const parc_augment_terrain_t *__restrict__ src_table,
                              const float *__restrict__ src_pool, int64_t src_pool_floats, const parc_augment_terrain_t &o,
                              const float *__restrict__ points, int64_t points_floats, const parc_augment_box_t *__restrict__ boxes,
                              const float *__restrict__ frames, int i, int j) {
    if (!r.ok) return quiet_nan();
    const parc_augment_terrain_t s = src_table[a.src];
    float h;
    if (a.slice) {
        h = padded_height(s, src_pool, src_pool_floats, a.pad, point_at(points, points_floats, (int64_t)o.off_x + i),
                          point_at(points, points_floats, (int64_t)o.off_y + j));
        h = sub_rn(h, r.cz);
    } else {
        // the padded grid itself
        const int si = i - a.pad, sj = j - a.pad;
        h = 0.f;
        if (si >= 0 && si < s.dim_x && sj >= 0 && sj < s.dim_y) {
            const int64_t at = (int64_t)s.off_hf + (int64_t)si * s.dim_y + sj;
            h = (at < 0 || at >= src_pool_floats) ? quiet_nan() : src_pool[at];
        }
    }
    if (a.mode == PARC_AUG_HEIGHT_SCALE) {
        h = mul_rn(a.scale, h);
    } else if (a.mode == PARC_AUG_BOXES_ALONG_PATH) {
        for (int k = 0; k < a.box_count; ++k) {
            const parc_augment_box_t b = boxes[a.box_off + k];
            if (b.frame_ind < 0 || b.frame_ind >= a.frame_len) return quiet_nan();
            const float *f = frames + ((size_t)a.frame_off + b.frame_ind) * PARC_AUG_FRAME_DIM;
            const float bcx = sub_rn(sub_rn(f[0], r.cx), r.lmx) / o.dx, bcy = sub_rn(sub_rn(f[1], r.cy), r.lmy) / o.dy;
            if (in_box(b, bcx, bcy, i, j)) h = b.h;
        }
    }
    return h;
}

// the variant that owns flat cell `cell`: the last v with cell_start[v] <= cell (cell_start ascending, cell < cell_start[n])
PARC_AUG_FN int variant_of_cell(const int64_t *__restrict__ cell_start, int n_variants, int64_t cell) {
    int lo = 0, hi = n_variants - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (cell_start[mid] <= cell) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// one output cell
PARC_AUG_FN void terrain_thread(int64_t cell, int n_variants, const int64_t *__restrict__ cell_start, const parc_augment_variant_t *__restrict__ vars,
                                int n_sources, const parc_augment_terrain_t *__restrict__ src_table, const float *__restrict__ src_pool,
                                int64_t src_pool_floats, const parc_augment_terrain_t *__restrict__ out_table, const float *__restrict__ points,
                                int64_t points_floats, const parc_augment_box_t *__restrict__ boxes, int n_boxes, const float *__restrict__ frames,
                                int n_rows, float *__restrict__ out_pool, int64_t out_pool_floats, float *__restrict__ canon) {
    const int v = variant_of_cell(cell_start, n_variants, cell);
    const int64_t local = cell - cell_start[v];
    const parc_augment_terrain_t o = out_table[v];
    const parc_augment_variant_t a = vars[v];
    const int64_t n_local = (o.dim_x > 0 && o.dim_y > 0) ? (int64_t)o.dim_x * o.dim_y : 0;
    if (local < 0 || local >= n_local) return;         // the running sum disagrees with the table: nothing of this cell is known
    const Variant r = variant_setup(a, n_sources, src_table, src_pool, src_pool_floats, o, points, points_floats, n_boxes, frames, n_rows);
    const int i = (int)(local / o.dim_y), j = (int)(local % o.dim_y);
    const float h = cell_height(a, r, src_table, src_pool, src_pool_floats, o, points, points_floats, boxes, frames, i, j);
    const int64_t at = (int64_t)o.off_hf + local;
    if (at >= 0 && at < out_pool_floats) out_pool[at] = h;
    if (local == 0) {
        const float n = quiet_nan();
        canon[(size_t)v * 3 + 0] = r.ok ? r.cx : n;
        canon[(size_t)v * 3 + 1] = r.ok ? r.cy : n;
        canon[(size_t)v * 3 + 2] = r.ok ? r.cz : n;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// localise
// ---------------------------------------------------------------------------------------------------------------------------------
PARC_AUG_FN void localize_lane(const parc_augment_variant_t &a, int v, int lane, int lanes, const float *__restrict__ canon, float *__restrict__ frames,
                               int n_rows, parc_moopt_terrain_t *hf_table) {
    if (!a.slice) return;
    const float cx = canon[(size_t)v * 3], cy = canon[(size_t)v * 3 + 1], cz = canon[(size_t)v * 3 + 2];
    const bool rows_ok = a.frame_len > 0 && a.frame_off >= 0 && (int64_t)a.frame_off + a.frame_len <= (int64_t)n_rows;
    if (rows_ok)
        for (int t = lane; t < a.frame_len; t += lanes) {
            float *f = frames + ((size_t)a.frame_off + t) * PARC_AUG_FRAME_DIM;
            f[0] = sub_rn(f[0], cx), f[1] = sub_rn(f[1], cy), f[2] = sub_rn(f[2], cz);
        }
    if (lane == 0 && hf_table) {
        hf_table[v].ox = sub_rn(hf_table[v].ox, cx);
        hf_table[v].oy = sub_rn(hf_table[v].oy, cy);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// argument rules (host side of every entry point, before any HIP call)
// ---------------------------------------------------------------------------------------------------------------------------------
PARC_AUG_HOST_FN int check_frames(int n_variants, int n_src_rows, int contact_width, const void *src_frames, const void *src_contacts, const void *vars,
                                  int n_out_rows, const void *out_frames, const void *out_contacts, const void *bounds) {
    if (n_variants < 0 || n_src_rows < 0 || contact_width < 0 || n_out_rows < 0) return PARC_EINVAL;
    if (n_variants == 0) return PARC_AUG_NOTHING;
    if (!vars || !bounds) return PARC_EINVAL;
    if (n_src_rows > 0 && (!src_frames || (contact_width > 0 && !src_contacts))) return PARC_EINVAL;
    if (n_out_rows > 0 && (!out_frames || (contact_width > 0 && !out_contacts))) return PARC_EINVAL;
    return PARC_OK;
}

PARC_AUG_HOST_FN int check_terrains(int n_variants, int64_t n_cells, const void *cell_start, const void *vars, int n_sources, const void *src_table,
                                    const void *src_pool, int64_t src_pool_floats, const void *out_table, const void *points, int64_t points_floats,
                                    const void *boxes, int n_boxes, const void *frames, int n_rows, const void *out_pool, int64_t out_pool_floats,
                                    const void *canon) {
    if (n_variants < 0 || n_cells < 0 || n_sources < 0 || src_pool_floats < 0 || points_floats < 0 || n_boxes < 0 || n_rows < 0 || out_pool_floats < 0)
        return PARC_EINVAL;
    if (n_variants == 0) return PARC_AUG_NOTHING;
    if (!cell_start || !vars || !out_table || !canon) return PARC_EINVAL;
    if ((n_sources > 0 && !src_table) || (src_pool_floats > 0 && !src_pool) || (points_floats > 0 && !points) || (n_boxes > 0 && !boxes) ||
        (n_rows > 0 && !frames) || (out_pool_floats > 0 && !out_pool))
        return PARC_EINVAL;
    return PARC_OK;
}

PARC_AUG_HOST_FN int check_localize(int n_variants, const void *vars, const void *canon, const void *frames, int n_rows) {
    if (n_variants < 0 || n_rows < 0) return PARC_EINVAL;
    if (n_variants == 0) return PARC_AUG_NOTHING;
    if (!vars || !canon || (n_rows > 0 && !frames)) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_aug
