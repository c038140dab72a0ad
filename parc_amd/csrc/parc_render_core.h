// Offscreen ray caster: all ray and geometry arithmetic of parc_render, one pixel per call.
//
// The same source compiles for the device (parc_render.hip: one thread per pixel, the frame of a view staged in LDS by its
// workgroup) and for the host (g++: tests/tools/render_host.cpp, the CPU tests and the sanitizer program).
//
// Conventions
//   * rays: origin o, unit direction d, hits at o + t d with t > 0.  Only ENTRIES count: a ray that starts inside a solid does not
//     see that solid's surface from within.
//   * terrain: the column field of hf_lookup (parc_hf_lookup.h).  Cell (i, j) is centred at min + (i, j) * dx, owns rint((p - min) / dx),
//     i.e. the square [i - 1/2, i + 1/2) x [j - 1/2, j + 1/2) in grid units, has its top at hf[i, j] and reaches down without end, so
//     neighbours of different height are joined by vertical walls.  Traversal: a 2-D DDA over the cells from where the ray enters the
//     grid's bounding box; outside the grid there is nothing.  In grid units u = (x - min_x) / dx + 1/2 cell i is floor(u).
//   * a capsule is the union of a finite cylinder and two spheres; a box is tested by slabs in its own frame.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/parc_render.h"
#include "parc_rot.h"       // v3, q4, their operators, ld3/ld4, qmul, qrot

#if defined(__HIPCC__)
#define PARC_RHD __host__ __device__ __forceinline__
#else
#define PARC_RHD static inline
#endif

namespace parc_rc {

PARC_RHD v3 normalize_or(v3 a, v3 fallback) {
    const float l2 = dot3(a, a);
    return (l2 > 1e-20f && l2 < 1e30f) ? (1.0f / sqrtf(l2)) * a : fallback;       // (NaN fails both comparisons)
}
PARC_RHD v3 qrot_inv(q4 q, v3 v) { return qrot(qconj(q), v); }
// float -> index in [0, hi]; NaN -> 0 (fmaxf returns the other operand)
PARC_RHD int clamp_index(float f, int hi) { return (int)fminf(fmaxf(f, 0.0f), (float)hi); }

constexpr float kInf = __builtin_inff();
constexpr float kShadowBias = 1e-3f;      // the shadow ray starts this far off the surface, along the normal

// A primitive in world space (64 bytes; a workgroup keeps 2 x PARC_RENDER_MAX_PRIMS of them in LDS)
struct WPrim {
    int32_t type, id, tint;
    float a[3], b[3], radius, q[4];
    float _pad[2];
};

struct Camera {
    v3 eye, fwd, right, up;
    float tan_half, aspect;
};

// Everything the pixels of one view share
struct Frame {
    Camera cam;
    const WPrim *prims;      // n_char[0] rows of the simulated character, then n_char[1] of the reference character
    int32_t n_char[2];
    v3 bound_c[2];           // one bounding sphere per character
    float bound_r[2];
    parc_terrain_t ter;
    v3 light;
    float ambient;
    v3 color[2];
    int32_t shadows, num_bodies;
};

struct Hit {
    float t;
    int32_t id, tint;
    v3 n;
};

// ---------------------------------------------------------------------------------------------- staging (once per view)
PARC_RHD int view_env(const parc_render_view_t &v, int n_envs) { return v.env < 0 ? 0 : (v.env >= n_envs ? n_envs - 1 : v.env); }

PARC_RHD void camera_setup(const parc_render_view_t &v, const float *root_state, const float *env_offsets, int n_envs, int width, int height,
                           Camera &cam) {
    const int e = view_env(v, n_envs);
    v3 eye = ld3(v.vec), tar = ld3(v.target);
    if (v.mode == PARC_RENDER_CAM_TRACK) {
        const float rx = root_state[13 * (size_t)e] + env_offsets[3 * (size_t)e], ry = root_state[13 * (size_t)e + 1] + env_offsets[3 * (size_t)e + 1];
        eye = mk3(rx + v.vec[0], ry + v.vec[1], v.vec[2]);
        tar = mk3(rx, ry, 1.0f);
    }
    cam.eye = eye;
    cam.fwd = normalize_or(tar - eye, mk3(0.f, 1.f, 0.f));
    v3 r = cross3(cam.fwd, mk3(0.f, 0.f, 1.f));
    if (!(dot3(r, r) > 1e-6f)) r = cross3(cam.fwd, mk3(0.f, 1.f, 0.f));        // looking along z: image up = world +y
    cam.right = normalize_or(r, mk3(1.f, 0.f, 0.f));
    cam.up = cross3(cam.right, cam.fwd);
    const float fov = fminf(fmaxf(v.fov_y, 0.02f), 3.1f);                   // (NaN -> 0.02)
    cam.tan_half = tanf(0.5f * fov);
    cam.aspect = (float)width / (float)height;
}

// prim (body frame) -> world, for body pose (pos, rot) and a translation (env offset, + ref_char_offset for the reference character)
PARC_RHD void prim_to_world(const parc_render_prim_t &p, v3 pos, q4 rot, v3 shift, int id, int tint, WPrim &w) {
    w.type = p.type;
    w.id = id;
    w.tint = tint;
    const v3 a = pos + qrot(rot, ld3(p.a)) + shift;
    w.a[0] = a.x; w.a[1] = a.y; w.a[2] = a.z;
    w.radius = p.radius;
    if (p.type == PARC_RENDER_CAPSULE) {
        const v3 b = pos + qrot(rot, ld3(p.b)) + shift;
        w.b[0] = b.x; w.b[1] = b.y; w.b[2] = b.z;
    } else {
        w.b[0] = p.b[0]; w.b[1] = p.b[1]; w.b[2] = p.b[2];
    }
    const q4 q = qmul(rot, ld4(p.q));
    w.q[0] = q.x; w.q[1] = q.y; w.q[2] = q.z; w.q[3] = q.w;
    w._pad[0] = w._pad[1] = 0.f;
}

// radius of the sphere around c that holds the n primitives
PARC_RHD float bound_radius(const WPrim *w, int n, v3 c) {
    float r = 0.f;
    for (int k = 0; k < n; ++k) {
        const v3 a = ld3(w[k].a) - c;
        float rk = sqrtf(dot3(a, a));
        if (w[k].type == PARC_RENDER_CAPSULE) {
            const v3 b = ld3(w[k].b) - c;
            rk = fmaxf(rk, sqrtf(dot3(b, b))) + w[k].radius;
        } else if (w[k].type == PARC_RENDER_BOX) {
            rk += sqrtf(dot3(ld3(w[k].b), ld3(w[k].b)));
        } else {
            rk += w[k].radius;
        }
        r = fmaxf(r, rk);
    }
    return 1.001f * r + 1e-4f;
}

// The staging of one view, in three pieces that the kernel hands to different threads and the host build runs one after the other.
// The device pointers a launch reads:
struct Inputs {
    const float *root_state, *rigid_body_state, *ref_body_pos, *ref_body_rot, *contact_forces, *env_offsets;
    int n_envs;
};
PARC_RHD int n_staged_prims(const parc_render_scene_t &sc, const Inputs &in) { return sc.n_prims * (in.ref_body_pos ? 2 : 1); }

// piece 1, for k in [0, n_staged_prims): primitive k of the view's env into wp[k] (the simulated character's first, then the reference's)
PARC_RHD void stage_prim(int k, const parc_render_scene_t &sc, const Inputs &in, int e, WPrim *wp) {
    const int B = sc.num_bodies, n = sc.n_prims;
    const int c = k >= n ? 1 : 0;
    const parc_render_prim_t p = sc.prims[k - c * n];
    const int b = p.body < 0 ? 0 : (p.body >= B ? B - 1 : p.body);
    const size_t row = (size_t)e * B + b;
    const v3 off = ld3(in.env_offsets + 3 * (size_t)e);
    if (c == 0) {
        int tint = 0;
        if (sc.show_contacts) {
            const v3 cf = ld3(in.contact_forces + 3 * row);
            tint = dot3(cf, cf) > sc.contact_eps * sc.contact_eps;
        }
        prim_to_world(p, ld3(in.rigid_body_state + 13 * row), ld4(in.rigid_body_state + 13 * row + 3), off, b, tint, wp[k]);
    } else {
        prim_to_world(p, ld3(in.ref_body_pos + 3 * row), ld4(in.ref_body_rot + 4 * row), off + ld3(sc.ref_char_offset), B + b, 0, wp[k]);
    }
}

// piece 2: camera and scalars
PARC_RHD void stage_frame(const parc_render_view_t &view, const parc_terrain_t &ter, const parc_render_scene_t &sc, const Inputs &in, int width,
                          int height, const WPrim *wp, Frame &fr) {
    camera_setup(view, in.root_state, in.env_offsets, in.n_envs, width, height, fr.cam);
    fr.prims = wp;
    fr.n_char[0] = sc.n_prims;
    fr.n_char[1] = in.ref_body_pos ? sc.n_prims : 0;
    fr.ter = ter;
    fr.light = normalize_or(ld3(sc.light_dir), mk3(0.f, 0.f, 1.f));
    fr.ambient = sc.ambient;
    fr.color[0] = ld3(sc.sim_color);
    fr.color[1] = ld3(sc.ref_color);
    fr.shadows = sc.shadows;
    fr.num_bodies = sc.num_bodies;
}

// piece 3, for c in {0, 1}, after piece 1 is complete: the bounding sphere of character c, around its root body
PARC_RHD void stage_bound(int c, const parc_render_scene_t &sc, const Inputs &in, int e, const WPrim *wp, Frame &fr) {
    const size_t row = (size_t)e * sc.num_bodies;
    const bool has_ref = in.ref_body_pos != nullptr;
    const v3 off = ld3(in.env_offsets + 3 * (size_t)e);
    const v3 cen = c == 0 ? ld3(in.rigid_body_state + 13 * row) + off : (has_ref ? ld3(in.ref_body_pos + 3 * row) + off + ld3(sc.ref_char_offset) : off);
    fr.bound_c[c] = cen;
    fr.bound_r[c] = bound_radius(wp + c * sc.n_prims, c == 0 || has_ref ? sc.n_prims : 0, cen);
}

// ---------------------------------------------------------------------------------------------- primitives
PARC_RHD bool hit_sphere(v3 o, v3 d, v3 c, float r, float &t, v3 &n) {
    const v3 oc = o - c;
    const float b = dot3(oc, d), cc = dot3(oc, oc) - r * r;
    const float h = b * b - cc;
    if (!(h > 0.f)) return false;
    const float tt = -b - sqrtf(h);
    if (!(tt > 0.f)) return false;
    t = tt;
    n = (1.0f / r) * (oc + tt * d);
    return true;
}

PARC_RHD bool hit_capsule(v3 o, v3 d, v3 pa, v3 pb, float r, float &t, v3 &n) {
    bool any = false;
    float tb = kInf;
    v3 nb = mk3(0.f, 0.f, 1.f);
    float tk;
    v3 nk;
    if (hit_sphere(o, d, pa, r, tk, nk)) { any = true; tb = tk; nb = nk; }
    if (hit_sphere(o, d, pb, r, tk, nk) && tk < tb) { any = true; tb = tk; nb = nk; }
    // the side: |oa + t d - ((oa + t d).ba / ba.ba) ba|^2 = r^2, kept where the foot point lies strictly between the ends
    const v3 ba = pb - pa, oa = o - pa;
    const float baba = dot3(ba, ba), bard = dot3(ba, d), baoa = dot3(ba, oa), rdoa = dot3(d, oa), oaoa = dot3(oa, oa);
    const float a = baba - bard * bard, b = baba * rdoa - baoa * bard, c = baba * oaoa - baoa * baoa - r * r * baba;
    const float h = b * b - a * c;
    if (a > 1e-12f * baba && h > 0.f) {
        const float ts = (-b - sqrtf(h)) / a;
        const float y = baoa + ts * bard;
        if (ts > 0.f && y > 0.f && y < baba && ts < tb) {
            any = true;
            tb = ts;
            nb = (1.0f / r) * (oa + ts * d - (y / baba) * ba);
        }
    }
    t = tb;
    n = nb;
    return any;
}

PARC_RHD bool hit_box(v3 o, v3 d, v3 c, v3 half, q4 q, float &t, v3 &n) {
    const v3 ol = qrot_inv(q, o - c), dl = qrot_inv(q, d);
    const float oo[3] = {ol.x, ol.y, ol.z}, dd[3] = {dl.x, dl.y, dl.z}, hh[3] = {half.x, half.y, half.z};
    float tn = -kInf, tf = kInf, sgn = 0.f;
    int ax = 0;
    for (int k = 0; k < 3; ++k) {
        if (dd[k] == 0.f) {
            if (!(fabsf(oo[k]) < hh[k])) return false;
            continue;
        }
        const float inv = 1.0f / dd[k];
        float t1 = (-hh[k] - oo[k]) * inv, t2 = (hh[k] - oo[k]) * inv;
        float s = -1.f;
        if (t1 > t2) { const float x = t1; t1 = t2; t2 = x; s = 1.f; }
        if (t1 > tn) { tn = t1; ax = k; sgn = s; }
        tf = fminf(tf, t2);
    }
    if (!(tn < tf) || !(tn > 0.f)) return false;
    t = tn;
    n = qrot(q, mk3(ax == 0 ? sgn : 0.f, ax == 1 ? sgn : 0.f, ax == 2 ? sgn : 0.f));
    return true;
}

PARC_RHD bool hit_prim(const WPrim &w, v3 o, v3 d, float &t, v3 &n) {
    if (w.type == PARC_RENDER_SPHERE) return hit_sphere(o, d, ld3(w.a), w.radius, t, n);
    if (w.type == PARC_RENDER_CAPSULE) return hit_capsule(o, d, ld3(w.a), ld3(w.b), w.radius, t, n);
    if (w.type == PARC_RENDER_BOX) return hit_box(o, d, ld3(w.a), ld3(w.b), ld4(w.q), t, n);
    return false;
}

// does the ray meet the sphere at all (t >= 0), or start inside it?
PARC_RHD bool touches_sphere(v3 o, v3 d, v3 c, float r) {
    const v3 oc = o - c;
    const float b = dot3(oc, d), cc = dot3(oc, oc) - r * r;
    if (cc <= 0.f) return true;
    return b < 0.f && b * b - cc >= 0.f;
}

// nearest entry into a primitive of either character closer than hit.t
PARC_RHD void trace_chars(const Frame &f, v3 o, v3 d, Hit &hit) {
    int k0 = 0;
    for (int c = 0; c < 2; ++c) {
        const int n = f.n_char[c];
        if (n > 0 && touches_sphere(o, d, f.bound_c[c], f.bound_r[c])) {
            for (int k = k0; k < k0 + n; ++k) {
                float t;
                v3 nn;
                if (hit_prim(f.prims[k], o, d, t, nn) && t < hit.t) {
                    hit.t = t;
                    hit.n = nn;
                    hit.id = f.prims[k].id;
                    hit.tint = f.prims[k].tint;
                }
            }
        }
        k0 += n;
    }
}

// ---------------------------------------------------------------------------------------------- terrain
// 2-D DDA over the cells.  At most dim_x + dim_y + 2 steps; every index is clamped before the load.
PARC_RHD void trace_terrain(const parc_terrain_t &ter, int id_base, v3 o, v3 d, Hit &hit) {
    const int nx = ter.dim_x, ny = ter.dim_y;
    const float ou = (o.x - ter.min_x) / ter.dx + 0.5f, ov = (o.y - ter.min_y) / ter.dy + 0.5f;
    const float du = d.x / ter.dx, dv = d.y / ter.dy;
    // the part of the ray inside the bounding box 0 <= u <= nx, 0 <= v <= ny
    float t0 = 0.f, t1 = kInf;
    int axis = -1;          // which face the ray came in through (-1: it starts inside)
    if (du != 0.f) {
        const float inv = 1.0f / du;
        const float ta = (0.f - ou) * inv, tb = ((float)nx - ou) * inv;
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        if (lo > t0) { t0 = lo; axis = 0; }
        t1 = fminf(t1, hi);
    } else if (!(ou >= 0.f && ou <= (float)nx)) {
        return;
    }
    if (dv != 0.f) {
        const float inv = 1.0f / dv;
        const float ta = (0.f - ov) * inv, tb = ((float)ny - ov) * inv;
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        if (lo > t0) { t0 = lo; axis = 1; }
        t1 = fminf(t1, hi);
    } else if (!(ov >= 0.f && ov <= (float)ny)) {
        return;
    }
    if (!(t0 <= t1) || !(t0 < hit.t)) return;        // (NaN: return)
    const int su = du > 0.f ? 1 : -1, sv = dv > 0.f ? 1 : -1;
    const float inv_du = du != 0.f ? 1.0f / du : 0.f, inv_dv = dv != 0.f ? 1.0f / dv : 0.f;
    int i = clamp_index(floorf(ou + t0 * du), nx - 1), j = clamp_index(floorf(ov + t0 * dv), ny - 1);
    // on a face of the box the cell is the one behind the face, whatever the rounding of ou + t0 du says
    if (axis == 0) i = du > 0.f ? 0 : nx - 1;
    if (axis == 1) j = dv > 0.f ? 0 : ny - 1;
    float t_in = t0;
    const int max_steps = nx + ny + 2;
    for (int step = 0; step < max_steps; ++step) {
        const int ci = i < 0 ? 0 : (i >= nx ? nx - 1 : i), cj = j < 0 ? 0 : (j >= ny ? ny - 1 : j);
        const float h = ter.hf[(size_t)ci * ny + cj];
        if (axis >= 0) {            // came in through a wall plane at t_in: below the top, that wall is hit
            const float z_in = o.z + t_in * d.z;
            if (z_in < h) {
                if (t_in > 0.f && t_in < hit.t) {
                    hit.t = t_in;
                    hit.id = id_base + ci * ny + cj;
                    hit.tint = 0;
                    hit.n = axis == 0 ? mk3((float)-su, 0.f, 0.f) : mk3(0.f, (float)-sv, 0.f);
                }
                return;
            }
        }
        // leaves the cell through u, v or the bounding box, whichever comes first
        const float tu = du != 0.f ? ((float)(i + (su > 0 ? 1 : 0)) - ou) * inv_du : kInf;
        const float tv = dv != 0.f ? ((float)(j + (sv > 0 ? 1 : 0)) - ov) * inv_dv : kInf;
        const float t_out = fminf(fminf(tu, tv), t1);
        const bool inside_start = axis < 0 && o.z < h;       // started inside this column: its surface is not seen from within
        if (d.z < 0.f && !inside_start) {
            const float tt = (h - o.z) / d.z;
            if (tt <= t_out) {
                if (tt > 0.f && tt < hit.t) {
                    hit.t = tt;
                    hit.id = id_base + ci * ny + cj;
                    hit.tint = 0;
                    hit.n = mk3(0.f, 0.f, 1.f);
                }
                return;
            }
        }
        if (!(t_out < t1) || !(t_out < hit.t)) return;       // out of the box, or past the nearest hit so far
        if (tu <= tv) { i += su; axis = 0; } else { j += sv; axis = 1; }
        if (i < 0 || i >= nx || j < 0 || j >= ny) return;
        t_in = t_out;
    }
}

PARC_RHD void trace(const Frame &f, v3 o, v3 d, Hit &hit) {
    hit.t = kInf;
    hit.id = -1;
    hit.tint = 0;
    hit.n = mk3(0.f, 0.f, 1.f);
    trace_chars(f, o, d, hit);
    trace_terrain(f.ter, 2 * f.num_bodies, o, d, hit);
}

// ---------------------------------------------------------------------------------------------- one pixel
PARC_RHD uint32_t pack_rgba(v3 c) {
    const uint32_t r = (uint32_t)(fminf(fmaxf(c.x, 0.f), 1.f) * 255.f + 0.5f), g = (uint32_t)(fminf(fmaxf(c.y, 0.f), 1.f) * 255.f + 0.5f),
                   b = (uint32_t)(fminf(fmaxf(c.z, 0.f), 1.f) * 255.f + 0.5f);
    return r | (g << 8) | (b << 16) | 0xFF000000u;
}

PARC_RHD v3 pixel_ray(const Camera &cam, int px, int py, int width, int height) {
    const float sx = (2.0f * ((float)px + 0.5f) / (float)width - 1.0f) * cam.tan_half * cam.aspect;
    const float sy = (1.0f - 2.0f * ((float)py + 0.5f) / (float)height) * cam.tan_half;
    return normalize_or(cam.fwd + sx * cam.right + sy * cam.up, cam.fwd);
}

// normal_out (3 floats, optional): the shading normal, for the host tests
PARC_RHD void shade_pixel(const Frame &f, int px, int py, int width, int height, uint32_t &rgba, float &depth, int32_t &id, float *normal_out) {
    const v3 o = f.cam.eye, d = pixel_ray(f.cam, px, py, width, height);
    Hit hit;
    trace(f, o, d, hit);
    depth = hit.t;
    id = hit.id;
    if (normal_out) { normal_out[0] = hit.n.x; normal_out[1] = hit.n.y; normal_out[2] = hit.n.z; }
    if (hit.id < 0) {
        rgba = pack_rgba(mk3(0.62f, 0.74f, 0.90f));     // sky
        return;
    }
    v3 albedo;
    const int B = f.num_bodies;
    if (hit.id < 2 * B) {
        albedo = f.color[hit.id < B ? 0 : 1];
        if (hit.tint) albedo = 0.4f * albedo + mk3(0.6f, 0.06f, 0.03f);
    } else {
        const int cell = hit.id - 2 * B, ci = cell / f.ter.dim_y, cj = cell - ci * f.ter.dim_y;
        const float h = f.ter.hf[(size_t)ci * f.ter.dim_y + cj];        // (ci, cj were clamped when the id was made)
        const float k = fminf(fmaxf(0.5f + 0.25f * h, 0.f), 1.f);       // tint by height ...
        albedo = mk3(0.45f + 0.35f * k, 0.55f + 0.10f * k, 0.42f - 0.12f * k);
        if ((ci + cj) & 1) albedo = 0.85f * albedo;                     // ... and a checker by cell parity
    }
    float diffuse = fmaxf(dot3(hit.n, f.light), 0.f);
    if (f.shadows && diffuse > 0.f) {
        Hit sh;
        trace(f, o + hit.t * d + kShadowBias * hit.n, f.light, sh);
        if (sh.id >= 0) diffuse = 0.f;
    }
    rgba = pack_rgba((f.ambient + (1.0f - f.ambient) * diffuse) * albedo);
}

// the argument rules of parc_render (include/parc_render.h), checked on the host before any launch
static inline int check_args(const parc_terrain_t &terrain, const parc_render_scene_t *scene, int n_views, const void *views, int width, int height,
                             const void *root_state, const void *rigid_body_state, const void *ref_body_pos, const void *ref_body_rot,
                             const void *contact_forces, const void *env_offsets, int n_envs, const void *rgba) {
    if (width <= 0 || height <= 0 || n_views < 0 || n_views > 65535 || n_envs <= 0) return PARC_EINVAL;
    if (!scene || !views || !rgba || !rigid_body_state || !root_state || !env_offsets) return PARC_EINVAL;
    if ((ref_body_pos == nullptr) != (ref_body_rot == nullptr)) return PARC_EINVAL;
    if (scene->n_prims < 0 || scene->n_prims > PARC_RENDER_MAX_PRIMS || scene->num_bodies < 1) return PARC_EINVAL;
    if (scene->n_prims > 0 && !scene->prims) return PARC_EINVAL;
    if (scene->show_contacts && !contact_forces) return PARC_EINVAL;
    if (!terrain.hf || !(terrain.dx > 0.f) || !(terrain.dy > 0.f) || terrain.dim_x <= 0 || terrain.dim_y <= 0) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_rc
