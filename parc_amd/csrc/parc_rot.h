// Plain-fp32 rotation algebra in torch's operation order, with its adjoints: the one place for it, for the device (hipcc) and for the host
// (g++: the CPU tests of the shared cores).  Quaternions are xyzw as in the reference's util/torch_util.py.  Fast approximations and the
// FMA-grouped product live in parc_math.h, on top of these types.
//
// Three parts:
//   * types and algebra.  No contraction pragma: these fuse or not as the including translation unit is built.
//   * torch-order functions.  Each expression once, with explicit grouping.  The torch-exact maps (qunit, aa_to_quat, em_to_quat) carry
//     `#pragma clang fp contract(off)`: they give torch's bits also in a translation unit built with contraction on (the clip database
//     build, the pose chain).  The pragma covers the lexical body only, so inside them the sums are written out, not handed to dot3.
//   * adjoints, derived by hand:
//       q = a (x) b bilinear               =>  g_a = g (x) conj(b),  g_b = conj(a) (x) g
//       r = v + w t + u x t, t = 2 u x v   =>  g_w = g.t,  g_t = w g + g x u,  g_u = t x g + 2 v x g_t
//       q = unit(n(axis) sin h, cos h), h = angle / 2   (axis_angle_to_quat: both normalisations are projections at unit length)
//       angle = 2 atan2(|v|, w) of the w >= 0 representative; e = angle v / |v|
//     and the singular-input rule: a rotation in the reference's "below 1e-5" branch has gradient 0 (that branch is constant).
#pragma once
#include <math.h>

// __host__ as well under hipcc: the functions of parc_render_core.h are __host__ __device__ and call these.  (Today no host code of a
// .hip file calls one: parc_render.hip's host side runs check_args only.)
#if defined(__HIPCC__)
#define PARC_ROT_FN __host__ __device__ __forceinline__
#else
#define PARC_ROT_FN static inline
#endif

// ---- types and algebra ----
struct v3 {
    float x, y, z;
};
struct q4 {
    float x, y, z, w;
};

PARC_ROT_FN v3 mk3(float x, float y, float z) { return v3{x, y, z}; }
PARC_ROT_FN q4 mk4(float x, float y, float z, float w) { return q4{x, y, z, w}; }
PARC_ROT_FN v3 operator+(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
PARC_ROT_FN v3 operator-(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
PARC_ROT_FN v3 operator*(float s, v3 a) { return v3{s * a.x, s * a.y, s * a.z}; }
PARC_ROT_FN float dot3(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
PARC_ROT_FN v3 cross3(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
PARC_ROT_FN q4 qadd(q4 a, q4 b) { return q4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
PARC_ROT_FN q4 qscale(float s, q4 a) { return q4{s * a.x, s * a.y, s * a.z, s * a.w}; }
PARC_ROT_FN q4 qconj(q4 q) { return q4{-q.x, -q.y, -q.z, q.w}; }
PARC_ROT_FN v3 ld3(const float *p) { return v3{p[0], p[1], p[2]}; }
PARC_ROT_FN q4 ld4(const float *p) { return q4{p[0], p[1], p[2], p[3]}; }
PARC_ROT_FN void st3(float *p, v3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
PARC_ROT_FN void st4(float *p, q4 q) { p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }

// ---- torch-order functions ----
// util/torch_util.py:577-594 quat_multiply: the 16 products, summed left to right (quat_mul at :40-58, which the reference's
// kinematics call, is the same product in a 9-multiplication grouping; parc_math.h's FMA-grouped quat_mul cites that one)
PARC_ROT_FN q4 qmul(q4 a, q4 b) {
    return q4{((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y, ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x,
              ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w, ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z};
}
// util/torch_util.py:60-66 quat_rotate: v + w t + u x t, t = 2 u x v
PARC_ROT_FN v3 qrot(q4 q, v3 v) {
    const v3 u = mk3(q.x, q.y, q.z);
    const v3 t = 2.f * cross3(u, v);
    const v3 c = cross3(u, t);
    return v3{(v.x + q.w * t.x) + c.x, (v.y + q.w * t.y) + c.y, (v.z + q.w * t.z) + c.z};
}
// util/torch_util.py:9-12 (eps 1e-9) on a quaternion
PARC_ROT_FN q4 qunit(q4 q) {
#pragma clang fp contract(off)      // op by op like torch: no fused multiply-adds in the three torch-exact maps
    const float n = fmaxf(sqrtf(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w), 1e-9f);
    return q4{q.x / n, q.y / n, q.z / n, q.w / n};
}
// util/torch_util.py:311-317
PARC_ROT_FN q4 aa_to_quat(v3 axis, float angle) {
#pragma clang fp contract(off)
    const float th = angle / 2.f;
    const float n = fmaxf(sqrtf((axis.x * axis.x + axis.y * axis.y) + axis.z * axis.z), 1e-9f);
    const float s = sinf(th);
    return qunit(q4{axis.x / n * s, axis.y / n * s, axis.z / n * s, cosf(th)});
}
// util/torch_util.py:394-419
PARC_ROT_FN q4 em_to_quat(v3 em) {
#pragma clang fp contract(off)
    float a = sqrtf((em.x * em.x + em.y * em.y) + em.z * em.z);
    v3 ax = v3{em.x / a, em.y / a, em.z / a};
    a = atan2f(sinf(a), cosf(a));
    if (!(fabsf(a) > 1e-5f)) {
        ax = mk3(0.f, 0.f, 1.f);
        a = 0.f;
    }
    return aa_to_quat(ax, a);
}
// util/torch_util.py:68-88 and :346-351: the w >= 0 representative's angle and exponential map
PARC_ROT_FN float qangle(q4 d) {
    const float s = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    return s > 1e-5f ? 2.0f * atan2f(s, fabsf(d.w)) : 0.f;
}
PARC_ROT_FN v3 quat_to_em(q4 d) {
    const float sg = d.w < 0.f ? -1.f : 1.f;
    const v3 v = mk3(sg * d.x, sg * d.y, sg * d.z);
    const float s = sqrtf(dot3(v, v));
    if (!(s > 1e-5f)) return mk3(0.f, 0.f, 0.f);          // angle 0 times the z axis
    const float a = 2.0f * atan2f(s, sg * d.w);
    return mk3(v.x / s * a, v.y / s * a, v.z / s * a);
}
// util/torch_util.py:421-431
PARC_ROT_FN float qdiff_angle(q4 q0, q4 q1) { return qangle(qmul(q1, qconj(q0))); }

// ---- adjoints ----
// cotangent of d for angle = qangle(d)
PARC_ROT_FN q4 qangle_bwd(q4 d, float g) {
    const float s = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    if (!(s > 1e-5f)) return q4{0.f, 0.f, 0.f, 0.f};
    const float sg = d.w < 0.f ? -1.0f : 1.0f;           // the representative with w >= 0
    const float w = sg * d.w, den = s * s + w * w;
    const float gs = 2.0f * w / den * g / s;               // d angle / d|v| * (v / |v|): the two flips of the vector part cancel
    return q4{gs * d.x, gs * d.y, gs * d.z, sg * (-2.0f * s / den * g)};
}
// cotangent of d for e = quat_to_em(d)
PARC_ROT_FN q4 quat_to_em_bwd(q4 d, v3 g) {
    const float sg = d.w < 0.f ? -1.f : 1.f;
    const v3 v = mk3(sg * d.x, sg * d.y, sg * d.z);
    const float w = sg * d.w;
    const float s = sqrtf(dot3(v, v));
    if (!(s > 1e-5f)) return q4{0.f, 0.f, 0.f, 0.f};
    const float a = 2.0f * atan2f(s, w), den = s * s + w * w;
    const v3 u = mk3(v.x / s, v.y / s, v.z / s);
    const float gu = dot3(g, u);
    const float c0 = a / s, c1 = 2.0f * w / den * gu;
    const v3 gv = mk3(c0 * (g.x - gu * u.x) + c1 * u.x, c0 * (g.y - gu * u.y) + c1 * u.y, c0 * (g.z - gu * u.z) + c1 * u.z);
    return q4{sg * gv.x, sg * gv.y, sg * gv.z, sg * (-2.0f * s / den * gu)};
}
// d = b (x) conj(a): cotangents of a and b from the cotangent of d
PARC_ROT_FN q4 qdiff_bwd_a(q4 b, q4 gd) {
    const q4 gc = qmul(qconj(b), gd);          // the cotangent of conj(a)
    return q4{-gc.x, -gc.y, -gc.z, gc.w};
}
PARC_ROT_FN q4 qdiff_bwd_b(q4 a, q4 gd) { return qmul(gd, a); }

// cotangent of q for r = qrot(q, v), given the cotangent g of r
PARC_ROT_FN q4 qrot_bwd_q(q4 q, v3 v, v3 g) {
    const v3 u = mk3(q.x, q.y, q.z);
    const v3 t = 2.f * cross3(u, v);
    const v3 gxu = cross3(g, u);
    const v3 gt = mk3(q.w * g.x + gxu.x, q.w * g.y + gxu.y, q.w * g.z + gxu.z);
    const v3 gu = cross3(t, g) + 2.f * cross3(v, gt);
    return q4{gu.x, gu.y, gu.z, dot3(g, t)};
}
// cotangents of axis and angle for q = aa_to_quat(axis, angle), given the cotangent g of q
struct aa_grad {
    v3 g_axis;
    float g_angle;
};
PARC_ROT_FN aa_grad aa_to_quat_bwd(v3 axis, float angle, q4 q, q4 g) {
    // through qunit: q = raw / |raw| with |raw| = 1 up to rounding -> g_raw = g - (g.q) q
    const float gq = ((g.x * q.x + g.y * q.y) + g.z * q.z) + g.w * q.w;
    const q4 gr = q4{g.x - gq * q.x, g.y - gq * q.y, g.z - gq * q.z, g.w - gq * q.w};
    const float h = 0.5f * angle;
    const float sh = sinf(h), ch = cosf(h);
    const float na = fmaxf(sqrtf(dot3(axis, axis)), 1e-9f);
    const v3 a = mk3(axis.x / na, axis.y / na, axis.z / na);
    const v3 grv = mk3(gr.x, gr.y, gr.z);
    aa_grad o;
    o.g_angle = 0.5f * (ch * dot3(a, grv) - sh * gr.w);
    // through normalize(axis): g_axis = (I - a a^T) (sin h g_v) / |axis|
    const v3 ga = mk3(sh * grv.x, sh * grv.y, sh * grv.z);
    const float gaa = dot3(ga, a);
    o.g_axis = mk3((ga.x - gaa * a.x) / na, (ga.y - gaa * a.y) / na, (ga.z - gaa * a.z) / na);
    return o;
}
// em_to_quat = aa_to_quat(e / |e|, wrap(|e|)), z axis / angle 0 below 1e-5
PARC_ROT_FN v3 em_to_quat_bwd(v3 em, q4 q, q4 g) {
    const float raw = sqrtf(dot3(em, em));
    const float ang = atan2f(sinf(raw), cosf(raw));
    if (!(fabsf(ang) > 1e-5f)) return mk3(0.f, 0.f, 0.f);
    const v3 a = mk3(em.x / raw, em.y / raw, em.z / raw);
    const aa_grad ag = aa_to_quat_bwd(a, ang, q, g);
    // axis = e / raw: J^T g = (g - (g.a) a) / raw;  angle = wrap(raw): d/de = a
    const float ga = dot3(ag.g_axis, a);
    return mk3((ag.g_axis.x - ga * a.x) / raw + ag.g_angle * a.x, (ag.g_axis.y - ga * a.y) / raw + ag.g_angle * a.y,
               (ag.g_axis.z - ga * a.z) / raw + ag.g_angle * a.z);
}
