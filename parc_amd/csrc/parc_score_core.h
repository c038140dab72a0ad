// Motion scorer: all arithmetic of parc_motion_score (include/parc_score.h), from the body poses of one frame on.
//
// The same source compiles for the device (parc_score.hip: a 16-lane group per frame, its lanes striping every body's sample points)
// and for the host (g++: tests/tools/score_host.cpp, the CPU tests and the sanitizer program), where the 16 lanes of a group and the
// threads of the fold are loops that add in the kernel's order.
//
// Reference: tools/procgen/mdm_path.py:31-127 (compute_motion_loss) and tools/motion_tests/compute_losses.py:158-169 (jerk).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/parc_score.h"
#include "parc_rot.h"       // v3, q4, qrot
#include "parc_sdf_core.h"

#if defined(__HIPCC__)
#define PARC_SC_FN __device__ __forceinline__
#else
#define PARC_SC_FN static inline
#endif

namespace parc_sc {

constexpr int kLanes = 16;          // lanes of a frame group (= PARC_MAX_BODIES: lane b holds body b)
constexpr int kFoldThreads = 64;    // threads of the per-candidate fold

// false for NaN and for +-inf
PARC_SC_FN bool finite1(float x) { return fabsf(x) <= 3.4028234663852886e38f; }
PARC_SC_FN bool finite_pose(v3 p, q4 q) {
    return finite1(p.x) && finite1(p.y) && finite1(p.z) && finite1(q.x) && finite1(q.y) && finite1(q.z) && finite1(q.w);
}

// What every point of a launch shares
struct Field {
    parc_score_terrain_t t;
    float half_x, half_y, base_z;
};
PARC_SC_FN Field make_field(const parc_score_terrain_t &t, float base_z) { return Field{t, t.dx / 2.0f, t.dy / 2.0f, base_z}; }

// One sample point: pen = -min(sdf_inverted, 0) = max(min over the air columns, 0), d_out = max(min over the ground columns, 0).
// fmaxf drops NaNs, so a non-finite world position raises `bad` instead.
PARC_SC_FN void point_terms(const Field &f, v3 pos, q4 rot, const float *local, float &pen, float &d_out, int &bad) {
    const v3 r = qrot(rot, ld3(local));
    const float px = pos.x + r.x, py = pos.y + r.y, pz = pos.z + r.z;
    if (!(finite1(px) && finite1(py) && finite1(pz))) {
        bad = 1;
        pen = 0.f;
        d_out = 0.f;
        return;          // (the scan of a non-finite point would cover the whole field for nothing)
    }
    int cell;
    const float air = hf_window_min(px, py, pz, f.t.hf, f.t.dim_x, f.t.dim_y, f.t.min_x, f.t.min_y, f.t.x_points, f.t.y_points, f.half_x, f.half_y,
                                    f.base_z, 1, cell);
    const float ground = hf_window_min(px, py, pz, f.t.hf, f.t.dim_x, f.t.dim_y, f.t.min_x, f.t.min_y, f.t.x_points, f.t.y_points, f.half_x,
                                       f.half_y, f.base_z, 0, cell);
    pen = fmaxf(air, 0.f);
    d_out = fmaxf(ground, 0.f);
}

// Lane `lane` of a frame group on body b (pose pos, rot; points p0 .. p1-1): the lane takes points p0 + lane, p0 + lane + 16, ...  Adds
// their penetration to pen_acc in that order and returns the smallest d_out among them (+inf when the lane has none).
PARC_SC_FN float body_lane_terms(const Field &f, v3 pos, q4 rot, const float *local, int p0, int p1, int lane, float &pen_acc, int &bad) {
    float lane_min = INFINITY;
    for (int p = p0 + lane; p < p1; p += kLanes) {
        float pen, d_out;
        point_terms(f, pos, rot, local + 3 * (size_t)p, pen, d_out, bad);
        pen_acc += pen;
        lane_min = fminf(lane_min, d_out);
    }
    return lane_min;
}

// the point range of body b, forced into [0, n_points] and non-decreasing (start is device data nobody has looked at)
PARC_SC_FN void body_range(const int32_t *start, int b, int n_points, int &p0, int &p1) {
    const int a = start[b], e = start[b + 1];
    p0 = a < 0 ? 0 : (a > n_points ? n_points : a);
    p1 = e < p0 ? p0 : (e > n_points ? n_points : e);
}

// frames that count for a candidate
PARC_SC_FN int counted_frames(const int32_t *num_frames, int cand, int F) {
    if (!num_frames) return F;
    const int n = num_frames[cand];
    return n < 0 ? 0 : (n > F ? F : n);
}

// |third difference| / dt^3 of one body over frames f .. f+3, step by step as compute_losses.py:159-162 (p = body_pos rows of one
// body, `stride` floats apart)
PARC_SC_FN float jerk_magnitude(const float *p, size_t stride, float dt) {
    float j[3];
    for (int k = 0; k < 3; ++k) {
        const float x0 = p[k], x1 = p[stride + k], x2 = p[2 * stride + k], x3 = p[3 * stride + k];
        const float v0 = (x1 - x0) / dt, v1 = (x2 - x1) / dt, v2 = (x3 - x2) / dt;
        const float a0 = (v1 - v0) / dt, a1 = (v2 - v1) / dt;
        j[k] = (a1 - a0) / dt;
    }
    return sqrtf(j[0] * j[0] + j[1] * j[1] + j[2] * j[2]);
}

// Thread t of the fold: its share (items t, t + 64, ...) of the frame terms and of the jerk items of one candidate, added in that order.
struct FoldPartial {
    float pen, contact, jerk_sum;
    int32_t over, bad;
};
PARC_SC_FN FoldPartial fold_partial(int t, int n, int num_bodies, const float *frame_terms, const float *body_pos, float dt, float max_jerk) {
    FoldPartial a = {0.f, 0.f, 0.f, 0, 0};
    for (int f = t; f < n; f += kFoldThreads) {
        const float pen = frame_terms[2 * (size_t)f], con = frame_terms[2 * (size_t)f + 1];
        if (!(pen == pen) || !(con == con)) a.bad = 1;
        a.pen += pen;
        a.contact += con;
    }
    if (body_pos && n > 3) {
        const int items = (n - 3) * num_bodies;
        for (int i = t; i < items; i += kFoldThreads) {
            const int f = i / num_bodies, b = i - f * num_bodies;
            const float m = jerk_magnitude(body_pos + ((size_t)f * num_bodies + b) * 3, (size_t)num_bodies * 3, dt);
            a.jerk_sum += m;
            if (m > max_jerk) a.over += 1;
        }
    }
    return a;
}
PARC_SC_FN void fold_add(FoldPartial &a, const FoldPartial &b) {
    a.pen += b.pen;
    a.contact += b.contact;
    a.jerk_sum += b.jerk_sum;
    a.over += b.over;
    a.bad |= b.bad;
}
// the outputs of one candidate from the sum of all partials
PARC_SC_FN void fold_finish(const FoldPartial &s, int n, int num_bodies, float w_contact, float w_pen, float *losses, float *jerk) {
    const float nanv = __builtin_nanf("");
    const float pen = w_pen * s.pen, contact = w_contact * s.contact;
    losses[0] = s.bad ? nanv : pen + contact;
    losses[1] = s.bad ? nanv : contact;
    losses[2] = s.bad ? nanv : pen;
    if (jerk) {
        const bool ok = n > 3 && !s.bad;
        jerk[0] = ok ? s.jerk_sum / (float)((n - 3) * num_bodies) : nanv;
        jerk[1] = ok ? (float)s.over / (float)(n - 3) : nanv;
    }
}

// the argument rules of parc_motion_score, checked on the host before any HIP call
static inline int check_args(const parc_char_model_t &model, int B, int F, const void *root_pos, const void *root_rot, const void *joint_rot,
                             const void *contacts, int n_points, const void *local, const void *start, const parc_score_terrain_t &ter,
                             const void *body_pos_ws, const void *frame_terms, const void *losses, const void *jerk) {
    if (B < 0 || F < 0 || n_points <= 0) return PARC_EINVAL;
    if (model.num_bodies < 1 || model.num_bodies > PARC_MAX_BODIES || model.num_bodies > kLanes) return PARC_EINVAL;
    if (!root_pos || !root_rot || !contacts || !local || !start || !frame_terms || !losses) return PARC_EINVAL;
    if (model.num_bodies > 1 && !joint_rot) return PARC_EINVAL;
    if (jerk && !body_pos_ws) return PARC_EINVAL;
    if (!ter.hf || !ter.x_points || !ter.y_points || ter.dim_x <= 0 || ter.dim_y <= 0 || !(ter.dx > 0.f) || !(ter.dy > 0.f)) return PARC_EINVAL;
    if ((int64_t)ter.dim_x * ter.dim_y > (int64_t)1 << 30) return PARC_EINVAL;
    if (B > 65535) return PARC_EUNSUPPORTED;
    return PARC_OK;
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- the host's lanes and trees
// all-reduce of a 16-lane row as the kernel's DPP rotations do it (row_ror 8, 4, 2, 1): the value lane 0 ends with
static inline float row_sum16(const float *v) {
    float a[kLanes], b[kLanes];
    for (int i = 0; i < kLanes; ++i) a[i] = v[i];
    for (int n = 8; n >= 1; n >>= 1) {
        for (int i = 0; i < kLanes; ++i) b[i] = a[i] + a[(i + kLanes - n) % kLanes];
        for (int i = 0; i < kLanes; ++i) a[i] = b[i];
    }
    return a[0];
}

// one frame from its body poses [Bd,3] / [Bd,4]: (pen_f, contact_f), NaN both when the pose or a point is not finite
static inline void frame_terms_host(const Field &f, int num_bodies, const float *body_pos, const float *body_rot, const float *contacts, int n_points,
                                    const float *local, const int32_t *start, float *out) {
    float pen_acc[kLanes], con[kLanes];
    int bad = 0;
    for (int l = 0; l < kLanes; ++l) pen_acc[l] = con[l] = 0.f;
    for (int b = 0; b < num_bodies; ++b) {
        const v3 pos = ld3(body_pos + 3 * b);
        const q4 rot = ld4(body_rot + 4 * b);
        if (!finite_pose(pos, rot)) bad = 1;
        int p0, p1;
        body_range(start, b, n_points, p0, p1);
        float m = INFINITY;
        for (int l = 0; l < kLanes; ++l) m = fminf(m, body_lane_terms(f, pos, rot, local, p0, p1, l, pen_acc[l], bad));
        con[b] = p1 > p0 ? contacts[b] * m : 0.f;
    }
    const float nanv = __builtin_nanf("");
    out[0] = bad ? nanv : row_sum16(pen_acc);
    out[1] = bad ? nanv : row_sum16(con);
}

// the fold of one candidate: 64 partials, then the kernel's halving tree
static inline void fold_host(int n, int num_bodies, const float *frame_terms, const float *body_pos, float w_contact, float w_pen, float dt,
                             float max_jerk, float *losses, float *jerk) {
    FoldPartial p[kFoldThreads];
    for (int t = 0; t < kFoldThreads; ++t) p[t] = fold_partial(t, n, num_bodies, frame_terms, jerk ? body_pos : nullptr, dt, max_jerk);
    for (int s = kFoldThreads / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) fold_add(p[t], p[t + s]);
    fold_finish(p[0], n, num_bodies, w_contact, w_pen, losses, jerk);
}
#endif

}  // namespace parc_sc
