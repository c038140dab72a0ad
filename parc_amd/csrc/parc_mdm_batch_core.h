// Training-batch sampler of the motion generator: all arithmetic of include/parc_mdm_batch.h.
//
// The same source compiles for the device (parc_mdm_batch.hip) and for the host (g++: tests/tools/mdm_batch_host.cpp, the CPU tests and
// the sanitizer program), where the lanes of a launch are loops and a barrier is nothing.  Both are compiled with floating-point
// contraction OFF: the products and sums below are the separately rounded fp32 operations of the torch code they restate, in its order.
//
// Reference: diffusion/mdm_heightfield_contact_motion_sampler.py:270-488, anim/motion_lib.py:80-112,443-475,528-538 (clip lookup),
// anim/kin_char_model.py:509-541 (FK), util/torch_util.py (quaternion rules), util/terrain_util.py:123-126 (grid index), :864-917
// (boxes), :1595-1621 (pools), :1999-2006 (mask).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/parc_mdm_batch.h"
#include "parc_rot.h"       // v3, q4, qmul (:577-594 quat_multiply, the grouping the canonicalisation uses), qrot (:61-66)

#if defined(__HIPCC__)
#define PARC_MDM_FN __device__ __forceinline__
#else
#define PARC_MDM_FN static inline
#endif
#define PARC_MDM_HOST_FN static inline

#if defined(__HIP_DEVICE_COMPILE__)
#define PARC_MDM_SYNC() __syncthreads()
#define PARC_MDM_OR(p, v) atomicOr((p), (v))
#else
#define PARC_MDM_SYNC() ((void)0)
#define PARC_MDM_OR(p, v) (*(p) |= (v))
#endif

#define PARC_MDM_NOTHING 1          // argument check: valid, and nothing to do
#define PARC_MDM_HF_THREADS 256     // workgroup of the heightfield kernel
#define PARC_MDM_WIN_THREADS 64     // workgroup of the window kernel
#define PARC_MDM_FK_FLOATS 7        // FK workspace per body: position 3, rotation 4

namespace parc_mdm {

PARC_MDM_FN float quiet_nan() { return __builtin_nanf(""); }

// ---------------------------------------------------------------------------------------------------------------------------------
// util/torch_util.py
// ---------------------------------------------------------------------------------------------------------------------------------
// :41-58 quat_mul (the grouping the FK uses)
PARC_MDM_FN q4 quat_mul(q4 a, q4 b) {
    const float ww = (a.z + a.x) * (b.x + b.y);
    const float yy = (a.w - a.y) * (b.w + b.z);
    const float zz = (a.w + a.y) * (b.w - b.z);
    const float xx = (ww + yy) + zz;
    const float qq = 0.5f * (xx + (a.z - a.x) * (b.x - b.y));
    q4 o;
    o.w = (qq - ww) + (a.z - a.y) * (b.y - b.z);
    o.x = (qq - xx) + (a.x + a.w) * (b.x + b.w);
    o.y = (qq - yy) + (a.w - a.x) * (b.y + b.z);
    o.z = (qq - zz) + (a.z + a.y) * (b.w - b.x);
    return o;
}

// :471-479
PARC_MDM_FN float calc_heading(q4 q) {
    const v3 d = qrot(q, v3{1.f, 0.f, 0.f});
    return atan2f(d.y, d.x);
}

// :312-317 about +z, :492-499 with the angle negated by the caller.  Not aa_to_quat (parc_rot.h) about +z: its x and y are
// 0 / n * sin, -0 for a negative angle, where this function gives +0, and a zero's sign is a bit of the result
PARC_MDM_FN q4 heading_quat(float angle) {
    const float theta = angle / 2.f;
    const float z = 1.f * sinf(theta), w = cosf(theta);
    const float n = fmaxf(sqrtf(((0.f + 0.f) + z * z) + w * w), 1e-9f);
    return q4{0.f / n, 0.f / n, z / n, w / n};
}

// :444-468
PARC_MDM_FN q4 slerp(q4 q0, q4 q1, float t) {
    float c = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
    if (c < 0.f) q1 = q4{-q1.x, -q1.y, -q1.z, -q1.w};
    c = fabsf(c);
    const float ht = acosf(c);
    const float s = sqrtf(1.0f - c * c);
    const float ra = sinf((1.f - t) * ht) / s, rb = sinf(t * ht) / s;
    q4 o = q4{ra * q0.x + rb * q1.x, ra * q0.y + rb * q1.y, ra * q0.z + rb * q1.z, ra * q0.w + rb * q1.w};
    if (fabsf(s) < 0.001f) o = q4{0.5f * q0.x + 0.5f * q1.x, 0.5f * q0.y + 0.5f * q1.y, 0.5f * q0.z + 0.5f * q1.z, 0.5f * q0.w + 0.5f * q1.w};
    if (c >= 1.f) o = q0;
    return o;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// clip lookup (anim/motion_lib.py:80-112; the blend, wrap offset and clamp of parc_calc_motion_frame)
// ---------------------------------------------------------------------------------------------------------------------------------
struct Query {
    const float *row0, *row1;
    float blend, loop_phase;
    int wrap;
};

PARC_MDM_FN Query make_query(const parc_motion_lib_t &ml, int64_t id, float time) {
    Query fq;
    const float len = ml.length[id];
    fq.wrap = ml.loop_mode[id] == 1;
    float phase = time / len;
    fq.loop_phase = floorf(phase);
    if (fq.wrap) phase = phase - floorf(phase);
    phase = fminf(fmaxf(phase, 0.f), 1.f);
    const int nf = ml.num_frames[id];
    const float fp = phase * (float)(nf - 1);
    int i0 = (int)fp;
    if (!(i0 >= 0)) i0 = 0;                 // a NaN phase (a clip of one frame) reads frame 0
    if (i0 > nf - 1) i0 = nf - 1;
    const int i1 = i0 + 1 < nf - 1 ? i0 + 1 : nf - 1;
    fq.blend = fp - (float)i0;
    const int64_t st = ml.start_idx[id];
    fq.row0 = ml.frames + (size_t)(st + i0) * ml.row_stride;
    fq.row1 = ml.frames + (size_t)(st + i1) * ml.row_stride;
    return fq;
}

PARC_MDM_FN float lerp(float a, float b, float t) { return (1.0f - t) * a + t * b; }

PARC_MDM_FN q4 query_quat(const Query &fq, int b) {
    const float *a = fq.row0 + 4 * b, *c = fq.row1 + 4 * b;
    return slerp(q4{a[0], a[1], a[2], a[3]}, q4{c[0], c[1], c[2], c[3]}, fq.blend);
}

PARC_MDM_FN v3 query_root_pos(const parc_motion_lib_t &ml, const Query &fq, int64_t id) {
    const float *p0 = fq.row0 + ml.off_pos, *p1 = fq.row1 + ml.off_pos;
    v3 p = v3{lerp(p0[0], p1[0], fq.blend), lerp(p0[1], p1[1], fq.blend), lerp(p0[2], p1[2], fq.blend)};
    if (fq.wrap) {
        const float *d = ml.pos_delta + 3 * id;
        p.x = p.x + fq.loop_phase * d[0], p.y = p.y + fq.loop_phase * d[1], p.z = p.z + fq.loop_phase * d[2];
    } else {
        p.x = p.x + 0.f, p.y = p.y + 0.f, p.z = p.z + 0.f;
    }
    return p;
}

PARC_MDM_FN bool id_ok(const parc_motion_lib_t &ml, int64_t id) { return id >= 0 && id < (int64_t)ml.num_motions; }

// ---------------------------------------------------------------------------------------------------------------------------------
// windows: lane (s, k).  ws is the lane's FK workspace: element e of body b at ws[(b * PARC_MDM_FK_FLOATS + e) * ws_stride] (LDS on the
// device, so the walk indexes no register array by the parent table)
// ---------------------------------------------------------------------------------------------------------------------------------
PARC_MDM_FN void window_lane(const parc_char_model_t &m, const parc_motion_lib_t &ml, const parc_mdm_cfg_t &cfg, int s, int k,
                             const int64_t *__restrict__ motion_ids, const float *__restrict__ start_times, const float *__restrict__ motion_times,
                             const float *__restrict__ center_h, const float *__restrict__ future_time, const float *__restrict__ future_noise,
                             float *__restrict__ root_pos, float *__restrict__ root_rot, float *__restrict__ body_pos, float *__restrict__ joint_rot,
                             float *__restrict__ contacts, float *__restrict__ future_pos, float *__restrict__ future_rot, float *ws, int ws_stride) {
    const int S = cfg.seq_len, B = m.num_bodies;
    const size_t row = (size_t)s * S + k;
    const int64_t id = motion_ids[s];
    if (!id_ok(ml, id)) {
        const float n = quiet_nan();
        for (int e = 0; e < 3; ++e) root_pos[row * 3 + e] = n;
        for (int e = 0; e < 4; ++e) root_rot[row * 4 + e] = n;
        for (int e = 0; e < (B - 1) * 3; ++e) body_pos[row * (B - 1) * 3 + e] = n;
        for (int e = 0; e < (B - 1) * 4; ++e) joint_rot[row * (B - 1) * 4 + e] = n;
        for (int e = 0; e < B; ++e) contacts[row * B + e] = n;
        if (k == 0 && future_pos) {
            for (int e = 0; e < 3; ++e) future_pos[(size_t)s * 3 + e] = n;
            for (int e = 0; e < 4; ++e) future_rot[(size_t)s * 4 + e] = n;
        }
        return;
    }
    const float start = start_times[s];
    // the reference frame, looked up again by every lane of the sample
    const Query rq = make_query(ml, id, start + motion_times[cfg.ref_idx]);
    const v3 cpos = query_root_pos(ml, rq, id);
    const q4 hinv = heading_quat(-calc_heading(query_quat(rq, 0)));

    const Query fq = make_query(ml, id, start + motion_times[k]);
    v3 p = query_root_pos(ml, fq, id);
    if (center_h) p.z = p.z - center_h[s];
    p = qrot(hinv, v3{p.x - cpos.x, p.y - cpos.y, p.z - cpos.z});
    const q4 r = qmul(hinv, query_quat(fq, 0));
    root_pos[row * 3 + 0] = p.x, root_pos[row * 3 + 1] = p.y, root_pos[row * 3 + 2] = p.z;
    root_rot[row * 4 + 0] = r.x, root_rot[row * 4 + 1] = r.y, root_rot[row * 4 + 2] = r.z, root_rot[row * 4 + 3] = r.w;
    {
        const float *c0 = fq.row0 + ml.off_contacts, *c1 = fq.row1 + ml.off_contacts;
        for (int b = 0; b < B; ++b) contacts[row * B + b] = lerp(c0[b], c1[b], fq.blend);
    }
#define PARC_MDM_WS(b, e) ws[((b) * PARC_MDM_FK_FLOATS + (e)) * ws_stride]
    PARC_MDM_WS(0, 0) = p.x, PARC_MDM_WS(0, 1) = p.y, PARC_MDM_WS(0, 2) = p.z;
    PARC_MDM_WS(0, 3) = r.x, PARC_MDM_WS(0, 4) = r.y, PARC_MDM_WS(0, 5) = r.z, PARC_MDM_WS(0, 6) = r.w;
    for (int j = 1; j < B; ++j) {
        const q4 jq = query_quat(fq, j);
        float *jr = joint_rot + (row * (B - 1) + (j - 1)) * 4;
        jr[0] = jq.x, jr[1] = jq.y, jr[2] = jq.z, jr[3] = jq.w;
        int par = m.parent[j];
        if (par < 0 || par >= j) par = 0;
        const v3 pp = v3{PARC_MDM_WS(par, 0), PARC_MDM_WS(par, 1), PARC_MDM_WS(par, 2)};
        const q4 pr = q4{PARC_MDM_WS(par, 3), PARC_MDM_WS(par, 4), PARC_MDM_WS(par, 5), PARC_MDM_WS(par, 6)};
        const v3 wt = qrot(pr, v3{m.local_translation[j][0], m.local_translation[j][1], m.local_translation[j][2]});
        const v3 cp = v3{pp.x + wt.x, pp.y + wt.y, pp.z + wt.z};
        const q4 lr = q4{m.local_rotation[j][0], m.local_rotation[j][1], m.local_rotation[j][2], m.local_rotation[j][3]};
        const q4 cr = quat_mul(pr, quat_mul(lr, jq));
        PARC_MDM_WS(j, 0) = cp.x, PARC_MDM_WS(j, 1) = cp.y, PARC_MDM_WS(j, 2) = cp.z;
        PARC_MDM_WS(j, 3) = cr.x, PARC_MDM_WS(j, 4) = cr.y, PARC_MDM_WS(j, 5) = cr.z, PARC_MDM_WS(j, 6) = cr.w;
        float *bp = body_pos + (row * (B - 1) + (j - 1)) * 3;
        bp[0] = cp.x, bp[1] = cp.y, bp[2] = cp.z;
    }
#undef PARC_MDM_WS
    if (k == 0 && future_pos) {
        const Query tq = make_query(ml, id, future_time[s]);
        v3 f = query_root_pos(ml, tq, id);
        f.x = f.x + future_noise[(size_t)s * 3 + 0], f.y = f.y + future_noise[(size_t)s * 3 + 1], f.z = f.z + future_noise[(size_t)s * 3 + 2];
        f = qrot(hinv, v3{f.x - cpos.x, f.y - cpos.y, f.z - cpos.z});
        const q4 fr = qmul(hinv, query_quat(tq, 0));
        future_pos[(size_t)s * 3 + 0] = f.x, future_pos[(size_t)s * 3 + 1] = f.y, future_pos[(size_t)s * 3 + 2] = f.z;
        future_rot[(size_t)s * 4 + 0] = fr.x, future_rot[(size_t)s * 4 + 1] = fr.y, future_rot[(size_t)s * 4 + 2] = fr.z;
        future_rot[(size_t)s * 4 + 3] = fr.w;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// heightfields: sample s by `lanes` lanes; hf, bmax, bmin, tmp are planes of dim_x * dim_y floats and bits holds mask_cells bits, all
// shared by the lanes (LDS on the device)
// ---------------------------------------------------------------------------------------------------------------------------------
// clamp(round(f), 0, n - 1) of SubTerrain.get_grid_index; a NaN lands on 0 (n >= 1)
PARC_MDM_FN int grid_index(float f, int n) {
    const float r = rintf(f);
    if (!(r >= 0.f)) return 0;
    if (r >= (float)(n - 1)) return n - 1;
    return (int)r;
}

// torch.clamp(x, lo, hi) = min(max(x, lo), hi), also where lo > hi
PARC_MDM_FN float clamp_torch(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

PARC_MDM_FN bool clip_ok(const parc_mdm_clip_t &c, int64_t pool_floats, int64_t n_cell_start, int mask_cells) {
    if (c.dim_x < 1 || c.dim_y < 1) return false;
    const int64_t tc = (int64_t)c.dim_x * c.dim_y;
    if (tc > (int64_t)mask_cells) return false;
    if (c.off_hf < 0 || (int64_t)c.off_hf + tc > pool_floats || c.off_band < 0 || (int64_t)c.off_band + 2 * tc > pool_floats) return false;
    if (c.num_frames < 0 || c.frame_off < 0 || (int64_t)c.frame_off + c.num_frames + 1 > n_cell_start) return false;
    return true;
}

// one max-pool of radius r along x (first index) or y from src to dst, padding -inf
PARC_MDM_FN void pool_pass(const float *src, float *dst, int X, int Y, int r, bool along_x, int lane, int lanes) {
    for (int c = lane; c < X * Y; c += lanes) {
        const int i = c / Y, j = c % Y;
        float m = -INFINITY;
        if (along_x) {
            const int lo = i - r > 0 ? i - r : 0, hi = (int64_t)i + r < X - 1 ? i + r : X - 1;
            for (int a = lo; a <= hi; ++a) m = fmaxf(m, src[a * Y + j]);
        } else {
            const int lo = j - r > 0 ? j - r : 0, hi = (int64_t)j + r < Y - 1 ? j + r : Y - 1;
            for (int a = lo; a <= hi; ++a) m = fmaxf(m, src[i * Y + a]);
        }
        dst[c] = m;
    }
}

// util/terrain_util.py:889-901 for one cell
PARC_MDM_FN bool in_box(const parc_mdm_box_t &b, int i, int j) {
    const float ca = cosf(b.angle), sa = sinf(b.angle);
    const float px = (float)i - b.cx, py = (float)j - b.cy;
    const float tx = (px * ca - py * sa) + b.cx, ty = (px * sa + py * ca) + b.cy;
    const float hx = b.lx / 2.f, hy = b.ly / 2.f;
    return tx < b.cx + hx && tx > b.cx - hx && ty < b.cy + hy && ty > b.cy - hy;
}

PARC_MDM_FN void hf_sample(const parc_motion_lib_t &ml, const parc_mdm_cfg_t &cfg, int s, const int64_t *__restrict__ motion_ids,
                           const float *__restrict__ start_times, const float *__restrict__ motion_times, const float *__restrict__ grid_x,
                           const float *__restrict__ grid_y, int n_clips, const parc_mdm_clip_t *__restrict__ clips, const float *__restrict__ pool,
                           int64_t pool_floats, const int32_t *__restrict__ cell_start, int64_t n_cell_start, const int32_t *__restrict__ cells,
                           int64_t n_cells, int mask_cells, const parc_mdm_draw_t *__restrict__ draws, const parc_mdm_box_t *__restrict__ boxes,
                           const float *__restrict__ noise, float *__restrict__ hfs, float *__restrict__ center_h, float *__restrict__ pre,
                           int32_t *__restrict__ cell_code, int lane, int lanes, float *hf, float *bmax, float *bmin, float *tmp, uint32_t *bits) {
    const int X = cfg.dim_x, Y = cfg.dim_y, XY = X * Y;
    const int64_t id = motion_ids[s];
    float *out = hfs + (size_t)s * XY;
    bool ok = id_ok(ml, id) && id < (int64_t)n_clips;
    parc_mdm_clip_t c = parc_mdm_clip_t{0, 0, 1, 1, 0.f, 0.f, 1.f, 1.f, 0, 0};
    if (ok) {
        c = clips[id];
        ok = clip_ok(c, pool_floats, n_cell_start, mask_cells);
    }
    if (!ok) {                                      // the same for every lane of the sample: no barrier is skipped by some
        for (int k = lane; k < XY; k += lanes) out[k] = quiet_nan();
        if (lane == 0) center_h[s] = quiet_nan();
        return;
    }
    const int TX = c.dim_x, TY = c.dim_y, TC = TX * TY;
    const float start = start_times[s];

    // 1. the mask: the union of the cell lists of frames rint(start / dt) + [0, S), intersected with the clip's frames
    for (int w = lane; w < (TC + 31) / 32; w += lanes) bits[w] = 0u;
    PARC_MDM_SYNC();
    {
        const float f0f = rintf(start / cfg.dt);
        int64_t f0 = f0f >= 0.f ? (f0f < 2147483648.f ? (int64_t)f0f : (int64_t)c.num_frames) : 0;        // NaN and negatives: frame 0
        int64_t f1 = f0 + cfg.seq_len;
        if (f0 > c.num_frames) f0 = c.num_frames;
        if (f1 > c.num_frames) f1 = c.num_frames;
        int64_t a = cell_start[c.frame_off + f0], b = cell_start[c.frame_off + f1];
        if (a < 0) a = 0;
        if (b > n_cells) b = n_cells;
        for (int64_t e = a + lane; e < b; e += lanes) {
            const int32_t cell = cells[e];
            if (cell >= 0 && cell < TC) PARC_MDM_OR(&bits[cell >> 5], 1u << (cell & 31));
        }
    }
    PARC_MDM_SYNC();

    // 2. gather: generic grid point turned by the reference heading + reference root xy -> terrain cell -> height and band
    const Query rq = make_query(ml, id, start + motion_times[cfg.ref_idx]);
    const v3 cpos = query_root_pos(ml, rq, id);
    const float heading = calc_heading(query_quat(rq, 0));
    const float ch = cosf(heading), sh = sinf(heading);
    for (int k = lane; k < XY; k += lanes) {
        const int i = k / Y, j = k % Y;
        const float gx = grid_x[i], gy = grid_y[j];
        const float px = (gx * ch - gy * sh) + cpos.x, py = (gx * sh + gy * ch) + cpos.y;
        const int ti = grid_index((px - c.min_x) / c.dx, TX), tj = grid_index((py - c.min_y) / c.dy, TY);
        const int cell = ti * TY + tj;
        const bool masked = (bits[cell >> 5] >> (cell & 31)) & 1u;
        hf[k] = pool[(int64_t)c.off_hf + cell];
        bmax[k] = masked ? pool[(int64_t)c.off_band + 2 * (int64_t)cell] : cfg.max_h * 2.0f;
        bmin[k] = masked ? pool[(int64_t)c.off_band + 2 * (int64_t)cell + 1] : cfg.min_h * 2.0f;
        if (cell_code) cell_code[(size_t)s * XY + k] = cell | (masked ? (1 << 30) : 0);
    }
    PARC_MDM_SYNC();

    // 3. and 4. the height under the character, then the z style
    const float center = hf[cfg.num_x_neg * Y + cfg.num_y_neg];
    const float sub = cfg.z_style == PARC_MDM_Z_ROOT_FLOOR ? center : cpos.z;
    PARC_MDM_SYNC();                                // every lane has read the centre before it changes
    if (lane == 0) center_h[s] = center;
    for (int k = lane; k < XY; k += lanes) {
        hf[k] = hf[k] - sub, bmax[k] = bmax[k] - sub, bmin[k] = bmin[k] - sub;
        if (pre) {
            float *p = pre + (size_t)s * 3 * XY;
            p[k] = hf[k], p[XY + k] = bmax[k], p[2 * XY + k] = bmin[k];
        }
    }
    PARC_MDM_SYNC();

    // 5. the augmentation
    if (cfg.mode == PARC_MDM_AUG_NOISE) {
        // :411 clamps with the band's maximum as the lower and its minimum as the upper bound; kept
        for (int k = lane; k < XY; k += lanes) hf[k] = clamp_torch(noise[(size_t)s * XY + k], bmax[k], bmin[k]);
    } else if (cfg.mode == PARC_MDM_AUG_MAXPOOL_AND_BOXES) {
        const parc_mdm_draw_t d = draws[s];
        if (d.change_height)
            for (int k = lane; k < XY; k += lanes) hf[k] = d.new_height;
        PARC_MDM_SYNC();
        for (int q = 0; q < 3; ++q) {
            const int kind = d.pool_kind[q];
            if (kind != PARC_MDM_POOL_2D && kind != PARC_MDM_POOL_X && kind != PARC_MDM_POOL_Y) continue;
            int r = d.pool_radius[q];
            if (r < 0) r = 0;
            if (r > X + Y) r = X + Y;               // any radius >= the grid's size pools the whole line
            if (kind == PARC_MDM_POOL_2D) {
                // the (2r + 1)^2 window is the x pool of the y pool: max is exact in any order
                pool_pass(hf, tmp, X, Y, r, false, lane, lanes);
                PARC_MDM_SYNC();
                pool_pass(tmp, hf, X, Y, r, true, lane, lanes);
                PARC_MDM_SYNC();
                for (int k = lane; k < XY; k += lanes) hf[k] = clamp_torch(hf[k], bmin[k], bmax[k]);
            } else {
                pool_pass(hf, tmp, X, Y, r, kind == PARC_MDM_POOL_X, lane, lanes);
                PARC_MDM_SYNC();
                for (int k = lane; k < XY; k += lanes) hf[k] = clamp_torch(tmp[k], bmin[k], bmax[k]);
            }
            PARC_MDM_SYNC();
        }
        int nb = d.num_boxes;
        if (nb > cfg.max_boxes) nb = cfg.max_boxes;
        const parc_mdm_box_t *bx = boxes + (size_t)s * cfg.max_boxes;
        for (int k = lane; k < XY; k += lanes) {
            const int i = k / Y, j = k % Y;
            float h = hf[k];
            for (int b = 0; b < nb; ++b)
                if (in_box(bx[b], i, j)) h = bx[b].h;
            hf[k] = clamp_torch(h, bmin[k], bmax[k]);
        }
    }
    // then the clamp of sample_motion_data :308
    for (int k = lane; k < XY; k += lanes) out[k] = clamp_torch(hf[k], cfg.min_h, cfg.max_h);
}

PARC_MDM_HOST_FN size_t hf_lds_bytes(const parc_mdm_cfg_t &cfg, int mask_cells) {
    return (size_t)4 * cfg.dim_x * cfg.dim_y * sizeof(float) + (size_t)((mask_cells + 31) / 32) * sizeof(uint32_t);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// argument rules (host side of both entry points, before any HIP call)
// ---------------------------------------------------------------------------------------------------------------------------------
PARC_MDM_HOST_FN int check_cfg(const parc_mdm_cfg_t &cfg) {
    if (cfg.seq_len < 1 || cfg.ref_idx < 0 || cfg.ref_idx >= cfg.seq_len) return PARC_EINVAL;
    if (cfg.dim_x < 1 || cfg.dim_y < 1 || cfg.num_x_neg < 0 || cfg.num_x_neg >= cfg.dim_x || cfg.num_y_neg < 0 || cfg.num_y_neg >= cfg.dim_y)
        return PARC_EINVAL;
    if (cfg.z_style != PARC_MDM_Z_ROOT && cfg.z_style != PARC_MDM_Z_ROOT_FLOOR) return PARC_EINVAL;
    if (cfg.mode != PARC_MDM_AUG_NOISE && cfg.mode != PARC_MDM_AUG_MAXPOOL_AND_BOXES && cfg.mode != PARC_MDM_AUG_NONE) return PARC_EINVAL;
    if (cfg.max_boxes < 0) return PARC_EINVAL;
    if (cfg.seq_len > PARC_MDM_MAX_SEQ_LEN || (int64_t)cfg.dim_x * cfg.dim_y > PARC_MDM_MAX_LOCAL_CELLS || cfg.max_boxes > PARC_MDM_MAX_BOXES)
        return PARC_EUNSUPPORTED;
    return PARC_OK;
}

PARC_MDM_HOST_FN int check_heightfields(const parc_motion_lib_t &ml, const parc_mdm_cfg_t &cfg, int n, const void *motion_ids, const void *start_times,
                                        const void *motion_times, const void *grid_x, const void *grid_y, int n_clips, const void *clips,
                                        const void *pool, int64_t pool_floats, const void *cell_start, int64_t n_cell_start, const void *cells,
                                        int64_t n_cells, int mask_cells, const void *draws, const void *boxes, const void *noise, const void *hfs,
                                        const void *center_h) {
    if (n < 0 || n_clips < 0 || pool_floats < 0 || n_cell_start < 0 || n_cells < 0 || mask_cells < 0 || ml.num_motions < 0) return PARC_EINVAL;
    const int rc = check_cfg(cfg);
    if (rc != PARC_OK) return rc;
    if (mask_cells > PARC_MDM_MAX_TERRAIN_CELLS) return PARC_EUNSUPPORTED;
    if (n == 0) return PARC_MDM_NOTHING;
    if (!motion_ids || !start_times || !motion_times || !grid_x || !grid_y || !hfs || !center_h) return PARC_EINVAL;
    if (!ml.num_frames || !ml.start_idx || !ml.length || !ml.loop_mode || !ml.pos_delta || !ml.frames) return PARC_EINVAL;
    if ((n_clips > 0 && !clips) || (pool_floats > 0 && !pool) || (n_cell_start > 0 && !cell_start) || (n_cells > 0 && !cells)) return PARC_EINVAL;
    if (cfg.mode == PARC_MDM_AUG_MAXPOOL_AND_BOXES && (!draws || (cfg.max_boxes > 0 && !boxes))) return PARC_EINVAL;
    if (cfg.mode == PARC_MDM_AUG_NOISE && !noise) return PARC_EINVAL;
    return PARC_OK;
}

PARC_MDM_HOST_FN int check_windows(const parc_char_model_t &m, const parc_motion_lib_t &ml, const parc_mdm_cfg_t &cfg, int n, const void *motion_ids,
                                   const void *start_times, const void *motion_times, const void *future_time, const void *future_noise,
                                   const void *root_pos, const void *root_rot, const void *body_pos, const void *joint_rot, const void *contacts,
                                   const void *future_pos, const void *future_rot) {
    if (n < 0 || ml.num_motions < 0) return PARC_EINVAL;
    const int rc = check_cfg(cfg);
    if (rc != PARC_OK) return rc;
    if (m.num_bodies < 1 || m.num_bodies > PARC_MAX_BODIES || ml.num_bodies != m.num_bodies) return PARC_EINVAL;
    if ((int64_t)n * cfg.seq_len > 0x7fffffffLL - PARC_MDM_WIN_THREADS) return PARC_EUNSUPPORTED;
    if (n == 0) return PARC_MDM_NOTHING;
    if (!motion_ids || !start_times || !motion_times || !root_pos || !root_rot || !contacts) return PARC_EINVAL;
    if (m.num_bodies > 1 && (!body_pos || !joint_rot)) return PARC_EINVAL;
    if (!ml.num_frames || !ml.start_idx || !ml.length || !ml.loop_mode || !ml.pos_delta || !ml.frames) return PARC_EINVAL;
    const int given = (future_time ? 1 : 0) + (future_noise ? 1 : 0) + (future_pos ? 1 : 0) + (future_rot ? 1 : 0);
    if (given != 0 && given != 4) return PARC_EINVAL;
    return PARC_OK;
}

}  // namespace parc_mdm
