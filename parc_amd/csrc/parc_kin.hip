// Kinematic / observation / reward / termination / TD(lambda) kernels of the PARC tracker hot path,
// written for gfx950 (MI355X): 64-lane wavefronts, 16-lane body groups, LDS-staged observation rows.
// C-ABI in include/parc_hip.h.  Reference citations are relative to the reference root.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_math.h"
#include "parc_math_pk.h"
#include "parc_fk_group.h"     // GRP, shfl16, sum16, any16, fk_consts_of, group_fk
#include "parc_moopt_core.h"   // tt_args, tt_forward_body, tt_backward_body

// 4 floats moved by one 16-byte instruction from / to an address that is only 4-byte aligned (global memory takes it)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
// The observation rows are written with the non-temporal hint: a launch ends when its last dirty line has left the XCD's L2 (the L2s
// of the 8 XCDs are not coherent, the next kernel may read the row from another one), and 22 MB of rows held back until then were a
// 1 us tail; streamed out as they are produced they overlap the pose arithmetic (15.8 -> 14.7 us per launch, same box).
#ifndef POST_PLAIN_STORES
#define POST_STORE4(p, v) __builtin_nontemporal_store((v), reinterpret_cast<f4u *>(p))
#else
#define POST_STORE4(p, v) (*reinterpret_cast<f4u *>(p) = (v))
#endif

#define PARC_CHECK_LAUNCH()                         \
    do {                                            \
        hipError_t _e = hipGetLastError();          \
        if (_e != hipSuccess) return (int)_e;       \
    } while (0)

// =============================================================================================
// K5  local heightmap gather
// =============================================================================================
// One workgroup = HF_EPB consecutive envs; every thread owns one 16-byte output slot (4 ray points) whose
// template coordinates stay in registers across those envs, so a wave stores 1 KiB contiguous per
// instruction (the row's misaligned head/tail elements are slot 0 / the last slot).  The heightfield is
// L1/L2-resident (a 441-point fan touches ~100 cells), so the kernel is bound by instruction issue, not
// HBM: per env the lookup is folded into two affine maps in CELL units,
//     u_i = x*(c/dx) - y*(s/dx) + (gx-min_x)/dx ,   u_j = x*(s/dy) + y*(c/dy) + (gy-min_y)/dy
// (c,s = cos/sin of the heading taken directly from the rotated x axis: cos(atan2(b,a)) = a/|(a,b)|),
// then rndne + clamp + one load per point.  This reassociates the reference's fp32 expression
// (rotate, add root, subtract min, divide): values agree except for queries within a few ulp of a cell
// boundary (tests bound this), the returned heights themselves are exact copies.
#define HF_THREADS 128

// util/terrain_util.py:107-126: torch.round (half to even) then clamp to the grid
PARC_DEV float hf_lookup(const parc_terrain_t &t, float px, float py) {
    float fi = rintf((px - t.min_x) / t.dx);
    float fj = rintf((py - t.min_y) / t.dy);
    fi = fminf(fmaxf(fi, 0.f), (float)(t.dim_x - 1));
    fj = fminf(fmaxf(fj, 0.f), (float)(t.dim_y - 1));
    return t.hf[(int)fi * t.dim_y + (int)fj];
}

struct hf_env_prm {
    float ax, bx, cx, ay, by, cy, gz;
};

template <bool FROM_STATE>
PARC_DEV hf_env_prm hf_env_params(int e, const float *__restrict__ root, const float *__restrict__ aux, const parc_terrain_t &ter,
                                  float inv_dx, float inv_dy) {
    float gx, gy, gz, c, s;
    if (FROM_STATE) {
        // ig_parkour_env.py:640-641: global xyz = root pos + env offset; heading of R(q) e_x (torch_util.py:470-479)
        const float *rs = root + (size_t)e * 13;
        gx = rs[0] + aux[3 * e + 0];
        gy = rs[1] + aux[3 * e + 1];
        gz = rs[2] + aux[3 * e + 2];
        float qx = rs[3], qy = rs[4], qz = rs[5], qw = rs[6];
        float a = 1.0f - 2.0f * (qy * qy + qz * qz);
        float b = 2.0f * (qw * qz + qx * qy);
        float n2 = a * a + b * b;
        float inv = rsqrtf(n2);
        c = n2 > 0.f ? a * inv : 1.0f;   // atan2(0,0) = 0
        s = n2 > 0.f ? b * inv : 0.0f;
    } else {
        gx = root[3 * e + 0];
        gy = root[3 * e + 1];
        gz = root[3 * e + 2];
        sincosf(aux[e], &s, &c);
    }
    hf_env_prm p;
    p.ax = c * inv_dx;
    p.bx = -s * inv_dx;
    p.cx = (gx - ter.min_x) * inv_dx;
    p.ay = s * inv_dy;
    p.by = c * inv_dy;
    p.cy = (gy - ter.min_y) * inv_dy;
    p.gz = gz;
    return p;
}

// HF_G: groups of HF_THREADS threads per workgroup, each group working on its own HF_EPB envs (fewer, fatter workgroups for the
// same number of waves: at 4096 envs the launch is dispatch-bound)
template <bool FROM_STATE, int HF_EPB, int ABL = 0, int HF_G = 1>
__global__ __launch_bounds__(HF_THREADS *HF_G) void hf_gather_kernel(int n_envs, const float *__restrict__ ray_xy, int n_points,
                                                                      const float *__restrict__ root, const float *__restrict__ aux,
                                                                      parc_terrain_t ter, float min_h, float max_h,
                                                                      float *__restrict__ out, int64_t out_stride, int head) {
    const int tid = threadIdx.x % HF_THREADS;
    const int e0 = (blockIdx.x * HF_G + threadIdx.x / HF_THREADS) * HF_EPB;
    if (HF_G > 1 && e0 >= n_envs) return;
    const float inv_dx = 1.0f / ter.dx, inv_dy = 1.0f / ter.dy;
    const float max_i = (float)(ter.dim_x - 1), max_j = (float)(ter.dim_y - 1);
    hf_env_prm prm[HF_EPB];
    const unsigned out_bytes = (unsigned)min((unsigned long long)n_envs * (unsigned long long)out_stride * 4ull, 0xFFFFFFFFull);
    __amdgpu_buffer_rsrc_t out_rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, out_bytes, 0x00020000);
#pragma unroll
    for (int ee = 0; ee < HF_EPB; ++ee) prm[ee] = hf_env_params<FROM_STATE>(min(e0 + ee, n_envs - 1), root, aux, ter, inv_dx, inv_dy);
    // slot 0: the `head` leading scalars; slots 1..nbody: aligned float4s; last slot: trailing scalars
    const int nbody = (n_points - head) >> 2;
    const int tail = n_points - head - 4 * nbody;
    const int nslots = nbody + 2;
    for (int q = tid; q < nslots; q += HF_THREADS) {
        int p0, cnt;
        if (q == 0) {
            p0 = 0;
            cnt = head;
        } else if (q <= nbody) {
            p0 = head + 4 * (q - 1);
            cnt = 4;
        } else {
            p0 = head + 4 * nbody;
            cnt = tail;
        }
        if (cnt == 0) continue;
        float rx[4], ry[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int p = min(p0 + i, n_points - 1);
            rx[i] = ray_xy[2 * p];
            ry[i] = ray_xy[2 * p + 1];
        }
        float h[HF_EPB][4];
#pragma unroll
        for (int ee = 0; ee < HF_EPB; ++ee) {
            const hf_env_prm pr = prm[ee];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float ui = fmaf(rx[i], pr.ax, fmaf(ry[i], pr.bx, pr.cx));
                float uj = fmaf(rx[i], pr.ay, fmaf(ry[i], pr.by, pr.cy));
                ui = __builtin_amdgcn_fmed3f(rintf(ui), 0.f, max_i);
                uj = __builtin_amdgcn_fmed3f(rintf(uj), 0.f, max_j);
                float v = ((ABL == 1 || ABL == 5) ? (ui + uj) : ter.hf[(int)ui * ter.dim_y + (int)uj]) - pr.gz;
                h[ee][i] = __builtin_amdgcn_fmed3f(v, min_h, max_h);
            }
        }
#pragma unroll
        for (int ee = 0; ee < HF_EPB; ++ee) {
            int e = e0 + ee;
            if (e >= n_envs) break;
            const size_t off = (size_t)e * out_stride + p0;
            float *o = out + off;
            if (ABL == 2 || ABL == 5) {
                if (h[ee][0] + h[ee][1] + h[ee][2] + h[ee][3] == 12345.678f) o[0] = 1.f;   // ablation: keep the math, drop the stores
            } else if (cnt == 4) {
                if (ABL == 3 || ABL == 4) {
                    typedef float f32x4 __attribute__((ext_vector_type(4)));
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    f32x4 v = {h[ee][0], h[ee][1], h[ee][2], h[ee][3]};
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out_rsrc, (unsigned)(off * 4), 0, ABL == 3 ? 16 : 2);
                } else {
                    *reinterpret_cast<float4 *>(o) = make_float4(h[ee][0], h[ee][1], h[ee][2], h[ee][3]);
                }
            } else {
                for (int i = 0; i < cnt; ++i) o[i] = h[ee][i];
            }
        }
    }
}

// generic fallback (arbitrary row alignment): one thread per output value
template <bool FROM_STATE>
__global__ __launch_bounds__(256) void hf_gather_scalar_kernel(int n_envs, const float *__restrict__ ray_xy, int n_points,
                                                               const float *__restrict__ root, const float *__restrict__ aux,
                                                               parc_terrain_t ter, float min_h, float max_h,
                                                               float *__restrict__ out, int64_t out_stride) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n_envs * n_points) return;
    int e = (int)(idx / n_points), p = (int)(idx % n_points);
    float gx, gy, gz, hd;
    if (FROM_STATE) {
        const float *rs = root + (size_t)e * 13;
        gx = rs[0] + aux[3 * e + 0];
        gy = rs[1] + aux[3 * e + 1];
        gz = rs[2] + aux[3 * e + 2];
        hd = calc_heading(ld4(rs + 3));
    } else {
        gx = root[3 * e + 0];
        gy = root[3 * e + 1];
        gz = root[3 * e + 2];
        hd = aux[e];
    }
    float c = cosf(hd), s = sinf(hd);
    float x = ray_xy[2 * p], y = ray_xy[2 * p + 1];
    float v = hf_lookup(ter, (x * c - y * s) + gx, (x * s + y * c) + gy) - gz;
    out[(size_t)e * out_stride + p] = fminf(fmaxf(v, min_h), max_h);
}

// Measurement knobs of the standalone heightmap kernel exist only in the diagnostics build (-DPARC_DIAG_BUILD: tools/parc_diag.py builds
// libparc_hip_diag.so, tools/parc_diag.h declares its extra entry points); the product library has them as constants and
// exports no setter, so nothing a test or tool does can leave a later product launch on another kernel.
#ifdef PARC_DIAG_BUILD
static int g_hf_epb = 2;
static int g_hf_groups = 1;   // 128-thread env groups per workgroup (1, 2, 4, 8)
static int g_hf_abl = 0;      // timing-only ablations (outputs wrong): 1 no gather, 2 no stores, ...
#define PARC_DIAG(...) __VA_ARGS__
#else
static constexpr int g_hf_epb = 2;
#define PARC_DIAG(...)
#endif

static int launch_hf(bool from_state, void *stream, int n_envs, const float *ray_xy, int n_points, const float *root,
                     const float *aux, parc_terrain_t ter, float min_h, float max_h, float *out, int64_t out_stride) {
    if (n_envs < 0 || n_points <= 0 || !ray_xy || !root || !aux || !out || !ter.hf || out_stride < n_points) return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    int head;
    if ((out_stride & 3) == 0) {
        head = (int)(((16 - ((uintptr_t)out & 15)) & 15) >> 2);  // same misalignment on every row
        if (head > n_points) head = n_points;
    } else {
        head = n_points;  // rows are differently aligned: all-scalar path through slot 0 (not vectorised)
    }
    hipStream_t st = (hipStream_t)stream;
    if (head == n_points && n_points > 3) {
        // rows are not uniformly 16-byte aligned: one thread per point, dword stores
        long total = (long)n_envs * n_points;
        dim3 g2((unsigned)((total + 255) / 256)), b2(256);
        if (from_state)
            hipLaunchKernelGGL(hf_gather_scalar_kernel<true>, g2, b2, 0, st, n_envs, ray_xy, n_points, root, aux, ter, min_h, max_h, out, out_stride);
        else
            hipLaunchKernelGGL(hf_gather_scalar_kernel<false>, g2, b2, 0, st, n_envs, ray_xy, n_points, root, aux, ter, min_h, max_h, out, out_stride);
        PARC_CHECK_LAUNCH();
        return PARC_OK;
    }
#define HF_LAUNCH3(FS, EPB, AB)                                                                                          \
    hipLaunchKernelGGL((hf_gather_kernel<FS, EPB, AB>), dim3((n_envs + EPB - 1) / EPB), dim3(HF_THREADS), 0, st, n_envs, ray_xy, \
                       n_points, root, aux, ter, min_h, max_h, out, out_stride, head)
#define HF_LAUNCH(FS, EPB)                                                                                               \
    hipLaunchKernelGGL((hf_gather_kernel<FS, EPB>), dim3((n_envs + EPB - 1) / EPB), dim3(HF_THREADS), 0, st, n_envs, ray_xy, \
                       n_points, root, aux, ter, min_h, max_h, out, out_stride, head)
    const int epb = g_hf_epb;
#ifdef PARC_DIAG_BUILD
#define HF_LAUNCH_G(AB, G)                                                                                                              \
    hipLaunchKernelGGL((hf_gather_kernel<true, 2, AB, G>), dim3((n_envs + 2 * G - 1) / (2 * G)), dim3(HF_THREADS * G), 0, st, n_envs, ray_xy, \
                       n_points, root, aux, ter, min_h, max_h, out, out_stride, head)
    if (from_state && g_hf_groups > 1) {
        const bool empty = g_hf_abl == 5;
        if (g_hf_groups == 2) { if (empty) HF_LAUNCH_G(5, 2); else HF_LAUNCH_G(0, 2); }
        else if (g_hf_groups == 4) { if (empty) HF_LAUNCH_G(5, 4); else HF_LAUNCH_G(0, 4); }
        else { if (empty) HF_LAUNCH_G(5, 8); else HF_LAUNCH_G(0, 8); }
        PARC_CHECK_LAUNCH();
        return PARC_OK;
    }
#undef HF_LAUNCH_G
    if (from_state && g_hf_abl == 1) HF_LAUNCH3(true, 2, 1);
    else if (from_state && g_hf_abl == 2) HF_LAUNCH3(true, 2, 2);
    else if (from_state && g_hf_abl == 3) HF_LAUNCH3(true, 2, 3);
    else if (from_state && g_hf_abl == 4) HF_LAUNCH3(true, 2, 4);
    else if (from_state && g_hf_abl == 5) HF_LAUNCH3(true, 2, 5);
    else
#endif
    if (from_state) {
        if (epb == 1) HF_LAUNCH(true, 1);
        else if (epb == 4) HF_LAUNCH(true, 4);
        else if (epb == 8) HF_LAUNCH(true, 8);
        else HF_LAUNCH(true, 2);
    } else {
        if (epb == 1) HF_LAUNCH(false, 1);
        else if (epb == 4) HF_LAUNCH(false, 4);
        else if (epb == 8) HF_LAUNCH(false, 8);
        else HF_LAUNCH(false, 2);
    }
#undef HF_LAUNCH
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

#ifdef PARC_DIAG_BUILD
// tuning knob (envs per workgroup of the heightmap kernel: 1, 2, 4 or 8); not part of the stable ABI
extern "C" int parc_tune_hf_groups(int g) {
    if (g != 1 && g != 2 && g != 4 && g != 8) return PARC_EINVAL;
    g_hf_groups = g;
    return PARC_OK;
}
extern "C" int parc_tune_hf_ablation(int a) {
    g_hf_abl = a;
    return PARC_OK;
}

extern "C" int parc_tune_hf_envs_per_block(int epb) {
    if (epb != 1 && epb != 2 && epb != 4 && epb != 8) return PARC_EINVAL;
    g_hf_epb = epb;
    return PARC_OK;
}
#endif

extern "C" int parc_refresh_ray_obs_hfs(void *stream, int n_envs, const float *ray_xy, int n_points, const float *root_pos_xyz,
                                        const float *heading, parc_terrain_t terrain, float min_h, float max_h, float *out,
                                        int64_t out_stride) {
    return launch_hf(false, stream, n_envs, ray_xy, n_points, root_pos_xyz, heading, terrain, min_h, max_h, out, out_stride);
}

extern "C" int parc_refresh_obs_hfs(void *stream, int n_envs, const float *ray_xy, int n_points, const float *root_state,
                                    const float *env_offsets, parc_terrain_t terrain, float min_h, float max_h, float *out,
                                    int64_t out_stride) {
    return launch_hf(true, stream, n_envs, ray_xy, n_points, root_state, env_offsets, terrain, min_h, max_h, out, out_stride);
}

// =============================================================================================
// Body-per-lane helpers: a pose is handled by a 16-lane group, lane b = body b (b = 0 root).
// =============================================================================================

static bool model_ok(const parc_char_model_t &m) { return m.num_bodies >= 1 && m.num_bodies <= PARC_MAX_BODIES && m.dof_size <= PARC_MAX_DOFS; }

// anim/kin_char_model.py:57-77: one joint's dofs -> quaternion (lane b >= 1)
template <bool LIB = false>
PARC_DEV q4 joint_dof_to_rot(const parc_char_model_t &m, int b, const float *dof, int stride) {
    int jt = m.joint_type[b];
    if (jt == PARC_JOINT_HINGE) {
        v3 ax = mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]);
        float an = dof[m.dof_idx[b] * stride];
        return LIB ? axis_angle_to_quat_lib(ax, an) : axis_angle_to_quat(ax, an);
    } else if (jt == PARC_JOINT_SPHERICAL) {
        int d = m.dof_idx[b];
        v3 em = mk3(dof[d * stride], dof[(d + 1) * stride], dof[(d + 2) * stride]);
        return LIB ? exp_map_to_quat_lib(em) : exp_map_to_quat(em);
    }
    return mk4(0.f, 0.f, 0.f, 1.f);
}

// the same with the joint's constants already at hand (type, first dof, hinge axis)
// Both joint kinds end in axis_angle_to_quat (exp_map_to_quat of parc_math.h = the steps below, then that call): the lanes of a group
// differ in kind, so each kind's branch only prepares (axis, angle) and the common tail is issued once instead of once per kind.
PARC_DEV q4 joint_dof_to_rot(int jt, int d, v3 ax, const float *dof, int stride) {
    float an = 0.f;
    if (jt == PARC_JOINT_HINGE) {
        an = dof[d * stride];
    } else if (jt == PARC_JOINT_SPHERICAL) {
        const v3 em = mk3(dof[d * stride], dof[(d + 1) * stride], dof[(d + 2) * stride]);
        float a = fsqrt(dot3(em, em));
        const float ia = frcp(a);
        ax = v3{em.x * ia, em.y * ia, em.z * ia};
        if (!(a < 3.1415925f)) a = normalize_angle(a);       // identity below pi
        if (!(fabsf(a) > 1e-5f)) {
            ax = mk3(0.f, 0.f, 1.f);
            a = 0.f;
        }
        an = a;
    }
    const q4 q = axis_angle_to_quat(ax, an);
    return (jt == PARC_JOINT_HINGE || jt == PARC_JOINT_SPHERICAL) ? q : mk4(0.f, 0.f, 0.f, 1.f);
}

// anim/kin_char_model.py:79-100: one joint's quaternion -> dofs
// (dof2, when given, receives the same values at stride 2: the position slots of an interleaved dof_state row)
PARC_DEV void joint_rot_to_dof(const parc_char_model_t &m, int b, q4 q, float *dof, float *dof2 = nullptr) {
    int jt = m.joint_type[b];
    if (jt == PARC_JOINT_HINGE) {
        v3 ax;
        float an;
        quat_to_axis_angle(q, ax, an);
        float d = m.joint_axis[b][0] * ax.x + m.joint_axis[b][1] * ax.y + m.joint_axis[b][2] * ax.z;
        if (d < 0.f) an *= -1.f;
        dof[m.dof_idx[b]] = an;
        if (dof2) dof2[2 * m.dof_idx[b]] = an;
    } else if (jt == PARC_JOINT_SPHERICAL) {
        v3 e = quat_to_exp_map(q);
        int d = m.dof_idx[b];
        dof[d] = e.x;
        dof[d + 1] = e.y;
        dof[d + 2] = e.z;
        if (dof2) {
            dof2[2 * d] = e.x;
            dof2[2 * d + 2] = e.y;
            dof2[2 * d + 4] = e.z;
        }
    }
}

// ---- the same on two poses per lane (parc_math_pk.h): the cross-lane moves are per component, the arithmetic is packed
PARC_DEV f2 shfl16(f2 v, int src) { return f2{shfl16(v.x, src), shfl16(v.y, src)}; }
PARC_DEV q4p shfl16(q4p q, int src) { return q4p{shfl16(q.x, src), shfl16(q.y, src), shfl16(q.z, src), shfl16(q.w, src)}; }
PARC_DEV v3p shfl16(v3p v, int src) { return v3p{shfl16(v.x, src), shfl16(v.y, src), shfl16(v.z, src)}; }
template <bool LEAF_ROT = true>
PARC_DEV void group_fk(const fk_consts &k, int max_depth, v3p root_pos, q4p root_rot, q4p jq, v3p &pos, q4p &rot) {
    q4p lq = sp4(mk4(0.f, 0.f, 0.f, 1.f));
    if (k.dep > 0) lq = quat_mul(sp4(k.lrot), jq);
    const v3p lt = sp3(k.lt);
    pos = root_pos;
    rot = root_rot;
    for (int lev = 1; lev <= max_depth; ++lev) {
        v3p pp = shfl16(pos, k.par);
        q4p pr = shfl16(rot, k.par);
        if (k.dep == lev) {
            pos = pp + quat_rotate(pr, lt);
            if (LEAF_ROT || lev < max_depth) rot = quat_mul(pr, lq);
        }
    }
}

struct frame_query {
    const float *row0, *row1;
    float blend, loop_phase;
    int wrap, idx0, idx1;     // idx = absolute frame row
};

// anim/motion_lib.py:443-456,527-538 (+ :458-475 loop offset)
PARC_DEV frame_query make_query(const parc_motion_lib_t &ml, int64_t id, float time) {
    frame_query fq;
    float len = ml.length[id];
    fq.wrap = ml.loop_mode[id] == 1;
    float phase = time / len;
    fq.loop_phase = floorf(phase);
    if (fq.wrap) phase = phase - floorf(phase);
    phase = fminf(fmaxf(phase, 0.f), 1.f);
    int nf = ml.num_frames[id];
    float fp = phase * (float)(nf - 1);
    int i0 = (int)fp;
    int i1 = min(i0 + 1, nf - 1);
    fq.blend = fp - (float)i0;
    int st = ml.start_idx[id];
    fq.idx0 = st + i0;
    fq.idx1 = st + i1;
    fq.row0 = ml.frames + (size_t)fq.idx0 * ml.row_stride;
    fq.row1 = ml.frames + (size_t)fq.idx1 * ml.row_stride;
    return fq;
}

// lane b: slerped quaternion b of the frame pair (b = 0 root rotation, b >= 1 joint b-1)
PARC_DEV q4 query_quat(const frame_query &fq, int b) {
    float4 a = *reinterpret_cast<const float4 *>(fq.row0 + 4 * b);
    float4 c = *reinterpret_cast<const float4 *>(fq.row1 + 4 * b);
    return slerp(mk4(a.x, a.y, a.z, a.w), mk4(c.x, c.y, c.z, c.w), fq.blend);
}

PARC_DEV float lerp_ref(float a, float b, float t) { return (1.0f - t) * a + t * b; }

PARC_DEV v3 query_root_pos(const parc_motion_lib_t &ml, const frame_query &fq, int64_t id) {
    const float *p0 = fq.row0 + ml.off_pos, *p1 = fq.row1 + ml.off_pos;
    v3 p = mk3(lerp_ref(p0[0], p1[0], fq.blend), lerp_ref(p0[1], p1[1], fq.blend), lerp_ref(p0[2], p1[2], fq.blend));
    if (fq.wrap) {
        const float *d = ml.pos_delta + 3 * id;
        p = p + mk3(fq.loop_phase * d[0], fq.loop_phase * d[1], fq.loop_phase * d[2]);
    }
    return p;
}

// =============================================================================================
// K3 standalone (16 lanes per query, 4 queries per wave)
// =============================================================================================
__global__ __launch_bounds__(256) void motion_frame_kernel(parc_motion_lib_t ml, int nq, const int64_t *__restrict__ ids,
                                                           const float *__restrict__ times, float *root_pos, float *root_rot,
                                                           float *root_vel, float *root_ang_vel, float *joint_rot,
                                                           float *dof_vel, float *contacts) {
    int q = (blockIdx.x * blockDim.x + threadIdx.x) / GRP;
    int b = threadIdx.x % GRP;
    if (q >= nq) return;
    const int B = ml.num_bodies, J = B - 1, D = ml.dof_size;
    int64_t id = ids[q];
    frame_query fq = make_query(ml, id, times[q]);
    if (b < B) {
        q4 r = query_quat(fq, b);
        if (b == 0) st4(root_rot + 4 * (size_t)q, r);
        else st4(joint_rot + ((size_t)q * J + (b - 1)) * 4, r);
        contacts[(size_t)q * B + b] = lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend);
    }
    if (b == 0) {
        st3(root_pos + 3 * (size_t)q, query_root_pos(ml, fq, id));
        st3(root_vel + 3 * (size_t)q, ld3(fq.row0 + ml.off_root_vel));
        st3(root_ang_vel + 3 * (size_t)q, ld3(fq.row0 + ml.off_root_ang_vel));
    }
    for (int d = b; d < D; d += GRP) dof_vel[(size_t)q * D + d] = fq.row0[ml.off_dof_vel + d];
}

extern "C" int parc_calc_motion_frame(void *stream, parc_motion_lib_t mlib, int nq, const int64_t *ids, const float *times,
                                      float *root_pos, float *root_rot, float *root_vel, float *root_ang_vel, float *joint_rot,
                                      float *dof_vel, float *contacts) {
    if (nq < 0 || mlib.num_bodies > PARC_MAX_BODIES || (mlib.row_stride & 3)) return PARC_EINVAL;
    if (nq == 0) return PARC_OK;
    int threads = 256, per = threads / GRP;
    hipLaunchKernelGGL(motion_frame_kernel, dim3((nq + per - 1) / per), dim3(threads), 0, (hipStream_t)stream, mlib, nq, ids, times,
                       root_pos, root_rot, root_vel, root_ang_vel, joint_rot, dof_vel, contacts);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}


// =============================================================================================
// Clip database build: MotionLib._load_motions  anim/motion_lib.py:264-290,405-423 and
// KinCharModel.compute_frame_dof_vel  anim/kin_char_model.py:543-581, for ALL clips in one launch.
// pass 1: pose rows (quaternions, root position, contacts); pass 2: finite-difference velocities.
// =============================================================================================
__global__ __launch_bounds__(256) void motion_rows_kernel(parc_char_model_t m, parc_motion_lib_t ml, int total_frames,
                                                          const float *__restrict__ frames, const float *__restrict__ contacts,
                                                          float *rows) {
    int f = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (f >= total_frames || b >= m.num_bodies) return;
    const float *fr = frames + (size_t)f * (6 + m.dof_size);
    float *row = rows + (size_t)f * ml.row_stride;
    q4 q;
    if (b == 0) {
        q = exp_map_to_quat_lib(mk3(fr[3], fr[4], fr[5]));        // motion_lib.py:418
        st3(row + ml.off_pos, ld3(fr));
    } else {
        q = quat_pos(joint_dof_to_rot<true>(m, b, fr + 6, 1));     // motion_lib.py:420-421
    }
    st4(row + 4 * b, q);
    row[ml.off_contacts + b] = contacts ? contacts[(size_t)f * m.num_bodies + b] : 0.f;
}

__global__ __launch_bounds__(256) void motion_vel_kernel(parc_char_model_t m, parc_motion_lib_t ml, int total_frames,
                                                         const int32_t *__restrict__ frame_clip, const float *__restrict__ clip_fps,
                                                         float *rows) {
    int f = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (f >= total_frames || b >= m.num_bodies) return;
    int c = frame_clip[f];
    int nf = ml.num_frames[c], st = ml.start_idx[c];
    float *row = rows + (size_t)f * ml.row_stride;
    if (nf < 2) {
        if (b == 0) {
            st3(row + ml.off_root_vel, mk3(0.f, 0.f, 0.f));
            st3(row + ml.off_root_ang_vel, mk3(0.f, 0.f, 0.f));
        }
        for (int d = b; d < m.dof_size; d += GRP) row[ml.off_dof_vel + d] = 0.f;
        return;
    }
    int f0 = min(f - st, nf - 2) + st;  // the last frame repeats the previous difference (motion_lib.py:283,288)
    const float *r0 = rows + (size_t)f0 * ml.row_stride, *r1 = r0 + ml.row_stride;
    float fps = clip_fps[c];
    float dt = 1.0f / fps;
    if (b == 0) {
        v3 p0 = ld3(r0 + ml.off_pos), p1 = ld3(r1 + ml.off_pos);
        st3(row + ml.off_root_vel, fps * (p1 - p0));                                        // :281-283
        v3 em = quat_to_exp_map(quat_mul(ld4(r1), quat_conj(ld4(r0))));                     // quat_diff :286-287
        st3(row + ml.off_root_ang_vel, fps * em);
    } else {
        q4 dr = quat_unit(quat_pos(quat_mul(quat_conj(ld4(r0 + 4 * b)), ld4(r1 + 4 * b))));  // kin_char_model.py:558-559
        int jt = m.joint_type[b];
        if (jt == PARC_JOINT_HINGE) {
            v3 e = quat_to_exp_map(dr);
            row[ml.off_dof_vel + m.dof_idx[b]] = m.joint_axis[b][0] * (e.x / dt) + m.joint_axis[b][1] * (e.y / dt) + m.joint_axis[b][2] * (e.z / dt);
        } else if (jt == PARC_JOINT_SPHERICAL) {
            v3 e = quat_to_exp_map(dr);
            float *o = row + ml.off_dof_vel + m.dof_idx[b];
            o[0] = e.x / dt;
            o[1] = e.y / dt;
            o[2] = e.z / dt;
        }
    }
}

extern "C" int parc_motion_lib_build(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, int total_frames,
                                     const float *frames, const float *contacts, const int32_t *frame_clip, const float *clip_fps,
                                     float *rows) {
    if (!model_ok(model) || total_frames < 0 || mlib.num_bodies != model.num_bodies || (mlib.row_stride & 3)) return PARC_EINVAL;
    if (total_frames == 0) return PARC_OK;
    dim3 grid((total_frames + 15) / 16), block(256);
    (void)hipMemsetAsync(rows, 0, sizeof(float) * (size_t)total_frames * mlib.row_stride, (hipStream_t)stream);
    hipLaunchKernelGGL(motion_rows_kernel, grid, block, 0, (hipStream_t)stream, model, mlib, total_frames, frames, contacts, rows);
    hipLaunchKernelGGL(motion_vel_kernel, grid, block, 0, (hipStream_t)stream, model, mlib, total_frames, frame_clip, clip_fps, rows);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K1 / K4 / K2 standalone (16 lanes per pose)
// =============================================================================================
__global__ __launch_bounds__(256) void dof_to_rot_kernel(parc_char_model_t m, int n, const float *__restrict__ dof, float *jrot) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (i >= n || b == 0 || b >= m.num_bodies) return;
    st4(jrot + ((size_t)i * (m.num_bodies - 1) + (b - 1)) * 4, joint_dof_to_rot(m, b, dof + (size_t)i * m.dof_size, 1));
}

__global__ __launch_bounds__(256) void rot_to_dof_kernel(parc_char_model_t m, int n, const float *__restrict__ jrot, float *dof) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    if (i >= n || b == 0 || b >= m.num_bodies) return;
    joint_rot_to_dof(m, b, ld4(jrot + ((size_t)i * (m.num_bodies - 1) + (b - 1)) * 4), dof + (size_t)i * m.dof_size);
}

__global__ __launch_bounds__(256) void fk_kernel(parc_char_model_t m, int n, const float *__restrict__ root_pos,
                                                 const float *__restrict__ root_rot, const float *__restrict__ jrot,
                                                 float *body_pos, float *body_rot) {
    int i = (blockIdx.x * blockDim.x + threadIdx.x) / GRP, b = threadIdx.x % GRP;
    bool live = i < n;
    int ii = live ? i : 0;
    q4 jq = mk4(0.f, 0.f, 0.f, 1.f);
    if (b >= 1 && b < m.num_bodies) jq = ld4(jrot + ((size_t)ii * (m.num_bodies - 1) + (b - 1)) * 4);
    v3 pos;
    q4 rot;
    group_fk(m, b, ld3(root_pos + 3 * (size_t)ii), ld4(root_rot + 4 * (size_t)ii), jq, pos, rot);
    if (live && b < m.num_bodies) {
        st3(body_pos + ((size_t)i * m.num_bodies + b) * 3, pos);
        st4(body_rot + ((size_t)i * m.num_bodies + b) * 4, rot);
    }
}

extern "C" int parc_dof_to_rot(void *stream, parc_char_model_t model, int n, const float *dof, float *joint_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(dof_to_rot_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, dof, joint_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_rot_to_dof(void *stream, parc_char_model_t model, int n, const float *joint_rot, float *dof) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    (void)hipMemsetAsync(dof, 0, sizeof(float) * (size_t)n * model.dof_size, (hipStream_t)stream);
    hipLaunchKernelGGL(rot_to_dof_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, joint_rot, dof);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_forward_kinematics(void *stream, parc_char_model_t model, int n, const float *root_pos, const float *root_rot,
                                       const float *joint_rot, float *body_pos, float *body_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(fk_kernel, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, model, n, root_pos, root_rot, joint_rot,
                       body_pos, body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Pose chain with its adjoint, one thread per frame: (root position, root exponential map, joint dofs) -> root quaternion, joint
// rotations, body positions / rotations, and the vector-Jacobian product back.  This is what stage 2's motion optimiser
// differentiates thousands of times per clip (tools/motion_opt/motion_optimization.py:203-213: exp_map_to_quat, KinCharModel.dof_to_rot,
// forward_kinematics and their autograd); as torch ops it is ~190 autograd nodes per evaluation, here two launches.
// Forward uses the library-precision maps (the values torch computes); the adjoint is exact for those formulas:
//   q = a (x) b  bilinear          =>  g_a = g (x) conj(b),  g_b = conj(a) (x) g
//   r = v + w t + u x t, t = 2 u x v  =>  g_w = g.t,  g_t = w g + g x u,  g_u = t x g + 2 v x g_t
//   q = unit(n(axis) sin h, cos h), h = angle / 2   (torch_util.axis_angle_to_quat: both normalisations are projections at unit length)
// =============================================================================================
struct aa_grad { v3 g_axis; float g_angle; };

PARC_DEV aa_grad axis_angle_to_quat_bwd(v3 axis, float angle, q4 q, q4 g) {
    // through quat_unit: q = raw / |raw| with |raw| = 1 up to rounding -> g_raw = g - (g.q) q
    const float gq = g.x * q.x + g.y * q.y + g.z * q.z + g.w * q.w;
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

// torch_util.exp_map_to_quat = axis_angle_to_quat(e / |e|, wrap(|e|)), z axis / angle 0 below 1e-5 (that branch is constant)
PARC_DEV v3 exp_map_to_quat_bwd(v3 em, q4 q, q4 g) {
    const float raw = sqrtf((em.x * em.x + em.y * em.y) + em.z * em.z);
    const float ang = atan2f(sinf(raw), cosf(raw));
    if (!(fabsf(ang) > 1e-5f)) return mk3(0.f, 0.f, 0.f);
    const v3 a = mk3(em.x / raw, em.y / raw, em.z / raw);
    const aa_grad ag = axis_angle_to_quat_bwd(a, ang, q, g);
    // axis = e / raw: J^T g = (g - (g.a) a) / raw;  angle = wrap(raw): d/de = a
    const float ga = dot3(ag.g_axis, a);
    return mk3((ag.g_axis.x - ga * a.x) / raw + ag.g_angle * a.x, (ag.g_axis.y - ga * a.y) / raw + ag.g_angle * a.y,
               (ag.g_axis.z - ga * a.z) / raw + ag.g_angle * a.z);
}

PARC_DEV q4 qadd(q4 a, q4 b) { return q4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// cotangent of q for r = quat_rotate(q, v) = v + w t + u x t, t = 2 u x v (u = q.xyz), given the cotangent g of r
PARC_DEV q4 quat_rotate_bwd_q(q4 q, v3 v, v3 g) {
    const v3 u = mk3(q.x, q.y, q.z);
    const v3 t = 2.f * cross3(u, v);
    const v3 gxu = cross3(g, u);
    const v3 gt = mk3(q.w * g.x + gxu.x, q.w * g.y + gxu.y, q.w * g.z + gxu.z);
    const v3 gu = cross3(t, g) + 2.f * cross3(v, gt);
    return q4{gu.x, gu.y, gu.z, dot3(g, t)};
}

__global__ __launch_bounds__(64) void pose_chain_fwd_kernel(parc_char_model_t m, int n, const float *__restrict__ root_pos,
                                                            const float *__restrict__ root_exp, const float *__restrict__ dof,
                                                            float *root_quat, float *joint_rot, float *body_pos, float *body_rot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int B = m.num_bodies;
    q4 rot[PARC_MAX_BODIES];
    v3 pos[PARC_MAX_BODIES];
    rot[0] = exp_map_to_quat_lib(ld3(root_exp + 3 * (size_t)i));
    pos[0] = ld3(root_pos + 3 * (size_t)i);
    st4(root_quat + 4 * (size_t)i, rot[0]);
    const float *d = dof + (size_t)i * m.dof_size;
    for (int b = 1; b < B; ++b) {
        const int p = m.parent[b];
        const q4 jq = joint_dof_to_rot<true>(m, b, d, 1);
        st4(joint_rot + ((size_t)i * (B - 1) + (b - 1)) * 4, jq);
        const q4 loc = quat_mul(mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]), jq);
        rot[b] = quat_mul(rot[p], loc);
        pos[b] = pos[p] + quat_rotate(rot[p], mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]));
    }
    for (int b = 0; b < B; ++b) {
        st3(body_pos + ((size_t)i * B + b) * 3, pos[b]);
        st4(body_rot + ((size_t)i * B + b) * 4, rot[b]);
    }
}

__global__ __launch_bounds__(64) void pose_chain_bwd_kernel(parc_char_model_t m, int n, const float *__restrict__ root_exp,
                                                            const float *__restrict__ dof, const float *__restrict__ g_root_quat,
                                                            const float *__restrict__ g_joint_rot, const float *__restrict__ g_body_pos,
                                                            const float *__restrict__ g_body_rot, float *g_root_pos, float *g_root_exp,
                                                            float *g_dof) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int B = m.num_bodies;
    q4 rot[PARC_MAX_BODIES], jq[PARC_MAX_BODIES], loc[PARC_MAX_BODIES], grot[PARC_MAX_BODIES];
    v3 gpos[PARC_MAX_BODIES];
    const v3 em = ld3(root_exp + 3 * (size_t)i);
    const float *d = dof + (size_t)i * m.dof_size;
    float *gd = g_dof + (size_t)i * m.dof_size;
    for (int k = 0; k < m.dof_size; ++k) gd[k] = 0.f;
    rot[0] = exp_map_to_quat_lib(em);
    for (int b = 1; b < B; ++b) {
        jq[b] = joint_dof_to_rot<true>(m, b, d, 1);
        loc[b] = quat_mul(mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]), jq[b]);
        rot[b] = quat_mul(rot[m.parent[b]], loc[b]);
    }
    for (int b = 0; b < B; ++b) {
        gpos[b] = ld3(g_body_pos + ((size_t)i * B + b) * 3);
        grot[b] = ld4(g_body_rot + ((size_t)i * B + b) * 4);
    }
    for (int b = B - 1; b >= 1; --b) {          // children before parents: a body's index exceeds its parent's
        const int p = m.parent[b];
        // pos[b] = pos[p] + rotate(rot[p], t_b)
        gpos[p] = gpos[p] + gpos[b];
        grot[p] = qadd(grot[p], quat_rotate_bwd_q(rot[p], mk3(m.local_translation[b][0], m.local_translation[b][1], m.local_translation[b][2]), gpos[b]));
        // rot[b] = rot[p] (x) loc[b]
        grot[p] = qadd(grot[p], quat_mul(grot[b], quat_conj(loc[b])));
        const q4 gloc = quat_mul(quat_conj(rot[p]), grot[b]);
        // loc[b] = lrot (x) jq[b], + the cotangent handed in for the joint rotation itself
        const q4 lr = mk4(m.local_rotation[b][0], m.local_rotation[b][1], m.local_rotation[b][2], m.local_rotation[b][3]);
        const q4 gj = qadd(quat_mul(quat_conj(lr), gloc), ld4(g_joint_rot + ((size_t)i * (B - 1) + (b - 1)) * 4));
        const int jt = m.joint_type[b], d0 = m.dof_idx[b];
        if (jt == PARC_JOINT_HINGE) {
            const v3 ax = mk3(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2]);
            gd[d0] = axis_angle_to_quat_bwd(ax, d[d0], jq[b], gj).g_angle;
        } else if (jt == PARC_JOINT_SPHERICAL) {
            const v3 ge = exp_map_to_quat_bwd(mk3(d[d0], d[d0 + 1], d[d0 + 2]), jq[b], gj);
            gd[d0] = ge.x;
            gd[d0 + 1] = ge.y;
            gd[d0 + 2] = ge.z;
        }
    }
    st3(g_root_pos + 3 * (size_t)i, gpos[0]);
    st3(g_root_exp + 3 * (size_t)i, exp_map_to_quat_bwd(em, rot[0], qadd(grot[0], ld4(g_root_quat + 4 * (size_t)i))));
}

// Angle between two rotations, torch_util.quat_diff_angle(q0, q1) = angle of q1 (x) conj(q0) (util/torch_util.py:421-431,68-88: the
// w >= 0 representative, 2 atan2(|v|, w), 0 below |v| = 1e-5), and its adjoint; one thread per pair.  The optimiser evaluates it for
// the root, every joint and every body-to-next-frame pair of every frame.
__global__ __launch_bounds__(256) void quat_diff_angle_kernel(size_t n, const float *__restrict__ q0, const float *__restrict__ q1, float *angle) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const q4 d = quat_mul(ld4(q1 + 4 * i), quat_conj(ld4(q0 + 4 * i)));
    const float s = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    angle[i] = s > 1e-5f ? 2.0f * atan2f(s, fabsf(d.w)) : 0.f;
}

__global__ __launch_bounds__(256) void quat_diff_angle_grad_kernel(size_t n, const float *__restrict__ q0, const float *__restrict__ q1,
                                                                   const float *__restrict__ g_angle, float *g_q0, float *g_q1) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const q4 a = ld4(q0 + 4 * i), b = ld4(q1 + 4 * i);
    const q4 d = quat_mul(b, quat_conj(a));
    const float s = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    q4 ga = mk4(0.f, 0.f, 0.f, 0.f), gb = ga;
    if (s > 1e-5f) {
        const float sg = d.w < 0.f ? -1.0f : 1.0f;           // quat_pos: the representative with w >= 0
        const float w = sg * d.w, den = s * s + w * w, g = g_angle[i];
        const float gs = 2.0f * w / den * g / s;               // d angle / d|v| * (v / |v|), on the flipped vector part ...
        const q4 gd = q4{sg * gs * (sg * d.x), sg * gs * (sg * d.y), sg * gs * (sg * d.z), sg * (-2.0f * s / den * g)};     // ... and flipped back
        gb = quat_mul(gd, a);                                   // d = b (x) conj(a):  g_b = g_d (x) a
        const q4 gc = quat_mul(quat_conj(b), gd);               //                     g_conj(a) = conj(b) (x) g_d
        ga = q4{-gc.x, -gc.y, -gc.z, gc.w};
    }
    st4(g_q0 + 4 * i, ga);
    st4(g_q1 + 4 * i, gb);
}

extern "C" int parc_quat_diff_angle(void *stream, int64_t n, const float *q0, const float *q1, float *angle) {
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(quat_diff_angle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (size_t)n, q0, q1, angle);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_quat_diff_angle_grad(void *stream, int64_t n, const float *q0, const float *q1, const float *g_angle, float *g_q0, float *g_q1) {
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(quat_diff_angle_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (size_t)n, q0, q1, g_angle,
                       g_q0, g_q1);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// The frame-to-frame terms of stage 2's motion loss and their adjoint: the bodies live in parc_moopt_core.h (tt_forward_body /
// tt_backward_body), shared with the packed-motions pair of parc_moopt.hip.  One thread per (frame, body).
__global__ __launch_bounds__(256) void temporal_terms_kernel(int T, int B, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                                                             const float *__restrict__ src_vel, const float *__restrict__ keep,
                                                             const float *__restrict__ pair_contact, tt_args a, float *partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int t = i / B, b = i - t * B;
    float sm, sl, jl;
    tt_forward_body(T, B, t, b, i, pos, rot_err_sq, src_vel, keep, pair_contact, a, sm, sl, jl);
    const size_t n = (size_t)T * B;
    partial[i] = sm;
    partial[n + i] = sl;
    partial[2 * n + i] = jl;
}

__global__ __launch_bounds__(256) void temporal_terms_grad_kernel(int T, int B, const float *__restrict__ pos, const float *__restrict__ rot_err_sq,
                                                                  const float *__restrict__ src_vel, const float *__restrict__ keep,
                                                                  const float *__restrict__ pair_contact, tt_args a,
                                                                  const float *__restrict__ w /* cotangents of the 3 sums */, float *g_pos,
                                                                  float *g_rot_err_sq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * B) return;
    const int t = i / B, b = i - t * B;
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    float g_r;
    bool has_r;
    const v3 g = tt_backward_body(T, B, t, b, i, pos, rot_err_sq, src_vel, keep, pair_contact, a, w0, w1, w2, g_r, has_r);
    st3(g_pos + (size_t)i * 3, g);
    if (has_r) g_rot_err_sq[i] = g_r;
}

extern "C" int parc_temporal_terms(void *stream, int n_frames, int num_bodies, const float *body_pos, const float *rot_err_sq, const float *src_vel,
                                   const float *keep, const float *pair_contact, float c, float c2, float jerk_limit, float *partial) {
    if (n_frames < 0 || num_bodies <= 0) return PARC_EINVAL;
    const int n = n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(temporal_terms_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, body_pos, rot_err_sq,
                       src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, partial);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_temporal_terms_grad(void *stream, int n_frames, int num_bodies, const float *body_pos, const float *rot_err_sq,
                                        const float *src_vel, const float *keep, const float *pair_contact, float c, float c2, float jerk_limit,
                                        const float *cotangents, float *g_body_pos, float *g_rot_err_sq) {
    if (n_frames < 0 || num_bodies <= 0) return PARC_EINVAL;
    const int n = n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(temporal_terms_grad_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, body_pos,
                       rot_err_sq, src_vel, keep, pair_contact, tt_args{c, c2, jerk_limit}, cotangents, g_body_pos, g_rot_err_sq);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// Sample points of the bodies in the world frame, x[t, p] = pos[t, owner(p)] + rotate(rot[t, owner(p)], local[p]), and the adjoint
// (the points of a body are contiguous: body b owns [start[b], start[b + 1])), one thread per point / per (frame, body).
__global__ __launch_bounds__(256) void body_points_world_kernel(int n_frames, int B, int P, const float *__restrict__ body_pos,
                                                                const float *__restrict__ body_rot, const float *__restrict__ local,
                                                                const int32_t *__restrict__ owner, float *world) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * P) return;
    const int t = (int)(i / P), p = (int)(i - (size_t)t * P), b = owner[p];
    const v3 x = ld3(body_pos + ((size_t)t * B + b) * 3) + quat_rotate(ld4(body_rot + ((size_t)t * B + b) * 4), ld3(local + 3 * (size_t)p));
    st3(world + i * 3, x);
}

__global__ __launch_bounds__(256) void body_points_world_grad_kernel(int n_frames, int B, int P, const float *__restrict__ body_rot,
                                                                     const float *__restrict__ local, const int32_t *__restrict__ start,
                                                                     const float *__restrict__ g_world, float *g_body_pos, float *g_body_rot) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n_frames * B) return;
    const int t = (int)(i / B), b = (int)(i - (size_t)t * B);
    const q4 q = ld4(body_rot + i * 4);
    v3 gp = mk3(0.f, 0.f, 0.f);
    q4 gq = mk4(0.f, 0.f, 0.f, 0.f);
    for (int p = start[b]; p < start[b + 1]; ++p) {
        const v3 g = ld3(g_world + ((size_t)t * P + p) * 3);
        gp = gp + g;
        gq = qadd(gq, quat_rotate_bwd_q(q, ld3(local + 3 * (size_t)p), g));
    }
    st3(g_body_pos + i * 3, gp);
    st4(g_body_rot + i * 4, gq);
}

extern "C" int parc_body_points_world(void *stream, int n_frames, int num_bodies, int num_points, const float *body_pos, const float *body_rot,
                                      const float *local, const int32_t *owner, float *world) {
    if (n_frames < 0 || num_bodies <= 0 || num_points < 0) return PARC_EINVAL;
    const size_t n = (size_t)n_frames * num_points;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(body_points_world_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies, num_points,
                       body_pos, body_rot, local, owner, world);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_body_points_world_grad(void *stream, int n_frames, int num_bodies, int num_points, const float *body_rot, const float *local,
                                           const int32_t *start, const float *g_world, float *g_body_pos, float *g_body_rot) {
    if (n_frames < 0 || num_bodies <= 0 || num_points < 0) return PARC_EINVAL;
    const size_t n = (size_t)n_frames * num_bodies;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(body_points_world_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_frames, num_bodies,
                       num_points, body_rot, local, start, g_world, g_body_pos, g_body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_pose_chain_forward(void *stream, parc_char_model_t model, int n, const float *root_pos, const float *root_exp,
                                       const float *dof, float *root_quat, float *joint_rot, float *body_pos, float *body_rot) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    for (int b = 1; b < model.num_bodies; ++b)
        if (model.parent[b] < 0 || model.parent[b] >= b) return PARC_EUNSUPPORTED;      // the sweeps rely on parents-first order
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(pose_chain_fwd_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, model, n, root_pos, root_exp, dof, root_quat,
                       joint_rot, body_pos, body_rot);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_pose_chain_backward(void *stream, parc_char_model_t model, int n, const float *root_exp, const float *dof,
                                        const float *g_root_quat, const float *g_joint_rot, const float *g_body_pos, const float *g_body_rot,
                                        float *g_root_pos, float *g_root_exp, float *g_dof) {
    if (n < 0 || !model_ok(model)) return PARC_EINVAL;
    for (int b = 1; b < model.num_bodies; ++b)
        if (model.parent[b] < 0 || model.parent[b] >= b) return PARC_EUNSUPPORTED;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(pose_chain_bwd_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, model, n, root_exp, dof, g_root_quat,
                       g_joint_rot, g_body_pos, g_body_rot, g_root_pos, g_root_exp, g_dof);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Fused post-physics pass.  A pose (simulated character, reference at t, targets at t+dt_s - two of those per group) is handled by a
// 16-lane group, lane b = body b; every wave writes the observation columns it produces itself.
// =============================================================================================
#define POST_EPB 4            // envs per workgroup
#define POST_MAX_THREADS 384  // 64 * (3 + (PARC_MAX_TAR_STEPS + 1) / 2): character, reference, target waves (two target steps per lane), heightmap wave
#define POST_MAX_ROW 1408
#define POST_STAGE_T 248      // two target steps of one env: 2 (9 + 6 (PARC_MAX_BODIES - 1) + 3 PARC_MAX_KEY_BODIES) = 246 floats
#define POST_STAGE_C 192      // the character's own columns: 12 + 6 (PARC_MAX_BODIES - 1) + PARC_MAX_DOFS + 3 PARC_MAX_KEY_BODIES = 190 floats
// Kernel arguments passed by value are loaded by the compiler in the entry block, all of them, and then live in scalar registers
// for the whole kernel: with ~2 KB of argument structs that is far more than the 102 SGPRs a wave has, and the overflow is kept in
// VGPR lanes (v_writelane at entry, v_readlane at every use - vector-issue slots).  kernarg_late hands out a pointer to a struct
// inside the kernel-argument segment that the optimiser cannot see through, so loads through it stay where they are written.
// Offsets = the by-value parameters of track_post_kernel in order, each 8-byte aligned (checked against the code object's
// metadata by tools/check_kernarg_offsets.py).
#define KARG_ALIGN8(x) (((x) + 7) & ~(size_t)7)
#define KARG_OFF_ML KARG_ALIGN8(sizeof(parc_char_model_t))
#define KARG_OFF_TER KARG_ALIGN8(KARG_OFF_ML + sizeof(parc_motion_lib_t))
#define KARG_OFF_CFG KARG_ALIGN8(KARG_OFF_TER + sizeof(parc_terrain_t))
#define KARG_OFF_BUF KARG_ALIGN8(KARG_OFF_CFG + sizeof(parc_track_cfg_t))
template <typename T>
PARC_DEV const __attribute__((address_space(4))) T *kernarg_late(size_t off) {
    const __attribute__((address_space(4))) char *p = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return (const __attribute__((address_space(4))) T *)(p + off);
}

#ifndef POST_MIN_WAVES
// 6 waves per workgroup at <= 72 VGPRs: four workgroups per CU, all 1024 workgroups of a 4096-env launch resident in one round
// (measured, profiles/r03_wg_residency.txt: 6-wave workgroups stay one round at 72 VGPRs and need two at 80, 5-wave ones stay one round
// up to 80; until round 3 the kernel ran 8 waves per workgroup at 64 VGPRs)
#define POST_MIN_WAVES 7
#endif

// The columns a 16-lane group has written to its LDS segment go to the observation row as 16-byte stores, 4 consecutive floats per lane:
// the launch is bound by the number of vector-memory instructions (a wave-wide store of one float per lane at a 24-byte stride costs the
// CU's address path the same ~22 cycles as a store of 16 contiguous bytes per lane), so 23 strided stores of a target wave become 5.
// LDS operations of one wave complete in order: the wave barrier + fences only keep the compiler from moving them.
PARC_DEV void stage_out(const float *seg, float *dst, int n, int b) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int n4 = n >> 2;
    for (int c = b; c < n4; c += GRP) {
        const float4 v = *reinterpret_cast<const float4 *>(seg + 4 * c);
        f4u o;
        o.x = v.x, o.y = v.y, o.z = v.z, o.w = v.w;
        POST_STORE4(dst + 4 * c, o);
    }
    for (int i = 4 * n4 + b; i < n; i += GRP) dst[i] = seg[i];
}

// Workgroup = POST_EPB envs, one ROLE per wave so no wave diverges:
//   wave 0          the simulated character of the 4 envs   (4 x 16 body lanes)  -> its own observation columns
//   wave 1          their reference poses at t                                   -> reward, done
//   wave 2 + p      target steps 2p and 2p + 1 of the 4 envs, one in each half of packed float2 values (p < ceil(S / 2))
//   last wave       the 4 x 441 heightmap samples (only launched with PARC_POST_HF)
// Phase 0 (28 lanes of wave 0: per-env and per-query scalars -> LDS) is the only thing the one barrier waits for; behind it the waves
// never meet again: each collects the columns it produces in an LDS segment of its own and writes them as 16-byte stores (stage_out).
__global__ __launch_bounds__(POST_MAX_THREADS, POST_MIN_WAVES) void track_post_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_terrain_t ter,
                                                                     parc_track_cfg_t cfg, parc_env_buffers_t buf,
                                                                     const int64_t *__restrict__ env_ids, int n_total, int what,
                                                                     const float *__restrict__ ray_xy) {
    __shared__ __attribute__((aligned(16))) float envd[POST_EPB][20];   // root pos 3 | root rot 4 | heading^-1 4 | env id | root vel 3 | ang vel 3
    __shared__ __attribute__((aligned(16))) float qryd[1 + PARC_MAX_TAR_STEPS][POST_EPB][12];   // idx0 idx1 blend - | loop shift xyz, time | tile offset xy, motion end
    __shared__ float tgt_xy[POST_EPB][2];
    // per-wave staging of the observation columns a wave produces (see stage_out): never shared between waves, no barrier
    __shared__ __attribute__((aligned(16))) float stage_t[(PARC_MAX_TAR_STEPS + 1) / 2][POST_EPB][POST_STAGE_T];
    __shared__ __attribute__((aligned(16))) float stage_c[POST_EPB][POST_STAGE_C];
    // per-body constants of the tree walk + the body's key slot, loaded once per workgroup (by the reference wave, which has nothing
    // else to do in front of the barrier) instead of as four (character and reference wave: nine) vector loads in every pose wave: lrot 4 | lt 3, parent | depth, key slot,
    // | joint type, first dof, - | hinge axis 3, -
    __shared__ __attribute__((aligned(16))) float bodyk[GRP][16];
    PARC_DIAG(if (what & 0x100000) return;)          // (timing diagnostic: the launch alone)
    const int tid = threadIdx.x;
    const int wv = tid >> 6, gg = (tid & 63) >> 4, b = tid & 15;
    const int B = m.num_bodies, J = B - 1, D = m.dof_size, K = cfg.num_key_bodies, S = cfg.num_tar_steps;
    const int H = (S + 1) >> 1;                          // target waves: two target steps per lane
    const bool is_char = wv == 0, is_ref = wv == 1, is_tar = wv >= 2 && wv < 2 + H, is_gat = wv == 2 + H;
    const int le = gg;
    const int el = blockIdx.x * POST_EPB + le;
    const bool masked = (what & PARC_POST_MASKED) != 0;
    if (masked) {
        // device-side reset: nothing to do for a workgroup whose envs all kept running (uniform: every wave leaves)
        int any = 0;
#pragma unroll
        for (int k = 0; k < POST_EPB; ++k) {
            int ek = blockIdx.x * POST_EPB + k;
            if (ek < n_total) any |= buf.env_mask[ek];
        }
        if (!any) return;
    }
    const bool live = el < n_total && (!masked || buf.env_mask[el] != 0);
    const int RS = cfg.obs_dim;
    const int Wc = 12 + 6 * J + D + 3 * K;   // char_obs width (136)
    const int Wt = 9 + 6 * J + 3 * K;        // one target step (105)
    const int row_len = cfg.obs_dim - cfg.num_ray_points;  // 871
    const bool valid = b < B;

    // ---- phase 0 (wave 0): the per-env and per-query scalars, ONE lane each instead of once per 16-lane group in
    // every wave: lane l -> env l & 3, query l >> 2 (0 = reference at t, s + 1 = target step s)
    if (wv == 0 && tid < POST_EPB * (1 + S)) {
        const int ple = tid & (POST_EPB - 1), pq = tid >> 2;
        const int pel = min((int)blockIdx.x * POST_EPB + ple, n_total - 1);
        const int pe = env_ids ? (int)env_ids[pel] : pel;
        const int64_t mid = buf.motion_ids[pe];
        // dataset clips: env time + the clip time the episode started at (dm_env.py:597-602); generated plans: the plan clock itself
        // (mgdm_env.py:476-480), handed over in the same per-env slot so that it is the exact number and not a rounded sum
        const float mtime = (what & PARC_POST_PLAN_CLOCK) ? buf.motion_time_offsets[pe] : buf.time_buf[pe] + buf.motion_time_offsets[pe];
        if (pq == 0) {
            const float *prs = buf.root_state + (size_t)pe * 13;
            const q4 cr = ld4(prs + 3);
            // global_obs (ig_char_env.py:585-590, mgdm_dm_util.py:476-500): the observation stays in world axes - the "heading frame" every
            // wave rotates into is the identity, and a target's key bodies are not offset by its root (selector in ed[4].z)
            const q4 hi = cfg.global_obs ? mk4(0.f, 0.f, 0.f, 1.f) : calc_heading_quat_inv_alg(cr);
            float4 *ed = reinterpret_cast<float4 *>(envd[ple]);
            ed[0] = make_float4(prs[0], prs[1], prs[2], cr.x);
            ed[1] = make_float4(cr.y, cr.z, cr.w, hi.x);
            ed[2] = make_float4(hi.y, hi.z, hi.w, __int_as_float(pe));
            ed[3] = make_float4(prs[7], prs[8], prs[9], prs[10]);
            ed[4] = make_float4(prs[11], prs[12], cfg.global_obs ? 0.f : 1.f, 0.f);
        }
        // K3 index part: MotionLib.calc_motion_frame at t (ref) or t + dt_s (targets); dm_env.py:570-582, mgdm_dm_util.py:279-302
        const float t = mtime + (pq > 0 ? cfg.tar_dt[pq - 1] : 0.f);
        const frame_query fq = make_query(ml, mid, t);
        // The frame rows themselves (root position included) are loaded by the pose lanes after the barrier, together with the
        // quaternions: this lane only publishes what does not need them - indices, blend, the loop shift of wrapping clips
        // (motion_lib.py:458-475) and the tile offset (_move_to_motion_terrain dm_env.py:604-615) - so the barrier is reached one
        // memory round trip earlier.
        v3 shift = mk3(0.f, 0.f, 0.f);
        if (fq.wrap) {
            const float *d = ml.pos_delta + 3 * mid;
            shift = mk3(fq.loop_phase * d[0], fq.loop_phase * d[1], fq.loop_phase * d[2]);
        }
        float4 *qd = reinterpret_cast<float4 *>(qryd[pq][ple]);
        qd[0] = make_float4(__int_as_float(fq.idx0), __int_as_float(fq.idx1), fq.blend, 0.f);
        // (reference query only) env time and the motion-end flag of DeepMimicEnv.update_done, dm_env.py:746-783: the clip
        // length / loop mode were just loaded for the query, the termination code reads the result from LDS
        const int motion_end = (pq == 0) && !(what & PARC_POST_PLAN_CLOCK) && (mtime >= ml.length[mid]) && (ml.loop_mode[mid] != 1);
        qd[1] = make_float4(shift.x, shift.y, shift.z, buf.time_buf[pe]);
        qd[2] = make_float4(buf.motion_xy_offset[2 * pe] - buf.env_offsets[3 * pe], buf.motion_xy_offset[2 * pe + 1] - buf.env_offsets[3 * pe + 1],
                            __int_as_float(motion_end), 0.f);
    }
    // xy target resample (PARC_POST_TARGETS): lanes 4 (1 + S) .. 4 (2 + S) - 1 of wave 0, one per env
    if (wv == 0 && tid >= POST_EPB * (1 + S) && tid < POST_EPB * (2 + S)) {
        const int ple = tid - POST_EPB * (1 + S);
        const int pel = blockIdx.x * POST_EPB + ple;
        const int pelc = min(pel, n_total - 1);
        const int pe = env_ids ? (int)env_ids[pelc] : pelc;
        float tx = buf.target_xy[2 * pe], ty = buf.target_xy[2 * pe + 1];
        if ((what & PARC_POST_TARGETS) && pel < n_total && (!masked || buf.env_mask[pe] != 0)) {
            // DeepMimicEnv._update_motion_targets  dm_env.py:617-654
            const float tm = buf.time_buf[pe];
            if (tm >= buf.next_target_time[pe]) {
                const float *u = buf.target_rand + 3 * (size_t)pe;
                const float fut = u[0] * (cfg.target_future_max - cfg.target_future_min) + cfg.target_future_min;
                const int64_t mid = buf.motion_ids[pe];
                const frame_query fq = make_query(ml, mid, tm + buf.motion_time_offsets[pe] + fut);
                const v3 pr = query_root_pos(ml, fq, mid);
                // N(0, 0.05) noise from the two remaining uniforms (Box-Muller)
                const float rr = 0.05f * fsqrt(-2.0f * __logf(fmaxf(1.0f - u[1], 1e-12f)));
                float sn, cs;
                fsincos(6.283185307179586f * u[2], sn, cs);
                tx = pr.x + buf.motion_xy_offset[2 * pe] - buf.env_offsets[3 * pe] + rr * cs;
                ty = pr.y + buf.motion_xy_offset[2 * pe + 1] - buf.env_offsets[3 * pe + 1] + rr * sn;
                float *wt = const_cast<float *>(buf.target_xy);
                wt[2 * pe] = tx;
                wt[2 * pe + 1] = ty;
                buf.next_target_time[pe] = tm + fut;
            }
        }
        tgt_xy[ple][0] = tx;
        tgt_xy[ple][1] = ty;
    }
    // K5 fused: RefCharEnv._refresh_ray_obs_hfs (mgdm_dm_util.py:158-179) for the 4 envs of this workgroup, by a wave of its own (the
    // last one, launched only when PARC_POST_HF is asked for): 16 lanes per env, 28 points per lane, same affine cell-unit form as
    // hf_gather_kernel.  The heightmap columns need the simulated root state only, nothing of phase 0: the wave derives the map of its
    // envs while wave 0 walks the dependent loads of phase 0, and walks its points while the pose waves work - nobody waits for it.
    // (Until round 3 all waves but wave 0 shared the gather in front of the barrier: 3.2 us during which no pose wave computed.)
    hf_env_prm gpr;
    int ghe = 0;
    bool glive = false;
    if (is_gat) {
        const int hel = (int)blockIdx.x * POST_EPB + gg;
        const int helc = min(hel, n_total - 1);
        ghe = env_ids ? (int)env_ids[helc] : helc;
        gpr = hf_env_params<true>(ghe, buf.root_state, buf.env_offsets, ter, 1.0f / ter.dx, 1.0f / ter.dy);
        glive = hel < n_total && (!masked || buf.env_mask[helc] != 0);
    }
    PARC_DIAG(if (what & 0x200000) return;)          // (timing diagnostic: launch + phase 0 + heightmap gather, no barrier)
    if (is_ref && gg == 0) {
        const fk_consts k = fk_consts_of(m, b);
        int ks = -1;
        for (int i = 0; i < K; ++i)
            if (cfg.key_body_ids[i] == b) ks = i;
        float4 *bk = reinterpret_cast<float4 *>(bodyk[b]);
        bk[0] = make_float4(k.lrot.x, k.lrot.y, k.lrot.z, k.lrot.w);
        bk[1] = make_float4(k.lt.x, k.lt.y, k.lt.z, __int_as_float(k.par));
        const bool jv = b > 0 && b < B;
        bk[2] = make_float4(__int_as_float(k.dep), __int_as_float(ks), __int_as_float(jv ? m.joint_type[b] : -1), __int_as_float(jv ? m.dof_idx[b] : 0));
        bk[3] = jv ? make_float4(m.joint_axis[b][0], m.joint_axis[b][1], m.joint_axis[b][2], 0.f) : make_float4(0.f, 0.f, 1.f, 0.f);
    }
    __syncthreads();
    const int key_slot = __float_as_int(bodyk[b][9]);
    auto joint_rot_lds = [&](const float *dof2) {                // K1 (kin_char_model.py:478-491) on the staged joint constants
        const float4 k3 = reinterpret_cast<const float4 *>(bodyk[b])[3];
        return joint_dof_to_rot(__float_as_int(bodyk[b][10]), __float_as_int(bodyk[b][11]), mk3(k3.x, k3.y, k3.z), dof2, 2);
    };
    auto fk_consts_lds = [&]() {                                 // read where the walk starts, not held in registers until then
        fk_consts k;
        const float4 k0 = reinterpret_cast<const float4 *>(bodyk[b])[0], k1 = reinterpret_cast<const float4 *>(bodyk[b])[1];
        k.lrot = mk4(k0.x, k0.y, k0.z, k0.w);
        k.lt = mk3(k1.x, k1.y, k1.z);
        k.par = __float_as_int(k1.w);
        k.dep = __float_as_int(bodyk[b][8]);
        return k;
    };
    // diagnostic role ablations (timing only): bits 16/17/18 drop the target / reference / character waves
    PARC_DIAG(if (((what & 0x10000) && is_tar) || ((what & 0x20000) && is_ref) || ((what & 0x40000) && is_char)) return;)
    if (is_gat) {
        PARC_DIAG(if (what & 0x80000) return;)                   // (timing diagnostic: no heightmap wave)
        const int P = cfg.num_ray_points;
        const float max_i = (float)(ter.dim_x - 1), max_j = (float)(ter.dim_y - 1);
        // straight into the observation row; the 441 columns are a third of the row's bytes.  The launch is bound by the NUMBER of
        // vector-memory instructions its waves issue (about 22 cycles of a CU's address path each, whatever they move), so a lane takes
        // 4 consecutive points: their (x, y) pairs arrive as two 16-byte loads and leave as one 16-byte store, 4 scattered cell reads
        // in between - 7 instructions per 4 points instead of 12.
        float *hrow = buf.obs + (size_t)ghe * RS + (RS - P);
        auto cell = [&](float rx, float ry) {
            float ui = fmaf(rx, gpr.ax, fmaf(ry, gpr.bx, gpr.cx));
            float uj = fmaf(rx, gpr.ay, fmaf(ry, gpr.by, gpr.cy));
            ui = __builtin_amdgcn_fmed3f(rintf(ui), 0.f, max_i);
            uj = __builtin_amdgcn_fmed3f(rintf(uj), 0.f, max_j);
            return __builtin_amdgcn_fmed3f(ter.hf[(int)ui * ter.dim_y + (int)uj] - gpr.gz, cfg.min_obs_h, cfg.max_obs_h);
        };
        const int full = P >> 2;                                 // chunks of 4 points
#pragma unroll 2
        for (int c = glive ? b : full; c < full; c += GRP) {
            const f4u r0 = *reinterpret_cast<const f4u *>(ray_xy + 8 * c), r1 = *reinterpret_cast<const f4u *>(ray_xy + 8 * c + 4);
            f4u h;
            h.x = cell(r0.x, r0.y);
            h.y = cell(r0.z, r0.w);
            h.z = cell(r1.x, r1.y);
            h.w = cell(r1.z, r1.w);
            POST_STORE4(hrow + 4 * c, h);
        }
        for (int p = glive ? 4 * full + b : P; p < P; p += GRP) hrow[p] = cell(ray_xy[2 * p], ray_xy[2 * p + 1]);
        return;
    }
    if (is_ref && !(what & PARC_POST_REWARD_DONE)) return;      // the reference wave computes reward / termination; the reference STATE is ref_state_group's

    // ---- target waves: DeepMimicEnv.compute_tar_obs + compute_tar_obs  dm_env.py:686-718, mgdm_dm_util.py:462-519
    // Wave 2 + p carries target steps 2p and 2p + 1 of the 4 envs, one in each component of float2 values: the clip
    // sampling (K3), the tree walk (K2) and the heading-frame epilogue (K7) of both steps issue as packed multiply-adds.
    if (is_tar) {
        if (!((what & PARC_POST_OBS) && live)) return;          // (a whole 16-lane group: the cross-lane moves stay inside a group)
        const int sA = 2 * (wv - 2), sB = sA + 1;                // adjacent steps: their columns are one contiguous run of the row
        const bool hasB = sB < S;                                // odd S: the last wave's second component repeats step sA and stores nothing
        const int qB = hasB ? sB : sA;
        const int e = __float_as_int(envd[le][11]);
        float *row = buf.obs + (size_t)e * RS;
        const float4 a0 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[0], a1 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[1],
                     a2 = reinterpret_cast<const float4 *>(qryd[1 + sA][le])[2];
        const float4 b0 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[0], b1 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[1],
                     b2 = reinterpret_cast<const float4 *>(qryd[1 + qB][le])[2];
        const float *rA0 = ml.frames + (size_t)__float_as_int(a0.x) * ml.row_stride, *rA1 = ml.frames + (size_t)__float_as_int(a0.y) * ml.row_stride;
        const float *rB0 = ml.frames + (size_t)__float_as_int(b0.x) * ml.row_stride, *rB1 = ml.frames + (size_t)__float_as_int(b0.y) * ml.row_stride;
        const f2 blend = mk2(a0.z, b0.z);
        q4p jq = sp4(mk4(0.f, 0.f, 0.f, 1.f));
        if (valid) {
            const float4 xa = *reinterpret_cast<const float4 *>(rA0 + 4 * b), ya = *reinterpret_cast<const float4 *>(rA1 + 4 * b);
            const float4 xb = *reinterpret_cast<const float4 *>(rB0 + 4 * b), yb = *reinterpret_cast<const float4 *>(rB1 + 4 * b);
            jq = slerp(q4p{mk2(xa.x, xb.x), mk2(xa.y, xb.y), mk2(xa.z, xb.z), mk2(xa.w, xb.w)},
                       q4p{mk2(ya.x, yb.x), mk2(ya.y, yb.y), mk2(ya.z, yb.z), mk2(ya.w, yb.w)}, blend);
        }
        PARC_DIAG(if ((what & 0x400000) && jq.x.x != 123.f) return;)       // (timing diagnostic: a target wave up to its blended joint rotations)
        // root position: lerp of the two rows, + loop shift, + tile offset (the order of query_root_pos and dm_env.py:604-615)
        v3p p_root;
        {
            const float *pa0 = rA0 + ml.off_pos, *pa1 = rA1 + ml.off_pos, *pb0 = rB0 + ml.off_pos, *pb1 = rB1 + ml.off_pos;
            p_root = v3p{lerp_ref(mk2(pa0[0], pb0[0]), mk2(pa1[0], pb1[0]), blend), lerp_ref(mk2(pa0[1], pb0[1]), mk2(pa1[1], pb1[1]), blend),
                         lerp_ref(mk2(pa0[2], pb0[2]), mk2(pa1[2], pb1[2]), blend)};
            p_root = p_root + v3p{mk2(a1.x, b1.x), mk2(a1.y, b1.y), mk2(a1.z, b1.z)};
            p_root.x += mk2(a2.x, b2.x);
            p_root.y += mk2(a2.y, b2.y);
        }
        if (valid) {
            const f2 ct = lerp_ref(mk2(rA0[ml.off_contacts + b], rB0[ml.off_contacts + b]), mk2(rA1[ml.off_contacts + b], rB1[ml.off_contacts + b]), blend);
            row[Wc + S * Wt + sA * B + b] = ct.x;
            if (hasB) row[Wc + S * Wt + sB * B + b] = ct.y;
        }
        // The tree walk starts from (root position, root rotation) in lane 0 and overwrites every other lane at its level, so the lanes'
        // own joint rotations serve as the initial value; the root pose is fetched from lane 0 again afterwards instead of being kept
        // in 14 registers through the walk.
        v3p pos;
        q4p rot;
        group_fk<false>(fk_consts_lds(), m.max_depth, p_root, jq, jq, pos, rot);
        asm volatile("" ::: "memory");                          // the simulated root pose and heading are only needed from here on
        PARC_DIAG(if ((what & 0x800000) && pos.x.x != 123.f) return;)      // (timing diagnostic: a target wave up to the end of its tree walk)
        p_root = shfl16(pos, 0);
        const float4 e0 = reinterpret_cast<const float4 *>(envd[le])[0], e1 = reinterpret_cast<const float4 *>(envd[le])[1],
                     e2 = reinterpret_cast<const float4 *>(envd[le])[2];
        const v3p c_pos = sp3(mk3(e0.x, e0.y, e0.z));
        const q4p hinv = sp4(mk4(e1.w, e2.x, e2.y, e2.z));
        float *seg = stage_t[wv - 2][le];                        // step sA at seg[0, Wt), step sB at seg[Wt, 2 Wt)
        const v3p rpo = quat_rotate(hinv, p_root - c_pos);
        if (b == 0) {
            seg[0] = rpo.x.x, seg[1] = rpo.y.x, seg[2] = rpo.z.x;
            seg[Wt] = rpo.x.y, seg[Wt + 1] = rpo.y.y, seg[Wt + 2] = rpo.z.y;
        }
        // lane 0: heading-relative root rotation at o+3 (the lane's own quaternion IS the root rotation); lane b: joint b-1 at
        // o + 9 + 6 (b-1) = o + 3 + 6 b
        const q4p hr = quat_mul(hinv, jq);
        if (valid) {
            f2 tn[6];
            quat_to_tan_norm(b == 0 ? hr : jq, tn);
#pragma unroll
            for (int k = 0; k < 6; ++k) seg[3 + 6 * b + k] = tn[k].x, seg[Wt + 3 + 6 * b + k] = tn[k].y;
        }
        if (key_slot >= 0) {
            const v3p kp = quat_rotate(hinv, pos - p_root) + envd[le][18] * rpo;     // (+ rpo unless global_obs)
            float *ka = seg + 9 + 6 * J + 3 * key_slot;
            ka[0] = kp.x.x, ka[1] = kp.y.x, ka[2] = kp.z.x;
            ka[Wt] = kp.x.y, ka[Wt + 1] = kp.y.y, ka[Wt + 2] = kp.z.y;
        }
        PARC_DIAG(if ((what & 0x1000000) && seg[b] != 123.f) return;)      // (timing diagnostic: a target wave without its stores)
        stage_out(seg, row + Wc + sA * Wt, hasB ? 2 * Wt : Wt, b);
        return;
    }

    const int e = __float_as_int(envd[le][11]);
    const float *dofs = buf.dof_state + (size_t)e * D * 2;  // interleaved pos,vel
    // every wave writes its own columns of the observation row straight to memory as it produces them: after the first barrier the
    // waves of a workgroup never meet again, so the stores of the early finishers overlap the arithmetic of the late ones (until
    // round 3 the rows were assembled in LDS and streamed out behind a second barrier: 3.6 of 17.7 us with every SIMD idle)
    float *row = buf.obs + (size_t)e * RS;

    // ---- phase A: every group gets its pose (root transform + one joint rotation per lane)
    frame_query fq;
    q4 jq = mk4(0.f, 0.f, 0.f, 1.f);
    v3 p_root = mk3(0.f, 0.f, 0.f);
    q4 r_root = mk4(0.f, 0.f, 0.f, 1.f);
    if (is_char) {
        p_root = mk3(envd[le][0], envd[le][1], envd[le][2]);
        r_root = mk4(envd[le][3], envd[le][4], envd[le][5], envd[le][6]);
        if (valid && b > 0) jq = joint_rot_lds(dofs);      // K1 (kin_char_model.py:478-491)
    } else {
        const float4 q0 = reinterpret_cast<const float4 *>(qryd[0][le])[0];
        const float4 q1 = reinterpret_cast<const float4 *>(qryd[0][le])[1];
        const float4 q2 = reinterpret_cast<const float4 *>(qryd[0][le])[2];
        fq.idx0 = __float_as_int(q0.x);
        fq.idx1 = __float_as_int(q0.y);
        fq.blend = q0.z;
        fq.row0 = ml.frames + (size_t)fq.idx0 * ml.row_stride;
        fq.row1 = ml.frames + (size_t)fq.idx1 * ml.row_stride;
        if (valid) jq = query_quat(fq, b);
        {
            // root position: lerp of the two rows, + loop shift, + tile offset (the order of query_root_pos and dm_env.py:604-615)
            const float *p0 = fq.row0 + ml.off_pos, *p1 = fq.row1 + ml.off_pos;
            p_root = mk3(lerp_ref(p0[0], p1[0], fq.blend), lerp_ref(p0[1], p1[1], fq.blend), lerp_ref(p0[2], p1[2], fq.blend));
            p_root = p_root + mk3(q1.x, q1.y, q1.z);
            p_root.x += q2.x;
            p_root.y += q2.y;
        }
        r_root = shfl16(jq, 0);
    }
    // ---- phase B: K2 forward kinematics, level-synchronous inside the 16-lane group
    // (kept in the reference's composition order root -> leaf: slerp between nearly identical frames returns slightly
    // non-unit quaternions, for which the rotation formula is not associative, so a reassociated tree walk - e.g. pointer
    // doubling in the root frame - drifts ~1e-4 from the reference's body positions)
    v3 pos;
    q4 rot;
    group_fk<false>(fk_consts_lds(), m.max_depth, p_root, r_root, jq, pos, rot);

    // the simulated root pose and heading are only needed from here on: read them after the tree walk (11 fewer live
    // registers through it; the compiler barrier keeps the LDS reads from being hoisted back up)
    asm volatile("" ::: "memory");
    const float4 e0 = reinterpret_cast<const float4 *>(envd[le])[0], e1 = reinterpret_cast<const float4 *>(envd[le])[1],
                 e2 = reinterpret_cast<const float4 *>(envd[le])[2];
    const v3 c_pos = mk3(e0.x, e0.y, e0.z);
    const q4 c_rot = mk4(e0.w, e1.x, e1.y, e1.z);
    const q4 hinv = mk4(e1.w, e2.x, e2.y, e2.z);

    // ---- phase C: per-group epilogues
    if (is_char) {
        if ((what & PARC_POST_OBS) && live) {
            // compute_char_obs  envs/ig_char_env.py:582-626 (global_obs False, no root height); the Wc columns are collected in the
            // wave's LDS segment and leave as 16-byte stores (stage_out)
            float *seg = stage_c[le];
            if (b == 0) {
                quat_to_tan_norm(quat_mul(hinv, c_rot), seg);
                st3(seg + 6, quat_rotate(hinv, ld3(envd[le] + 12)));     // simulated root velocities, staged by phase 0
                st3(seg + 9, quat_rotate(hinv, ld3(envd[le] + 15)));
            } else if (valid) {
                quat_to_tan_norm(jq, seg + 12 + 6 * (b - 1));
            }
            #pragma unroll 1
            for (int d = b; d < D; d += GRP) seg[12 + 6 * J + d] = dofs[2 * d + 1];
            if (key_slot >= 0) st3(seg + 12 + 6 * J + D + 3 * key_slot, quat_rotate(hinv, pos - c_pos));
            stage_out(seg, row, Wc, b);
            // char contacts  ig_parkour_env.py:841-848
            if (valid) {
                v3 f = ld3(buf.contact_forces + ((size_t)e * B + b) * 3);
                row[Wc + S * Wt + S * B + b] = fsqrt(dot3(f, f)) > cfg.contact_eps ? 1.f : 0.f;
            }
        }
        if ((what & PARC_POST_OBS) && b == 0 && live) {
            // values of the optional observation columns (has_target_xy_obs ig_parkour_env.py:1212-1224: the xy target seen from the
            // root, rotate_2d_vec(target - root_xy, -heading) = the heading-inverse rotation of (dx, dy, 0); global_root_height_obs
            // ig_char_env.py:618-620: root height) for parc_assemble_obs
            float *aux = kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF)->obs_aux;
            if (aux) {
                const q4 th = kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG)->global_obs ? calc_heading_quat_inv_alg(c_rot) : hinv;   // always the heading
                const v3 lt = quat_rotate(th, mk3(tgt_xy[le][0] - c_pos.x, tgt_xy[le][1] - c_pos.y, 0.f));
                reinterpret_cast<float4 *>(aux)[e] = make_float4(c_pos.z, lt.x, lt.y, 0.f);
            }
        }
        if ((what & PARC_POST_REWARD_DONE) && b == 0 && live) {
            // task terms  ig_parkour_env.py:1346-1393 (logged; they scale the reward only if rel_task_w > 0).  They read the simulated
            // root and the xy target only - nothing of the reference pose - so the character wave, the first to finish, computes them
            // instead of the reward wave, whose instruction stream is the longest of the workgroup.
            const auto &rbuf = *kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF);
            const auto &rcfg = *kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG);
            const int N = rbuf.reward_terms_stride > 0 ? rbuf.reward_terms_stride : rbuf.num_envs;
            float tx = tgt_xy[le][0] - c_pos.x, ty = tgt_xy[le][1] - c_pos.y;
            float terr = tx * tx + ty * ty;
            float task_r1 = fexp(-0.075f * terr);
            float tl = fsqrt(terr);
            float itl = frcp(tl);
            float dxn = tl > 0.01f ? tx * itl : 0.f, dyn = tl > 0.01f ? ty * itl : 0.f;
            float mve = fmaxf(2.0f - (dxn * envd[le][12] + dyn * envd[le][13]), 0.f);
            float min_vel_r = fexp(-(mve * mve));
            // heading direction (cos h, sin h) = normalised xy of the rotated x axis
            float ha = 1.0f - 2.0f * (c_rot.y * c_rot.y + c_rot.z * c_rot.z), hb = 2.0f * (c_rot.w * c_rot.z + c_rot.x * c_rot.y);
            float hn2 = ha * ha + hb * hb;
            float hir = __builtin_amdgcn_rsqf(hn2);
            float chd = hn2 > 0.f ? ha * hir : 1.0f, shd = hn2 > 0.f ? hb * hir : 0.0f;
            float he = fmaxf(1.0f - (dxn * chd + dyn * shd), 0.f);
            float task2 = min_vel_r * fexp(-(he * he));
            float task_r = rcfg.task1_w * task_r1 + rcfg.task2_w * task2;
            if (terr < rcfg.target_radius * rcfg.target_radius) task_r = 1.0f;
            rbuf.reward_terms[6 * (size_t)N + e] = task_r1;
            rbuf.reward_terms[7 * (size_t)N + e] = task2;
            rbuf.reward_terms[8 * (size_t)N + e] = task_r;
        }
    }
    // ---- reference wave, part 1 (before the barrier, while the target waves are still busy): reference state out
    // Everything the reference wave does lives in this one branch (its values never meet the other roles' registers), including
    // its own copies of the two barriers: it requests the simulator outputs it needs, writes the reference state, meets the
    // other waves at B1, passes B2 at once, and finishes reward / termination while they gather the heightmap and copy out.
    if (is_ref) {
      // the reference wave is the only user of most output pointers and of the reward / termination parameters: it reads them from the
      // kernel-argument block HERE (see kernarg_late) instead of having them loaded at kernel entry and kept in - or spilled from -
      // scalar registers by every wave
      const auto &rbuf = *kernarg_late<parc_env_buffers_t>(KARG_OFF_BUF);
      const auto &rcfg = *kernarg_late<parc_track_cfg_t>(KARG_OFF_CFG);
      const v3 r_pos = p_root;
      const q4 r_rot = r_root;
      const q4 rq = jq;
      float r_contact = 0.f;
      v3 r_vel = mk3(0.f, 0.f, 0.f), r_avel = mk3(0.f, 0.f, 0.f);
      if (what & (PARC_POST_REF | PARC_POST_REWARD_DONE)) {
        // DeepMimicEnv._update_ref_motion  dm_env.py:570-595
        r_contact = valid ? lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend) : 0.f;
        r_vel = ld3(fq.row0 + ml.off_root_vel);
        r_avel = ld3(fq.row0 + ml.off_root_ang_vel);
    }
        if (what & (PARC_POST_REF | PARC_POST_REWARD_DONE)) {
            if (what & PARC_POST_REWARD_DONE) {
                // compute_deepmimic_reward  mgdm_dm_util.py:327-390 (track_root, track_root_h)
                float pose_e = 0.f, vel_e = 0.f, key_e = 0.f, cpen = 0.f;
                int pose_fail = 0, fall_contact = 0, fall_height = 0;
                const v3 sim_pos = ld3(rbuf.rigid_body_state + ((size_t)e * B + (valid ? b : 0)) * 13);
                const v3 sim_root = shfl16(sim_pos, 0);          // body 0 is the root
                const v3 sim_f = ld3(rbuf.contact_forces + ((size_t)e * B + (valid ? b : 0)) * 3);
                // rotation differences, one evaluation for the group: lane b > 0 its joint (simulated vs reference), lane 0 - which has no
                // joint - the ROOT rotation difference that the reward's root term and the termination test need (same function, same inputs
                // as a second call by lane 0 alone would see)
                float rot_diff = 0.f;
                if (valid) {
                    // the simulated character's joint rotation (K1), computed here too: taking it from the character wave would need a
                    // second barrier, and with it every wave of the workgroup would wait for the slowest one
                    q4 cj = c_rot;
                    if (b > 0) cj = joint_rot_lds(dofs);
                    q4 rj = rq;                                         // (lane 0: rq = r_rot, the reference root rotation)
                    if (!rcfg.track_root && b == 0) {                   // convert_to_local (mgdm_dm_util.py:304-325,358-360): heading-relative root rotations
                        cj = quat_mul(calc_heading_quat_inv_alg(c_rot), c_rot);
                        rj = quat_mul(calc_heading_quat_inv_alg(r_rot), r_rot);
                    }
                    rot_diff = quat_diff_angle(cj, rj);
                    if (b > 0) pose_e = rcfg.joint_err_w[b - 1] * rot_diff * rot_diff;
                }
                #pragma unroll 1
                for (int d = b; d < D; d += GRP) {
                    float dv = fq.row0[ml.off_dof_vel + d] - dofs[2 * d + 1];
                    vel_e += rcfg.dof_err_w[d] * dv * dv;
                }
                if (key_slot >= 0) {
                    v3 kr = pos - r_pos, kc = sim_pos - c_pos;
                    if (!rcfg.track_root) {                             // key bodies in each character's own heading frame
                        kr = quat_rotate(calc_heading_quat_inv_alg(r_rot), kr);
                        kc = quat_rotate(calc_heading_quat_inv_alg(c_rot), kc);
                    }
                    v3 df = kr - kc;
                    key_e = dot3(df, df);
                }
                if (valid) {
                    // compute_contact_reward  mgdm_dm_util.py:555-576
                    const v3 f = sim_f;
                    float fn = fminf(fsqrt(dot3(f, f)), 1.0f);
                    float cr = -(1.0f - r_contact) * fn;
                    cr += r_contact * fn;
                    cpen = rcfg.contact_w[b] * cr;
                    // compute_done  mgdm_dm_util.py:392-460
                    if (b > 0) {
                        v3 df = (pos - r_pos) - (sim_pos - sim_root);
                        float lim = rcfg.pose_termination_dist[b - 1];
                        pose_fail = dot3(df, df) > lim * lim;
                    }
                    if (rcfg.num_contact_bodies > 0 && !rcfg.contact_body_mask[b]) {
                        fall_contact = fabsf(f.x) > 0.1f || fabsf(f.y) > 0.1f || fabsf(f.z) > 0.1f;
                        float th = hf_lookup(ter, sim_pos.x + rbuf.env_offsets[3 * e], sim_pos.y + rbuf.env_offsets[3 * e + 1]) + rcfg.termination_height;
                        fall_height = sim_pos.z < th;
                    }
                }
                pose_e = sum16(pose_e);
                vel_e = sum16(vel_e);
                key_e = sum16(key_e);
                cpen = sum16(cpen);
                pose_fail = any16(pose_fail);
                fall_contact = any16(fall_contact);
                fall_height = any16(fall_height);
                if (b == 0 && live) {
                    v3 dp = r_pos - c_pos;
                    if (!rcfg.track_root) dp.x = dp.y = 0.f;     // mgdm_dm_util.py:346-347
                    if (!rcfg.track_root_h) dp.z = 0.f;          // mgdm_dm_util.py:349-350
                    float root_pos_err = dot3(dp, dp);
                    const float rre = rot_diff;
                    float rre2 = rre * rre;
                    v3 cv = ld3(envd[le] + 12), cw = ld3(envd[le] + 15), rv = r_vel, rw = r_avel;
                    if (!rcfg.track_root) {                      // root velocities in each character's own heading frame
                        const q4 hc = calc_heading_quat_inv_alg(c_rot), hr = calc_heading_quat_inv_alg(r_rot);
                        cv = quat_rotate(hc, cv); cw = quat_rotate(hc, cw);
                        rv = quat_rotate(hr, rv); rw = quat_rotate(hr, rw);
                    }
                    v3 dv = rv - cv, dw = rw - cw;
                    float pose_r = fexp(-0.25f * pose_e);
                    float vel_r = fexp(-0.01f * vel_e);
                    float root_pose_r = fexp(-5.0f * (root_pos_err + 0.1f * rre2));
                    float root_vel_r = fexp(-1.0f * (dot3(dv, dv) + 0.1f * dot3(dw, dw)));
                    float key_r = fexp(-10.0f * key_e);
                    float cp = cpen / (float)B;
                    // ig_parkour_env.py:1317-1339,1404
                    float dm = rcfg.reward_w[0] * pose_r + rcfg.reward_w[1] * vel_r + rcfg.reward_w[2] * root_pose_r +
                               rcfg.reward_w[3] * root_vel_r + rcfg.reward_w[4] * key_r;
                    if (rcfg.use_contact_info) dm += cp;        // ig_parkour_env.py:1323-1339
                    rbuf.reward[e] = rcfg.rel_deepmimic_w * dm;
                    const int N = rbuf.reward_terms_stride > 0 ? rbuf.reward_terms_stride : rbuf.num_envs;
                    rbuf.reward_terms[0 * (size_t)N + e] = pose_r;
                    rbuf.reward_terms[1 * (size_t)N + e] = vel_r;
                    rbuf.reward_terms[2 * (size_t)N + e] = root_pose_r;
                    rbuf.reward_terms[3 * (size_t)N + e] = root_vel_r;
                    rbuf.reward_terms[4 * (size_t)N + e] = key_r;
                    rbuf.reward_terms[5 * (size_t)N + e] = cp;
                    // done
                    const float tm = qryd[0][le][7];
                    int done = PARC_DONE_NULL;
                    if (tm >= rcfg.episode_length) done = PARC_DONE_TIME;
                    if (rcfg.enable_early_termination) {
                        int failed = 0;
                        if (rcfg.num_contact_bodies > 0) failed = fall_contact && fall_height;
                        if (rcfg.pose_termination) {
                            int pf = pose_fail;
                            if (rcfg.track_root) {
                                v3 dr = sim_root - r_pos;
                                pf |= dot3(dr, dr) > rcfg.root_pos_termination_dist * rcfg.root_pos_termination_dist;
                                pf |= fabsf(rre) > rcfg.root_rot_termination_angle;
                            }
                            failed |= pf;
                        }
                        if (!(tm > 1e-5f)) failed = 0;
                        if (failed) done = PARC_DONE_FAIL;
                    }
                    // DeepMimicEnv.update_done  dm_env.py:746-783
                    const int motion_end = __float_as_int(qryd[0][le][10]);
                    int kind = 0;
                    if (done != PARC_DONE_NULL || motion_end) kind = (done == PARC_DONE_FAIL) ? 1 : 2;
                    if (motion_end) done = PARC_DONE_FAIL;
                    rbuf.done[e] = done;
                    rbuf.done_kind[e] = kind;
                }
            }
        }
        return;
    }
}

// =============================================================================================
// The reference STATE of one env: DeepMimicEnv._update_ref_motion (dm_env.py:570-595: ref_* buffers, K3 + K2 + K4 at the clip time) and,
// for a restart, the character state initialised from it (RefCharEnv._char_state_init_from_ref + add_noise_to_char_state,
// mgdm_dm_util.py:119-136), by one 16-lane group (lane b = body b).
// Until round 3 this was the first half of the reference wave of track_post_kernel, in front of the reward: the tail every launch
// waited for (full launch 16.5 us, without these stores 15.1 us).  Nothing in a step reads what it writes - the reward wave samples the
// pose itself - so it left the fused kernel: ref_state_kernel runs it alone (a restart's first launch is this small kernel instead of
// the 8-wave one), and in the rollout step it rides as extra workgroups of the fail-rate launch (step_tail_kernel), whose 64 workgroups
// leave almost the whole chip idle for the 10 us their serial walk takes.
// =============================================================================================
PARC_DEV void ref_state_group(const parc_char_model_t &m, const parc_motion_lib_t &ml, const parc_env_buffers_t &buf, const int64_t *env_ids,
                              int n_total, int what, int el, int b) {
    const bool masked = (what & PARC_POST_MASKED) != 0;
    const int elc = min(el, n_total - 1);
    const bool live = el < n_total && (!masked || buf.env_mask[elc] != 0);
    if (masked && !__any(live)) return;                         // wave-uniform: nothing flagged among this wave's 4 envs
    const int e = env_ids ? (int)env_ids[elc] : elc;
    const int B = m.num_bodies, J = B - 1, D = m.dof_size;
    const bool valid = b < B;
    const int64_t mid = buf.motion_ids[e];
    // dataset clips: env time + the clip time the episode started at; generated plans: the plan clock itself (see track_post_kernel)
    const float mtime = (what & PARC_POST_PLAN_CLOCK) ? buf.motion_time_offsets[e] : buf.time_buf[e] + buf.motion_time_offsets[e];
    const frame_query fq = make_query(ml, mid, mtime);
    q4 rq = mk4(0.f, 0.f, 0.f, 1.f);
    if (valid) rq = query_quat(fq, b);
    // root position in the reference's order: lerp, + loop shift, + tile offset (query_root_pos, dm_env.py:604-615)
    v3 r_pos = query_root_pos(ml, fq, mid);
    r_pos.x += buf.motion_xy_offset[2 * e] - buf.env_offsets[3 * e];
    r_pos.y += buf.motion_xy_offset[2 * e + 1] - buf.env_offsets[3 * e + 1];
    const q4 r_rot = shfl16(rq, 0);
    v3 pos;
    q4 rot;
    group_fk<false>(m, b, r_pos, r_rot, rq, pos, rot);
    if (!live) return;
    const float r_contact = valid ? lerp_ref(fq.row0[ml.off_contacts + b], fq.row1[ml.off_contacts + b], fq.blend) : 0.f;
    const v3 r_vel = ld3(fq.row0 + ml.off_root_vel), r_avel = ld3(fq.row0 + ml.off_root_ang_vel);
    if (b == 0) {
        st3(buf.ref_root_pos + 3 * (size_t)e, r_pos);
        st4(buf.ref_root_rot + 4 * (size_t)e, r_rot);
        st3(buf.ref_root_vel + 3 * (size_t)e, r_vel);
        st3(buf.ref_root_ang_vel + 3 * (size_t)e, r_avel);
    } else if (valid) {
        st4(buf.ref_joint_rot + ((size_t)e * J + (b - 1)) * 4, rq);
        joint_rot_to_dof(m, b, rq, buf.ref_dof_pos + (size_t)e * D);      // K4
    }
    if (valid) {
        buf.ref_contacts[(size_t)e * B + b] = r_contact;
        st3(buf.ref_body_pos + ((size_t)e * B + b) * 3, pos);
    }
#pragma unroll 1
    for (int d = b; d < D; d += GRP) buf.ref_dof_vel[(size_t)e * D + d] = fq.row0[ml.off_dof_vel + d];
    if (what & PARC_POST_INIT_CHAR) {
        float *wrs = const_cast<float *>(buf.root_state) + (size_t)e * 13;
        float *wds = const_cast<float *>(buf.dof_state) + (size_t)e * D * 2;
        if (b == 0) {
            v3 ip = r_pos;
            if (buf.init_noise_xy) {
                ip.x += buf.init_noise_xy[2 * e];
                ip.y += buf.init_noise_xy[2 * e + 1];
            }
            st3(wrs, ip);
            st4(wrs + 3, r_rot);
            st3(wrs + 7, r_vel);
            st3(wrs + 10, r_avel);
        } else if (valid) {
            joint_rot_to_dof(m, b, rq, buf.ref_dof_pos + (size_t)e * D, wds);
        }
#pragma unroll 1
        for (int d = b; d < D; d += GRP) wds[2 * d + 1] = fq.row0[ml.off_dof_vel + d];
    }
}

#define REF_STATE_THREADS 256      // 16 envs per workgroup
__global__ __launch_bounds__(REF_STATE_THREADS) void ref_state_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_env_buffers_t buf,
                                                                      const int64_t *__restrict__ env_ids, int n_total, int what) {
    ref_state_group(m, ml, buf, env_ids, n_total, what, (int)(blockIdx.x * (REF_STATE_THREADS / GRP) + (threadIdx.x >> 4)), threadIdx.x & 15);
}

#ifdef PARC_DIAG_BUILD
// occupancy probe: bytes of dynamic LDS added to every workgroup of track_post_kernel (fewer workgroups resident per CU); diagnostics build only
static int g_post_lds_pad = 0;
extern "C" int parc_tune_post_lds_pad(int bytes) {
    if (bytes < 0 || bytes > 120 * 1024) return PARC_EINVAL;
    g_post_lds_pad = bytes;
    return PARC_OK;
}
#define POST_LDS_PAD g_post_lds_pad
#else
#define POST_LDS_PAD 0
#endif

static int track_post_step_impl(void *stream, const parc_char_model_t &model, const parc_motion_lib_t &mlib, const parc_terrain_t &terrain,
                                const parc_track_cfg_t &cfg, const parc_env_buffers_t &buf, const int64_t *env_ids, int n_sel, int what,
                                const float *ray_xy, hipEvent_t start_event, hipEvent_t stop_event) {
    if (!model_ok(model) || mlib.num_bodies != model.num_bodies || mlib.dof_size != model.dof_size) return PARC_EINVAL;
#ifndef PARC_DIAG_BUILD
    if (what & ~PARC_POST_ALL) return PARC_EINVAL;   // only the documented PARC_POST_* bits (the timing-ablation bits exist in the diagnostics build only)
#endif
    if (cfg.num_tar_steps < 0 || cfg.num_tar_steps > PARC_MAX_TAR_STEPS || cfg.num_key_bodies > PARC_MAX_KEY_BODIES) return PARC_EUNSUPPORTED;
    const int B = model.num_bodies, J = B - 1, D = model.dof_size, K = cfg.num_key_bodies, S = cfg.num_tar_steps;
    const int row_len = (12 + 6 * J + D + 3 * K) + S * (9 + 6 * J + 3 * K) + S * B + B;
    if (row_len + cfg.num_ray_points != cfg.obs_dim || cfg.obs_dim > POST_MAX_ROW || (cfg.obs_dim & 3)) return PARC_EINVAL;
    if (what & PARC_POST_HF) {
        if (!(what & PARC_POST_OBS) || !ray_xy || !terrain.hf) return PARC_EINVAL;
    }
    if (((uintptr_t)buf.obs & 15) || ((uintptr_t)mlib.frames & 15) || (mlib.row_stride & 3)) return PARC_EINVAL;
    if ((what & PARC_POST_MASKED) && (env_ids || !buf.env_mask)) return PARC_EINVAL;
    if ((what & PARC_POST_INIT_CHAR) && !(what & PARC_POST_REF)) return PARC_EINVAL;
    if ((what & PARC_POST_TARGETS) && (!buf.next_target_time || !buf.target_rand)) return PARC_EINVAL;
    int n = env_ids ? n_sel : buf.num_envs;
    if (n < 0) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    if (what & PARC_POST_REF) {
        // the reference state is its own small kernel (a caller that also updates the fail rates can have it co-scheduled with that
        // launch instead: parc_step_tail, and leave PARC_POST_REF out here)
        hipLaunchKernelGGL(ref_state_kernel, dim3((n + REF_STATE_THREADS / GRP - 1) / (REF_STATE_THREADS / GRP)), dim3(REF_STATE_THREADS), 0,
                           (hipStream_t)stream, model, mlib, buf, env_ids, n, what);
        PARC_CHECK_LAUNCH();
    }
    if (what & (PARC_POST_OBS | PARC_POST_REWARD_DONE)) {
        const dim3 grid((n + POST_EPB - 1) / POST_EPB);
        const dim3 block(64 * (2 + (cfg.num_tar_steps > 0 ? (cfg.num_tar_steps + 1) / 2 : 0) + (((what & PARC_POST_OBS) && (what & PARC_POST_HF)) ? 1 : 0)));
        if (start_event || stop_event)
            // the same launch with a pair of events bound to THIS dispatch: they carry the kernel's own begin / end time stamps (what a
            // profiler reads from the dispatch), not the time between two separate event records around it
            hipExtLaunchKernelGGL(track_post_kernel, grid, block, POST_LDS_PAD, (hipStream_t)stream, start_event, stop_event, 0, model, mlib, terrain, cfg, buf,
                                  env_ids, n, what, ray_xy);
        else
            hipLaunchKernelGGL(track_post_kernel, grid, block, POST_LDS_PAD, (hipStream_t)stream, model, mlib, terrain, cfg, buf, env_ids, n, what, ray_xy);
        PARC_CHECK_LAUNCH();
    }
    return PARC_OK;
}

extern "C" int parc_track_post_step(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_terrain_t terrain,
                                    parc_track_cfg_t cfg, parc_env_buffers_t buf, const int64_t *env_ids, int n_sel, int what,
                                    const float *ray_xy) {
    return track_post_step_impl(stream, model, mlib, terrain, cfg, buf, env_ids, n_sel, what, ray_xy, nullptr, nullptr);
}

extern "C" int parc_track_post_step_timed(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_terrain_t terrain,
                                          parc_track_cfg_t cfg, parc_env_buffers_t buf, const int64_t *env_ids, int n_sel, int what,
                                          const float *ray_xy, void *start_event, void *stop_event) {
    if (!start_event || !stop_event) return PARC_EINVAL;
    return track_post_step_impl(stream, model, mlib, terrain, cfg, buf, env_ids, n_sel, what, ray_xy, (hipEvent_t)start_event, (hipEvent_t)stop_event);
}

// =============================================================================================
// Observation rows of the non-default layouts: a column gather from [obs row | aux | scalar] (parc_hip.h, parc_assemble_obs)
// =============================================================================================
__global__ __launch_bounds__(256) void assemble_obs_kernel(const float *__restrict__ obs, int obs_dim, const float *__restrict__ aux,
                                                           const float *__restrict__ scalar, const int32_t *__restrict__ col_map,
                                                           float *__restrict__ out, int out_dim, const int64_t *__restrict__ env_ids) {
    const int e = env_ids ? (int)env_ids[blockIdx.y] : (int)blockIdx.y;
    const float sc = scalar ? scalar[0] : 0.f;
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < out_dim; c += gridDim.x * blockDim.x) {
        const int k = col_map[c];
        float v;
        if (k < obs_dim) v = obs[(size_t)e * obs_dim + k];
        else if (k < obs_dim + 4) v = aux[4 * (size_t)e + (k - obs_dim)];
        else v = sc;
        out[(size_t)e * out_dim + c] = v;
    }
}

extern "C" int parc_assemble_obs(void *stream, int n_envs, const float *obs, int obs_dim, const float *aux, const float *scalar,
                                 const int32_t *col_map, float *out, int out_dim, const int64_t *env_ids, int n_sel) {
    if (n_envs < 0 || obs_dim <= 0 || out_dim <= 0 || !obs || !col_map || !out || (env_ids && n_sel < 0)) return PARC_EINVAL;
    const int rows = env_ids ? n_sel : n_envs;
    if (rows == 0) return PARC_OK;
    if (rows > 65535) return PARC_EUNSUPPORTED;          // grid.y
    const int bx = (out_dim + 255) / 256;
    hipLaunchKernelGGL(assemble_obs_kernel, dim3(bx > 2 ? 2 : bx, rows), dim3(256), 0, (hipStream_t)stream, obs, obs_dim, aux, scalar, col_map,
                       out, out_dim, env_ids);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Device-side reset bookkeeping (dm_env.py:517-568, ig_env.py:100-121,693-721), one thread per env
// =============================================================================================
__global__ __launch_bounds__(256) void reset_apply_kernel(int n, const int32_t *__restrict__ mask, const int64_t *__restrict__ new_mid,
                                                          const int64_t *__restrict__ new_tid, const float *__restrict__ new_t,
                                                          const float *__restrict__ offs, int R, int64_t *mid, int64_t *tid, float *toff,
                                                          float *xyoff, int32_t *timestep, float *time_buf, int32_t *done,
                                                          float *next_target_time, int64_t *ep_num) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || mask[e] == 0) return;
    int64_t mi = new_mid[e], ti = new_tid[e];
    mid[e] = mi;
    tid[e] = ti;
    toff[e] = new_t[e];
    xyoff[2 * e] = offs[(mi * R + ti) * 2];
    xyoff[2 * e + 1] = offs[(mi * R + ti) * 2 + 1];
    timestep[e] = 0;
    time_buf[e] = 0.f;
    done[e] = PARC_DONE_NULL;
    next_target_time[e] = 0.f;
    ep_num[e] += 1;
}

extern "C" int parc_reset_apply(void *stream, int n_envs, const int32_t *mask, const int64_t *new_motion_ids, const int64_t *new_terrain_ids,
                                const float *new_time_offsets, const float *motion_offsets, int terrains_per_motion, int64_t *motion_ids,
                                int64_t *motion_terrain_ids, float *motion_time_offsets, float *motion_xy_offset, int32_t *timestep_buf,
                                float *time_buf, int32_t *done, float *next_target_time, int64_t *ep_num) {
    if (n_envs < 0 || terrains_per_motion < 1 || !mask) return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    hipLaunchKernelGGL(reset_apply_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, mask, new_motion_ids,
                       new_terrain_ids, new_time_offsets, motion_offsets, terrains_per_motion, motion_ids, motion_terrain_ids,
                       motion_time_offsets, motion_xy_offset, timestep_buf, time_buf, done, next_target_time, ep_num);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Device-side reset, sampling included (dm_env.py:517-568 + MotionLib.sample_motions / sample_time  anim/motion_lib.py:48-63):
// which envs restart (done != NULL), on which clip (probability ~ weight * max(fail rate, floor)), on which tile copy of the
// clip's terrain (uniform), from which phase (uniform in [0, clip length)), with which xy start noise (uniform in +-scale) -
// all from five uniforms per env that the caller drew in one launch.  Kernel 1 (one workgroup) builds the cumulative weights,
// kernel 2 (one thread per env) inverts them by bisection and does the bookkeeping of reset_apply_kernel.
// =============================================================================================
__global__ __launch_bounds__(256) void reset_cdf_kernel(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w,
                                                        float *cdf);

#define RESET_CDF_LDS 4096          // clips whose cumulative weights a workgroup builds for itself in LDS (16 KB); more: reset_cdf_kernel first

// fp32 product a clip is drawn in proportion to; __fmul_rn so that it never contracts into the addition that follows it
PARC_DEV float reset_clip_product(const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w, int i) {
    return __fmul_rn(fail_rates ? fmaxf(fail_rates[i], min_w) : 1.0f, weights[i]);
}

// cumulative weights into `out` (LDS or global), by the 256 threads of one workgroup - the same steps, hence the same fp32 sums, in
// every workgroup that runs it.  table[i] = base[t] + (running sum inside chunk t), and base[t + 1] IS the last entry of chunk t:
// base[t + 1] = base[t] + (sum of chunk t), the chunk sum being the same chain of additions as the chunk's last running sum.  Rounding
// is monotonic, so the table never decreases and stays flat across clips whose product is 0, inside a chunk and over its seams, which
// the bisection below and "a clip of weight 0 is never drawn" rely on.  (Chunk bases from a parallel scan are another rounding of the
// same sums than the running sums next to them: that table stepped down at seams and up on weight-0 clips, DESIGN.md.)  The bases are a
// serial chain over the chunks, by one thread: at most 256 dependent additions.
PARC_DEV void build_reset_cdf(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w, float *out, float *part) {
    const int chunk = (M + 255) / 256;
    const int nchunks = (M + chunk - 1) / chunk;
    const int i0 = min((int)threadIdx.x * chunk, M), i1 = min(i0 + chunk, M);
    float s = 0.f;
    for (int i = i0; i < i1; ++i) s = __fadd_rn(s, reset_clip_product(weights, fail_rates, min_w, i));
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float base = 0.f;
#pragma unroll 8
        for (int t = 0; t < nchunks; ++t) {
            const float v = part[t];
            part[t] = base;
            base = __fadd_rn(base, v);
        }
    }
    __syncthreads();
    const float base = part[threadIdx.x];
    float run = 0.f;
    for (int i = i0; i < i1; ++i) {
        run = __fadd_rn(run, reset_clip_product(weights, fail_rates, min_w, i));
        out[i] = __fadd_rn(base, run);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void reset_cdf_kernel(int M, const float *__restrict__ weights, const float *__restrict__ fail_rates, float min_w,
                                                        float *cdf) {
    __shared__ float part[256];
    build_reset_cdf(M, weights, fail_rates, min_w, cdf, part);
}

template <bool CDF_IN_LDS>
__global__ __launch_bounds__(256) void reset_sample_apply_kernel(int n, const int32_t *__restrict__ done_in, int32_t *mask, const float *__restrict__ u,
                                                                 int M, const float *__restrict__ cdf_global, const float *__restrict__ weights,
                                                                 const float *__restrict__ fail_rates, float min_w,
                                                                 const float *__restrict__ lengths,
                                                                 const float *__restrict__ offs, int R, float noise_scale, int64_t *mid, int64_t *tid,
                                                                 float *toff, float *xyoff, int32_t *timestep, float *time_buf, int32_t *done,
                                                                 float *next_target_time, int64_t *ep_num, float *init_noise_xy) {
    __shared__ float s_cdf[CDF_IN_LDS ? RESET_CDF_LDS : 1];
    __shared__ float s_part[256];
    const float *cdf = cdf_global;
    if (CDF_IN_LDS) {
        // every workgroup builds the table for itself (M <= 4096 entries: a few hundred flops) instead of a one-workgroup launch in
        // front of this one; workgroup 0 also publishes it (tests read it back)
        build_reset_cdf(M, weights, fail_rates, min_w, s_cdf, s_part);
        if (blockIdx.x == 0 && cdf_global)
            for (int i = threadIdx.x; i < M; i += 256) const_cast<float *>(cdf_global)[i] = s_cdf[i];
        cdf = s_cdf;
    }
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int finished = done_in[e] != PARC_DONE_NULL;
    mask[e] = finished;
    if (!finished) return;
    // clip: first index whose cumulative weight exceeds u * total (searchsorted(..., right=True)), kept inside the table
    const float x = u[e] * cdf[M - 1];
    int lo = 0, hi = M;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (cdf[m] > x) hi = m; else lo = m + 1;
    }
    const int64_t mi = min(lo, M - 1);
    const int64_t ti = min((int)(u[n + e] * (float)R), R - 1);
    mid[e] = mi;
    tid[e] = ti;
    toff[e] = u[2 * n + e] * lengths[mi];
    xyoff[2 * e] = offs[(mi * R + ti) * 2];
    xyoff[2 * e + 1] = offs[(mi * R + ti) * 2 + 1];
    init_noise_xy[2 * e] = (2.0f * u[3 * n + e] - 1.0f) * noise_scale;
    init_noise_xy[2 * e + 1] = (2.0f * u[4 * n + e] - 1.0f) * noise_scale;
    timestep[e] = 0;
    time_buf[e] = 0.f;
    done[e] = PARC_DONE_NULL;
    next_target_time[e] = 0.f;
    ep_num[e] += 1;
}

extern "C" int parc_reset_sample_apply(void *stream, int n_envs, const int32_t *done_flags, int32_t *mask, const float *uniforms, int n_motions,
                                       const float *motion_weights, const float *fail_rates, float min_weight, const float *motion_lengths,
                                       const float *motion_offsets, int terrains_per_motion, float noise_scale, float *cdf_workspace,
                                       int64_t *motion_ids, int64_t *motion_terrain_ids, float *motion_time_offsets, float *motion_xy_offset,
                                       int32_t *timestep_buf, float *time_buf, int32_t *done, float *next_target_time, int64_t *ep_num,
                                       float *init_noise_xy) {
    if (n_envs < 0 || n_motions < 1 || terrains_per_motion < 1 || !done_flags || !mask || !uniforms || !motion_weights || !motion_lengths ||
        !cdf_workspace || !init_noise_xy)
        return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    if (n_motions <= RESET_CDF_LDS) {
        hipLaunchKernelGGL(reset_sample_apply_kernel<true>, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, done_flags, mask,
                           uniforms, n_motions, cdf_workspace, motion_weights, fail_rates, min_weight, motion_lengths, motion_offsets,
                           terrains_per_motion, noise_scale, motion_ids, motion_terrain_ids, motion_time_offsets, motion_xy_offset, timestep_buf,
                           time_buf, done, next_target_time, ep_num, init_noise_xy);
    } else {
        hipLaunchKernelGGL(reset_cdf_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_motions, motion_weights, fail_rates, min_weight, cdf_workspace);
        hipLaunchKernelGGL(reset_sample_apply_kernel<false>, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, done_flags, mask,
                           uniforms, n_motions, cdf_workspace, motion_weights, fail_rates, min_weight, motion_lengths, motion_offsets,
                           terrains_per_motion, noise_scale, motion_ids, motion_terrain_ids, motion_time_offsets, motion_xy_offset, timestep_buf,
                           time_buf, done, next_target_time, ep_num, init_noise_xy);
    }
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Fail-rate EMA (dm_env.py:758-772): for every env that finished this step, in env order,
//     fail_rate[clip] = (1 - w) fail_rate[clip] + w [episode failed]
// One 256-thread workgroup per clip.  Pass i reads the done flags of envs 256 i .. 256 i + 255 coalesced; a wave-wide ballot
// turns "finished on this clip" / "and failed" into two 64-bit masks per (pass, wave), parked in LDS.  Thread 0 then walks the
// set bits in env order and applies the updates one by one - the same fp32 operations in the same order as the reference's
// loop over done envs, so the result is bit-identical to it.  Clips nobody finished on (almost all of them, every step) cost
// the flag reads and nothing else.
// =============================================================================================
#define FR_THREADS 256
#define FR_MAX_PASSES 64          // up to 16384 envs per launch segment; larger counts loop over segments
typedef unsigned long long fr_masks_t[FR_MAX_PASSES][FR_THREADS / 64];
PARC_DEV void fail_rate_block(int mi, int n_envs, const int64_t *__restrict__ motion_ids, const int32_t *__restrict__ done_kind, float ema_w,
                              float *fail_rates, fr_masks_t &hit, fr_masks_t &fail) {
    const int wv = threadIdx.x >> 6;
    const float keep = (float)(1.0 - (double)ema_w);       // the reference multiplies by the python double (1.0 - w), cast to fp32
    float fr = 0.f;
    bool touched = false;
    if (threadIdx.x == 0) fr = fail_rates[mi];
    for (int seg = 0; seg < n_envs; seg += FR_MAX_PASSES * FR_THREADS) {
        const int passes = min(FR_MAX_PASSES, (n_envs - seg + FR_THREADS - 1) / FR_THREADS);
        for (int i0 = 0; i0 < passes; i0 += 8) {          // 8 passes at a time: their flag loads are in flight together
            int ks[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = seg + (i0 + u) * FR_THREADS + threadIdx.x;
                ks[u] = (i0 + u < passes && e < n_envs) ? done_kind[e] : 0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + u >= passes) break;
                const int e = seg + (i0 + u) * FR_THREADS + threadIdx.x;
                const int k = ks[u];
                const bool h = k != 0 && motion_ids[e] == mi;
                const unsigned long long hm = __ballot(h), fm = __ballot(h && k == 1);
                if ((threadIdx.x & 63) == 0) {
                    hit[i0 + u][wv] = hm;
                    fail[i0 + u][wv] = fm;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 0; i < passes; ++i)
                for (int w = 0; w < FR_THREADS / 64; ++w) {
                    unsigned long long hm = hit[i][w];
                    const unsigned long long fm = fail[i][w];
                    while (hm) {
                        const int bit = __ffsll((long long)hm) - 1;
                        hm &= hm - 1;
                        fr = mul_add_unfused(fr, keep, ((fm >> bit) & 1ull) ? ema_w : 0.f);     // two roundings, like fr * keep + w in torch
                        touched = true;
                    }
                }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && touched) fail_rates[mi] = fr;
}

__global__ __launch_bounds__(FR_THREADS) void fail_rate_kernel(int n_envs, int n_motions, const int64_t *__restrict__ motion_ids,
                                                               const int32_t *__restrict__ done_kind, float ema_w, float *fail_rates) {
    __shared__ fr_masks_t hit, fail;
    fail_rate_block(blockIdx.x, n_envs, motion_ids, done_kind, ema_w, fail_rates, hit, fail);
}

// The tail of an env step in ONE launch of heterogeneous workgroups: blocks [0, n_motions) walk the fail-rate EMA of one clip each
// (64 workgroups that keep the chip almost idle for the ~10 us the bit-exact serial walk takes), blocks behind them publish the
// reference STATE of 16 envs each (ref_state_group) on the idle CUs.  Both only read what the fused launch and the simulator left.
static_assert(FR_THREADS == REF_STATE_THREADS, "one block size for both kinds of workgroup");
__global__ __launch_bounds__(FR_THREADS) void step_tail_kernel(parc_char_model_t m, parc_motion_lib_t ml, parc_env_buffers_t buf, int n_envs, int what,
                                                               int n_motions, const int32_t *__restrict__ done_kind, float ema_w, float *fail_rates) {
    __shared__ fr_masks_t hit, fail;
    if ((int)blockIdx.x < n_motions) {
        fail_rate_block(blockIdx.x, n_envs, buf.motion_ids, done_kind, ema_w, fail_rates, hit, fail);
        return;
    }
    const int blk = (int)blockIdx.x - n_motions;
    ref_state_group(m, ml, buf, nullptr, n_envs, what, blk * (REF_STATE_THREADS / GRP) + (int)(threadIdx.x >> 4), threadIdx.x & 15);
}

extern "C" int parc_step_tail(void *stream, parc_char_model_t model, parc_motion_lib_t mlib, parc_env_buffers_t buf, int what, int n_motions,
                              const int32_t *done_kind, float ema_w, float *fail_rates) {
    if (!model_ok(model) || mlib.num_bodies != model.num_bodies || mlib.dof_size != model.dof_size) return PARC_EINVAL;
    if (n_motions != mlib.num_motions || !done_kind || !fail_rates || buf.num_envs < 0) return PARC_EINVAL;
    if (what & ~(PARC_POST_REF | PARC_POST_PLAN_CLOCK)) return PARC_EINVAL;      // the per-step publication only (no restart variants)
    const int n = buf.num_envs;
    if (n == 0) return PARC_OK;
    const int state_blocks = (what & PARC_POST_REF) ? (n + REF_STATE_THREADS / GRP - 1) / (REF_STATE_THREADS / GRP) : 0;
    hipLaunchKernelGGL(step_tail_kernel, dim3(n_motions + state_blocks), dim3(FR_THREADS), 0, (hipStream_t)stream, model, mlib, buf, n, what, n_motions,
                       done_kind, ema_w, fail_rates);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_update_fail_rates(void *stream, int n_envs, int n_motions, const int64_t *motion_ids, const int32_t *done_kind,
                                      float ema_w, float *fail_rates) {
    if (n_envs < 0 || n_motions <= 0) return PARC_EINVAL;
    hipLaunchKernelGGL(fail_rate_kernel, dim3(n_motions), dim3(FR_THREADS), 0, (hipStream_t)stream, n_envs, n_motions, motion_ids, done_kind,
                       ema_w, fail_rates);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K16 TD(lambda): one env per lane, backward recurrence in a register; [T,N] loads coalesce over envs
// =============================================================================================
__global__ __launch_bounds__(256) void td_lambda_kernel(int T, int N, const float *__restrict__ r, const float *__restrict__ nv,
                                                        const int32_t *__restrict__ done, float discount, float lam, float *ret) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= N) return;
    size_t i = (size_t)(T - 1) * N + e;
    float next_ret = r[i] + discount * nv[i];
    ret[i] = next_ret;
    for (int t = T - 2; t >= 0; --t) {
        i = (size_t)t * N + e;
        float reset = done[i] != PARC_DONE_NULL ? 1.f : 0.f;
        float cl = lam * (1.0f - reset);
        float cur = r[i] + discount * ((1.0f - cl) * nv[i] + cl * next_ret);
        ret[i] = cur;
        next_ret = cur;
    }
}

extern "C" int parc_td_lambda_return(void *stream, int T, int N, const float *reward, const float *next_vals, const int32_t *done,
                                     float discount, float td_lambda, float *ret) {
    if (T <= 0 || N < 0) return PARC_EINVAL;
    if (N == 0) return PARC_OK;
    hipLaunchKernelGGL(td_lambda_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, T, N, reward, next_vals, done,
                       discount, td_lambda, ret);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K17 advantage normalisation: deterministic two-stage (sum, sumsq, count) in fp64, then normalise.
// Non-finite input as torch.std_mean / clamp_min / clamp (dm_ppo_agent.py:393-400): no selected sample -> mean and std NaN, one -> std
// NaN, a NaN or Inf among the selected advantages -> both NaN (torch's running mean meets inf - inf); a NaN std makes every advantage
// NaN; a NaN return or value of an unselected sample stays in its element.
// =============================================================================================
#define ADV_BLOCKS 1024
__global__ __launch_bounds__(256) void adv_partial_kernel(int n, const float *__restrict__ ret, const float *__restrict__ vals,
                                                          const float *__restrict__ mask, double *ws) {
    __shared__ double sh[3][256];
    double s = 0.0, ss = 0.0, c = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (mask[i] == 1.0f) {
            double a = (double)(ret[i] - vals[i]);
            s += a;
            ss += a * a;
            c += 1.0;
        }
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = ss;
    sh[2][threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + st];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + st];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + st];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = sh[0][0];
        ws[ADV_BLOCKS + blockIdx.x] = sh[1][0];
        ws[2 * ADV_BLOCKS + blockIdx.x] = sh[2][0];
    }
}

__global__ __launch_bounds__(256) void adv_apply_kernel(int n, int nblocks, const float *__restrict__ ret, const float *__restrict__ vals,
                                                        float clip, const double *__restrict__ ws, float *out, float *mean_std) {
    __shared__ double sh[3][256];
    double s = 0.0, ss = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s += ws[i];
        ss += ws[ADV_BLOCKS + i];
        c += ws[2 * ADV_BLOCKS + i];
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = ss;
    sh[2][threadIdx.x] = c;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + st];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + st];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + st];
        }
        __syncthreads();
    }
    double cnt = sh[2][0];
    double mean = sh[0][0] / cnt;                                          // (cnt 0: 0 / 0)
    double var = (sh[1][0] - cnt * mean * mean) / (cnt - 1.0);             // torch.std_mean: unbiased  (cnt 1: 0 / 0)
    var = var < 0.0 ? 0.0 : var;                                           // (a NaN passes)
    if (!(sh[1][0] < (double)INFINITY)) mean = (double)NAN;                // (fp32 squares cannot overflow a double: a non-finite sample)
    float meanf = (float)mean, stdf = (float)sqrt(var);
    float den = stdf < 1e-5f ? 1e-5f : stdf;                               // torch.clamp_min: NaN stays NaN
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mean_std[0] = meanf;
        mean_std[1] = stdf;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float a = ((ret[i] - vals[i]) - meanf) / den;
        out[i] = a < -clip ? -clip : (a > clip ? clip : a);              // torch.clamp: NaN stays NaN
    }
}

extern "C" int parc_adv_normalize(void *stream, int n, const float *ret, const float *vals, const float *rand_action_mask, float clip,
                                  float *norm_adv, float *mean_std_out, double *workspace) {
    if (n <= 0 || !workspace) return PARC_EINVAL;
    int nb = (n + 255) / 256;
    if (nb > ADV_BLOCKS) nb = ADV_BLOCKS;
    hipLaunchKernelGGL(adv_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, n, ret, vals, rand_action_mask, workspace);
    hipLaunchKernelGGL(adv_apply_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, n, nb, ret, vals, clip, workspace, norm_adv, mean_std_out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_abi_version(void) { return 1; }
