// The stand-alone local heightmap gather (K5) of the environment, with its measurement knobs in the diagnostics build.
// C-ABI in include/parc_hip.h.  Reference citations are relative to the reference root.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_math.h"
#include "parc_hf_lookup.h"     // hf_lookup, hf_env_params

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
#else
static constexpr int g_hf_epb = 2;
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
