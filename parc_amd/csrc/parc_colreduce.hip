// Passes over the rows of a [rows, dim] array (gfx950): the observation normaliser, and the column reductions of the learner - the
// normaliser's running moments (alone and inside parc_obs_ingest), the bias gradient behind a ReLU and the weighted column sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_learner_math.h"

// =============================================================================================
// K12 observation normalisation: Normalizer.normalize (learning/normalizer.py:60-63)  out = clamp((x - mean) / std, -clip, clip)
// in one pass (torch: subtract, divide, clamp = three passes).  Same fp32 operations: finite results are bit-identical, and a NaN (a NaN
// observation, mean or std, 0 / 0 under a zero std) comes out as NaN, as from torch.clamp; +-inf clamps to +-clip.
// =============================================================================================
__global__ __launch_bounds__(256) void normalize_clamp_kernel(size_t n4, int dim4, const float4 *__restrict__ x, const float4 *__restrict__ mean,
                                                              const float4 *__restrict__ stdv, float clip, float4 *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % (size_t)dim4);
        const float4 v = x[i], m = mean[c], s = stdv[c];
        float4 o;
        o.x = clamp_nan((v.x - m.x) / s.x, -clip, clip);
        o.y = clamp_nan((v.y - m.y) / s.y, -clip, clip);
        o.z = clamp_nan((v.z - m.z) / s.z, -clip, clip);
        o.w = clamp_nan((v.w - m.w) / s.w, -clip, clip);
        out[i] = o;
    }
}

extern "C" int parc_normalize_clamp(void *stream, int64_t rows, int dim, const float *x, const float *mean, const float *stdv, float clip,
                                    float *out) {
    if (rows < 0 || dim <= 0 || (dim & 3) || (((uintptr_t)x | (uintptr_t)mean | (uintptr_t)stdv | (uintptr_t)out) & 15)) return PARC_EINVAL;
    if (rows == 0) return PARC_OK;
    const size_t n4 = (size_t)rows * (size_t)(dim / 4);
    hipLaunchKernelGGL(normalize_clamp_kernel, dim3(parc_capped_blocks(n4, 8192)), dim3(256), 0, (hipStream_t)stream, n4, dim / 4, (const float4 *)x,
                       (const float4 *)mean, (const float4 *)stdv, clip, (float4 *)out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// The column-chunk skeleton of the four stage-1 kernels below.  A 256-thread workgroup owns `chunk_rows` rows x 256 columns: 64 float4
// lanes x 4 row groups (the waves), grid = (column blocks, chunks).  Row group rg takes the rows r0 + rg, r0 + rg + 4, ... below r1 and
// keeps its column sums in registers; the four row groups are then parked in LDS and added as (0 + 1) + (2 + 3), and the workgroup
// stores one partial row.  Stage 2 adds the partial rows of a column in chunk order.  Fixed summation order, no atomics: the result
// does not depend on scheduling.
// =============================================================================================
struct col_chunk_t {
    int lane, rg, c, r0, r1;        // float4 lane, row group, float4 column (live when < dim4), the chunk's rows [r0, r1)
};

__device__ __forceinline__ col_chunk_t col_chunk(int rows, int chunk_rows) {
    const int lane = threadIdx.x & 63, r0 = blockIdx.y * chunk_rows;
    return {lane, (int)(threadIdx.x >> 6), (int)(blockIdx.x * 64 + lane), r0, min(r0 + chunk_rows, rows)};
}

__device__ __forceinline__ float4 fold_row_groups(const float4 (*red)[64], int lane) {
    const float4 a = red[0][lane], b = red[1][lane], d = red[2][lane], e = red[3][lane];
    float4 o;
    o.x = (a.x + b.x) + (d.x + e.x); o.y = (a.y + b.y) + (d.y + e.y); o.z = (a.z + b.z) + (d.z + e.z); o.w = (a.w + b.w) + (d.w + e.w);
    return o;
}

// one array of column sums: park, fold on wave 0, partial row `chunk`
__device__ __forceinline__ void fold_store(float4 (*red)[64], const float4 &s, const col_chunk_t &k, int dim4, float4 *__restrict__ partial) {
    red[k.rg][k.lane] = s;
    __syncthreads();
    if (k.rg == 0 && k.c < dim4) partial[(size_t)blockIdx.y * dim4 + k.c] = fold_row_groups(red, k.lane);
}

// sums and sums of squares: wave 0 folds the sums, wave 1 the sums of squares, partial rows 2 * chunk and 2 * chunk + 1
__device__ __forceinline__ void fold_store_moments(float4 (*red)[4][64], const float4 &s, const float4 &q, const col_chunk_t &k, int dim4,
                                                   float4 *__restrict__ partial) {
    red[0][k.rg][k.lane] = s;
    red[1][k.rg][k.lane] = q;
    __syncthreads();
    if (k.rg < 2 && k.c < dim4) partial[((size_t)blockIdx.y * 2 + k.rg) * dim4 + k.c] = fold_row_groups(red[k.rg], k.lane);
}

// Host side of the skeleton: the argument checks that the four entry points share (aligned16: the pointers that are read or written
// as float4, or-ed; missing: a required pointer is NULL) and, when rc is PARC_OK, the launch geometry.
struct col_grid_t {
    int rc, dim4, chunks;
    dim3 grid;
};

static col_grid_t col_chunk_grid(int64_t rows, int dim, int chunk_rows, uintptr_t aligned16, bool missing) {
    if (rows < 0 || dim <= 0 || (dim & 3) || missing || (aligned16 & 15)) return {PARC_EINVAL};
    if (rows > (int64_t)chunk_rows * 65535) return {PARC_EUNSUPPORTED};
    const int dim4 = dim / 4, chunks = (int)((rows + chunk_rows - 1) / chunk_rows);
    return {PARC_OK, dim4, chunks, dim3((dim4 + 63) / 64, chunks)};
}

// =============================================================================================
// K22 running-moment statistics: Normalizer.record (learning/normalizer.py:28-34)  acc[0] += sum_rows x, acc[1] += sum_rows x^2.
// torch: two column reductions + a square + two adds (and their temporaries) per call; here one pass over x.  Stage 1: a
// workgroup owns MOM_ROWS rows x 256 columns of the skeleton above and writes one partial row of sums and one of sums of squares;
// stage 2 adds the partial rows of a column in chunk order into acc.
// =============================================================================================
#define MOM_ROWS 64
__global__ __launch_bounds__(256) void moments_partial_kernel(int rows, int dim4, const float4 *__restrict__ x, float4 *__restrict__ partial) {
    __shared__ float4 red[2][4][64];
    const col_chunk_t k = col_chunk(rows, MOM_ROWS);
    const int rg = k.rg, c = k.c, r0 = k.r0, r1 = k.r1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    if (c < dim4) {
        for (int r = r0 + rg; r < r1; r += 4) {
            const float4 v = x[(size_t)r * dim4 + c];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            q.x = fmaf(v.x, v.x, q.x); q.y = fmaf(v.y, v.y, q.y); q.z = fmaf(v.z, v.z, q.z); q.w = fmaf(v.w, v.w, q.w);
        }
    }
    fold_store_moments(red, s, q, k, dim4, partial);
}

// The rollout step's three passes over the observation rows in ONE (parc_obs_ingest): Normalizer.normalize for the policy forward
// (normalizer.py:60-63; same fp32 operations as normalize_clamp_kernel: bit-identical, NaN for NaN), ExperienceBuffer.record of the raw rows
// (experience_buffer.py:55-59) into time row *copy_row, and stage 1 of Normalizer.record (the kernel above: the same skeleton, hence the
// same partial rows).  The rows are read once instead of three times.
__global__ __launch_bounds__(256) void obs_ingest_kernel(int rows, int dim4, const float4 *__restrict__ x, const float4 *__restrict__ mean,
                                                         const float4 *__restrict__ stdv, float clip, float4 *__restrict__ norm_out,
                                                         float4 *copy_dst, const int64_t *__restrict__ copy_row, float4 *partial) {
    __shared__ float4 red[2][4][64];
    const col_chunk_t k = col_chunk(rows, MOM_ROWS);
    const int rg = k.rg, c = k.c, r0 = k.r0, r1 = k.r1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
    if (c < dim4) {
        const float4 m = mean[c], sd = stdv[c];
        float4 *dst = copy_dst ? copy_dst + (size_t)copy_row[0] * (size_t)rows * dim4 : nullptr;
        for (int r = r0 + rg; r < r1; r += 4) {
            const size_t i = (size_t)r * dim4 + c;
            const float4 v = x[i];
            float4 o;
            o.x = clamp_nan((v.x - m.x) / sd.x, -clip, clip);
            o.y = clamp_nan((v.y - m.y) / sd.y, -clip, clip);
            o.z = clamp_nan((v.z - m.z) / sd.z, -clip, clip);
            o.w = clamp_nan((v.w - m.w) / sd.w, -clip, clip);
            norm_out[i] = o;
            if (dst) {                       // (the buffer row is not read again before the update phase: streamed store)
                typedef float f32x4 __attribute__((ext_vector_type(4)));
                f32x4 vv = {v.x, v.y, v.z, v.w};
                __builtin_nontemporal_store(vv, reinterpret_cast<f32x4 *>(dst) + i);
            }
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            q.x = fmaf(v.x, v.x, q.x); q.y = fmaf(v.y, v.y, q.y); q.z = fmaf(v.z, v.z, q.z); q.w = fmaf(v.w, v.w, q.w);
        }
    }
    if (!partial) return;               // (uniform: a launch argument)
    fold_store_moments(red, s, q, k, dim4, partial);
}

// (stage 2 stays a launch of its own: folded into stage 1 behind per-column-block tickets - round 4 - the launch took 38 us instead of
// 6.8 + 4.9: the partial rows must be visible to the last workgroup, and a device-scope release fence per workgroup costs more than
// the launch it saves)
__global__ __launch_bounds__(256) void moments_final_kernel(int chunks, int dim4, const float4 *__restrict__ partial, float4 *acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // over [2, dim4]
    if (i >= 2 * dim4) return;
    const int which = i / dim4, c = i - which * dim4;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 16
    for (int k = 0; k < chunks; ++k) {          // (unrolled: the loads of 16 chunks are in flight together; the adds stay in chunk order)
        const float4 v = partial[((size_t)k * 2 + which) * dim4 + c];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    float4 a = acc[i];
    a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
    acc[i] = a;
}

static void launch_moments_final(void *stream, const col_grid_t &g, const float *workspace, float *acc) {
    hipLaunchKernelGGL(moments_final_kernel, dim3((2 * g.dim4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, g.chunks, g.dim4,
                       (const float4 *)workspace, (float4 *)acc);
}

extern "C" int64_t parc_moments_workspace_floats(int64_t rows, int dim) {
    if (rows < 0 || dim <= 0) return -1;
    return ((rows + MOM_ROWS - 1) / MOM_ROWS) * 2 * (int64_t)dim;
}

extern "C" int parc_obs_ingest(void *stream, int64_t rows, int dim, const float *x, const float *mean, const float *stdv, float clip, float *norm_out,
                               float *copy_dst, const int64_t *copy_row, float *acc, float *workspace) {
    const col_grid_t g = col_chunk_grid(rows, dim, MOM_ROWS,
                                        (uintptr_t)x | (uintptr_t)mean | (uintptr_t)stdv | (uintptr_t)norm_out | (uintptr_t)copy_dst | (uintptr_t)acc | (uintptr_t)workspace,
                                        !x || !mean || !stdv || !norm_out || (copy_dst && !copy_row) || (acc && !workspace));
    if (g.rc != PARC_OK || rows == 0) return g.rc;
    hipLaunchKernelGGL(obs_ingest_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, (int)rows, g.dim4, (const float4 *)x, (const float4 *)mean,
                       (const float4 *)stdv, clip, (float4 *)norm_out, (float4 *)copy_dst, copy_row, acc ? (float4 *)workspace : (float4 *)nullptr);
    if (acc) launch_moments_final(stream, g, workspace, acc);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_moments_accumulate(void *stream, int64_t rows, int dim, const float *x, float *acc, float *workspace) {
    const col_grid_t g = col_chunk_grid(rows, dim, MOM_ROWS, (uintptr_t)x | (uintptr_t)acc | (uintptr_t)workspace, false);
    if (g.rc != PARC_OK || rows == 0) return g.rc;
    hipLaunchKernelGGL(moments_partial_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, (int)rows, g.dim4, (const float4 *)x, (float4 *)workspace);
    launch_moments_final(stream, g, workspace, acc);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// Backward of y = relu(x W^T + b) between the two GEMMs: g = y <= 0 ? 0 : gy (threshold_backward: a NaN activation passes gy), written
// over gy, and the bias gradient db = column sums
// of g, in ONE pass over the [rows, dim] activations (autograd runs threshold_backward, then a separate reduction that re-reads g,
// then an accumulate into .grad).  RB_ROWS rows x 256 columns of the skeleton above per workgroup; stage 2 adds the per-chunk partial
// rows in chunk order and OVERWRITES db.  The forward pass is learning/nets/fc_3layers_2048units.py:4-22 of the reference; this is its
// derivative.
// =============================================================================================
#define RB_ROWS 128
__global__ __launch_bounds__(256) void relu_bwd_bias_partial_kernel(int rows, int dim4, float4 *__restrict__ gy, const float4 *__restrict__ y,
                                                                    float4 *__restrict__ partial) {
    __shared__ float4 red[4][64];
    const col_chunk_t k = col_chunk(rows, RB_ROWS);
    const int rg = k.rg, c = k.c, r0 = k.r0, r1 = k.r1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim4) {
#pragma unroll 4
        for (int r = r0 + rg; r < r1; r += 4) {
            const size_t i = (size_t)r * dim4 + c;
            float4 g = gy[i];
            const float4 a = y[i];
            g.x = a.x <= 0.f ? 0.f : g.x; g.y = a.y <= 0.f ? 0.f : g.y; g.z = a.z <= 0.f ? 0.f : g.z; g.w = a.w <= 0.f ? 0.f : g.w;
            gy[i] = g;
            s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
        }
    }
    fold_store(red, s, k, dim4, partial);
}

__global__ __launch_bounds__(256) void colsum_final_kernel(int chunks, int dim, const float *__restrict__ partial, float *__restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= dim) return;
    float t = 0.f;
#pragma unroll 16
    for (int k = 0; k < chunks; ++k) t += partial[(size_t)k * dim + c];
    out[c] = t;
}

// out[c] = sum_r w[r] * x[r, c]: the weight gradient of a Linear layer with ONE output (the value head: dW = g_pred^T h), which as
// a GEMM with M = 1 costs the library 62 us and as its transposed gemv 311 us for 33 MB of reading; same two stages as above.
__global__ __launch_bounds__(256) void weighted_colsum_partial_kernel(int rows, int dim4, const float4 *__restrict__ x, const float *__restrict__ w,
                                                                      float4 *__restrict__ partial) {
    __shared__ float4 red[4][64];
    const col_chunk_t k = col_chunk(rows, RB_ROWS);
    const int rg = k.rg, c = k.c, r0 = k.r0, r1 = k.r1;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim4) {
#pragma unroll 4
        for (int r = r0 + rg; r < r1; r += 4) {
            const float4 v = x[(size_t)r * dim4 + c];
            const float wr = w[r];
            s.x = fmaf(wr, v.x, s.x); s.y = fmaf(wr, v.y, s.y); s.z = fmaf(wr, v.z, s.z); s.w = fmaf(wr, v.w, s.w);
        }
    }
    fold_store(red, s, k, dim4, partial);
}

static void launch_colsum_final(void *stream, const col_grid_t &g, int dim, const float *workspace, float *out) {
    hipLaunchKernelGGL(colsum_final_kernel, dim3((dim + 255) / 256), dim3(256), 0, (hipStream_t)stream, g.chunks, dim, workspace, out);
}

extern "C" int parc_weighted_colsum(void *stream, int64_t rows, int dim, const float *x, const float *w, float *out, float *workspace) {
    const col_grid_t g = col_chunk_grid(rows, dim, RB_ROWS, (uintptr_t)x | (uintptr_t)workspace, !x || !w || !out || !workspace);
    if (g.rc != PARC_OK) return g.rc;
    if (rows > 0)
        hipLaunchKernelGGL(weighted_colsum_partial_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, (int)rows, g.dim4, (const float4 *)x, w,
                           (float4 *)workspace);
    launch_colsum_final(stream, g, dim, workspace, out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int64_t parc_relu_bwd_workspace_floats(int64_t rows, int dim) {
    if (rows < 0 || dim <= 0) return -1;
    return ((rows + RB_ROWS - 1) / RB_ROWS) * (int64_t)dim;
}

extern "C" int parc_relu_bwd_bias_grad(void *stream, int64_t rows, int dim, float *gy, const float *y, float *db, float *workspace) {
    const col_grid_t g = col_chunk_grid(rows, dim, RB_ROWS, (uintptr_t)gy | (uintptr_t)y | (uintptr_t)workspace, !gy || !y || !db || !workspace);
    if (g.rc != PARC_OK) return g.rc;
    if (rows > 0)
        hipLaunchKernelGGL(relu_bwd_bias_partial_kernel, g.grid, dim3(256), 0, (hipStream_t)stream, (int)rows, g.dim4, (float4 *)gy, (const float4 *)y,
                           (float4 *)workspace);
    launch_colsum_final(stream, g, dim, workspace, db);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}
