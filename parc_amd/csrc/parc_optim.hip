// The optimizer step over flat parameter buffers (gfx950): clipping by the global gradient norm, SGD with momentum and AdamW, as
// MPOptimizer (learning/mp_optimizer.py) applies them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_learner_math.h"

// =============================================================================================
// Gradient clipping by global norm (torch.nn.utils.clip_grad_norm_ as MPOptimizer applies it to its flat gradient buffer):
// x *= min(max_norm / (norm + 1e-6), 1) with norm read from device memory - one launch instead of add, reciprocal, mul, clamp, mul.
// A NaN norm scales every element by NaN, as torch's clamp of the coefficient does.
// =============================================================================================
__global__ __launch_bounds__(256) void scale_by_clipped_norm_kernel(size_t n, float *x, const float *__restrict__ norm, float max_norm) {
    const float s = clip_coef(max_norm, norm[0]);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] *= s;
}

extern "C" int parc_scale_by_clipped_norm(void *stream, int64_t n, float *x, const float *norm, float max_norm) {
    if (n < 0 || !x || !norm || !(max_norm > 0.f)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(scale_by_clipped_norm_kernel, dim3(parc_capped_blocks((size_t)n, 8192)), dim3(256), 0, (hipStream_t)stream, (size_t)n, x, norm,
                       max_norm);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K20 optimizer step over flat buffers: MPOptimizer.step (learning/mp_optimizer.py:20-40) = clip_grad_norm_ + SGD with momentum, as
// TWO passes over the 10.6 M parameters instead of four (norm, scale, multi-tensor SGD, + a zero fill): pass 1 the squared norm of
// the flat gradient (1024 block partials), pass 2 every block first adds the partials in block order (fixed order, the same value
// in every block), coef = min(max_norm / (norm + 1e-6), 1), then for its elements g' = coef g (+ wd p), m = mu m + g', p -= lr m
// (torch.optim.SGD, dampening 0, no Nesterov; a zero momentum buffer reproduces its first-step rule buf = g').  A NaN in the gradient
// makes the norm and with it coef NaN: every parameter and momentum element becomes NaN, as after clip_grad_norm_ (max_norm <= 0: no
// norm, the NaN stays in its element).
// =============================================================================================
#define SGD_PARTS 1024
__global__ __launch_bounds__(256) void sumsq_partial_kernel(size_t n4, const float4 *__restrict__ g, size_t n, const float *__restrict__ gs,
                                                            float *__restrict__ partial) {
    __shared__ float red[4];
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 v = g[i];
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {       // tail elements beyond the last whole float4
        const float t = gs[4 * n4 + threadIdx.x];
        acc = fmaf(t, t, acc);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// pass 1 of both steps (max_norm > 0 only: without a clip nobody reads the norm)
static void launch_sumsq_partial(hipStream_t st, int64_t n, const float *grad, float *workspace) {
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(SGD_PARTS), dim3(256), 0, st, (size_t)n / 4, (const float4 *)grad, (size_t)n, grad, workspace);
}

// The head of pass 2, for a whole 256-thread block: the clip coefficient from the SGD_PARTS partials of pass 1, added in the same order
// in every block (1 when max_norm <= 0); block 0 also stores the norm.  The LDS it folds through is its own.
__device__ __forceinline__ float clip_coef_of_partials(const float *__restrict__ partial, float max_norm, float *norm_out) {
    __shared__ float s_red[256];
    float coef = 1.0f;
    if (max_norm > 0.f) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < SGD_PARTS / 256; ++k) a += partial[threadIdx.x * (SGD_PARTS / 256) + k];      // consecutive partials per thread
        s_red[threadIdx.x] = a;
        __syncthreads();
        for (int w = 128; w >= 1; w >>= 1) {          // pairwise tree over the 256 per-thread sums: the same order in every block
            if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
            __syncthreads();
        }
        const float norm = sqrtf(s_red[0]);
        coef = clip_coef(max_norm, norm);
        if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
    }
    return coef;
}

__global__ __launch_bounds__(256) void sgd_momentum_clip_kernel(size_t n, float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                                const float *__restrict__ partial, float max_norm, float lr, float mu, float wd,
                                                                float *norm_out) {
    const float coef = clip_coef_of_partials(partial, max_norm, norm_out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float pi = p[i];
        float gi = coef * g[i];
        if (wd != 0.f) gi = fmaf(wd, pi, gi);
        const float mi = fmaf(mu, m[i], gi);
        m[i] = mi;
        p[i] = fmaf(-lr, mi, pi);
    }
}

extern "C" int64_t parc_sgd_workspace_floats(void) { return SGD_PARTS; }

extern "C" int parc_sgd_momentum_step(void *stream, int64_t n, float *params, const float *grad, float *momentum_buf, float max_norm, float lr,
                                      float momentum, float weight_decay, float *workspace, float *norm_out) {
    if (n < 0 || !params || !grad || !momentum_buf || !workspace || ((uintptr_t)grad & 15)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (max_norm > 0.f) launch_sumsq_partial(st, n, grad, workspace);
    hipLaunchKernelGGL(sgd_momentum_clip_kernel, dim3(parc_capped_blocks((size_t)n, 8192)), dim3(256), 0, st, (size_t)n, params, grad, momentum_buf,
                       workspace, max_norm, lr, momentum, weight_decay, norm_out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// The same two passes for `optimizer.type: Adam` (MPOptimizer -> torch.optim.AdamW, learning/mp_optimizer.py:51-62): pass 1 is
// sumsq_partial_kernel above, pass 2 folds the partials like the SGD step and then runs torch's single-tensor AdamW on its elements,
// operation for operation and in torch's order (each line below is one rounded fp32 operation of _single_tensor_adamw; contraction is
// off so that the compiler fuses nothing else):
//   g' = coef g;  p *= 1 - lr wd;  m = fma(1 - b1, g' - m, m) [lerp_];  v = fma((1 - b2) g', g', b2 v) [mul_, addcmul_];
//   p += ((-lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps) [addcdiv_]
// 28 B per element of plain 16-byte loads and stores, no cache-policy bits: the parameters are read again by the next minibatch's
// GEMMs and all four buffers (170 MB at the model's size) by the next step, which the 256 MB last-level cache can serve; a
// non-temporal variant was not measured.  One resident round of workgroups (8 x 256 threads per CU), grid-stride.
// =============================================================================================
struct adamw_consts_t {
    float decay, w1, beta2, w2, neg_step, bc2_sqrt, eps;
};

__device__ __forceinline__ void adamw_element(float &p, float g, float &m, float &v, float coef, const adamw_consts_t &c) {
#pragma clang fp contract(off)
    g = coef * g;
    const float pd = p * c.decay;
    m = fmaf(c.w1, g - m, m);
    v = fmaf(c.w2 * g, g, v * c.beta2);
    const float den = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = pd + (c.neg_step * m) / den;
}

__global__ __launch_bounds__(256) void adamw_clip_kernel(size_t n, size_t n4, float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                                                         float *__restrict__ v, const float *__restrict__ partial, float max_norm, adamw_consts_t c,
                                                         float *norm_out) {
    const float coef = clip_coef_of_partials(partial, max_norm, norm_out);
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4 *p4 = (float4 *)p, *m4 = (float4 *)m, *v4 = (float4 *)v;       // n4 > 0 only when all four buffers are 16-byte aligned
    const float4 *g4 = (const float4 *)g;
    for (size_t i = tid; i < n4; i += stride) {
        float4 pi = p4[i], mi = m4[i], vi = v4[i];
        const float4 gi = g4[i];
        adamw_element(pi.x, gi.x, mi.x, vi.x, coef, c);
        adamw_element(pi.y, gi.y, mi.y, vi.y, coef, c);
        adamw_element(pi.z, gi.z, mi.z, vi.z, coef, c);
        adamw_element(pi.w, gi.w, mi.w, vi.w, coef, c);
        p4[i] = pi; m4[i] = mi; v4[i] = vi;
    }
    for (size_t i = 4 * n4 + tid; i < n; i += stride) {       // the tail of the vector path, or every element when a buffer is misaligned
        float pi = p[i], mi = m[i], vi = v[i];
        adamw_element(pi, g[i], mi, vi, coef, c);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}

// A float hyper-parameter as the double its shortest decimal form names (0.999f -> 0.999, not 0.99900001287...): the settings are
// decimal literals that torch keeps as Python doubles, and 1 - beta2 taken from the widened float would be off by 1.3e-5 relative.
static double decimal_double(float x) {
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof buf, "%.*g", digits, (double)x);
        if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
    }
    return (double)x;
}

#define ADAMW_MAX_BLOCKS 2048
extern "C" int parc_adamw_step(void *stream, int64_t n, float *params, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t step,
                               float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, float *workspace, float *norm_out) {
    if (n < 0 || step < 1 || !params || !grad || !exp_avg || !exp_avg_sq || !workspace || ((uintptr_t)grad & 15)) return PARC_EINVAL;
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f)) return PARC_EINVAL;
    if (n == 0) return PARC_OK;
    static thread_local float key[5] = {-1.f, -1.f, -1.f, -1.f, -1.f};      // the settings do not change between steps: convert them once
    static thread_local double val[5];
    const float in[5] = {lr, beta1, beta2, eps, weight_decay};
    for (int k = 0; k < 5; ++k)
        if (!(in[k] == key[k])) { val[k] = decimal_double(in[k]); key[k] = in[k]; }
    const double lr_d = val[0], b1 = val[1], b2 = val[2];
    adamw_consts_t c;
    c.decay = (float)(1.0 - lr_d * val[4]);
    c.w1 = (float)(1.0 - b1);
    c.beta2 = (float)b2;
    c.w2 = (float)(1.0 - b2);
    c.neg_step = (float)(-(lr_d / (1.0 - pow(b1, (double)step))));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(b2, (double)step));
    c.eps = (float)val[3];
    hipStream_t st = (hipStream_t)stream;
    if (max_norm > 0.f) launch_sumsq_partial(st, n, grad, workspace);
    const bool vec = !(((uintptr_t)params | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15);
    const size_t n4 = vec ? (size_t)n / 4 : 0, work = vec ? n4 + 3 : (size_t)n;
    hipLaunchKernelGGL(adamw_clip_kernel, dim3(parc_capped_blocks(work, ADAMW_MAX_BLOCKS)), dim3(256), 0, st, (size_t)n, n4, params, grad, exp_avg,
                       exp_avg_sq, workspace, max_norm, c, norm_out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}
