// The learner's returns: TD(lambda) and the advantage normalisation of the PPO update.  C-ABI in include/parc_hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"

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
