// PPO surrogate + critic loss of the tracker agent with its gradient in one pass (gfx950).
// Restates PPOAgent._compute_loss / DMPPOAgent (learning/ppo_agent.py:186-330, learning/dm_ppo_agent.py) for a diagonal
// Gaussian policy with state-independent log-std: the ~120 small elementwise / reduction launches of the autograd
// graph between the two MLP outputs and the scalar loss become three launches with a deterministic reduction order.
#include <hip/hip_runtime.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_learner_math.h"

#define PPO_THREADS 256
#define PPO_MAX_A 64
#define PPO_NSCAL 8      // cnt_raw, critic_sum, surr_sum, clip_sum, ratio_sum, viol_sum, reg_sum, (spare)
#define PPO_W (PPO_NSCAL + PPO_MAX_A)

// The per-sample chain logp -> ratio -> clamp -> minimum -> c and the critic's gradient, one copy for both sample kernels.
// The reference SELECTS the random-action rows before it evaluates them (ppo_agent.py:286-290): a row with mask != 1 (sel false, m = 0)
// adds exactly 0 to every sum and gets a zero g_mean row whatever it holds (sel ? x : 0 - a product with m = 0 would turn its NaN / Inf
// into NaN), and a NaN in a selected row reaches actor_loss as it does through torch.clamp and torch.minimum.
struct ppo_surr_t {
    float ratio, surr, c;       // importance ratio, clipped surrogate, c = d(-sum m surr) / d logp_i (x 1/cnt later)
};

// of sample si, from zz = sum_j z_j^2 over its action dimensions (old_logp[si] and adv[si] are read in here, between the arithmetic
// that needs them: read at the call they move ahead of it, and the kernels' instruction order with them)
__device__ __forceinline__ ppo_surr_t ppo_surrogate(int A, float zz, float sum_logstd, const float *old_logp, const float *adv, size_t si, bool sel,
                                                    float m, parc_ppo_cfg_t cfg) {
    ppo_surr_t s;
    const float logp = -0.5f * zz + (-0.5f * (float)A * 1.8378770664093453f - sum_logstd);     // log(2 pi)
    s.ratio = __expf(logp - old_logp[si]);
    const float ad = adv[si];
    const float lo = 1.0f - cfg.clip_ratio, hi = 1.0f + cfg.clip_ratio;
    const float rc = clamp_nan(s.ratio, lo, hi);
    const float l0 = ad * s.ratio, l1 = ad * rc;
    s.surr = minimum_nan(l0, l1);
    // d surr / d ratio: torch.minimum sends the gradient to l0 when l0 <= l1, else to l1, whose clamp passes it inside [lo, hi]
    const float dsurr = (l0 <= l1) ? ad : ((s.ratio >= lo && s.ratio <= hi) ? ad : 0.f);
    s.c = sel ? -m * dsurr * s.ratio : 0.f;
    return s;
}

// unscaled d critic_loss / d pred of one sample (diff = tar_val - pred): L1 or L2
__device__ __forceinline__ float ppo_critic_grad(parc_ppo_cfg_t cfg, float diff) {
    return cfg.critic_l1 ? (diff > 0.f ? -1.f : (diff < 0.f ? 1.f : 0.f)) : -2.0f * diff;
}

// pass 1: one thread per sample.  Unscaled gradients (the 1/cnt and gate factors are only known after the reduction).
__global__ __launch_bounds__(PPO_THREADS) void ppo_sample_kernel(int B, int A, const float *__restrict__ mean, const float *__restrict__ logstd,
                                                                 const float *__restrict__ norm_a, const float *__restrict__ old_logp,
                                                                 const float *__restrict__ adv, const float *__restrict__ mask,
                                                                 const float *__restrict__ pred, const float *__restrict__ tar_val,
                                                                 parc_ppo_cfg_t cfg, float *g_mean, float *g_pred, float *ws, int a_stride,
                                                                 int s_stride) {
    __shared__ float s_istd[PPO_MAX_A];
    __shared__ float s_part[PPO_THREADS / 64][PPO_W];
    const int tid = threadIdx.x, i = blockIdx.x * PPO_THREADS + tid;
    float sum_logstd = 0.f;
    if (tid < A) s_istd[tid] = __expf(-logstd[tid]);       // std^-1 = exp(-logstd)
    __syncthreads();
    for (int j = 0; j < A; ++j) sum_logstd += logstd[j];
    const bool live = i < B;
    const int ii = live ? i : 0;
    // (a_stride / s_stride: row stride of norm_a and element stride of the four per-sample scalars; A and 1 for separate dense arrays,
    //  the record width for the packed layout of parc_ppo_loss_packed)
    const size_t si = (size_t)ii * s_stride;
    const bool sel = live && mask[si] == 1.0f;
    const float m = sel ? 1.f : 0.f;
    const float *mu = mean + (size_t)ii * A, *ac = norm_a + (size_t)ii * a_stride;
    float zz = 0.f, viol = 0.f, reg = 0.f;
    for (int j = 0; j < A; ++j) {
        float mj = mu[j];
        float z = (ac[j] - mj) * s_istd[j];
        zz = fmaf(z, z, zz);
        float vmin = clamp_max_nan(mj + 1.0f, 0.f), vmax = clamp_min_nan(mj - 1.0f, 0.f);
        viol += vmin * vmin + vmax * vmax;
        reg = fmaf(mj, mj, reg);
    }
    const ppo_surr_t sr = ppo_surrogate(A, zz, sum_logstd, old_logp, adv, si, sel, m, cfg);
    const float c = sr.c;
    const float diff = tar_val[si] - pred[ii];
    if (live) {
        g_pred[i] = ppo_critic_grad(cfg, diff);
        float *gm = g_mean + (size_t)i * A;
        for (int j = 0; j < A; ++j) {
            float mj = mu[j];
            float z = (ac[j] - mj) * s_istd[j];
            float vmin = clamp_max_nan(mj + 1.0f, 0.f), vmax = clamp_min_nan(mj - 1.0f, 0.f);
            gm[j] = sel ? c * z * s_istd[j] + m * (cfg.bound_w * 2.0f * (vmin + vmax) + cfg.reg_w * 2.0f * mj) : 0.f;
        }
    }
    // block partials, fixed order: lanes -> waves -> block.  (These seven addends are written out here and, accumulated, in
    // ppo_sample32_kernel: filled in by a shared helper the array is kept in other registers and both kernels come out different.)
    float sc[PPO_NSCAL];
    sc[0] = m;
    sc[1] = live ? (cfg.critic_l1 ? fabsf(diff) : diff * diff) : 0.f;
    sc[2] = sel ? m * sr.surr : 0.f;
    sc[3] = m * (fabsf(sr.ratio - 1.0f) > cfg.clip_ratio ? 1.f : 0.f);      // (a NaN ratio counts as unclipped, as in torch)
    sc[4] = sel ? m * sr.ratio : 0.f;
    sc[5] = sel ? m * viol : 0.f;
    sc[6] = sel ? m * reg : 0.f;
    sc[7] = 0.f;
    const int wv = tid >> 6, ln = tid & 63;
#pragma unroll
    for (int k = 0; k < PPO_NSCAL; ++k) {
        float v = wave_sum(sc[k]);
        if (ln == 0) s_part[wv][k] = v;
    }
    for (int j = 0; j < A; ++j) {
        float z = live ? (ac[j] - mu[j]) * s_istd[j] : 0.f;
        float v = wave_sum(sel ? c * (z * z - 1.0f) : 0.f);   // d logp / d logstd_j = z^2 - 1
        if (ln == 0) s_part[wv][PPO_NSCAL + j] = v;
    }
    __syncthreads();
    if (tid < PPO_NSCAL + A) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < PPO_THREADS / 64; ++w) v += s_part[w][tid];
        ws[(size_t)blockIdx.x * PPO_W + tid] = v;
    }
}

// pass 1 for A <= 32 (the humanoid has 28 actuated dofs): 32 lanes per sample, lane j = action dimension j, so the [B, A] rows of mean /
// action / gradient are read and written coalesced (one thread per sample walks them with a 112-byte stride between lanes: 22 us for
// 16384 samples).  A block takes 64 samples in 8 passes; the per-sample scalars accumulate on lane 0 of each group and the log-std
// gradient of dimension j on lane j, folded over the 8 groups through LDS at the end (fixed order).
#define PPO32_SPB 64
__global__ __launch_bounds__(256) void ppo_sample32_kernel(int B, int A, const float *__restrict__ mean, const float *__restrict__ logstd,
                                                           const float *__restrict__ norm_a, const float *__restrict__ old_logp,
                                                           const float *__restrict__ adv, const float *__restrict__ mask,
                                                           const float *__restrict__ pred, const float *__restrict__ tar_val, parc_ppo_cfg_t cfg,
                                                           float *g_mean, float *g_pred, float *ws, int a_stride, int s_stride) {
    __shared__ float s_part[8][PPO_W];
    const int tid = threadIdx.x, g = tid >> 5, j = tid & 31;
    const bool vj = j < A;
    const float ls = vj ? logstd[j] : 0.f;
    const float istd = __expf(-ls);
    float sum_logstd = ls;
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) sum_logstd += __shfl_xor(sum_logstd, o, 32);
    float acc[PPO_NSCAL];
#pragma unroll
    for (int k = 0; k < PPO_NSCAL; ++k) acc[k] = 0.f;
    float acc_ls = 0.f;
#pragma unroll 2
    for (int it = 0; it < PPO32_SPB / 8; ++it) {
        const int i = blockIdx.x * PPO32_SPB + it * 8 + g;
        const bool live = i < B;
        const int ii = live ? i : 0;
        const size_t si = (size_t)ii * s_stride;
        const bool sel = live && mask[si] == 1.0f;
        const float m = sel ? 1.f : 0.f;
        const float mj = vj ? mean[(size_t)ii * A + j] : 0.f;
        const float aj = vj ? norm_a[(size_t)ii * a_stride + j] : 0.f;
        const float z = (aj - mj) * istd;
        const float vmin = clamp_max_nan(mj + 1.0f, 0.f), vmax = clamp_min_nan(mj - 1.0f, 0.f);
        float zz = vj ? z * z : 0.f, viol = vj ? vmin * vmin + vmax * vmax : 0.f, reg = vj ? mj * mj : 0.f;
#pragma unroll
        for (int o = 16; o >= 1; o >>= 1) {
            zz += __shfl_xor(zz, o, 32);
            viol += __shfl_xor(viol, o, 32);
            reg += __shfl_xor(reg, o, 32);
        }
        const ppo_surr_t sr = ppo_surrogate(A, zz, sum_logstd, old_logp, adv, si, sel, m, cfg);
        const float c = sr.c;
        const float diff = tar_val[si] - pred[ii];
        if (live) {
            if (j == 0) g_pred[i] = ppo_critic_grad(cfg, diff);
            if (vj) g_mean[(size_t)i * A + j] = sel ? c * z * istd + m * (cfg.bound_w * 2.0f * (vmin + vmax) + cfg.reg_w * 2.0f * mj) : 0.f;
        }
        // (every lane of the group holds the same scalars; lane 0's copy is the one that is kept)
        acc[0] += m;
        acc[1] += live ? (cfg.critic_l1 ? fabsf(diff) : diff * diff) : 0.f;
        acc[2] += sel ? m * sr.surr : 0.f;
        acc[3] += m * (fabsf(sr.ratio - 1.0f) > cfg.clip_ratio ? 1.f : 0.f);
        acc[4] += sel ? m * sr.ratio : 0.f;
        acc[5] += sel ? m * viol : 0.f;
        acc[6] += sel ? m * reg : 0.f;
        acc_ls += (sel && vj) ? c * (z * z - 1.0f) : 0.f;
    }
    if (j == 0) {
#pragma unroll
        for (int k = 0; k < PPO_NSCAL; ++k) s_part[g][k] = acc[k];
    }
    if (vj) s_part[g][PPO_NSCAL + j] = acc_ls;
    __syncthreads();
    if (tid < PPO_NSCAL + A) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) v += s_part[w][tid];
        ws[(size_t)blockIdx.x * PPO_W + tid] = v;
    }
}

// pass 2: one small block reduces the block partials in order and produces the scalars, the log-std gradient and the scale factors
#define PPO_RED_THREADS (4 * PPO_W)
__global__ __launch_bounds__(PPO_RED_THREADS) void ppo_reduce_kernel(int B, int A, int nblk, const float *__restrict__ logstd, parc_ppo_cfg_t cfg,
                                                                    const float *__restrict__ ws, float *g_logstd, float *out) {
    __shared__ float s[PPO_W];
    __shared__ double s4[PPO_W][4];
    const int tid = threadIdx.x;
    {
        // value v of the block partials: four threads add a quarter of the blocks each, in block order, their sums are then added in
        // quarter order (fixed summation order, deterministic); unrolled so that 16 loads are in flight instead of one dependent load
        // per step (that loop was most of the kernel's 26 us)
        const int v = tid >> 2, part = tid & 3;
        const int per = (nblk + 3) >> 2, b0 = part * per, b1 = min(b0 + per, nblk);
        double acc = 0.0;
        if (v < PPO_NSCAL + A) {
#pragma unroll 16
            for (int b = b0; b < b1; ++b) acc += (double)ws[(size_t)b * PPO_W + v];
        }
        s4[v][part] = acc;
    }
    __syncthreads();
    if (tid < PPO_NSCAL + A) s[tid] = (float)((s4[tid][0] + s4[tid][1]) + (s4[tid][2] + s4[tid][3]));
    __syncthreads();
    const float msum = s[0];
    // no random-action sample in the batch: the reference takes means over an empty selection, which are NaN, and its NaN trap
    // then stops the run (ppo_agent.py:242-252).  Dividing by the raw count reproduces that (0/0) instead of hiding it.
    const float cnt = msum;
    const float critic_loss = s[1] / (float)B;
    float sum_logstd = 0.f;
    for (int j = 0; j < A; ++j) sum_logstd += logstd[j];
    const float ent = (sum_logstd + 0.5f * (float)A * 2.8378770664093453f) * (msum / cnt);     // log(2 pi e)
    const float abl = s[5] / cnt, regl = s[6] / cnt;
    float actor_loss = -s[2] / cnt;
    if (cfg.bound_w != 0.f) actor_loss += cfg.bound_w * abl;
    if (cfg.entropy_w != 0.f) actor_loss -= cfg.entropy_w * ent;
    if (cfg.reg_w != 0.f) actor_loss += cfg.reg_w * regl;
    // "LARGE CRITIC LOSS" guard (ppo_agent.py:225-238): the actor term gives no gradient while the critic is off
    const float gate = critic_loss > cfg.large_critic_loss ? 0.f : 1.f;
    if (tid < A) g_logstd[tid] = gate * (s[PPO_NSCAL + tid] / cnt - cfg.entropy_w * (msum / cnt));
    if (tid == 0) {
        out[0] = actor_loss + cfg.critic_w * critic_loss;
        out[1] = critic_loss;
        out[2] = actor_loss;
        out[3] = s[3] / cnt;
        out[4] = s[4] / cnt;
        out[5] = abl;
        out[6] = ent;
        out[7] = regl;
        out[8] = cnt;
        out[9] = gate / cnt;                         // scale of g_mean
        out[10] = cfg.critic_w / (float)B;           // scale of g_pred
    }
}

// pass 3: apply the scale factors
__global__ __launch_bounds__(256) void ppo_scale_kernel(int n_mean, int n_pred, const float *__restrict__ out, float *g_mean, float *g_pred) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const float sa = out[9], sp = out[10];
    if (i < n_mean) g_mean[i] *= sa;
    if (i < n_pred) g_pred[i] *= sp;
}

static int ppo_loss_impl(void *stream, int B, int A, const float *mean, const float *logstd, const float *norm_a, const float *old_logp,
                         const float *adv, const float *mask, const float *pred, const float *tar_val, parc_ppo_cfg_t cfg, float *g_mean,
                         float *g_logstd, float *g_pred, float *out, float *workspace, int a_stride, int s_stride) {
    if (B <= 0 || A <= 0 || A > PPO_MAX_A) return PARC_EINVAL;
    int nblk = (B + PPO_THREADS - 1) / PPO_THREADS;
    hipStream_t st = (hipStream_t)stream;
    if (A <= 32) {
        nblk = (B + PPO32_SPB - 1) / PPO32_SPB;
        hipLaunchKernelGGL(ppo_sample32_kernel, dim3(nblk), dim3(256), 0, st, B, A, mean, logstd, norm_a, old_logp, adv, mask, pred, tar_val, cfg,
                           g_mean, g_pred, workspace, a_stride, s_stride);
    } else {
        hipLaunchKernelGGL(ppo_sample_kernel, dim3(nblk), dim3(PPO_THREADS), 0, st, B, A, mean, logstd, norm_a, old_logp, adv, mask, pred, tar_val,
                           cfg, g_mean, g_pred, workspace, a_stride, s_stride);
    }
    hipLaunchKernelGGL(ppo_reduce_kernel, dim3(1), dim3(PPO_RED_THREADS), 0, st, B, A, nblk, logstd, cfg, workspace, g_logstd, out);
    const int n = B * A;
    hipLaunchKernelGGL(ppo_scale_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, B, out, g_mean, g_pred);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_ppo_loss(void *stream, int B, int A, const float *mean, const float *logstd, const float *norm_a, const float *old_logp,
                             const float *adv, const float *mask, const float *pred, const float *tar_val, parc_ppo_cfg_t cfg, float *g_mean,
                             float *g_logstd, float *g_pred, float *out, float *workspace) {
    return ppo_loss_impl(stream, B, A, mean, logstd, norm_a, old_logp, adv, mask, pred, tar_val, cfg, g_mean, g_logstd, g_pred, out, workspace, A, 1);
}

// the same loss on PACKED per-sample records rec[B, rec_stride] = [norm_action (A) | a_logp | adv | rand_action_mask | tar_val | pad]:
// what one row gather of a minibatch delivers (the update phase gathers two arrays per minibatch instead of six)
extern "C" int parc_ppo_loss_packed(void *stream, int B, int A, const float *mean, const float *logstd, const float *rec, int rec_stride,
                                    const float *pred, parc_ppo_cfg_t cfg, float *g_mean, float *g_logstd, float *g_pred, float *out,
                                    float *workspace) {
    if (!rec || rec_stride < A + 4) return PARC_EINVAL;
    return ppo_loss_impl(stream, B, A, mean, logstd, rec, rec + A, rec + A + 1, rec + A + 2, pred, rec + A + 3, cfg, g_mean, g_logstd, g_pred, out,
                         workspace, rec_stride, rec_stride);
}

extern "C" int parc_ppo_workspace_floats(int B) { return ((B + PPO32_SPB - 1) / PPO32_SPB) * PPO_W; }      // (the finer of the two block sizes)
