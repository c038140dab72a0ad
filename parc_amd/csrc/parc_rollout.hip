// What a rollout step runs beside the simulator and the networks (gfx950): the experience record, the step's random numbers, the
// episodic return tracker and the action head of the policy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/parc_hip.h"
#include "parc_launch.h"
#include "parc_learner_math.h"

// =============================================================================================
// K15 experience record: ExperienceBuffer.record (learning/experience_buffer.py:55-59) for a whole group of named buffers in one
// launch: field f copies its [N, row] source into row `*head` of its time-major [T, N, row] buffer.  head is a DEVICE scalar
// so the launch can sit inside the captured rollout graph.
// =============================================================================================
#define PARC_RECORD_MAX_FIELDS 12
struct record_fields_t {
    parc_record_field_t f[PARC_RECORD_MAX_FIELDS];
};

__global__ __launch_bounds__(256) void record_step_kernel(int n_envs, const int64_t *__restrict__ head, record_fields_t fields) {
    const parc_record_field_t f = fields.f[blockIdx.y];
    const size_t total = (size_t)n_envs * (size_t)f.row_bytes;            // bytes of one time row
    const size_t h = (size_t)head[0];
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (size_t)gridDim.x * blockDim.x;
    if (f.convert == 1) {                                                 // int64 source -> int32 buffer (ep_num)
        const int64_t *s = (const int64_t *)f.src;
        int32_t *d = (int32_t *)f.dst + h * (total / 8);
        for (size_t i = tid; i < total / 8; i += nthr) d[i] = (int32_t)s[i];
        return;
    }
    if (f.convert == 2) {                                                 // one 4-byte value for every env (the plan clock: replan_timer)
        const uint32_t v = *(const uint32_t *)f.src;
        uint32_t *d = (uint32_t *)f.dst + h * (total / 4);
        for (size_t i = tid; i < total / 4; i += nthr) d[i] = v;
        return;
    }
    char *d = (char *)f.dst + h * total;
    const char *s = (const char *)f.src;
    if (((total | (uintptr_t)d | (uintptr_t)s) & 15) == 0) {
        // (the buffer row is not read again before the update phase: streamed stores)
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        for (size_t i = tid; i < total / 16; i += nthr) __builtin_nontemporal_store(((const u32x4 *)s)[i], (u32x4 *)d + i);
    } else {
        for (size_t i = tid; i < total / 4; i += nthr) ((uint32_t *)d)[i] = ((const uint32_t *)s)[i];
    }
}

extern "C" int parc_record_step(void *stream, int n_envs, const int64_t *head, int n_fields, const parc_record_field_t *fields) {
    if (n_envs <= 0 || n_fields <= 0 || n_fields > PARC_RECORD_MAX_FIELDS || !head || !fields) return PARC_EINVAL;
    record_fields_t args;
    int max_row = 0;
    for (int i = 0; i < n_fields; ++i) {
        args.f[i] = fields[i];
        if (fields[i].row_bytes <= 0 || (fields[i].row_bytes & 3) || !fields[i].src || !fields[i].dst) return PARC_EINVAL;
        if (fields[i].row_bytes > max_row) max_row = fields[i].row_bytes;
    }
    for (int i = n_fields; i < PARC_RECORD_MAX_FIELDS; ++i) args.f[i] = fields[0];
    size_t units = ((size_t)n_envs * (size_t)max_row + 15) / 16;
    const unsigned gx = parc_capped_blocks(units, 2048);                 // grid-stride beyond that
    hipLaunchKernelGGL(record_step_kernel, dim3(gx, (unsigned)n_fields), dim3(256), 0, (hipStream_t)stream, n_envs, head, args);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// The random numbers of one rollout step in ONE launch: Philox4x32-10 (Salmon et al. 2011; the generator torch's device RNG is built
// on), keyed by the seed, counter = (thread, 0, step counter lo, hi).  n_uniform floats in [0, 1) (24 random bits, like torch's
// uniform_) - the env's pool: xy-target resample, restart sampling - and n_normal floats ~ N(0, 1) (Box-Muller on pairs) - the
// policy's action noise.  state[0] = step counter, advanced by the launch's last workgroup; state[1] = its ticket (zero between launches).
// Replaces two torch generator launches per step, which inside a replayed hipGraph also cost two fills of the generator's
// seed / offset cells per replay.  Being the FIRST launch of a rollout step it can also carry the step's tick: tick_cell (optional) <-
// (tick_cell + 1) % tick_mod by the launch's last workgroup - ExperienceBuffer.inc (experience_buffer.py:41-44) for a write row that lives
// on the device.  (157 workgroups take the ticket here; taking it in the record launch - 14 000 workgroups on one atomic - cost 200 us.)
// =============================================================================================
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ __launch_bounds__(256) void rng_step_kernel(uint64_t seed, uint64_t *state, float *__restrict__ uniform_out, int64_t n_uniform,
                                                       float *__restrict__ normal_out, int64_t n_normal, int64_t *tick_cell, int tick_mod) {
    const uint64_t step = state[0];
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // one Philox block = 4 outputs
    const int64_t qu = (n_uniform + 3) / 4, qn = (n_normal + 3) / 4;
    if (q < qu + qn) {
        uint32_t r[4];
        philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
        if (q < qu) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < n_uniform) uniform_out[4 * q + k] = (float)(r[k] >> 8) * (1.0f / 16777216.0f);
        } else {
            const int64_t b = 4 * (q - qu);
            float z[4];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float u1 = ((float)(r[2 * k] >> 8) + 1.0f) * (1.0f / 16777216.0f);       // (0, 1]
                const float u2 = (float)(r[2 * k + 1] >> 8) * (1.0f / 16777216.0f);
                const float rad = sqrtf(-2.0f * __logf(u1));
                float sn, cs;
                __sincosf(6.283185307179586f * u2, &sn, &cs);
                z[2 * k] = rad * cs;
                z[2 * k + 1] = rad * sn;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (b + k < n_normal) normal_out[b + k] = z[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(state + 1);
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1ull) {
            state[0] = step + 1;
            *ticket = 0ull;
            if (tick_cell) tick_cell[0] = (tick_cell[0] + 1) % (int64_t)tick_mod;      // nothing of this launch reads it
        }
    }
}

extern "C" int parc_rng_step(void *stream, uint64_t seed, uint64_t *state, float *uniform_out, int64_t n_uniform, float *normal_out,
                             int64_t n_normal, int64_t *tick_cell, int tick_mod) {
    if (!state || n_uniform < 0 || n_normal < 0 || (n_uniform > 0 && !uniform_out) || (n_normal > 0 && !normal_out) || (tick_cell && tick_mod < 1))
        return PARC_EINVAL;
    const int64_t quads = (n_uniform + 3) / 4 + (n_normal + 3) / 4;
    if (quads == 0 && !tick_cell) return PARC_OK;
    hipLaunchKernelGGL(rng_step_kernel, dim3((unsigned)((quads + 255) / 256 > 0 ? (quads + 255) / 256 : 1)), dim3(256), 0, (hipStream_t)stream, seed,
                       state, uniform_out, n_uniform, normal_out, n_normal, tick_cell, tick_mod);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K21 episodic return tracker: DMPPOReturnTracker.update (learning/dm_ppo_return_tracker.py:6-99) in one launch.
// Accumulate the K reward terms and the episode length per env, fold the envs that finished into the running means (weights by
// episode count, as the reference), clear them.  Reductions in a fixed order (deterministic).
// =============================================================================================
#define TRK_THREADS 256
#define TRK_MAX_K 12
#define TRK_SLOTS (TRK_MAX_K + 2)          // K term sums | summed episode length | finished count

__device__ __forceinline__ float lerp_torch(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w); }

// Two launches: (1) one env per thread, ceil(N / 256) workgroups, each parks the sums of its finished envs in the workspace (folded in a
// fixed order: wave shuffle, then the four wave rows); (2) one small workgroup adds the workgroups' rows in workgroup order and updates
// the running means.  The result does not depend on scheduling.  (Round 1-3: one launch, the last workgroup to take a ticket did step
// 2 - the device-scope fences of that hand-over made it 13.6 us; one workgroup of 1024 threads over all envs - round 4, tried - 20-23 us:
// 180 KB through one CU.)
__global__ __launch_bounds__(TRK_THREADS) void return_tracker_kernel(int n_envs, int K, const float *__restrict__ rewards, int64_t reward_stride,
                                                                     const int32_t *__restrict__ done, float *return_buf, int64_t *ep_len,
                                                                     int64_t *eps_per_env, float *__restrict__ part) {
    __shared__ float s_part[TRK_THREADS / 64][TRK_SLOTS];
    const int tid = threadIdx.x;
    const int e = blockIdx.x * TRK_THREADS + tid;
    float acc[TRK_SLOTS];
#pragma unroll
    for (int k = 0; k < TRK_SLOTS; ++k) acc[k] = 0.f;
    if (e < n_envs) {
        const bool fin = done[e] != 0;
        const int64_t len = ep_len[e] + 1;
        if (fin) {
            acc[TRK_MAX_K] = (float)len;
            acc[TRK_MAX_K + 1] = 1.0f;
            eps_per_env[e] += 1;
        }
        ep_len[e] = fin ? 0 : len;
#pragma unroll
        for (int k = 0; k < TRK_MAX_K; ++k) {
            if (k < K) {
                const float v = return_buf[(size_t)k * n_envs + e] + rewards[(size_t)k * reward_stride + e];
                if (fin) acc[k] = v;
                return_buf[(size_t)k * n_envs + e] = fin ? 0.f : v;
            }
        }
    }
    const int wv = tid >> 6, ln = tid & 63;
#pragma unroll
    for (int k = 0; k < TRK_SLOTS; ++k) {
        const float v = wave_sum(acc[k]);
        if (ln == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (tid < TRK_SLOTS) {
        float v = 0.f;
        for (int w = 0; w < TRK_THREADS / 64; ++w) v += s_part[w][tid];
        part[(size_t)blockIdx.x * TRK_SLOTS + tid] = v;
    }
}

__global__ __launch_bounds__(64) void return_tracker_fold_kernel(int groups, int K, const float *__restrict__ part, float *mean_return,
                                                                 float *mean_ep_len, double *episodes) {
    __shared__ float s_tot[TRK_SLOTS];
    const int tid = threadIdx.x;
    if (tid < TRK_SLOTS) {
        float v = 0.f;
        for (int g = 0; g < groups; ++g) v += part[(size_t)g * TRK_SLOTS + tid];
        s_tot[tid] = v;
    }
    __syncthreads();
    // DMPPOReturnTracker.update's running means (dm_ppo_return_tracker.py:60-99): weights by episode count
    const float n_new = s_tot[TRK_MAX_K + 1];
    if (n_new > 0.f) {
        const double new_count = episodes[0] + (double)n_new;
        const float w_new = (float)((double)n_new / (new_count < 1.0 ? 1.0 : new_count));
        if (tid < K) mean_return[tid] = lerp_torch(mean_return[tid], s_tot[tid] / n_new, w_new);
        if (tid == K) mean_ep_len[0] = lerp_torch(mean_ep_len[0], s_tot[TRK_MAX_K] / n_new, w_new);
        __syncthreads();
        if (tid == 0) episodes[0] = new_count;
    }
}

extern "C" int64_t parc_return_tracker_workspace_floats(int n_envs) {
    if (n_envs <= 0) return -1;
    return (int64_t)((n_envs + TRK_THREADS - 1) / TRK_THREADS) * TRK_SLOTS + 4;
}

extern "C" int parc_return_tracker_update(void *stream, int n_envs, int K, const float *rewards, int64_t reward_stride, const int32_t *done,
                                          float *return_buf, int64_t *ep_len, int64_t *eps_per_env, float *mean_return, float *mean_ep_len,
                                          double *episodes, float *workspace) {
    if (n_envs <= 0 || K <= 0 || K > TRK_MAX_K || reward_stride < n_envs || !workspace) return PARC_EINVAL;
    const int groups = (n_envs + TRK_THREADS - 1) / TRK_THREADS;
    hipLaunchKernelGGL(return_tracker_kernel, dim3(groups), dim3(TRK_THREADS), 0, (hipStream_t)stream, n_envs, K, rewards, reward_stride, done,
                       return_buf, ep_len, eps_per_env, workspace);
    hipLaunchKernelGGL(return_tracker_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, groups, K, workspace, mean_return, mean_ep_len, episodes);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// =============================================================================================
// K14 action head of the rollout: PPOAgent._decide_action (learning/ppo_agent.py:87-119) after the actor MLP.
// norm_a = mean + std * noise where the env explores (mask 1), the mode otherwise; a_logp = log N(norm_a; mean, std);
// action = a_mean + a_std * norm_a (Normalizer.unnormalize).  One thread per env.
// =============================================================================================
__global__ __launch_bounds__(256) void action_head_kernel(int n, int A, const float *__restrict__ mean, const float *__restrict__ logstd,
                                                          const float *__restrict__ noise, const float *__restrict__ explore,
                                                          const float *__restrict__ a_mean, const float *__restrict__ a_std, float *action,
                                                          float *logp) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool ex = explore[i] == 1.0f;
    float acc = 0.f, sum_ls = 0.f;
    for (int j = 0; j < A; ++j) {
        const float ls = logstd[j], sd = __expf(ls);
        const float mu = mean[(size_t)i * A + j];
        const float na = ex ? mu + sd * noise[(size_t)i * A + j] : mu;
        const float z = (na - mu) / sd;
        acc = fmaf(z, z, acc);
        sum_ls += ls;
        action[(size_t)i * A + j] = na * a_std[j] + a_mean[j];
    }
    logp[i] = -0.5f * acc + (-0.5f * (float)A * 1.8378770664093453f - sum_ls);
}

// A <= 32 (the humanoid has 28 actuated dofs): 32 lanes per env, lane j = action dimension j - coalesced reads of the [n, A] rows and
// 512 workgroups at 4096 envs instead of 16; the two sums over j are 5-step xor-shuffle reductions inside the 32-lane group.
// (rec.head != NULL: the same launch also writes what ExperienceBuffer.record stores of this moment - action, a_logp,
// rand_action_mask and the contact forces the env holds before the step - into time row *head of their [T, n, ...] buffers:
// base_agent's _record_data_pre_step (ppo_agent.py:121-125, dm_ppo_agent.py:289-299) without a launch of its own)
struct action_record_t {
    float *action, *logp, *mask, *forces;      // [T, n, A] [T, n] [T, n] [T, n, n_forces]
    const float *forces_src;                    // [n, n_forces]
    int n_forces;
    const int64_t *head;
};

__global__ __launch_bounds__(256) void action_head32_kernel(int n, int A, const float *__restrict__ mean, const float *__restrict__ logstd,
                                                            const float *__restrict__ noise, const float *__restrict__ explore,
                                                            const float *__restrict__ a_mean, const float *__restrict__ a_std, float *action,
                                                            float *logp, action_record_t rec) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = min(gid >> 5, n - 1), j = gid & 31;           // (tail groups redo the last env; they skip the stores)
    const bool live = (gid >> 5) < n, valid = j < A;
    float zz = 0.f, ls = 0.f;
    if (valid) {
        ls = logstd[j];
        const float sd = __expf(ls);
        const float mu = mean[(size_t)i * A + j];
        const float na = explore[i] == 1.0f ? mu + sd * noise[(size_t)i * A + j] : mu;
        const float z = (na - mu) / sd;
        zz = z * z;
        if (live) {
            const float a = na * a_std[j] + a_mean[j];
            action[(size_t)i * A + j] = a;
            if (rec.head) rec.action[((size_t)rec.head[0] * n + i) * A + j] = a;
        }
    }
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) {
        zz += __shfl_xor(zz, o, 32);
        ls += __shfl_xor(ls, o, 32);
    }
    if (live && j == 0) {
        const float lp = -0.5f * zz + (-0.5f * (float)A * 1.8378770664093453f - ls);
        logp[i] = lp;
        if (rec.head) {
            const size_t row = (size_t)rec.head[0] * n + i;
            rec.logp[row] = lp;
            rec.mask[row] = explore[i];
        }
    }
    if (live && rec.head)
        for (int k = j; k < rec.n_forces; k += 32) rec.forces[((size_t)rec.head[0] * n + i) * rec.n_forces + k] = rec.forces_src[(size_t)i * rec.n_forces + k];
}

// the one launch of action_head32_kernel (A <= 32); an empty rec records nothing
static int launch_action_head32(void *stream, int n, int A, const float *mean, const float *logstd, const float *noise, const float *explore,
                                const float *a_mean, const float *a_std, float *action, float *logp, action_record_t rec) {
    const long long threads = (long long)n * 32;
    hipLaunchKernelGGL(action_head32_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, A, mean, logstd, noise, explore,
                       a_mean, a_std, action, logp, rec);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_action_head(void *stream, int n, int A, const float *mean, const float *logstd, const float *noise, const float *explore,
                                const float *a_mean, const float *a_std, float *action, float *logp) {
    if (n <= 0 || A <= 0) return PARC_EINVAL;
    if (A <= 32) return launch_action_head32(stream, n, A, mean, logstd, noise, explore, a_mean, a_std, action, logp, action_record_t{});
    hipLaunchKernelGGL(action_head_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, A, mean, logstd, noise, explore, a_mean,
                       a_std, action, logp);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_action_head_record(void *stream, int n, int A, const float *mean, const float *logstd, const float *noise, const float *explore,
                                       const float *a_mean, const float *a_std, float *action, float *logp, float *rec_action, float *rec_logp,
                                       float *rec_mask, const float *forces_src, float *rec_forces, int n_forces, const int64_t *head) {
    if (n <= 0 || A <= 0 || !rec_action || !rec_logp || !rec_mask || !forces_src || !rec_forces || n_forces < 0 || !head) return PARC_EINVAL;
    if (A > 32) return PARC_EUNSUPPORTED;
    const action_record_t rec = {rec_action, rec_logp, rec_mask, rec_forces, forces_src, n_forces, head};
    return launch_action_head32(stream, n, A, mean, logstd, noise, explore, a_mean, a_std, action, logp, rec);
}
