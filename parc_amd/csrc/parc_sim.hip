// Device entry points of the articulated-body simulator.  The product kernels are the body-per-lane ones below (16 lanes per env, 4 envs
// per 64-thread workgroup, parc_sim_bpl.h); the one-env-per-lane reference formulation is a separate translation unit
// (parc_sim_ref.hip) that is compiled into the diagnostics library only (tools/parc_diag.py, parc_diag_sim_step_env_per_lane).
#include <hip/hip_runtime.h>

#include <mutex>

#include "parc_launch.h"
#include "parc_sim_bpl.h"
#include "parc_sim_core.h"
#include "../../include/parc_sim.h"

// What one launch of the step reads and writes; the kernels fill it from their parameters, the entry points from their arguments.
namespace {
struct StepArgs {
    const parc_sim_model_t *model;
    parc_terrain_t terrain;
    int n_envs;
    float *root_state, *dof_state, *rigid_body_state, *contact_forces;
    const float *env_offsets, *action, *act_lo, *act_hi;
    int n_sub;
    float h;
    int32_t *timestep;                      // the env's clock (both or neither): IGEnv._update_time rides in the launch
    float *time_buf;
    float step_dt;
    int hold;                               // substeps per hold (modes other than pd)
    float *dof_torque;                      // [N,D] torque of the last hold (torque / pd_exp / pd_1d), optional
    parc_sim_env_params_t *env_params;      // [N] per-env physics parameters (PHYS)
};
}  // namespace

// The body-per-lane step of one workgroup: 16 lanes per env, 4 envs per 64-thread workgroup (parc_sim_bpl.h).  MODE: PARC_SIM_CTL_*, in
// holds of `hold` substeps.  PHYS: the rows of the workgroup's four envs are staged in LDS next to the model (one 64-byte row per 16-lane
// group: lane b copies word b), where the sweeps read each value at its point of use; the push counter of a real env goes down by one
// per launch.
template <int MODE, bool PHYS>
__device__ __forceinline__ void step_workgroup(const StepArgs a) {
    using namespace parc_sim_bpl;
    __shared__ float lds[BPL_EPB][BPL_G * BPL_CONTRIB];
    __shared__ float ccache[64][BPL_CC_SLOTS * BPL_CC_FLOATS + 1];     // +1: odd row stride against bank conflicts
    const int g = threadIdx.x / BPL_G, b = threadIdx.x % BPL_G;
    const int e = min((int)blockIdx.x * BPL_EPB + g, a.n_envs - 1);    // tail groups recompute the last env (same values)
    // the model (4.9 KB of per-body / per-dof / per-sphere constants, read ~70 times per lane and substep) staged in LDS once per
    // workgroup: 100.9 -> 97.2 us per 4096-env step (profiles/r04_sim_step_variants.txt)
    __shared__ parc_sim_model_t s_model;
    // the envs' rows.  Only `if constexpr (PHYS)` code names s_ep, so without a table it is never emitted and takes no LDS: the 34552
    // bytes per block of the kernels without a table (34816 with one) depend on that - check both after touching this function
    __shared__ parc_sim_env_params_t s_ep[BPL_EPB];
    const parc_sim_env_params_t *ep = nullptr;
    {
        static_assert(sizeof(parc_sim_model_t) % 4 == 0, "copied as 32-bit words");
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.model);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&s_model);
        for (unsigned i = threadIdx.x; i < sizeof(parc_sim_model_t) / 4; i += 64) dst[i] = src[i];
        if constexpr (PHYS) {
            static_assert(sizeof(parc_sim_env_params_t) == 4 * BPL_G, "one word of the row per lane of the env's group");
            reinterpret_cast<uint32_t *>(&s_ep[g])[b] = reinterpret_cast<const uint32_t *>(a.env_params + e)[b];
            ep = &s_ep[g];
        }
        __syncthreads();
    }
    const parc_sim_model_t &m = s_model;
    const int B = m.num_bodies, D = m.dof_size;
    step_lane<MODE, PHYS>(m, a.terrain, b, a.root_state + 13 * (size_t)e, a.dof_state + 2 * (size_t)D * e,
                          a.rigid_body_state + 13 * (size_t)B * e, a.contact_forces + 3 * (size_t)B * e, a.env_offsets + 3 * (size_t)e,
                          a.action + (size_t)D * e, a.act_lo, a.act_hi, a.n_sub, a.h, lds[g], ccache[threadIdx.x], a.hold,
                          a.dof_torque ? a.dof_torque + (size_t)D * e : nullptr, ep);
    if (b == 0 && (int)blockIdx.x * BPL_EPB + g < a.n_envs) {
        if constexpr (PHYS) {
            const int left = ep->push_steps_left;
            if (left > 0) a.env_params[e].push_steps_left = left - 1;
        }
        // IGEnv._update_time (ig_env.py:862-865) for callers that ask for it: the env's step counter and clock advance with the simulator
        if (a.timestep) {
            const int ts = a.timestep[e] + 1;
            a.timestep[e] = ts;
            a.time_buf[e] = (float)ts * a.step_dt;
        }
    }
}

// pd control mode without a table: parc_sim_step / parc_sim_step_tick, and parc_sim_step_ctl with PARC_SIM_CTL_PD
__global__ __launch_bounds__(64) void sim_step_bpl_kernel(const parc_sim_model_t *__restrict__ model, parc_terrain_t ter, int n_envs,
                                                          float *root_state, float *dof_state, float *rigid_body_state,
                                                          float *contact_forces, const float *__restrict__ env_offsets,
                                                          const float *__restrict__ action, const float *__restrict__ act_lo,
                                                          const float *__restrict__ act_hi, int n_sub, float h, int32_t *timestep,
                                                          float *time_buf, float step_dt) {
    step_workgroup<PARC_SIM_CTL_PD, false>(StepArgs{model, ter, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets,
                                                    action, act_lo, act_hi, n_sub, h, timestep, time_buf, step_dt, 1, nullptr, nullptr});
}

// the other control modes without a table (parc_sim_step_ctl)
template <int MODE>
__global__ __launch_bounds__(64) void sim_step_bpl_ctl_kernel(const parc_sim_model_t *__restrict__ model, parc_terrain_t ter, int n_envs,
                                                              float *root_state, float *dof_state, float *rigid_body_state,
                                                              float *contact_forces, const float *__restrict__ env_offsets,
                                                              const float *__restrict__ action, const float *__restrict__ act_lo,
                                                              const float *__restrict__ act_hi, int n_sub, float h, int32_t *timestep,
                                                              float *time_buf, float step_dt, int hold, float *dof_torque) {
    step_workgroup<MODE, false>(StepArgs{model, ter, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action,
                                         act_lo, act_hi, n_sub, h, timestep, time_buf, step_dt, hold, dof_torque, nullptr});
}

// every control mode with per-env physics parameters (parc_sim_step_phys)
template <int MODE>
__global__ __launch_bounds__(64) void sim_step_bpl_phys_kernel(const parc_sim_model_t *__restrict__ model, parc_terrain_t ter, int n_envs,
                                                               float *root_state, float *dof_state, float *rigid_body_state,
                                                               float *contact_forces, const float *__restrict__ env_offsets,
                                                               const float *__restrict__ action, const float *__restrict__ act_lo,
                                                               const float *__restrict__ act_hi, int n_sub, float h, int32_t *timestep,
                                                               float *time_buf, float step_dt, int hold, float *dof_torque,
                                                               parc_sim_env_params_t *env_params) {
    step_workgroup<MODE, true>(StepArgs{model, ter, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action,
                                        act_lo, act_hi, n_sub, h, timestep, time_buf, step_dt, hold, dof_torque, env_params});
}

// the rows' rules (parc_sim_core.h env_params_valid): *bad <- 1 if any row breaks one
__global__ __launch_bounds__(256) void phys_check_kernel(const parc_sim_env_params_t *__restrict__ env_params, int n_envs, int *bad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_envs && !parc_sim::env_params_valid(env_params[e])) *bad = 1;
}

// body-per-lane refresh: body poses / velocities from the state rows, for a list of envs (env_ids, n = list length), for
// the envs whose mask is set (device-side reset, n = env count), or for all (both null)
__global__ __launch_bounds__(64) void sim_refresh_bpl_kernel(const parc_sim_model_t *__restrict__ model, int n, const int64_t *__restrict__ env_ids,
                                                             const int32_t *__restrict__ mask, const float *__restrict__ root_state,
                                                             const float *__restrict__ dof_state, float *rigid_body_state, float *contact_forces) {
    using namespace parc_sim_bpl;
    const int g = threadIdx.x / BPL_G, b = threadIdx.x % BPL_G;
    const int k0 = (int)blockIdx.x * BPL_EPB;
    if (mask) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < BPL_EPB; ++k)
            if (k0 + k < n) any |= mask[k0 + k];
        if (!any) return;                               // uniform: nothing flagged in this workgroup
    }
    const int k = min(k0 + g, n - 1);
    const int e = env_ids ? (int)env_ids[k] : k;
    const bool live = k0 + g < n && (!mask || mask[e] != 0);
    const parc_sim_model_t &m = *model;
    const int B = m.num_bodies, D = m.dof_size;
    const Lane L = load_lane(m, b);
    int maxd = L.depth;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) maxd = max(maxd, __shfl_xor(maxd, o, BPL_G));
    LState x;
    // (PD targets are irrelevant here: the action / bound pointers are only read, point them at the dof row)
    const float *drow = dof_state + 2 * (size_t)D * e;
    load_lane_state(m, L, b, root_state + 13 * (size_t)e, drow, drow, drow, drow, x);
    if (!live) return;        // whole 16-lane groups leave together; the sweeps below only shuffle inside a group
    store_lane_state<false>(L, b, maxd, x, nullptr, nullptr, rigid_body_state + 13 * (size_t)B * e, contact_forces + 3 * (size_t)B * e);
}

static_assert(PARC_SIM_MAX_BODIES <= BPL_G, "one body per lane: a 16-lane group holds one env");

// The argument rules that the step entry points share, checked before any HIP call
static bool step_args_ok(const StepArgs &a, int mode) {
    if (!a.model || a.n_envs < 0 || a.n_sub <= 0 || !(a.h > 0.f) || !a.terrain.hf) return false;
    if (mode < PARC_SIM_CTL_PD || mode > PARC_SIM_CTL_PD_1D) return false;
    if (a.hold <= 0 || a.n_sub % a.hold != 0) return false;
    if ((a.timestep == nullptr) != (a.time_buf == nullptr)) return false;
    return !(a.dof_torque && (mode == PARC_SIM_CTL_PD || mode == PARC_SIM_CTL_VEL));
}

// The launch of checked arguments: the table's kernel if there is a table, else the pd kernel or the mode's
static int launch_step(void *stream, const StepArgs &a, int mode, bool table) {
    if (a.n_envs == 0) return PARC_OK;
    auto launch = [&](auto kernel, auto... more) {
        hipLaunchKernelGGL(kernel, dim3((a.n_envs + BPL_EPB - 1) / BPL_EPB), dim3(64), 0, (hipStream_t)stream, a.model, a.terrain, a.n_envs,
                           a.root_state, a.dof_state, a.rigid_body_state, a.contact_forces, a.env_offsets, a.action, a.act_lo, a.act_hi, a.n_sub,
                           a.h, a.timestep, a.time_buf, a.step_dt, more...);
    };
    parc_sim::ctl_dispatch(mode, [&](auto m) {
        constexpr int MODE = decltype(m)::value;
        if (table)
            launch(sim_step_bpl_phys_kernel<MODE>, a.hold, a.dof_torque, a.env_params);
        else if constexpr (MODE == PARC_SIM_CTL_PD)
            launch(sim_step_bpl_kernel);
        else
            launch(sim_step_bpl_ctl_kernel<MODE>, a.hold, a.dof_torque);
    });
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_sim_step(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                             float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                             const float *action, const float *action_low, const float *action_high, int n_substeps, float h) {
    const StepArgs a{model, terrain, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action, action_low,
                     action_high, n_substeps, h, nullptr, nullptr, 0.f, 1, nullptr, nullptr};
    return step_args_ok(a, PARC_SIM_CTL_PD) ? launch_step(stream, a, PARC_SIM_CTL_PD, false) : PARC_EINVAL;
}

extern "C" int parc_sim_step_tick(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                                  float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                                  const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                                  int32_t *timestep_buf, float *time_buf, float step_dt) {
    const StepArgs a{model, terrain, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action, action_low,
                     action_high, n_substeps, h, timestep_buf, time_buf, step_dt, 1, nullptr, nullptr};
    if (!timestep_buf || !step_args_ok(a, PARC_SIM_CTL_PD)) return PARC_EINVAL;
    return launch_step(stream, a, PARC_SIM_CTL_PD, false);
}

extern "C" int parc_sim_step_ctl(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                                 float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                                 const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                                 int substeps_per_hold, int control_mode, float *dof_torque, int32_t *timestep_buf, float *time_buf,
                                 float step_dt) {
    const StepArgs a{model, terrain, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action, action_low,
                     action_high, n_substeps, h, timestep_buf, time_buf, step_dt, substeps_per_hold, dof_torque, nullptr};
    return step_args_ok(a, control_mode) ? launch_step(stream, a, control_mode, false) : PARC_EINVAL;
}

// The verdict cell of phys_check_kernel: one word of pinned, portable host memory that the device writes directly, allocated at the first
// check (never inside a capture: a capturing stream skips the check).  ONE cell for the process - every device and stream - so a check
// holds the mutex from clearing the cell to reading it, the wait for the stream included: checks of concurrent callers run one after
// the other.  A caller that has already checked its table (parc_sim_env_params_check, or host-side as the env does) and wants no wait
// per step issues the step inside a capture.
static std::mutex g_check_mu;
static int *g_check_cell = nullptr;

extern "C" int parc_sim_env_params_check(void *stream, const parc_sim_env_params_t *env_params, int n_envs) {
    if (!env_params || n_envs < 0) return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    std::lock_guard<std::mutex> lock(g_check_mu);
    if (!g_check_cell) {
        hipError_t e0 = hipHostMalloc((void **)&g_check_cell, sizeof(int), hipHostMallocPortable | hipHostMallocMapped);
        if (e0 != hipSuccess) {
            g_check_cell = nullptr;
            return (int)e0;
        }
    }
    *g_check_cell = 0;
    hipLaunchKernelGGL(phys_check_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, env_params, n_envs, g_check_cell);
    PARC_CHECK_LAUNCH();
    const hipError_t e1 = hipStreamSynchronize((hipStream_t)stream);
    if (e1 != hipSuccess) return (int)e1;
    return *g_check_cell ? PARC_EINVAL : PARC_OK;
}

extern "C" int parc_sim_step_phys(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                                  float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                                  const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                                  int substeps_per_hold, parc_sim_env_params_t *env_params, int control_mode, float *dof_torque,
                                  int32_t *timestep_buf, float *time_buf, float step_dt) {
    const StepArgs a{model, terrain, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action, action_low,
                     action_high, n_substeps, h, timestep_buf, time_buf, step_dt, substeps_per_hold, dof_torque, env_params};
    if (!env_params || !step_args_ok(a, control_mode)) return PARC_EINVAL;
    if (n_envs > 0) {
        // the rows' rules: checked in front of the step unless the stream is being captured (nothing can be waited for there)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) {
            (void)hipGetLastError();
            cap = hipStreamCaptureStatusNone;
        }
        if (cap == hipStreamCaptureStatusNone) {
            const int rc = parc_sim_env_params_check(stream, env_params, n_envs);
            if (rc != PARC_OK) return rc;
        }
    }
    return launch_step(stream, a, control_mode, true);
}

// =============================================================================================
// Device-side sampler of the per-env table (parc_phys_rand): one thread per env, Philox4x32-10 keyed by the seed with counter
// (env, block, launch counter lo, hi) - block 0 / 1: the eight fields of a reset, block 2: a push, block 3: the interval after a reset.
// state[0] = launch counter, state[1] = ticket of the launch's last workgroup (the scheme of rng_step_kernel, parc_rollout.hip).
// =============================================================================================
__device__ __forceinline__ void phys_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
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
__device__ __forceinline__ float phys_u01(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }      // [0, 1), 24 bits
__device__ __forceinline__ float phys_uniform(const float *lohi, uint32_t r) {
    return fminf(lohi[0] + phys_u01(r) * (lohi[1] - lohi[0]), lohi[1]);
}
__device__ __forceinline__ float phys_log_uniform(const float *lohi, uint32_t r) {
    return fminf(fmaxf(lohi[0] * expf(phys_u01(r) * logf(lohi[1] / lohi[0])), lohi[0]), lohi[1]);
}
__device__ __forceinline__ int phys_uniform_int(const int32_t *lohi, uint32_t r) {
    const int span = lohi[1] - lohi[0] + 1;
    const int k = (int)(phys_u01(r) * (float)span);
    return lohi[0] + (k < span ? k : span - 1);
}

__global__ __launch_bounds__(256) void phys_rand_kernel(int n_envs, const int32_t *__restrict__ reset_mask, parc_phys_ranges_t rg, uint64_t seed,
                                                        uint64_t *state, parc_sim_env_params_t *env_params) {
    const uint64_t step = state[0];
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_envs) {
        parc_sim_env_params_t *row = env_params + e;
        const uint32_t s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        const bool pushes = rg.push_interval[1] > 0;
        uint32_t r[4];
        if (reset_mask && reset_mask[e] != 0) {
            if (rg.field_mask & 0x0Fu) {
                phys_philox((uint32_t)e, 0u, s0, s1, k0, k1, r);
                if (rg.field_mask & 1u) row->gravity = phys_uniform(rg.gravity, r[0]);
                if (rg.field_mask & 2u) row->friction_mu = phys_uniform(rg.friction_mu, r[1]);
                if (rg.field_mask & 4u) row->contact_kn = phys_log_uniform(rg.contact_kn, r[2]);
                if (rg.field_mask & 8u) row->contact_cn = phys_log_uniform(rg.contact_cn, r[3]);
            }
            if (rg.field_mask & 0xF0u) {
                phys_philox((uint32_t)e, 1u, s0, s1, k0, k1, r);
                if (rg.field_mask & 16u) row->contact_ct = phys_log_uniform(rg.contact_ct, r[0]);
                if (rg.field_mask & 32u) row->mass_scale = phys_log_uniform(rg.mass_scale, r[1]);
                if (rg.field_mask & 64u) row->kp_scale = phys_uniform(rg.kp_scale, r[2]);
                if (rg.field_mask & 128u) row->kd_scale = phys_uniform(rg.kd_scale, r[3]);
            }
            if (pushes) {          // a new episode starts unpushed, a whole interval away from its first push
                phys_philox((uint32_t)e, 3u, s0, s1, k0, k1, r);
                row->push_steps_left = 0;
                row->push_next_in = phys_uniform_int(rg.push_interval, r[0]);
            }
        } else if (pushes && rg.push_tick) {
            const int nx = row->push_next_in - 1;
            if (nx <= 0) {
                phys_philox((uint32_t)e, 2u, s0, s1, k0, k1, r);
                float sn, cs;
                sincosf(6.283185307179586f * phys_u01(r[0]), &sn, &cs);
                const float mag = phys_uniform(rg.push_force, r[1]);
                row->push_force[0] = mag * cs;
                row->push_force[1] = mag * sn;
                row->push_force[2] = 0.f;
                row->push_steps_left = phys_uniform_int(rg.push_duration, r[2]);
                row->push_next_in = phys_uniform_int(rg.push_interval, r[3]);
            } else {
                row->push_next_in = nx;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(state + 1);
        if (atomicAdd(ticket, 1ull) == (unsigned long long)gridDim.x - 1ull) {
            state[0] = step + 1;
            *ticket = 0ull;
        }
    }
}

static bool range_ok(const float *r, bool positive) {
    return r[0] - r[0] == 0.f && r[1] - r[1] == 0.f && r[0] <= r[1] && (!positive || r[0] > 0.f);
}

extern "C" int parc_phys_rand(void *stream, int n_envs, const int32_t *reset_mask, const parc_phys_ranges_t *ranges, uint64_t seed,
                              uint64_t *rng_state, parc_sim_env_params_t *env_params) {
    if (!ranges || !rng_state || !env_params || n_envs < 0) return PARC_EINVAL;
    const parc_phys_ranges_t &g = *ranges;
    const unsigned fm = g.field_mask;
    if (fm & ~0xFFu) return PARC_EINVAL;
    if (((fm & 1u) && !range_ok(g.gravity, false)) || ((fm & 2u) && !(range_ok(g.friction_mu, false) && g.friction_mu[0] >= 0.f)) ||
        ((fm & 4u) && !range_ok(g.contact_kn, true)) || ((fm & 8u) && !range_ok(g.contact_cn, true)) ||
        ((fm & 16u) && !range_ok(g.contact_ct, true)) || ((fm & 32u) && !range_ok(g.mass_scale, true)) ||
        ((fm & 64u) && !range_ok(g.kp_scale, true)) || ((fm & 128u) && !(range_ok(g.kd_scale, false) && g.kd_scale[0] >= 0.f)))
        return PARC_EINVAL;
    if (g.push_interval[1] > 0 && (g.push_interval[0] < 1 || g.push_interval[0] > g.push_interval[1] || g.push_duration[0] < 1 ||
                                   g.push_duration[0] > g.push_duration[1] || !range_ok(g.push_force, false)))
        return PARC_EINVAL;
    if (n_envs == 0) return PARC_OK;
    hipLaunchKernelGGL(phys_rand_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, n_envs, reset_mask, g, seed, rng_state,
                       env_params);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

// the refresh of n rows: a list of envs, a mask over the envs, or neither
static int launch_refresh(void *stream, const parc_sim_model_t *model, int n, const int64_t *env_ids, const int32_t *mask,
                          const float *root_state, const float *dof_state, float *rigid_body_state, float *contact_forces) {
    if (n == 0) return PARC_OK;
    hipLaunchKernelGGL(sim_refresh_bpl_kernel, dim3((n + BPL_EPB - 1) / BPL_EPB), dim3(64), 0, (hipStream_t)stream, model, n, env_ids, mask,
                       root_state, dof_state, rigid_body_state, contact_forces);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_sim_refresh_bodies(void *stream, const parc_sim_model_t *model, int n_envs, const int64_t *env_ids, int n_sel,
                                       const float *root_state, const float *dof_state, float *rigid_body_state, float *contact_forces) {
    const int n = env_ids ? n_sel : n_envs;
    if (!model || n_envs < 0 || n < 0) return PARC_EINVAL;
    return launch_refresh(stream, model, n, env_ids, nullptr, root_state, dof_state, rigid_body_state, contact_forces);
}

extern "C" int parc_sim_refresh_bodies_masked(void *stream, const parc_sim_model_t *model, int n_envs, const int32_t *mask,
                                              const float *root_state, const float *dof_state, float *rigid_body_state,
                                              float *contact_forces) {
    if (!model || n_envs < 0 || !mask) return PARC_EINVAL;
    return launch_refresh(stream, model, n_envs, nullptr, mask, root_state, dof_state, rigid_body_state, contact_forces);
}

extern "C" int parc_sim_abi(void) { return 1; }
