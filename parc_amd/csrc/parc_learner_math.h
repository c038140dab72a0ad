// Device helpers that more than one learner file uses (parc_ppo.hip, parc_rollout.hip, parc_optim.hip, parc_colreduce.hip): the 64-lane
// sum, the clamps that pass NaN on, and the clip coefficient of clip_grad_norm_.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Non-finite values surface where the reference's torch code surfaces them.  torch.clamp / clamp_min / clamp_max /
// minimum return NaN for a NaN operand; fminf / fmaxf return the other operand.  On finite input these give the bits of
// fminf(fmaxf(v, lo), hi), fminf(a, b), ...; a NaN falls through every compare and comes out.
__device__ __forceinline__ float clamp_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float clamp_min_nan(float v, float lo) { return v < lo ? lo : v; }
__device__ __forceinline__ float clamp_max_nan(float v, float hi) { return v > hi ? hi : v; }
__device__ __forceinline__ float minimum_nan(float a, float b) { return a <= b ? a : (b < a ? b : __builtin_nanf("")); }
// clip_grad_norm_: coef = clamp(max_norm / (norm + 1e-6), max = 1); a NaN norm gives a NaN coefficient, which reaches every element
__device__ __forceinline__ float clip_coef(float max_norm, float norm) { return clamp_max_nan(max_norm / (norm + 1e-6f), 1.0f); }
