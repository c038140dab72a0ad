// Actor unit statistics: the argument rules and all arithmetic of include/parc_netstats.h.
//
// The same source compiles for the device (parc_netstats.hip) and for the host (g++: tests/tools/netstats_host.cpp, the CPU tests and
// the sanitizer program), where the workgroups, row groups and chunks of the kernels are loops that add in the kernels' order.
//
// Reference: learning/dm_ppo_agent.py:683-736 (save_mean_net_output_and_update_util).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/parc_netstats.h"

#if defined(__HIPCC__)
#define PARC_NS_FN __host__ __device__ __forceinline__
#else
#define PARC_NS_FN static inline
#endif

namespace parc_ns {

constexpr int kRowGroups = 4;       // waves of a partial workgroup: wave g adds rows r0 + g, r0 + g + 4, ... of its chunk

PARC_NS_FN float fold4(float a, float b, float c, float d) { return (a + b) + (c + d); }
// m = |mean over the rows|
PARC_NS_FN float col_activity(float col_sum, int64_t rows) { return fabsf(col_sum / (float)rows); }
PARC_NS_FN float run_activation(float old, float eta, float gain, float m) { return eta * old + gain * m; }
PARC_NS_FN float run_utility(float old, float eta, float gain, float m, float out_abs_sum) { return eta * old + (gain * m) * out_abs_sum; }
PARC_NS_FN float run_mean_net(float old, float eta, float gain, float mean) { return eta * old + gain * fabsf(mean); }

PARC_NS_FN int64_t chunks_of(int64_t rows) { return (rows + PARC_NETSTATS_ROWS - 1) / PARC_NETSTATS_ROWS; }
PARC_NS_FN bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static inline int check_table(const parc_netstats_table_t &t) {
    if (t.num_layers < 1 || t.num_layers > PARC_NETSTATS_MAX_LAYERS) return PARC_EINVAL;
    for (int l = 0; l < t.num_layers; ++l)
        if (t.layer[l].dim <= 0 || !t.layer[l].activations) return PARC_EINVAL;
    return PARC_OK;
}

static inline int check_update(int64_t rows, const parc_netstats_table_t &t, int A, const float *mean, const float *mean_net_acts,
                               const float *workspace) {
    if (rows < 1 || A < 1 || !mean || !mean_net_acts || !workspace || !aligned16(workspace)) return PARC_EINVAL;
    const int rc = check_table(t);
    if (rc != PARC_OK) return rc;
    for (int l = 0; l < t.num_layers; ++l) {
        const parc_netstats_layer_t &y = t.layer[l];
        if ((y.dim & 3) || !y.act || !y.out_abs_sum || !y.utility) return PARC_EINVAL;
        if (!aligned16(y.act) || !aligned16(y.out_abs_sum) || !aligned16(y.activations) || !aligned16(y.utility)) return PARC_EINVAL;
    }
    if (rows > (int64_t)PARC_NETSTATS_ROWS * 65535) return PARC_EUNSUPPORTED;
    return PARC_OK;
}

static inline int64_t dim_sum(const parc_netstats_table_t &t, int upto) {
    int64_t s = 0;
    for (int l = 0; l < upto; ++l) s += t.layer[l].dim;
    return s;
}

static inline int64_t workspace_floats(int64_t rows, const parc_netstats_table_t &t) {
    if (rows < 1 || check_table(t) != PARC_OK) return -1;
    for (int l = 0; l < t.num_layers; ++l)
        if (t.layer[l].dim & 3) return -1;
    return chunks_of(rows) * dim_sum(t, t.num_layers);
}

#if !defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- the host build: the kernels as loops
// sum of column c over the rows of one chunk, as the four waves of a workgroup add it
static inline float chunk_col_sum(const float *act, int dim, int64_t r0, int64_t r1, int c) {
    float s[kRowGroups];
    for (int g = 0; g < kRowGroups; ++g) {
        s[g] = 0.f;
        for (int64_t r = r0 + g; r < r1; r += kRowGroups) s[g] += act[r * dim + c];
    }
    return fold4(s[0], s[1], s[2], s[3]);
}

static inline int update_host(int64_t rows, const parc_netstats_table_t &t, int A, const float *mean, float *mean_net_acts, float eta,
                              float gain, float *workspace) {
    const int rc = check_update(rows, t, A, mean, mean_net_acts, workspace);
    if (rc != PARC_OK) return rc;
    const int64_t chunks = chunks_of(rows);
    for (int l = 0; l < t.num_layers; ++l) {
        const parc_netstats_layer_t &y = t.layer[l];
        float *partial = workspace + chunks * dim_sum(t, l);
        for (int64_t k = 0; k < chunks; ++k) {
            const int64_t r0 = k * PARC_NETSTATS_ROWS, r1 = r0 + PARC_NETSTATS_ROWS < rows ? r0 + PARC_NETSTATS_ROWS : rows;
            for (int c = 0; c < y.dim; ++c) partial[k * y.dim + c] = chunk_col_sum(y.act, y.dim, r0, r1, c);
        }
        for (int c = 0; c < y.dim; ++c) {
            float s = 0.f;
            for (int64_t k = 0; k < chunks; ++k) s += partial[k * y.dim + c];
            const float m = col_activity(s, rows);
            y.activations[c] = run_activation(y.activations[c], eta, gain, m);
            y.utility[c] = run_utility(y.utility[c], eta, gain, m, y.out_abs_sum[c]);
        }
    }
    for (int64_t i = 0; i < rows * A; ++i) mean_net_acts[i] = run_mean_net(mean_net_acts[i], eta, gain, mean[i]);
    return PARC_OK;
}

static inline int abs_colsum_host(int rows, int dim, const float *w, float *out) {
    if (rows < 1 || dim < 1 || !w || !out) return PARC_EINVAL;
    for (int c = 0; c < dim; ++c) {
        float s = 0.f;
        for (int r = 0; r < rows; ++r) s += fabsf(w[(int64_t)r * dim + c]);
        out[c] = s;
    }
    return PARC_OK;
}

static inline int dormant_count_host(const parc_netstats_table_t &t, int64_t n_mean, const float *mean_net_acts, float threshold, int32_t *counts) {
    if (check_table(t) != PARC_OK || !counts || n_mean < 0 || n_mean > 2147483647LL || (n_mean > 0 && !mean_net_acts)) return PARC_EINVAL;
    for (int l = 0; l <= t.num_layers; ++l) {
        const float *v = l < t.num_layers ? t.layer[l].activations : mean_net_acts;
        const int64_t n = l < t.num_layers ? t.layer[l].dim : n_mean;
        int32_t k = 0;
        for (int64_t i = 0; i < n; ++i) k += v[i] < threshold;
        counts[l] = k;
    }
    return PARC_OK;
}
#endif

}  // namespace parc_ns
