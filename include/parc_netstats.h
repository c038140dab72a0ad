/*
 * parc_netstats.h -- C-ABI of the actor's unit statistics inside libparc_hip.so.
 *
 * The running activity and utility of every hidden unit that DMPPOAgent.test_model2 of the reference keeps with forward hooks
 * (learning/dm_ppo_agent.py:683-736), for all layers of the actor in one call per rollout step: two launches in a linear chain, no
 * allocation, host read, wait or float atomic.  Every sum is added in a fixed order, so two runs give the same bits.
 */
#ifndef PARC_NETSTATS_H
#define PARC_NETSTATS_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_NETSTATS_MAX_LAYERS 8
/* One workgroup of the partial kernel sums PARC_NETSTATS_ROWS rows of PARC_NETSTATS_COLS columns. */
#define PARC_NETSTATS_ROWS 64
#define PARC_NETSTATS_COLS 256

/* One hidden layer.  Every pointer is a DEVICE pointer, 16-byte aligned; dim % 4 == 0. */
typedef struct {
    const float *act;         /* [rows, dim] the layer's post-ReLU output of this step, row-major */
    int32_t dim;
    const float *out_abs_sum; /* [dim] S[j] = sum_i |W_next[i, j]| (parc_netstats_abs_colsum; constant during a rollout) */
    float *activations;       /* [dim] running mean of m[j] = |mean_r act[r, j]|, updated in place */
    float *utility;           /* [dim] running mean of m[j] * S[j], updated in place */
} parc_netstats_layer_t;

typedef struct {
    int32_t num_layers;       /* 1 .. PARC_NETSTATS_MAX_LAYERS */
    parc_netstats_layer_t layer[PARC_NETSTATS_MAX_LAYERS];
} parc_netstats_table_t;

/* Floats of workspace one update needs: ceil(rows / PARC_NETSTATS_ROWS) * sum of the dims; -1 for arguments the update refuses. */
int64_t parc_netstats_workspace_floats(int64_t rows, parc_netstats_table_t table);

/* One step.  With m_l[j] = |(sum_r act_l[r, j]) / rows|:
 *   activations_l[j] <- eta * activations_l[j] + gain * m_l[j]
 *   utility_l[j]     <- eta * utility_l[j] + (gain * m_l[j]) * out_abs_sum_l[j]
 *   mean_net_acts[r, a] <- eta * mean_net_acts[r, a] + gain * |mean[r, a]|        (mean, mean_net_acts: [rows, A], any A >= 1)
 * gain is 1 - eta, rounded by the caller from double (1.f - eta in float is off by 2^-24 / 0.01 for eta = 0.99).
 * PARC_EINVAL before any launch: rows < 1, num_layers outside 1 .. 8, a dim <= 0 or not a multiple of 4, A < 1, a NULL pointer, a
 * layer pointer or the workspace not 16-byte aligned.  PARC_EUNSUPPORTED: rows > 65535 * PARC_NETSTATS_ROWS. */
int parc_netstats_update(void *stream, int64_t rows, parc_netstats_table_t table, int A, const float *mean, float *mean_net_acts,
                         float eta, float gain, float *workspace);

/* out[j] <- sum_i |w[i, j]| for w [rows, dim] row-major (a Linear layer's weight: the summed outgoing weights of its input units),
 * added in row order.  PARC_EINVAL: rows < 1, dim < 1, a NULL pointer. */
int parc_netstats_abs_colsum(void *stream, int rows, int dim, const float *w, float *out);

/* counts[l] <- number of j with activations_l[j] < threshold, for every layer of the table (act / out_abs_sum / utility are not read
 * and may be NULL); counts[num_layers] <- number of the n_mean entries of mean_net_acts below the threshold (mean_net_acts may be NULL
 * with n_mean == 0).  counts: DEVICE int32 [num_layers + 1].  PARC_EINVAL: num_layers outside 1 .. 8, a dim <= 0, a NULL activations
 * pointer or counts, n_mean < 0 or above 2^31 - 1. */
int parc_netstats_dormant_count(void *stream, parc_netstats_table_t table, int64_t n_mean, const float *mean_net_acts, float threshold,
                                int32_t *counts);

int parc_netstats_abi(void);

#ifdef __cplusplus
}
#endif
#endif
