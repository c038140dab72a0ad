// Actor unit statistics (include/parc_netstats.h): what the reference's forward hooks of test_model2 compute, for every hidden layer at
// once.  The per-step update is two launches in a linear chain.
//
// netstats_partial_kernel   grid = (column tiles of the widest layer, row chunks, layers + 1), 256 threads.  In plane z < layers a
//   workgroup owns 64 rows x 256 columns of layer z: lane c holds a float4 of columns, the four waves take the rows round-robin, fold
//   their sums through LDS as (w0 + w1) + (w2 + w3) and write one partial row.  Workgroups past a narrower layer's last tile leave at
//   once.  The workgroups of plane z == layers stride over the [rows, A] mean-net output and apply its element-wise running update.
// netstats_finalize_kernel  grid = (column tiles, layers), 256 threads = 256 columns: adds the partial rows in chunk order and applies
//   both running updates of the column.
// No atomics and no data-dependent order: two runs give the same bits.  A single ticketed launch was not taken: a device-scope fence per
// workgroup costs more than the second launch.
// netstats_abs_colsum_kernel and netstats_dormant_kernel run once per rollout / per report.
#include <hip/hip_runtime.h>

#include "parc_launch.h"
#include "parc_netstats_core.h"

using namespace parc_ns;

#define NS_THREADS 256
#define NS_LANES (PARC_NETSTATS_COLS / 4)
static_assert(NS_LANES * kRowGroups == NS_THREADS, "one float4 lane per four columns, four row groups");

__global__ __launch_bounds__(NS_THREADS) void netstats_partial_kernel(int rows, parc_netstats_table_t t, int chunks, int64_t n_mean,
                                                                      const float *__restrict__ mean, float *__restrict__ mean_net_acts,
                                                                      float eta, float gain, float4 *__restrict__ workspace) {
    __shared__ float4 red[kRowGroups][NS_LANES];
    const int z = blockIdx.z;
    if (z == t.num_layers) {        // the element-wise plane
        const int64_t stride = (int64_t)gridDim.x * gridDim.y * NS_THREADS;
        for (int64_t i = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * NS_THREADS + threadIdx.x; i < n_mean; i += stride)
            mean_net_acts[i] = run_mean_net(mean_net_acts[i], eta, gain, mean[i]);
        return;
    }
    int dim4 = 0;
    int64_t before4 = 0;            // float4 columns of the layers in front of z
    const float4 *act = nullptr;
    for (int l = 0; l < PARC_NETSTATS_MAX_LAYERS; ++l) {        // (constant indices: the table stays in scalar registers)
        if (l < z) before4 += t.layer[l].dim / 4;
        if (l == z) {
            dim4 = t.layer[l].dim / 4;
            act = (const float4 *)t.layer[l].act;
        }
    }
    if (blockIdx.x * NS_LANES >= dim4) return;                  // whole workgroups leave: no barrier is skipped by a part of one
    const int lane = threadIdx.x % NS_LANES, rg = threadIdx.x / NS_LANES;
    const int c = blockIdx.x * NS_LANES + lane;
    const int r0 = blockIdx.y * PARC_NETSTATS_ROWS, r1 = min(r0 + PARC_NETSTATS_ROWS, rows);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < dim4) {
#pragma unroll 4
        for (int r = r0 + rg; r < r1; r += kRowGroups) {
            const float4 v = act[(size_t)r * dim4 + c];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[rg][lane] = s;
    __syncthreads();
    if (rg == 0 && c < dim4) {
        const float4 a = red[0][lane], b = red[1][lane], d = red[2][lane], e = red[3][lane];
        workspace[(size_t)chunks * before4 + (size_t)blockIdx.y * dim4 + c] =
            make_float4(fold4(a.x, b.x, d.x, e.x), fold4(a.y, b.y, d.y, e.y), fold4(a.z, b.z, d.z, e.z), fold4(a.w, b.w, d.w, e.w));
    }
}

__global__ __launch_bounds__(NS_THREADS) void netstats_finalize_kernel(int rows, parc_netstats_table_t t, int chunks, float eta, float gain,
                                                                       const float *__restrict__ workspace) {
    const int z = blockIdx.y;
    int dim = 0;
    int64_t before = 0;
    const float *out_abs_sum = nullptr;
    float *activations = nullptr, *utility = nullptr;
    for (int l = 0; l < PARC_NETSTATS_MAX_LAYERS; ++l) {
        if (l < z) before += t.layer[l].dim;
        if (l == z) {
            dim = t.layer[l].dim;
            out_abs_sum = t.layer[l].out_abs_sum;
            activations = t.layer[l].activations;
            utility = t.layer[l].utility;
        }
    }
    const int c = blockIdx.x * NS_THREADS + threadIdx.x;
    if (c >= dim) return;
    const float *partial = workspace + (size_t)chunks * before + c;
    float s = 0.f;
#pragma unroll 8
    for (int k = 0; k < chunks; ++k) s += partial[(size_t)k * dim];
    const float m = col_activity(s, rows);
    activations[c] = run_activation(activations[c], eta, gain, m);
    utility[c] = run_utility(utility[c], eta, gain, m, out_abs_sum[c]);
}

__global__ __launch_bounds__(NS_THREADS) void netstats_abs_colsum_kernel(int rows, int dim, const float *__restrict__ w, float *__restrict__ out) {
    const int c = blockIdx.x * NS_THREADS + threadIdx.x;
    if (c >= dim) return;
    float s = 0.f;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) s += fabsf(w[(size_t)r * dim + c]);
    out[c] = s;
}

// one workgroup per layer, the last one for the mean net; integer sums: their order does not matter
__global__ __launch_bounds__(NS_THREADS) void netstats_dormant_kernel(parc_netstats_table_t t, int64_t n_mean, const float *__restrict__ mean_net_acts,
                                                                      float threshold, int32_t *__restrict__ counts) {
    __shared__ int32_t red[NS_THREADS];
    const int z = blockIdx.x;
    const float *v = mean_net_acts;
    int64_t n = n_mean;
    for (int l = 0; l < PARC_NETSTATS_MAX_LAYERS; ++l) {
        if (l == z && z < t.num_layers) {
            v = t.layer[l].activations;
            n = t.layer[l].dim;
        }
    }
    int32_t k = 0;
    for (int64_t i = threadIdx.x; i < n; i += NS_THREADS) k += v[i] < threshold;
    red[threadIdx.x] = k;
    __syncthreads();
    for (int s = NS_THREADS / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[z] = red[0];
}

extern "C" int64_t parc_netstats_workspace_floats(int64_t rows, parc_netstats_table_t table) { return workspace_floats(rows, table); }

extern "C" int parc_netstats_update(void *stream, int64_t rows, parc_netstats_table_t table, int A, const float *mean, float *mean_net_acts,
                                    float eta, float gain, float *workspace) {
    const int rc = check_update(rows, table, A, mean, mean_net_acts, workspace);
    if (rc != PARC_OK) return rc;
    int max_dim = 0;
    for (int l = 0; l < table.num_layers; ++l) max_dim = table.layer[l].dim > max_dim ? table.layer[l].dim : max_dim;
    const int chunks = (int)chunks_of(rows);
    hipLaunchKernelGGL(netstats_partial_kernel, dim3((max_dim + PARC_NETSTATS_COLS - 1) / PARC_NETSTATS_COLS, chunks, table.num_layers + 1),
                       dim3(NS_THREADS), 0, (hipStream_t)stream, (int)rows, table, chunks, rows * A, mean, mean_net_acts, eta, gain,
                       (float4 *)workspace);
    PARC_CHECK_LAUNCH();
    hipLaunchKernelGGL(netstats_finalize_kernel, dim3((max_dim + NS_THREADS - 1) / NS_THREADS, table.num_layers), dim3(NS_THREADS), 0,
                       (hipStream_t)stream, (int)rows, table, chunks, eta, gain, workspace);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_netstats_abs_colsum(void *stream, int rows, int dim, const float *w, float *out) {
    if (rows < 1 || dim < 1 || !w || !out) return PARC_EINVAL;
    hipLaunchKernelGGL(netstats_abs_colsum_kernel, dim3((dim + NS_THREADS - 1) / NS_THREADS), dim3(NS_THREADS), 0, (hipStream_t)stream, rows, dim, w, out);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_netstats_dormant_count(void *stream, parc_netstats_table_t table, int64_t n_mean, const float *mean_net_acts, float threshold,
                                           int32_t *counts) {
    if (check_table(table) != PARC_OK || !counts || n_mean < 0 || n_mean > 2147483647LL || (n_mean > 0 && !mean_net_acts)) return PARC_EINVAL;
    hipLaunchKernelGGL(netstats_dormant_kernel, dim3(table.num_layers + 1), dim3(NS_THREADS), 0, (hipStream_t)stream, table, n_mean, mean_net_acts,
                       threshold, counts);
    PARC_CHECK_LAUNCH();
    return PARC_OK;
}

extern "C" int parc_netstats_abi(void) { return 1; }
