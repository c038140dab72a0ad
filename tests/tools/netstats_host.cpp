// HOST build of the actor unit statistics (parc_amd/csrc/parc_netstats_core.h) -- TEST INFRASTRUCTURE ONLY (tests/test_unit_stats.py builds
// it into a temporary directory with the host compiler).  The three entry points are the C ABI of include/parc_netstats.h with host
// pointers everywhere: the same argument checks, and the kernels' sums as loops in the kernels' order.  With -DNETSTATS_HOST_MAIN this
// is a stand-alone program that runs a case file written by tests/tools/netstats_host.py (dump_case) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_netstats_core.h"

using namespace parc_ns;

extern "C" int64_t netstats_workspace_floats_host(int64_t rows, parc_netstats_table_t t) { return workspace_floats(rows, t); }

extern "C" int netstats_update_host(int64_t rows, parc_netstats_table_t t, int A, const float *mean, float *mean_net_acts, float eta, float gain,
                                    float *workspace) {
    return update_host(rows, t, A, mean, mean_net_acts, eta, gain, workspace);
}

extern "C" int netstats_abs_colsum_host(int rows, int dim, const float *w, float *out) { return abs_colsum_host(rows, dim, w, out); }

extern "C" int netstats_dormant_count_host(parc_netstats_table_t t, int64_t n_mean, const float *mean_net_acts, float threshold, int32_t *counts) {
    return dormant_count_host(t, n_mean, mean_net_acts, threshold, counts);
}

#ifdef NETSTATS_HOST_MAIN
// case file: int32 header {L, N, A, K, dim_0 .. dim_7}, float {eta, gain, threshold}, then per layer W_next [d_next, d_l] (d_next = the
// next layer's dim, A for the last), then per step: every layer's activations [N, d_l], the mean [N, A].
// output: per step activations (all layers), utility (all layers), mean_net_acts [N, A]; at the end the L + 1 dormant counts as floats.
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

// 16-byte aligned storage of n floats
struct Buf {
    std::vector<float> raw;
    float *p;
    explicit Buf(size_t n) : raw(n + 4, 0.f) {
        p = raw.data();
        while ((uintptr_t)p & 15) ++p;
    }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<int32_t> h = rd<int32_t>(f, 4 + PARC_NETSTATS_MAX_LAYERS);
    const std::vector<float> g = rd<float>(f, 3);
    const int L = h[0], N = h[1], A = h[2], K = h[3];
    if (L < 1 || L > PARC_NETSTATS_MAX_LAYERS || N < 1 || N > 4096 || A < 1 || A > 256 || K < 0 || K > 4096) return 2;
    size_t total = 0;
    for (int l = 0; l < L; ++l) {
        if (h[4 + l] < 1 || h[4 + l] > 4096) return 2;
        total += h[4 + l];
    }
    std::vector<Buf> S, act, util, in;
    parc_netstats_table_t t;
    memset(&t, 0, sizeof(t));
    t.num_layers = L;
    for (int l = 0; l < L; ++l) {
        const int d = h[4 + l], d_next = l + 1 < L ? h[5 + l] : A;
        const std::vector<float> w = rd<float>(f, (size_t)d_next * d);
        S.emplace_back(d);
        act.emplace_back(d);
        util.emplace_back(d);
        in.emplace_back((size_t)N * d);
        if (abs_colsum_host(d_next, d, w.data(), S[l].p) != PARC_OK) return 3;
    }
    for (int l = 0; l < L; ++l) t.layer[l] = parc_netstats_layer_t{in[l].p, h[4 + l], S[l].p, act[l].p, util[l].p};
    const int64_t need = workspace_floats(N, t);
    if (need < 0) return 3;
    Buf ws((size_t)need), mna((size_t)N * A);
    FILE *o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !o) return 2;
    for (int k = 0; k < K; ++k) {
        for (int l = 0; l < L; ++l) {
            const std::vector<float> x = rd<float>(f, (size_t)N * h[4 + l]);
            memcpy(in[l].p, x.data(), x.size() * sizeof(float));
        }
        const std::vector<float> mean = rd<float>(f, (size_t)N * A);
        if (update_host(N, t, A, mean.data(), mna.p, g[0], g[1], ws.p) != PARC_OK) return 3;
        if (o) {
            for (int l = 0; l < L; ++l) fwrite(act[l].p, 4, h[4 + l], o);
            for (int l = 0; l < L; ++l) fwrite(util[l].p, 4, h[4 + l], o);
            fwrite(mna.p, 4, (size_t)N * A, o);
        }
    }
    fclose(f);
    std::vector<int32_t> counts(L + 1);
    if (dormant_count_host(t, (int64_t)N * A, mna.p, g[2], counts.data()) != PARC_OK) return 3;
    if (o) {
        for (int l = 0; l <= L; ++l) {
            const float c = (float)counts[l];
            fwrite(&c, 4, 1, o);
        }
        fclose(o);
    }
    printf("netstats ok %d %d %zu\n", L, K, total);
    return 0;
}
#endif
