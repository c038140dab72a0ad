// HOST build of the generator guidance step's kernel body (parc_amd/csrc/parc_mdm_guide_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_mdm_guide.py builds it into a temporary directory with the host compiler, -ffp-contract=off).  mdm_guide_step_host() is the
// entry point of include/parc_mdm_guide.h with host pointers: the same argument check, then the core's body for every sample with one
// lane (the sample's LDS is a vector of exactly the size the launch asks for).  With -DMDM_GUIDE_HOST_MAIN this is a stand-alone program
// that runs a case file written by tests/tools/mdm_guide_host.py (dump) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_mdm_guide_core.h"

using namespace parc_mg;

extern "C" int mdm_guide_step_host(parc_char_model_t model, parc_mdm_guide_cfg_t cfg, int B, const float *x, const float *mean, const float *std,
                                   const float *hfs, const float *target_xy, const float *grid_x, const float *grid_y, const float *points,
                                   const int32_t *point_start, float *x_out, float *terms) {
    const int rc = check_args(model, cfg, B, x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, x_out, terms);
    if (rc != PARC_OK) return rc == PARC_MG_NOTHING ? PARC_OK : rc;
    for (int b = 0; b < B; ++b) {
        std::vector<float> scr((size_t)lds_bytes(model, cfg) / sizeof(float));
        const gsample g = make_gsample(cfg, b, x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, scr.data());
        step_sample(model, cfg, g, b, B, x_out + (size_t)b * cfg.seq_len * cfg.feat_dim, terms, 0, 1);
    }
    return PARC_OK;
}

extern "C" int64_t mdm_guide_lds_bytes_host(parc_char_model_t model, parc_mdm_guide_cfg_t cfg) { return lds_bytes(model, cfg); }

extern "C" int mdm_guide_struct_sizes(int *out) {
    out[0] = (int)sizeof(parc_mdm_guide_cfg_t), out[1] = (int)sizeof(parc_char_model_t);
    return 2;
}

#ifdef MDM_GUIDE_HOST_MAIN
// case file (tests/tools/mdm_guide_host.py: dump): int64 header h[4] = {B, has_hf, has_target, in_place}, cfg, model, then x [B, S, D],
// mean [S, D], std [S, D], and, with has_hf, hfs [B, X, Y], grid_x, grid_y, points [P, 3], point_start [nb + 1]; with has_target,
// target_xy [B, 2].  output: terms [TERMS, B], x_out [B, S, D].
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !o) return 2;
    const std::vector<int64_t> h = rd<int64_t>(f, 4);
    if (h[0] < 0 || h[0] > (1 << 16)) return 2;
    const int B = (int)h[0];
    const parc_mdm_guide_cfg_t cfg = rd<parc_mdm_guide_cfg_t>(f, 1)[0];
    const parc_char_model_t model = rd<parc_char_model_t>(f, 1)[0];
    if (check_cfg(model, cfg, B) != PARC_OK) return 2;
    const size_t S = cfg.seq_len, D = cfg.feat_dim, nb = model.num_bodies, XY = (size_t)cfg.dim_x * cfg.dim_y, P = cfg.num_points;
    // exactly-sized vectors: an access one element too far is an error under the sanitizer
    std::vector<float> x = rd<float>(f, B * S * D);
    const std::vector<float> mean = rd<float>(f, S * D), std_ = rd<float>(f, S * D);
    std::vector<float> hfs, grid_x, grid_y, points, target;
    std::vector<int32_t> point_start;
    if (h[1]) {
        hfs = rd<float>(f, B * XY), grid_x = rd<float>(f, cfg.dim_x), grid_y = rd<float>(f, cfg.dim_y), points = rd<float>(f, P * 3);
        point_start = rd<int32_t>(f, nb + 1);
    }
    if (h[2]) target = rd<float>(f, (size_t)B * 2);
    std::vector<float> terms((size_t)PARC_MDM_GUIDE_TERMS * B), x_out(h[3] ? 0 : B * S * D);
    float *dst = h[3] ? x.data() : x_out.data();
    const int rc = mdm_guide_step_host(model, cfg, B, x.data(), mean.data(), std_.data(), h[1] ? hfs.data() : nullptr, h[2] ? target.data() : nullptr,
                                       h[1] ? grid_x.data() : nullptr, h[1] ? grid_y.data() : nullptr, h[1] ? points.data() : nullptr,
                                       h[1] ? point_start.data() : nullptr, dst, terms.data());
    if (o) {
        fwrite(terms.data(), sizeof(float), terms.size(), o);
        fwrite(dst, sizeof(float), B * S * D, o);
        fclose(o);
    }
    fclose(f);
    if (rc != PARC_OK) return 3;
    printf("mdm guide ok %d\n", B);
    return 0;
}
#endif
