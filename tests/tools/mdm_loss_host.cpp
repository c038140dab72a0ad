// HOST build of the generator loss's kernel bodies (parc_amd/csrc/parc_mdm_loss_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_mdm_loss.py builds it into a temporary directory with the host compiler, -ffp-contract=off).  Every mdm_loss_*_host() is the
// entry point of include/parc_mdm_loss.h with host pointers: the same argument check, then the core's body for every sample with one
// lane (the sample's LDS is a vector of exactly the size the launch asks for).  With -DMDM_LOSS_HOST_MAIN this is a stand-alone program
// that runs a case file written by tests/tools/mdm_loss_host.py (dump) through both entry points - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_mdm_loss_core.h"

using namespace parc_ml;

static int done(int rc) { return rc == PARC_ML_NOTHING ? PARC_OK : rc; }

extern "C" int mdm_loss_forward_host(parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean, const float *std,
                                     const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts, const float *hfs,
                                     const float *target_dir, const float *grid_x, const float *grid_y, const float *points, const int32_t *point_start,
                                     float *losses) {
    const int rc = check_args(model, cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                              point_start, losses, losses);
    if (rc != PARC_OK) return done(rc);
    for (int b = 0; b < B; ++b) {
        std::vector<float> scr((size_t)lds_bytes(model, cfg) / sizeof(float));
        const sample s = make_sample(model, cfg, b, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                                     point_start, scr.data());
        forward_sample(model, cfg, s, b, B, losses, 0, 1);
    }
    return PARC_OK;
}

extern "C" int mdm_loss_backward_host(parc_char_model_t model, parc_mdm_loss_cfg_t cfg, int B, const float *x, const float *mean, const float *std,
                                      const float *root_pos, const float *root_rot, const float *joint_rot, const float *contacts, const float *hfs,
                                      const float *target_dir, const float *grid_x, const float *grid_y, const float *points,
                                      const int32_t *point_start, const float *g_losses, float *g_x) {
    const int rc = check_args(model, cfg, B, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                              point_start, g_x, g_losses);
    if (rc != PARC_OK) return done(rc);
    for (int b = 0; b < B; ++b) {
        std::vector<float> scr((size_t)lds_bytes(model, cfg) / sizeof(float));
        const sample s = make_sample(model, cfg, b, x, mean, std, root_pos, root_rot, joint_rot, contacts, hfs, target_dir, grid_x, grid_y, points,
                                     point_start, scr.data());
        backward_sample(model, cfg, s, b, B, g_losses, g_x + (size_t)b * cfg.seq_len * cfg.feat_dim, 0, 1);
    }
    return PARC_OK;
}

extern "C" int64_t mdm_loss_lds_bytes_host(parc_char_model_t model, parc_mdm_loss_cfg_t cfg) { return lds_bytes(model, cfg); }

extern "C" int mdm_loss_struct_sizes(int *out) {
    out[0] = (int)sizeof(parc_mdm_loss_cfg_t), out[1] = (int)sizeof(parc_char_model_t);
    return 2;
}

#ifdef MDM_LOSS_HOST_MAIN
// case file (tests/tools/mdm_loss_host.py: dump): int64 header h[4] = {B, has_contacts, 0, 0}, cfg, model, then x [B, S, D], mean [S, D],
// std [S, D], root_pos, root_rot, joint_rot, contacts (if any), hfs, target_dir, grid_x, grid_y, points [max(P, 1), 3], point_start [nb + 1],
// g_losses [TERMS, B].  output: losses [TERMS, B], g_x [B, S, D].
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
    const parc_mdm_loss_cfg_t cfg = rd<parc_mdm_loss_cfg_t>(f, 1)[0];
    const parc_char_model_t model = rd<parc_char_model_t>(f, 1)[0];
    if (check_cfg(model, cfg, B) != PARC_OK) return 2;
    const size_t S = cfg.seq_len, D = cfg.feat_dim, nb = model.num_bodies, XY = (size_t)cfg.dim_x * cfg.dim_y, P = cfg.num_points;
    // exactly-sized vectors: an access one element too far is an error under the sanitizer
    const std::vector<float> x = rd<float>(f, B * S * D), mean = rd<float>(f, S * D), std_ = rd<float>(f, S * D), root_pos = rd<float>(f, B * S * 3),
                             root_rot = rd<float>(f, B * S * 4), joint_rot = rd<float>(f, B * S * (nb - 1) * 4),
                             contacts = rd<float>(f, h[1] ? B * S * nb : 0), hfs = rd<float>(f, B * XY), target_dir = rd<float>(f, (size_t)B * 2),
                             grid_x = rd<float>(f, cfg.dim_x), grid_y = rd<float>(f, cfg.dim_y), points = rd<float>(f, (P ? P : 1) * 3);
    const std::vector<int32_t> point_start = rd<int32_t>(f, nb + 1);
    const std::vector<float> g_losses = rd<float>(f, (size_t)PARC_MDM_LOSS_TERMS * B);
    std::vector<float> losses((size_t)PARC_MDM_LOSS_TERMS * B), g_x(B * S * D);
    int rc = mdm_loss_forward_host(model, cfg, B, x.data(), mean.data(), std_.data(), root_pos.data(), root_rot.data(), joint_rot.data(),
                                   contacts.empty() ? nullptr : contacts.data(), hfs.data(), target_dir.data(), grid_x.data(), grid_y.data(),
                                   points.data(), point_start.data(), losses.data());
    if (rc == PARC_OK)
        rc = mdm_loss_backward_host(model, cfg, B, x.data(), mean.data(), std_.data(), root_pos.data(), root_rot.data(), joint_rot.data(),
                                    contacts.empty() ? nullptr : contacts.data(), hfs.data(), target_dir.data(), grid_x.data(), grid_y.data(),
                                    points.data(), point_start.data(), g_losses.data(), g_x.data());
    if (o) {
        fwrite(losses.data(), sizeof(float), losses.size(), o);
        fwrite(g_x.data(), sizeof(float), g_x.size(), o);
        fclose(o);
    }
    fclose(f);
    if (rc != PARC_OK) return 3;
    printf("mdm loss ok %d\n", B);
    return 0;
}
#endif
