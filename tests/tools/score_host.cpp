// HOST build of the motion scorer (parc_amd/csrc/parc_score_core.h) -- TEST INFRASTRUCTURE ONLY (tests/test_motion_score.py builds it into
// a temporary directory with the host compiler).  score_host() is parc_motion_score from the body poses on, with host pointers
// everywhere: the same argument check, then the core's frame terms per counted frame and its fold per candidate, adding in the kernel's
// order.  body_pos [B,F,Bd,3] / body_rot [B,F,Bd,4] stand where the kernel has its forward kinematics.  With -DSCORE_HOST_MAIN this is
// a stand-alone program that scores a case file written by tests/tools/score_host.py (dump) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_score_core.h"

using namespace parc_sc;

extern "C" int score_host(int num_bodies, int B, int F, const int32_t *num_frames, const float *body_pos, const float *body_rot,
                          const float *contacts, int n_points, const float *local, const int32_t *start, parc_score_terrain_t ter, float base_z,
                          float w_contact, float w_pen, float dt, float max_jerk, float *frame_terms, float *losses, float *jerk) {
    parc_char_model_t model;
    memset(&model, 0, sizeof(model));
    model.num_bodies = num_bodies;
    const int rc = check_args(model, B, F, body_pos, body_rot, body_rot, contacts, n_points, local, start, ter, body_pos, frame_terms, losses, jerk);
    if (rc != PARC_OK) return rc;
    const Field fld = make_field(ter, base_z);
    const int Bd = num_bodies;
    for (int c = 0; c < B; ++c) {
        const int n = counted_frames(num_frames, c, F);
        for (int f = 0; f < n; ++f) {
            const size_t row = (size_t)c * F + f;
            frame_terms_host(fld, Bd, body_pos + row * Bd * 3, body_rot + row * Bd * 4, contacts + row * Bd, n_points, local, start,
                             frame_terms + 2 * row);
        }
        fold_host(n, Bd, frame_terms + 2 * (size_t)c * F, body_pos + (size_t)c * F * Bd * 3, w_contact, w_pen, dt, max_jerk, losses + 3 * (size_t)c,
                  jerk ? jerk + 2 * (size_t)c : nullptr);
    }
    return PARC_OK;
}

#ifdef SCORE_HOST_MAIN
// case file: int32 header {Bd, B, F, n_points, dim_x, dim_y, has_num_frames}, float {min_x, min_y, dx, dy, base_z, w_contact, w_pen, dt,
// max_jerk}, then [num_frames], start, body_pos, body_rot, contacts, local, hf, x_points, y_points
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
    const std::vector<int32_t> h = rd<int32_t>(f, 7);
    const std::vector<float> g = rd<float>(f, 9);
    const int Bd = h[0], B = h[1], F = h[2], P = h[3], X = h[4], Y = h[5];
    if (Bd < 1 || Bd > 16 || B < 0 || B > 256 || F < 0 || F > 4096 || P <= 0 || P > 65536 || X <= 0 || Y <= 0 || X > 4096 || Y > 4096) return 2;
    const std::vector<int32_t> nf = rd<int32_t>(f, h[6] ? B : 0), start = rd<int32_t>(f, Bd + 1);
    const size_t rows = (size_t)B * F;
    const std::vector<float> pos = rd<float>(f, rows * Bd * 3), rot = rd<float>(f, rows * Bd * 4), con = rd<float>(f, rows * Bd);
    const std::vector<float> local = rd<float>(f, (size_t)P * 3), hf = rd<float>(f, (size_t)X * Y), xs = rd<float>(f, X), ys = rd<float>(f, Y);
    fclose(f);
    const parc_score_terrain_t ter = {hf.data(), X, Y, g[0], g[1], g[2], g[3], xs.data(), ys.data()};
    std::vector<float> terms(rows * 2 + 1, -7.0f), losses((size_t)B * 3 + 1), jerk((size_t)B * 2 + 1);
    const int rc = score_host(Bd, B, F, h[6] ? nf.data() : nullptr, pos.data(), rot.data(), con.data(), P, local.data(), start.data(), ter, g[4], g[5], g[6],
                              g[7], g[8], terms.data(), losses.data(), jerk.data());
    if (rc != PARC_OK) return 3;
    if (argc > 2) {       // the results, for the caller to compare with the plain build's
        FILE *o = fopen(argv[2], "wb");
        if (!o) return 2;
        fwrite(terms.data(), 4, rows * 2, o);
        fwrite(losses.data(), 4, (size_t)B * 3, o);
        fwrite(jerk.data(), 4, (size_t)B * 2, o);
        fclose(o);
    }
    printf("score ok %d %d\n", B, F);
    return 0;
}
#endif
