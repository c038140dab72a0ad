// HOST build of the generator call's kernel bodies (parc_amd/csrc/parc_mdm_gen_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_mdm_gen.py builds it into a temporary directory with the host compiler, -ffp-contract=off).  mdm_gen_encode_host() and
// mdm_gen_decode_host() are the entry points of include/parc_mdm_gen.h with host pointers: the same argument checks, then the core's
// bodies for every sample with one lane (a sample's LDS is a vector of exactly the size the launch asks for).  With -DMDM_GEN_HOST_MAIN
// this is a stand-alone program that runs a case file written by tests/tools/mdm_gen_host.py (dump) - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_mdm_gen_core.h"

using namespace parc_mgn;

extern "C" int mdm_gen_encode_host(parc_char_model_t model, parc_mdm_gen_cfg_t cfg, parc_terrain_t terrain, int B, const float *root_pos,
                                   const float *root_rot, const float *joint_rot, const float *contacts, const float *target_world,
                                   const float *grid_x, const float *grid_y, const float *mean, const float *std, float *frame, float *out_root_pos,
                                   float *out_root_rot, float *out_body_pos, float *hf_z, float *target, float *target_dir, float *prev_state,
                                   float *obs) {
    const int rc = check_encode(model, cfg, terrain, B, root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std, frame,
                                out_root_pos, out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state);
    if (rc != PARC_OK) return rc == PARC_MGN_NOTHING ? PARC_OK : rc;
    for (int b = 0; b < B; ++b) {
        std::vector<float> scr((size_t)lds_bytes(model, cfg) / sizeof(float));
        const enc_sample e = make_enc_sample(model, cfg, b, root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std, frame,
                                             out_root_pos, out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state, obs, scr.data());
        encode_sample(model, cfg, terrain, e, 0, 1);
    }
    return PARC_OK;
}

extern "C" int mdm_gen_decode_host(parc_char_model_t model, parc_mdm_gen_cfg_t cfg, int B, const float *x, const float *prev_state,
                                   const uint8_t *no_noise, const float *mean, const float *std, const float *frame, float *root_pos,
                                   float *root_rot, float *joint_rot, float *contacts, float *frames) {
    const int rc = check_decode(model, cfg, B, x, prev_state, no_noise, mean, std, frame, root_pos, root_rot, joint_rot, contacts);
    if (rc != PARC_OK) return rc == PARC_MGN_NOTHING ? PARC_OK : rc;
    for (int b = 0; b < B; ++b)
        for (int s = 0; s < cfg.seq_len; ++s)
            decode_item(model, cfg, b, s, x, prev_state, no_noise, mean, std, frame, root_pos, root_rot, joint_rot, contacts, frames);
    return PARC_OK;
}

extern "C" int64_t mdm_gen_lds_bytes_host(parc_char_model_t model, parc_mdm_gen_cfg_t cfg) { return lds_bytes(model, cfg); }

extern "C" int mdm_gen_struct_sizes(int *out) {
    out[0] = (int)sizeof(parc_mdm_gen_cfg_t), out[1] = (int)sizeof(parc_char_model_t), out[2] = (int)sizeof(parc_terrain_t);
    return 3;
}

#ifdef MDM_GEN_HOST_MAIN
// case file (tests/tools/mdm_gen_host.py: dump): int64 header h[4] = {B, with_features, with_decode, with_keep}, the encode cfg, the
// decode cfg, the model, the terrain's {dim_x, dim_y} (int32) and {min_x, min_y, dx, dy} (float), hf [dim_x, dim_y], then root_pos
// [B, T, 3], root_rot [B, T, 4], joint_rot [B, T, J, 4], contacts [B, T, nb], target_world [B, 2], grid_x, grid_y, mean [S, D], std [S, D],
// and, with_decode, x [B, S, D] and, with_keep, no_noise [B] bytes.
// output: frame, root_pos, root_rot, body_pos, hf_z, target, target_dir, (prev_state, obs), then (decode) root_pos, root_rot, joint_rot,
// (contacts), frames.
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

static void wr(FILE *o, const std::vector<float> &v) {
    if (o && !v.empty()) fwrite(v.data(), sizeof(float), v.size(), o);
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
    const parc_mdm_gen_cfg_t ce = rd<parc_mdm_gen_cfg_t>(f, 1)[0], cd = rd<parc_mdm_gen_cfg_t>(f, 1)[0];
    const parc_char_model_t model = rd<parc_char_model_t>(f, 1)[0];
    if (check_cfg(model, ce, B, false) != PARC_OK || (h[2] && check_cfg(model, cd, B, true) != PARC_OK)) return 2;
    const std::vector<int32_t> td = rd<int32_t>(f, 2);
    const std::vector<float> tf = rd<float>(f, 4);
    if (td[0] < 1 || td[1] < 1 || td[0] > 4096 || td[1] > 4096) return 2;
    // exactly-sized vectors: an access one element too far is an error under the sanitizer
    const std::vector<float> hf = rd<float>(f, (size_t)td[0] * td[1]);
    const parc_terrain_t terrain = {hf.data(), td[0], td[1], tf[0], tf[1], tf[2], tf[3]};
    const size_t T = ce.num_frames, S = cd.seq_len, P = ce.num_prev_states, D = ce.feat_dim, nb = model.num_bodies, J = nb - 1;
    const size_t XY = (size_t)ce.dim_x * ce.dim_y, dofs = model.dof_size;
    const std::vector<float> root_pos = rd<float>(f, B * T * 3), root_rot = rd<float>(f, B * T * 4), joint_rot = rd<float>(f, B * T * J * 4);
    const std::vector<float> contacts = rd<float>(f, B * T * nb), target_world = rd<float>(f, (size_t)B * 2);
    const std::vector<float> grid_x = rd<float>(f, ce.dim_x), grid_y = rd<float>(f, ce.dim_y);
    const size_t rows = h[2] ? S : P;
    const std::vector<float> mean = rd<float>(f, rows * D), std_ = rd<float>(f, rows * D);
    std::vector<float> frame((size_t)B * PARC_MDM_GEN_FRAME), o_rp(B * T * 3), o_rr(B * T * 4), o_bp(B * T * J * 3), hf_z(B * XY), target((size_t)B * 2),
        target_dir((size_t)B * 2), prev_state(h[1] ? B * P * D : 0), obs(h[1] ? B * XY : 0);
    int rc = mdm_gen_encode_host(model, ce, terrain, B, root_pos.data(), root_rot.data(), joint_rot.data(), contacts.data(), target_world.data(),
                                 grid_x.data(), grid_y.data(), mean.data(), std_.data(), frame.data(), o_rp.data(), o_rr.data(), o_bp.data(),
                                 hf_z.data(), target.data(), target_dir.data(), h[1] ? prev_state.data() : nullptr, h[1] ? obs.data() : nullptr);
    if (rc != PARC_OK) return 3;
    for (const std::vector<float> *v : {&frame, &o_rp, &o_rr, &o_bp, &hf_z, &target, &target_dir, &prev_state, &obs}) wr(o, *v);
    if (h[2]) {
        const std::vector<float> x = rd<float>(f, B * S * D);
        const std::vector<uint8_t> keep = rd<uint8_t>(f, h[3] ? B : 0);
        const bool con = cd.off_contacts >= 0;
        std::vector<float> d_rp(B * S * 3), d_rr(B * S * 4), d_jr(B * S * J * 4), d_con(con ? B * S * nb : 0), d_fr(B * S * (6 + dofs));
        rc = mdm_gen_decode_host(model, cd, B, x.data(), h[3] ? prev_state.data() : nullptr, h[3] ? keep.data() : nullptr, mean.data(), std_.data(),
                                 frame.data(), d_rp.data(), d_rr.data(), d_jr.data(), con ? d_con.data() : nullptr, d_fr.data());
        if (rc != PARC_OK) return 3;
        for (const std::vector<float> *v : {&d_rp, &d_rr, &d_jr, &d_con, &d_fr}) wr(o, *v);
    }
    if (o) fclose(o);
    fclose(f);
    printf("mdm gen ok %d\n", B);
    return 0;
}
#endif
