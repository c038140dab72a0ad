// HOST build of the batch sampler's kernel bodies (parc_amd/csrc/parc_mdm_batch_core.h) -- TEST INFRASTRUCTURE ONLY
// (tests/test_mdm_sampler.py builds it into a temporary directory with the host compiler, -ffp-contract=off).  Every mdm_*_host() is the
// entry point of include/parc_mdm_batch.h with host pointers: the same argument check, then the core's body for every sample / lane (the
// LDS planes are vectors).  With -DMDM_BATCH_HOST_MAIN this is a stand-alone program that runs a case file written by
// tests/tools/mdm_batch_host.py (dump) through both entry points - the sanitizer build of the tests.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../parc_amd/csrc/parc_mdm_batch_core.h"

using namespace parc_mdm;

static int done(int rc) { return rc == PARC_MDM_NOTHING ? PARC_OK : rc; }

extern "C" int mdm_heightfields_host(parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids, const float *start_times,
                                     const float *motion_times, const float *grid_x, const float *grid_y, int n_clips, const parc_mdm_clip_t *clips,
                                     const float *pool, int64_t pool_floats, const int32_t *cell_start, int64_t n_cell_start, const int32_t *cells,
                                     int64_t n_cells, int mask_cells, const parc_mdm_draw_t *draws, const parc_mdm_box_t *boxes, const float *noise,
                                     float *hfs, float *center_h, float *pre, int32_t *cell_code) {
    const int rc = check_heightfields(ml, cfg, n, motion_ids, start_times, motion_times, grid_x, grid_y, n_clips, clips, pool, pool_floats, cell_start,
                                      n_cell_start, cells, n_cells, mask_cells, draws, boxes, noise, hfs, center_h);
    if (rc != PARC_OK) return done(rc);
    // exactly the bytes the launch asks LDS for: an access past a plane or the bitmap is an error under the sanitizer
    const size_t XY = (size_t)cfg.dim_x * cfg.dim_y;
    if (hf_lds_bytes(cfg, mask_cells) != 4 * XY * sizeof(float) + (size_t)((mask_cells + 31) / 32) * sizeof(uint32_t)) return PARC_EINVAL;
    for (int s = 0; s < n; ++s) {
        std::vector<float> hf(XY), bmax(XY), bmin(XY), tmp(XY);
        std::vector<uint32_t> bits((size_t)(mask_cells + 31) / 32);
        hf_sample(ml, cfg, s, motion_ids, start_times, motion_times, grid_x, grid_y, n_clips, clips, pool, pool_floats, cell_start, n_cell_start, cells,
                  n_cells, mask_cells, draws, boxes, noise, hfs, center_h, pre, cell_code, 0, 1, hf.data(), bmax.data(), bmin.data(), tmp.data(),
                  bits.data());
    }
    return PARC_OK;
}

extern "C" int mdm_windows_host(parc_char_model_t model, parc_motion_lib_t ml, parc_mdm_cfg_t cfg, int n, const int64_t *motion_ids,
                                const float *start_times, const float *motion_times, const float *center_h, const float *future_time,
                                const float *future_noise, float *root_pos, float *root_rot, float *body_pos, float *joint_rot, float *contacts,
                                float *future_pos, float *future_rot) {
    const int rc = check_windows(model, ml, cfg, n, motion_ids, start_times, motion_times, future_time, future_noise, root_pos, root_rot, body_pos,
                                 joint_rot, contacts, future_pos, future_rot);
    if (rc != PARC_OK) return done(rc);
    std::vector<float> ws((size_t)model.num_bodies * PARC_MDM_FK_FLOATS);
    for (int s = 0; s < n; ++s)
        for (int k = 0; k < cfg.seq_len; ++k)
            window_lane(model, ml, cfg, s, k, motion_ids, start_times, motion_times, center_h, future_time, future_noise, root_pos, root_rot, body_pos,
                        joint_rot, contacts, future_pos, future_rot, ws.data(), 1);
    return PARC_OK;
}

extern "C" int mdm_struct_sizes(int *out) {
    out[0] = (int)sizeof(parc_mdm_cfg_t), out[1] = (int)sizeof(parc_mdm_clip_t), out[2] = (int)sizeof(parc_mdm_draw_t), out[3] = (int)sizeof(parc_mdm_box_t);
    out[4] = (int)sizeof(parc_motion_lib_t), out[5] = (int)sizeof(parc_char_model_t);
    return 6;
}

#ifdef MDM_BATCH_HOST_MAIN
// case file (tests/tools/mdm_batch_host.py: dump): int64 header h[12] = {n, n_clips, pool_floats, n_cell_start, n_cells, mask_cells, total_rows,
// has_draws, has_noise, center_to_windows, 0, 0}, cfg, model, the motion library's struct (its pointers ignored), then num_frames [M],
// start_idx [M], length [M], loop_mode [M], pos_delta [M, 3], frames [total_rows, row_stride], ids [n], starts [n], motion_times [S], grid_x,
// grid_y, clips [M], pool, cell_start, cells, draws [n], boxes [n, max_boxes], noise [n, X, Y], future_time [n], future_noise [n, 3].
// output: root_pos, root_rot, body_pos, joint_rot, contacts, future_pos, future_rot, hfs, center_h.
template <class T>
static std::vector<T> rd(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short case file\n");
        exit(2);
    }
    return v;
}

template <class T>
static void wr(FILE *o, const std::vector<T> &v) {
    if (o && !v.empty()) fwrite(v.data(), sizeof(T), v.size(), o);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    FILE *o = argc > 2 ? fopen(argv[2], "wb") : nullptr;
    if (argc > 2 && !o) return 2;
    const std::vector<int64_t> h = rd<int64_t>(f, 12);
    for (int k = 0; k < 7; ++k)
        if (h[k] < 0 || h[k] > (1 << 24)) return 2;
    const int n = (int)h[0], M = (int)h[1], mask_cells = (int)h[5];
    const int64_t pool_floats = h[2], n_cell_start = h[3], n_cells = h[4], total_rows = h[6];
    const parc_mdm_cfg_t cfg = rd<parc_mdm_cfg_t>(f, 1)[0];
    const parc_char_model_t model = rd<parc_char_model_t>(f, 1)[0];
    parc_motion_lib_t ml = rd<parc_motion_lib_t>(f, 1)[0];
    if (check_cfg(cfg) != PARC_OK || ml.num_motions != M || ml.row_stride < 1 || ml.row_stride > 4096 || model.num_bodies < 1 ||
        model.num_bodies > PARC_MAX_BODIES)
        return 2;
    const int S = cfg.seq_len, X = cfg.dim_x, Y = cfg.dim_y, B = model.num_bodies;
    const std::vector<int32_t> num_frames = rd<int32_t>(f, M), start_idx = rd<int32_t>(f, M);
    const std::vector<float> length = rd<float>(f, M);
    const std::vector<int32_t> loop_mode = rd<int32_t>(f, M);
    const std::vector<float> pos_delta = rd<float>(f, (size_t)M * 3), frames = rd<float>(f, (size_t)total_rows * ml.row_stride);
    for (int m = 0; m < M; ++m)         // the library's own tables are trusted by the kernels, as by every kernel of the package
        if (num_frames[m] < 1 || start_idx[m] < 0 || (int64_t)start_idx[m] + num_frames[m] > total_rows) return 2;
    ml.num_frames = num_frames.data(), ml.start_idx = start_idx.data(), ml.length = length.data(), ml.loop_mode = loop_mode.data();
    ml.pos_delta = pos_delta.data(), ml.frames = frames.data();
    const std::vector<int64_t> ids = rd<int64_t>(f, n);
    const std::vector<float> starts = rd<float>(f, n), motion_times = rd<float>(f, S), grid_x = rd<float>(f, X), grid_y = rd<float>(f, Y);
    const std::vector<parc_mdm_clip_t> clips = rd<parc_mdm_clip_t>(f, M);
    const std::vector<float> pool = rd<float>(f, pool_floats);
    const std::vector<int32_t> cell_start = rd<int32_t>(f, n_cell_start), cells = rd<int32_t>(f, n_cells);
    const std::vector<parc_mdm_draw_t> draws = rd<parc_mdm_draw_t>(f, h[7] ? n : 0);
    const std::vector<parc_mdm_box_t> boxes = rd<parc_mdm_box_t>(f, h[7] ? (size_t)n * cfg.max_boxes : 0);
    const std::vector<float> noise = rd<float>(f, h[8] ? (size_t)n * X * Y : 0);
    const std::vector<float> future_time = rd<float>(f, n), future_noise = rd<float>(f, (size_t)n * 3);
    // exactly-sized vectors: an access one element too far is an error under the sanitizer
    std::vector<float> root_pos((size_t)n * S * 3), root_rot((size_t)n * S * 4), body_pos((size_t)n * S * (B - 1) * 3), joint_rot((size_t)n * S * (B - 1) * 4),
        contacts((size_t)n * S * B), future_pos((size_t)n * 3), future_rot((size_t)n * 4), hfs((size_t)n * X * Y), center_h(n);
    int rc = mdm_heightfields_host(ml, cfg, n, ids.data(), starts.data(), motion_times.data(), grid_x.data(), grid_y.data(), M, clips.data(),
                                   pool.data(), pool_floats, cell_start.data(), n_cell_start, cells.data(), n_cells, mask_cells,
                                   draws.empty() ? nullptr : draws.data(), boxes.empty() ? nullptr : boxes.data(), noise.empty() ? nullptr : noise.data(),
                                   hfs.data(), center_h.data(), nullptr, nullptr);
    if (rc == PARC_OK)
        rc = mdm_windows_host(model, ml, cfg, n, ids.data(), starts.data(), motion_times.data(), h[9] ? center_h.data() : nullptr, future_time.data(),
                              future_noise.data(), root_pos.data(), root_rot.data(), body_pos.data(), joint_rot.data(), contacts.data(),
                              future_pos.data(), future_rot.data());
    wr(o, root_pos), wr(o, root_rot), wr(o, body_pos), wr(o, joint_rot), wr(o, contacts), wr(o, future_pos), wr(o, future_rot), wr(o, hfs), wr(o, center_h);
    fclose(f);
    if (o) fclose(o);
    if (rc != PARC_OK) return 3;
    printf("mdm batch ok %d\n", n);
    return 0;
}
#endif
