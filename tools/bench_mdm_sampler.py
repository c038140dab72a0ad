#!/usr/bin/env python
"""Time the generator's training-batch sampler: the batch path (two kernels) against the loop path (the reference's algorithm in torch
ops, one sample at a time), in one process on one device.

Workload: synthetic.make_dataset(num_clips=16, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45)) with the bands and per-frame
cell lists computed by terrain_util.compute_hf_extra_vals, and the sampler keys of the shipped PARC/train_gen_default.yaml (31 x 31 grid,
S frames of 0.5 s at 30 fps, MAXPOOL_AND_BOXES).  Timed: sample_motion_data(num_samples=B) - draws included - for B = 64 (the shipped
batch size) and B = 1024.  Host clock with a synchronise at both ends, warm-up calls first, the two paths interleaved, every repeat
printed and written to profiles/mdm_sampler.json with the median, the fastest and the slowest repeat of each.  The device launches of
one batch (kernels and copies, counted by torch.profiler: of the whole call, and of build_batch alone) are given as well; when the profiler gives nothing the JSON says
"not measured".  Without a device the JSON says "not measured".

usage: python tools/bench_mdm_sampler.py [--batches 64 1024] [--repeats 15] [--loop-repeats 5]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "mdm_sampler.json")
SHIPPED = {"features": {"frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"], "canonicalize_samples": True},
           "autoregressive": True, "sequence_duration": 0.5, "sequence_fps": 30, "num_prev_states": 2, "use_saved_heightmaps": True,
           "use_hf_augmentation": True, "relative_z_style": "RELATIVE_TO_ROOT", "hf_augmentation_mode": "MAXPOOL_AND_BOXES", "max_num_boxes": 4,
           "box_min_len": 2, "box_max_len": 12, "hf_maxpool_chance": 0.15, "hf_max_maxpool_size": 10, "hf_change_height_chance": 0.1,
           "angle_noise_scale": 0.01, "pos_noise_scale": 0.01, "future_pos_noise_scale": 0.05,
           "heightmap": {"horizontal_scale": 0.2, "local_grid": {"num_x_neg": 10, "num_x_pos": 20, "num_y_neg": 15, "num_y_pos": 15}, "max_h": 3.0},
           "future_window_min": 0.4, "future_window_max": 1.5}


def build_samplers(dev):
    import torch
    from parc_amd import synthetic
    from parc_amd.anim import kin_char_model, motion_lib
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    from parc_amd.util import geom_util, terrain_util
    km = kin_char_model.KinCharModel(dev)
    km.load_char_file(kin_char_model.default_char_file())
    clips = synthetic.make_dataset(num_clips=16, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45))
    mlib = motion_lib.MotionLib(clips, km, dev, init_type="clips", contact_info=True)
    body_points = geom_util.get_char_point_samples(km)
    mlib._hf_mask_inds = []
    for c, ter in zip(clips, mlib._terrains):
        frames = torch.tensor(c["frames"], dtype=torch.float32, device=dev)
        mlib._hf_mask_inds.append(terrain_util.compute_hf_extra_vals(frames, ter, km, body_points))
    cfg = dict(SHIPPED, device=dev, char_file=kin_char_model.default_char_file(), motion_lib_file=mlib)
    return ms.MDMHeightfieldContactMotionSampler(cfg, path="batch"), ms.MDMHeightfieldContactMotionSampler(cfg, path="loop")


def count_launches(fn):
    """device activities (kernels, copies, memsets) of one call, or None when the profiler reports none"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n if n > 0 else None
    except Exception as e:       # noqa: BLE001  (a profiler that cannot start is a missing figure, not a failed measurement)
        print("profiler:", e)
        return None


def measure(batches, repeats, loop_repeats):
    import torch
    dev = "cuda:0"
    batch, loop = build_samplers(dev)

    def call(s, B):
        return lambda: s.sample_motion_data(num_samples=B)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    results = []
    for B in batches:
        random.seed(7)
        torch.manual_seed(7)
        fb, fl = call(batch, B), call(loop, B)
        for _ in range(3):
            timed(fb)
        timed(fl)
        assert batch.last_path == "batch" and loop.last_path == "loop"
        res = {"batch_size": B, "seq_len": batch.get_seq_len(), "grid": [batch._grid_dim_x, batch._grid_dim_y], "batch_ms": [], "loop_ms": []}
        n_loop = loop_repeats if B > 64 else repeats
        for r in range(repeats):
            res["batch_ms"].append(round(timed(fb), 4))
            if r < n_loop:
                res["loop_ms"].append(round(timed(fl), 4))
            print("B={} repeat {} batch {:9.3f} ms   loop {}".format(B, r, res["batch_ms"][-1], "{:9.3f} ms".format(res["loop_ms"][-1]) if r < n_loop else "-"),
                  flush=True)
        for key in ("batch", "loop"):
            v = res[key + "_ms"]
            res[key + "_median_ms"], res[key + "_min_ms"], res[key + "_max_ms"] = statistics.median(v), min(v), max(v)
        res["loop_over_batch"] = round(res["loop_median_ms"] / res["batch_median_ms"], 2)
        res["batch_median_below_loop_min"] = bool(res["batch_median_ms"] < res["loop_min_ms"])
        res["batch_launches"] = count_launches(fb)
        ids = batch._mlib.sample_motions(B)
        starts = batch._sample_motion_start_times(ids, batch._sample_seq_time)
        draws = batch.make_draws(ids, starts)
        res["build_batch_launches"] = count_launches(lambda: batch.build_batch(ids, starts, draws))      # the kernels and the draw table's copy alone
        res["loop_launches"] = count_launches(fl) if B <= 64 else None
        results.append(res)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--loop-repeats", type=int, default=5, help="repeats of the loop path at batch sizes above 64")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        doc = {"status": "not measured", "reason": "no device"}
    else:
        doc = {"status": "measured", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "what": "sample_motion_data, draws included, ms",
               "results": measure(args.batches, args.repeats, args.loop_repeats)}
        r64 = [r for r in doc["results"] if r["batch_size"] == 64]
        doc["batch_path_faster_at_64"] = bool(r64[0]["batch_median_below_loop_min"]) if r64 else None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc if doc["status"] != "measured" else {k: v for k, v in doc.items() if k != "results"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
