#!/usr/bin/env python
"""Time one guidance step of the motion generator: the device path (parc_mdm_guide_step, one launch, in place) against the torch-op path
(the reference's algorithm under autograd) on the same device, in one process.

Workload: the shipped generation configuration - S = 16 frames, the 31 x 31 grid at 0.2 m, the dense 304-point set of
get_char_point_samples, all five components, target and terrain terms on with the gen_util defaults (w_target 1, w_hf 10, guidance_str
0.1) - on windows of synthetic.make_dataset clips plus seeded noise over seeded stepped terrain, for B = 1, 64 and 1024.  Timed:
MDMGuidance.guidance_step(x, params, conds), which includes the Python wrapper.  Host clock with a synchronise at both ends, warm-up
calls first, the two paths interleaved, every repeat printed and written to profiles/mdm_guide.json with the median, the fastest and the
slowest repeat of each, torch.cuda.max_memory_allocated above the inputs for both paths, and the largest difference between the two
paths' results.  Where the torch path runs out of memory at a batch size the JSON says so for that size.  Without a device the JSON
says "not measured".

usage: python tools/bench_mdm_guide.py [--batches 1 64 1024] [--repeats 15]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "mdm_guide.json")
SHIPPED = {"features": {"frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"], "rot_type": "DEFAULT"},
           "sequence_fps": 30, "num_prev_states": 2, "use_pos_loss": False, "use_hf_collision_loss": False, "use_target_loss": False,
           "heightmap": {"horizontal_scale": 0.2, "local_grid": {"num_x_neg": 10, "num_x_pos": 20, "num_y_neg": 15, "num_y_pos": 15}, "max_h": 3.0}}
S, D = 16, 91


def build(dev, B, seed):
    import numpy as np
    import torch
    from parc_amd import synthetic
    from parc_amd.anim import kin_char_model
    from parc_amd.diffusion import diffusion_util, mdm_guidance
    from parc_amd.diffusion.diffusion_util import MDMFrameType as T
    from parc_amd.util import geom_util, torch_util
    rng = np.random.default_rng(seed)
    km = kin_char_model.KinCharModel(dev)
    km.load_char_file(kin_char_model.default_char_file())
    clips = synthetic.make_dataset(num_clips=8, seed=5, frames_range=(60, 90), tile_cells_range=(30, 45))
    frames = [torch.tensor(c["frames"], dtype=torch.float32) for c in clips]
    win = []
    for _ in range(B):
        f = frames[int(rng.integers(len(frames)))]
        t0 = int(rng.integers(0, f.shape[0] - S + 1))
        w = f[t0:t0 + S].clone()
        w[:, :2] -= w[1, :2].clone()
        win.append(w)
    win = torch.stack(win).to(dev)
    cfg = dict(SHIPPED, device=dev)
    mean = torch.tensor(0.2 * rng.standard_normal((S, D)), dtype=torch.float32)
    std = torch.tensor(rng.uniform(0.5, 1.5, size=(S, D)), dtype=torch.float32)
    Gd = mdm_guidance.MDMGuidance(cfg, km, mean, std)
    Gt = mdm_guidance.MDMGuidance(cfg, km, mean, std, path="torch")
    true = {T.ROOT_POS: win[..., 0:3].contiguous(), T.ROOT_ROT: torch_util.exp_map_to_quat(win[..., 3:6]), T.JOINT_ROT: km.dof_to_rot_torch(win[..., 6:34]),
            T.CONTACTS: torch.zeros((B, S, 15), device=dev)}
    true[T.JOINT_POS] = km.forward_kinematics_torch(true[T.ROOT_POS], true[T.ROOT_ROT], true[T.JOINT_ROT])[0][..., 1:, :].contiguous()
    x = (Gt._features.assemble_mdm_features(true) + torch.tensor(0.1 * rng.standard_normal((B, S, D)), dtype=torch.float32, device=dev)).contiguous()
    gp = diffusion_util.MDMCustomGuidance()
    gp.verbose = False
    gp.target_xy = torch.tensor(rng.uniform(-2.0, 2.0, size=(B, 1, 2)), dtype=torch.float32, device=dev)
    gp.body_points = geom_util.get_char_point_samples(km)
    conds = {diffusion_util.MDMKeyType.GUIDANCE_PARAMS: gp,
             diffusion_util.MDMKeyType.OBS_KEY: torch.tensor((0.45 + np.round(rng.uniform(-0.5, 0.5, size=(B, 1, 31, 31)), 1)) / 3.0, dtype=torch.float32,
                                                             device=dev)}
    return Gd, Gt, x, gp, conds


def measure(batches, repeats):
    import torch
    dev = "cuda:0"
    results = []
    for B in batches:
        Gd, Gt, x, gp, conds = build(dev, B, 7)

        def step(G):
            xr = x.clone()
            return G.guidance_step(xr, gp, conds), xr

        def timed(G):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(G)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def peak(G):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(G)
            torch.cuda.synchronize()
            return int(torch.cuda.max_memory_allocated() - base)

        res = {"batch_size": B, "seq_len": S, "grid": [31, 31], "points": 304, "device_ms": [], "torch_ms": []}
        paths = [("device", Gd), ("torch", Gt)]
        try:
            for _ in range(3):
                timed(Gt)
        except torch.cuda.OutOfMemoryError as e:
            res["torch"] = "out of memory: " + str(e).split("\n")[0][:200]
            paths = paths[:1]
            torch.cuda.empty_cache()
        for _ in range(3):
            timed(Gd)
        assert Gd.last_path == "device", Gd.last_path_reason
        if len(paths) == 2:
            (td, xd), (tt, xt) = step(Gd), step(Gt)
            unit = (x - xt).abs().reshape(B, -1).max(-1)[0].reshape(-1, 1, 1).clamp(min=1e-30)
            res["max_term_diff_rel"] = float(((td - tt).abs() / tt.abs().clamp(min=1.0)).max())
            res["max_step_diff_rel_to_sample_max"] = float(((xd - xt).abs() / unit).max())
        for r in range(repeats):
            for key, G in paths:
                res[key + "_ms"].append(round(timed(G), 4))
            print("B={} repeat {} ".format(B, r) + "   ".join("{} {:9.3f} ms".format(k, res[k + "_ms"][-1]) for k, _ in paths), flush=True)
        for key, G in paths:
            v = res[key + "_ms"]
            res[key + "_median_ms"], res[key + "_min_ms"], res[key + "_max_ms"] = statistics.median(v), min(v), max(v)
            res[key + "_peak_bytes"] = peak(G)
        if len(paths) == 2:
            res["torch_over_device"] = round(res["torch_median_ms"] / res["device_median_ms"], 2)
        results.append(res)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        doc = {"status": "not measured", "reason": "no device"}
    else:
        doc = {"status": "measured", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "what": "one guidance step (target + terrain terms, dense points) through MDMGuidance.guidance_step, Python wrapper included, ms; "
                       "peak bytes above the inputs",
               "results": measure(args.batches, args.repeats)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc if doc["status"] != "measured" else
                     [{k: v for k, v in r.items() if not k.endswith("_ms") or "median" in k} for r in doc["results"]]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
