#!/usr/bin/env python
"""Time the generator call around the sampling loop: the device path (parc_mdm_gen_encode + parc_mdm_gen_decode, one launch each) against
the torch-op path (the reference's algorithm in torch ops) on the same device, in one process.

Workload: the shipped generation configuration - 2 previous states, S = 16 frames, the 31 x 31 grid at 0.2 m, all five components
(D = 91) - in feature mode: MDMGenIO.encode of previous frames taken from synthetic.make_dataset clips and put on a seeded stepped
terrain, followed by MDMGenIO.decode of a seeded standardised sample, for B = 1, 32 (MDMPathSettings.mdm_batch_size) and 4096 (an env
count).  The sampling loop between the two is not part of the time.  Timed: encode + decode, which includes the Python wrapper (conds
dictionary, flag tensors, output allocation).  Host clock with a synchronise at both ends, warm-up calls first, the two paths
interleaved, every repeat printed and written to profiles/mdm_gen.json with the median, the fastest and the slowest repeat of each and
the largest difference between the two paths' plans.  Without a device the JSON says "not measured".

usage: python tools/bench_mdm_gen.py [--batches 1 32 4096] [--repeats 15]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "mdm_gen.json")
SHIPPED = {"features": {"frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"], "rot_type": "DEFAULT"},
           "sequence_fps": 30, "num_prev_states": 2, "use_pos_loss": False, "use_hf_collision_loss": False, "use_target_loss": False,
           "heightmap": {"horizontal_scale": 0.2, "local_grid": {"num_x_neg": 10, "num_x_pos": 20, "num_y_neg": 15, "num_y_pos": 15}, "max_h": 3.0}}
P, S, D = 2, 16, 91


def build(dev, B, seed):
    import numpy as np
    import torch
    from parc_amd import synthetic
    from parc_amd.anim import kin_char_model
    from parc_amd.diffusion import gen_util
    from parc_amd.util import terrain_util, torch_util
    from parc_amd.util.motion_util import MotionFrames
    rng = np.random.default_rng(seed)
    km = kin_char_model.KinCharModel(dev)
    km.load_char_file(kin_char_model.default_char_file())
    clips = synthetic.make_dataset(num_clips=8, seed=5, frames_range=(60, 90), tile_cells_range=(30, 45))
    frames = [torch.tensor(c["frames"], dtype=torch.float32) for c in clips]
    win = []
    for _ in range(B):
        f = frames[int(rng.integers(len(frames)))]
        t0 = int(rng.integers(0, f.shape[0] - P + 1))
        w = f[t0:t0 + P].clone()
        w[:, :2] += torch.tensor(rng.uniform(5.0, 45.0, size=2), dtype=torch.float32) - w[P - 1, :2].clone()
        win.append(w)
    win = torch.stack(win).to(dev)
    hf = 0.004 * np.arange(256)[:, None] + np.round(rng.uniform(-0.4, 0.4, size=(256, 256)) * 20) / 20
    terrain = terrain_util.SubTerrain.from_arrays(hf.astype(np.float32), (-0.6, -0.6), (0.2, 0.2), device=dev)
    prev = MotionFrames(root_pos=win[..., 0:3].contiguous(), root_rot=torch_util.exp_map_to_quat(win[..., 3:6]), joint_rot=km.dof_to_rot_torch(win[..., 6:34]),
                        contacts=torch.tensor(rng.integers(0, 2, size=(B, P, 15)), dtype=torch.float32, device=dev))
    target = prev.root_pos[:, P - 1, 0:2] + torch.tensor(rng.uniform(-3.0, 3.0, size=(B, 2)), dtype=torch.float32, device=dev)
    cfg = dict(SHIPPED, device=dev)
    mean = torch.tensor(0.2 * rng.standard_normal((S, D)), dtype=torch.float32)
    std = torch.tensor(rng.uniform(0.5, 1.5, size=(S, D)), dtype=torch.float32)
    iod = gen_util.MDMGenIO(cfg, km, mean, std)
    iot = gen_util.MDMGenIO(cfg, km, mean, std, path="torch")
    x = torch.tensor(0.5 * rng.standard_normal((B, S, D)), dtype=torch.float32, device=dev)
    settings = gen_util.MDMGenSettings()
    settings.use_prev_state = torch.tensor(rng.integers(0, 2, size=B).astype(bool), device=dev)
    return iod, iot, target, prev, terrain, settings, x


def measure(batches, repeats):
    import torch
    dev = "cuda:0"
    results = []
    for B in batches:
        iod, iot, target, prev, terrain, settings, x = build(dev, B, 7)

        def call(io):
            conds, ctx = io.encode(target, prev, terrain, settings)
            return io.decode(ctx, x)

        def timed(io):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(io)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        res = {"batch_size": B, "num_prev_states": P, "seq_len": S, "grid": [31, 31], "feat_dim": D, "device_ms": [], "torch_ms": []}
        paths = [("device", iod), ("torch", iot)]
        for _, io in paths:
            for _ in range(3):
                timed(io)
        assert iod.last_path == "device", iod.last_path_reason
        pd, pt = call(iod), call(iot)
        res["max_plan_diff"] = max(float((getattr(pd, k) - getattr(pt, k)).abs().max()) for k in ("root_pos", "root_rot", "joint_rot", "contacts", "frames"))
        for r in range(repeats):
            for key, io in paths:
                res[key + "_ms"].append(round(timed(io), 4))
            print("B={} repeat {} ".format(B, r) + "   ".join("{} {:9.3f} ms".format(k, res[k + "_ms"][-1]) for k, _ in paths), flush=True)
        for key, _ in paths:
            v = res[key + "_ms"]
            res[key + "_median_ms"], res[key + "_min_ms"], res[key + "_max_ms"] = statistics.median(v), min(v), max(v)
        res["torch_over_device"] = round(res["torch_median_ms"] / res["device_median_ms"], 2)
        results.append(res)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 4096])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        doc = {"status": "not measured", "reason": "no device"}
    else:
        doc = {"status": "measured", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
               "what": "MDMGenIO.encode + MDMGenIO.decode in feature mode (the sampling loop between them not included), Python wrapper included, ms",
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
