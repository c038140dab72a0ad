#!/usr/bin/env python
"""Time the batched dataset augmentation against the per-variant loop.

Seeds: synthetic.make_dataset(num_clips=8, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45)).  For V = 1, 8, 32 variants
(BOXES_ALONG_PATH, padding 3, sliced terrains, whole clips, 300 iterations), drawn once by augment_motions.draw_variants:
  (i)  preparation alone: augment_motions.prepare_variants (three launches, one host read)                        -- "prep_batch"
       against the per-variant torch statement of the same steps, kept below (prepare_one)                        -- "prep_loop"
  (ii) the whole call: prepare_variants + motion_contact_optimization_batch in groups of opt_batch_size = V       -- "all_batch"
       against a loop of prepare_one + motion_contact_optimization                                                -- "all_loop" (the yardstick)
Host clock with a synchronise at both ends, a warm-up call first, 5 repeats per configuration with the configurations interleaved.
Every repeat is printed and written to profiles/augment.json with the verdict on the expectation "at V = 8 and V = 32 the batched median
of (ii) lies below the loop's fastest repeat".  Without a device the JSON says "not measured".

Each V runs in a child process of its own under a time limit (usage: python tools/bench_augment.py [--v 1 8 32] [--iters 300]); a child
that fails or runs out of time ends the run - nothing more is started on the device after it.
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "augment.json")
CFG = dict(max_motion_len=10.0, min_heading_angle=-180.0, max_heading_angle=180.0, x_scale=[0.9, 1.1], y_scale=[0.9, 1.1], sample_weight_by_length=True,
           terrain_padding_size=3, slice_terrain=True, terrain_aug_type="BOXES_ALONG_PATH", min_num_boxes=2, max_num_boxes=6, min_len=3.0, max_len=8.0,
           min_angle=-3.14159, max_angle=3.14159, min_h=-0.5, max_h=0.5, step_size=0.001, w_root_pos=1.0, w_root_rot=10.0, w_joint_rot=1.0,
           w_smoothness=10.0, w_penetration=1000.0, w_contact=1000.0, w_sliding=10.0, w_jerk=1000.0, max_jerk=1000.0, use_wandb=False)


def prepare_one(spec, clip, device, pad):
    """The per-variant torch statement of the preparation, on the device, step by step as the reference's loop does it
    (augment_motions.py:147-205 with util/terrain_util.py:223-240, :1675-1740, :930-969): -> (frames, contacts, SubTerrain)"""
    import torch
    from parc_amd.util import terrain_util, torch_util
    terrain = clip.terrain.torch_copy()
    terrain.set_device(device)
    frames = clip.frames[spec.start:spec.start + spec.length].clone().to(device)
    contacts = clip.contacts[spec.start:spec.start + spec.length].clone().to(device)
    heading = torch.tensor([spec.heading], dtype=torch.float32, device=device) * torch.pi / 180.0
    frames[..., 0:2] = torch_util.rotate_2d_vec(frames[..., 0:2], heading)
    z_axis = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=device)
    dq = torch_util.axis_angle_to_quat(z_axis, heading)
    frames[..., 3:6] = torch_util.quat_to_exp_map(torch_util.quat_mul(dq.expand(frames.shape[0], 4), torch_util.exp_map_to_quat(frames[..., 3:6])))
    frames[..., 0] *= spec.sx
    frames[..., 1] *= spec.sy
    if pad > 0:
        terrain.pad(pad)
    # slice_terrain_around_motion, localize=True
    padding = terrain.dxdy[0].item() * 2
    lo = torch.tensor([torch.min(frames[..., 0]).item(), torch.min(frames[..., 1]).item()], dtype=torch.float32, device=device) - padding
    hi = torch.tensor([torch.max(frames[..., 0]).item(), torch.max(frames[..., 1]).item()], dtype=torch.float32, device=device) + padding
    gmin, gmax = terrain.round_point_to_grid_point(lo), terrain.round_point_to_grid_point(hi)
    xs = torch.arange(gmin[0], gmax[0] + terrain.dxdy[0], step=terrain.dxdy[0], device=device)
    ys = torch.arange(gmin[1], gmax[1] + terrain.dxdy[1], step=terrain.dxdy[1], device=device)
    gx, gy = torch.meshgrid(xs, ys, indexing="ij")
    g = terrain.get_grid_index(torch.stack([gx, gy], dim=-1))
    canon_xy = frames[0, 0:2].clone()
    frames[..., 0:2] -= canon_xy
    out = terrain_util.SubTerrain("terrain", int(g.shape[0]), int(g.shape[1]), terrain.dxdy[0].item(), terrain.dxdy[1].item(),
                                  gmin[0].item() - canon_xy[0].item(), gmin[1].item() - canon_xy[1].item(), device=device)
    out.hf = terrain.hf[g[..., 0], g[..., 1]].clone()
    out.hf_mask = terrain.hf_mask[g[..., 0], g[..., 1]].clone()
    out.hf_maxmin = terrain.hf_maxmin[g[..., 0], g[..., 1]].clone()
    canon_z = out.get_hf_val_from_points(frames[0, 0:2])
    frames[:, 2] -= canon_z
    out.hf = out.hf - canon_z
    # add_boxes_to_hf_at_xy_points with the drawn boxes, in torch ops
    centers = (frames[spec.frame_inds.to(device), 0:2] - out.min_point) / out.dxdy
    X, Y = int(out.hf.shape[0]), int(out.hf.shape[1])
    ii, jj = torch.meshgrid(torch.arange(X, device=device), torch.arange(Y, device=device), indexing="ij")
    ij = torch.stack([ii, jj], dim=-1).to(torch.float32)
    for b in range(int(spec.frame_inds.shape[0])):
        c = centers[b]
        turned = torch_util.rotate_2d_vec(ij - c, spec.box_angle[b] * torch.ones_like(ij[..., 0])) + c
        half = spec.box_len[b].to(device) / 2
        inside = (turned[..., 0] < c[0] + half[0]) & (turned[..., 0] > c[0] - half[0]) & (turned[..., 1] < c[1] + half[1]) & (turned[..., 1] > c[1] - half[1])
        out.hf[ii, jj] = torch.where(inside, torch.ones_like(out.hf) * spec.box_h[b], out.hf[ii, jj])
    return frames, contacts, out


def measure(V, iters, repeats):
    """one V in this process -> dict"""
    import torch
    from parc_amd import synthetic
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.tools.motion_opt import augment_motions as am
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.util import geom_util, terrain_util
    dev = "cuda:0"
    km = KinCharModel(dev)
    km.load_char_file(humanoid_spec.write_mjcf())
    body_points = geom_util.get_char_point_samples(km)
    clips = [am.SeedClip(c["name"], c["frames"], c["contacts"], terrain_util.SubTerrain.from_arrays(c["hf"], c["min_point"], c["dxdy"], device="cpu"), 30)
             for c in synthetic.make_dataset(num_clips=8, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45))]
    cfg = dict(CFG, num_new_motions=V, num_iters=iters, opt_batch_size=V, device=dev)
    random.seed(5)
    torch.manual_seed(5)
    specs = am.draw_variants(cfg, clips)
    pad = cfg["terrain_padding_size"]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def prep_batch():
        return am.prepare_variants(specs, clips, dev, pad, True)

    def prep_loop():
        return [prepare_one(s, clips[s.file_index], dev, pad) for s in specs]

    def all_batch():
        return am.optimize_prepared(prep_batch(), cfg, km, body_points, None, verbose=False)

    def all_loop():
        out = []
        for s in specs:
            f, c, t = prepare_one(s, clips[s.file_index], dev, pad)
            out.append(mo.motion_contact_optimization(src_frames=f, contacts=c, body_points=body_points, terrain=t, char_model=km, num_iters=iters,
                                                      step_size=cfg["step_size"], body_constraints=None, max_jerk=cfg["max_jerk"], exp_name=None,
                                                      use_wandb=False, log_file=None, use_graph=True, verbose=False, **am.loss_weights(cfg)))
        return out

    def prep_batch_terrains():          # ... with the SubTerrain objects the files need (a second host read)
        return prep_batch().terrains

    # warm-up calls; also recorded: how far the two preparations agree (the loop evaluates sin / cos of the heading on the device, so its
    # xy may differ in the last bit and a window may then round to another size)
    _, pb = timed(prep_batch)
    _, pl = timed(prep_loop)
    ters = pb.terrains
    same_shape = [tuple(ters[k].hf.shape) == tuple(pl[k][2].hf.shape) for k in range(V)]
    agree = [float((ters[k].hf == pl[k][2].hf).float().mean()) for k in range(V) if same_shape[k]]
    frame_diff = max(float((pb.frames[k] - pl[k][0]).abs().max()) for k in range(V))
    timed(all_batch)
    timed(all_loop)
    res = {"V": V, "iters": iters, "frames": [s.length for s in specs], "cells": [int(x * y) for x, y in pb.tplan.shapes],
           "boxes": [int(s.frame_inds.shape[0]) for s in specs], "same_shape": sum(same_shape), "heights_equal_share_min": min(agree) if agree else None,
           "frames_max_abs_diff": frame_diff, "prep_batch_ms": [], "prep_batch_terrains_ms": [], "prep_loop_ms": [], "all_batch_ms": [], "all_loop_ms": []}
    for r in range(repeats):          # the configurations interleaved
        for key, fn in (("prep_batch_ms", prep_batch), ("prep_batch_terrains_ms", prep_batch_terrains), ("prep_loop_ms", prep_loop),
                        ("all_batch_ms", all_batch), ("all_loop_ms", all_loop)):
            ms, _ = timed(fn)
            res[key].append(round(ms, 3))
            print("V={} repeat {} {:14s} {:10.3f} ms".format(V, r, key, ms), flush=True)
    for kind in ("prep", "all"):
        b, lo = res[kind + "_batch_ms"], res[kind + "_loop_ms"]
        res[kind + "_batch_median_ms"], res[kind + "_loop_median_ms"], res[kind + "_loop_min_ms"] = statistics.median(b), statistics.median(lo), min(lo)
    res["prep_batch_terrains_median_ms"] = statistics.median(res["prep_batch_terrains_ms"])
    res["all_batch_median_below_loop_min"] = bool(res["all_batch_median_ms"] < res["all_loop_min_ms"])
    res["prep_batch_median_below_loop_min"] = bool(res["prep_batch_median_ms"] < res["prep_loop_min_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", type=int, default=None, help="internal: measure this V in this process and print the JSON result")
    ap.add_argument("--limit", type=int, default=420, help="time limit of one child, seconds")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(measure(args.child, args.iters, args.repeats)), flush=True)
        return 0
    import torch
    if not torch.cuda.is_available():
        doc = {"status": "not measured", "reason": "no device"}
    else:
        doc = {"status": "measured", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "results": []}
        for V in args.v:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(V), "--iters", str(args.iters),
                   "--repeats", str(args.repeats)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(p.stdout)
            line = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stderr[-4000:])
                doc["status"] = "incomplete"
                doc["failed"] = {"V": V, "returncode": p.returncode}
                break           # nothing more is started on the device after a failure
            doc["results"].append(json.loads(line[0][len("RESULT "):]))
        if doc["status"] == "measured":
            big = [r for r in doc["results"] if r["V"] in (8, 32)]
            doc["expectation"] = "at V = 8 and V = 32 the batched median of the whole call lies below the loop's fastest repeat"
            doc["verdict"] = ("met" if all(r["all_batch_median_below_loop_min"] for r in big) else "NOT met") if big else "not tested (no V of 8 or 32)"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "results"}))
    return 0 if doc["status"] != "incomplete" else 1


if __name__ == "__main__":
    sys.exit(main())
