#!/usr/bin/env python3
"""Microseconds per motion-scoring call: 32 candidates x 300 frames x the humanoid's default sample points on a 128 x 128 field (run on
the GPU box).  The fused call (parc_motion_score, two launches) against the chain the other kernels offer - parc_forward_kinematics ->
parc_body_points_world -> 2 x parc_points_hf_sdf -> torch reductions, batched over the candidates, not looped.  HIP events around a
window of WINDOW calls, after a warm-up window, REPEATS times per configuration, the two configurations interleaved; every repeat is
printed and written to profiles/motion_score.json.  Without a device the JSON says "not measured"."""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

OUT = os.path.join(REPO, "profiles", "motion_score.json")
B, F, X, Y, WINDOW, REPEATS = 32, 300, 128, 128, 100, 5
shape = {"candidates": B, "frames": F, "field": [X, Y], "window": WINDOW, "repeats": REPEATS}
if not torch.cuda.is_available():
    with open(OUT, "w") as f:
        json.dump({"tool": "tools/bench_motion_score.py", "status": "not measured", "reason": "no device", **shape}, f, indent=1)
        f.write("\n")
    raise SystemExit("bench_motion_score.py measures on the GPU: no device found ({} says: not measured)".format(OUT))

from parc_amd.anim.kin_char_model import KinCharModel
from parc_amd.assets import humanoid_spec
from parc_amd.tools.procgen import mdm_path
from parc_amd.util import geom_util, terrain_util
from parc_amd.util.motion_util import MotionFrames

dev = "cuda:0"
torch.manual_seed(0)
km = KinCharModel(dev)
km.load_char_file(humanoid_spec.write_mjcf())
pts = geom_util.get_char_point_samples(km)
ter = terrain_util.SubTerrain("bench", X, Y, 0.4, 0.4, -25.6, -25.6, device=dev)
ter.hf[:] = 0.3 * torch.rand((X, Y), device=dev).round()          # boxes of 30 cm
J = km.get_num_joints() - 1
t = torch.linspace(0.0, 10.0, F, device=dev)
root_pos = torch.stack([2.0 * t.unsqueeze(0) + torch.randn((B, 1), device=dev), torch.randn((B, 1), device=dev) + 0.0 * t, 0.9 + 0.05 * torch.sin(3.0 * t).expand(B, F)], dim=-1)
dof = 0.4 * torch.sin(t.reshape(1, F, 1) * torch.rand((B, 1, km.get_dof_size()), device=dev) * 4.0)
root_rot = torch.zeros((B, F, 4), device=dev)
root_rot[..., 3] = 1.0
mf = MotionFrames(root_pos=root_pos.contiguous(), root_rot=root_rot, joint_rot=km.dof_to_rot(dof), contacts=(torch.rand((B, F, J + 1), device=dev) > 0.7).float())
scorer = mdm_path.MotionScorer(km, pts, ter)
points = terrain_util.BodyPoints(pts, dev)
grid = terrain_util.HfGrid(ter.hf, ter.dxdy, dev)
hf, mp = ter.hf.unsqueeze(0).expand(B, -1, -1), ter.min_point.unsqueeze(0).expand(B, -1)
base_z = scorer.base_z
seg = [(points.start[b], points.start[b + 1]) for b in range(points.num_bodies)]


def fused():
    return scorer.score(mf, 0.1, 0.1).total_loss


def chain():
    bp, br = km.forward_kinematics(mf.root_pos, mf.root_rot, mf.joint_rot)
    world = points.world(bp, br).reshape(B, F * points.num_points, 3)
    d_in = terrain_util.points_hf_sdf(world, hf, mp, ter.dxdy, base_z=base_z, inverted=True, grid=grid).clamp(max=0.0)
    d_out = terrain_util.points_hf_sdf(world, hf, mp, ter.dxdy, base_z=base_z, inverted=False, grid=grid).clamp(min=0.0).reshape(B, F, -1)
    pen = 0.1 * (-d_in).sum(dim=-1)
    con = torch.stack([d_out[..., a:b].min(dim=-1)[0] for a, b in seg], dim=-1)
    return pen + 0.1 * (con * mf.contacts).sum(dim=(1, 2))


a, b = fused(), chain()
torch.cuda.synchronize()
agree = float((a - b).abs().max() / b.abs().max())
configs = {"fused": fused, "chain": chain}
times = {k: [] for k in configs}
for rep in range(REPEATS + 1):          # round 0 is the warm-up
    for k, fn in configs.items():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(WINDOW):
            fn()
        e.record()
        torch.cuda.synchronize()
        if rep > 0:
            times[k].append(round(s.elapsed_time(e) * 1e3 / WINDOW, 2))
res = {"tool": "tools/bench_motion_score.py", "status": "measured", "device": torch.cuda.get_device_name(0), **shape, "points": points.num_points,
       "max_relative_difference_of_the_totals": agree, "us_per_call": times,
       "median": {k: sorted(v)[len(v) // 2] for k, v in times.items()}, "min": {k: min(v) for k, v in times.items()}}
res["fused_median_below_fastest_chain_repeat"] = res["median"]["fused"] < res["min"]["chain"]
for k, v in times.items():
    print(json.dumps({"config": k, "us_per_call": v, "median": res["median"][k], "min": res["min"][k]}))
print(json.dumps({k: res[k] for k in ("max_relative_difference_of_the_totals", "fused_median_below_fastest_chain_repeat")}))
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
