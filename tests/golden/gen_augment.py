#!/usr/bin/env python3
"""Generate tests/golden/g31_augment.npz from the REFERENCE's own functions (CPU, torch), called in the order of its
tools/motion_opt/augment_motions.py: rotate_2d_vec, axis_angle_to_quat / quat_multiply / exp_map_to_quat / quat_to_exp_map,
SubTerrain.pad, slice_terrain_around_motion, add_boxes_to_hf_at_xy_points.  (The script itself does not run against its own optimiser -
it calls motion_contact_optimization without w_jerk / max_jerk - so the golden data comes from the functions, not from the script.)

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference on
the path.  The fixture holds
  * four seed clips (37, 5, 2 and 1 frames; terrains 24 x 20, 7 x 9, 1 x 1 and 6 x 5),
  * DESIGNED variants that pin the edge cases (window at the last legal start, headings 0 / +-180 / generic, a zero root exp-map with
    heading 0, a composed quaternion with w < 0, the 1 x 1 terrain, padding 0 and 3, a path that leaves the source grid, all three
    terrain modes, 0 / 1 / 5 overlapping boxes, a box centred outside the grid, slice_terrain false), and
  * two DRAWN runs (HEIGHT_SCALE with its rejection loop, BOXES_ALONG_PATH) whose every draw is made in the script's order from seeded
    generators; the draws the reference makes inside add_boxes_to_hf_at_xy_points are recorded by restoring the generator states and
    replaying the same calls.
Per variant: every draw, the transformed frames (before and after localising), bounds, the output grid's dims, unlocalised and localised
min point, and the final heights.  The generator ASSERTS its preconditions (no rounding tie within 1e-3 in the grid points, no root
angle within 1e-3 of a branch threshold, at most 2 % unsafe cells per variant under the float64 restatement); if a seed violates one,
pick another seed - do not loosen the bound.

usage:  python tests/golden/gen_augment.py            # rewrites tests/golden/g31_augment.npz
        python tests/golden/gen_augment.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import json
import math
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util.terrain_util as terrain_util  # noqa: E402
import util.torch_util as torch_util  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import augment_ref  # noqa: E402  (tests/augment_ref.py: the float64 restatement, for the precondition checks)

FPS = 30
MAX_MOTION_LEN = 0.5        # seconds: 15 frames


def make_clips():
    rng = np.random.default_rng(31)
    clips = []

    def clip(T, X, Y, dxdy, p0, p1, rot_z, zero_rot=False):
        f = np.zeros((T, 34), np.float32)
        s = np.linspace(0.0, 1.0, T) if T > 1 else np.zeros(1)
        f[:, 0] = p0[0] + (p1[0] - p0[0]) * s + 0.05 * rng.standard_normal(T)
        f[:, 1] = p0[1] + (p1[1] - p0[1]) * s + 0.05 * rng.standard_normal(T)
        f[:, 2] = 0.9 + 0.05 * rng.standard_normal(T)
        if not zero_rot:
            f[:, 3:5] = 0.2 * rng.standard_normal((T, 2))
            f[:, 5] = rot_z + 0.2 * rng.standard_normal(T)
        f[:, 6:] = 0.5 * rng.uniform(-1, 1, size=(T, 28))
        con = (rng.uniform(size=(T, 15)) > 0.6).astype(np.float32)
        hf = np.round(rng.uniform(-1.0, 1.0, size=(X, Y)), 2).astype(np.float32)
        mp = np.array([-(X - 1) * dxdy[0] / 2 + 0.07, -(Y - 1) * dxdy[1] / 2 - 0.03], np.float32)
        clips.append(dict(frames=f, contacts=con, hf=hf, min_point=mp, dxdy=np.array(dxdy, np.float32)))

    clip(37, 24, 20, (0.4, 0.4), (-3.0, -2.0), (3.0, 2.2), 0.7)
    clip(5, 7, 9, (0.4, 0.25), (-0.5, -0.4), (0.6, 0.5), 2.6)
    clip(2, 1, 1, (0.5, 0.5), (0.1, -0.2), (0.4, 0.1), -1.1)
    clip(1, 6, 5, (0.4, 0.4), (0.3, 0.2), (0.3, 0.2), 0.0, zero_rot=True)
    return clips


DESIGNED = [
    dict(clip=0, start=21, length=15, heading=37.3, sx=0.9, sy=1.1, pad=3, slice=True, mode="NONE"),
    dict(clip=0, start=0, length=37, heading=0.0, sx=1.0, sy=1.0, pad=0, slice=True, mode="HEIGHT_SCALE", height_scale=1.7),
    dict(clip=0, start=0, length=37, heading=180.0, sx=1.05, sy=0.95, pad=3, slice=True, mode="BOXES_ALONG_PATH", frame_inds=[10, 11, 12, 11, 10], seed=5),
    dict(clip=0, start=0, length=37, heading=-180.0, sx=0.8, sy=1.2, pad=0, slice=True, mode="BOXES_ALONG_PATH", frame_inds=[30], seed=6),
    dict(clip=0, start=0, length=37, heading=-112.6, sx=3.0, sy=2.5, pad=3, slice=True, mode="BOXES_ALONG_PATH", frame_inds=[], seed=7),
    dict(clip=1, start=0, length=5, heading=170.0, sx=1.1, sy=0.9, pad=3, slice=True, mode="HEIGHT_SCALE", height_scale=-0.6),
    dict(clip=2, start=0, length=2, heading=37.3, sx=1.0, sy=1.0, pad=0, slice=True, mode="NONE"),
    dict(clip=2, start=0, length=2, heading=-64.0, sx=1.2, sy=0.7, pad=3, slice=True, mode="BOXES_ALONG_PATH", frame_inds=[1], seed=8),
    dict(clip=3, start=0, length=1, heading=0.0, sx=1.3, sy=0.8, pad=0, slice=True, mode="NONE"),
    dict(clip=0, start=0, length=37, heading=20.0, sx=1.8, sy=1.8, pad=3, slice=False, mode="BOXES_ALONG_PATH", frame_inds=[36, 0], seed=9),
    dict(clip=1, start=0, length=5, heading=-15.0, sx=1.0, sy=1.0, pad=0, slice=False, mode="HEIGHT_SCALE", height_scale=0.4),
]
BOX_CFG = dict(min_len=3.0, max_len=8.0, min_angle=-math.pi, max_angle=math.pi, min_h=-2.0, max_h=2.0)
RUNS = [
    dict(seed=101, cfg=dict(num_new_motions=4, max_motion_len=MAX_MOTION_LEN, min_heading_angle=-180.0, max_heading_angle=180.0, x_scale=[0.8, 1.2],
                            y_scale=[0.9, 1.1], sample_weight_by_length=True, terrain_padding_size=3, slice_terrain=True,
                            terrain_aug_type="HEIGHT_SCALE", min_h_scale=-1.5, max_h_scale=1.5, bad_h_range=[-0.9, 0.9])),
    dict(seed=202, cfg=dict(num_new_motions=4, max_motion_len=MAX_MOTION_LEN, min_heading_angle=-90.0, max_heading_angle=90.0, x_scale=[0.8, 1.2],
                            y_scale=[0.9, 1.1], sample_weight_by_length=False, terrain_padding_size=0, slice_terrain=True,
                            terrain_aug_type="BOXES_ALONG_PATH", min_num_boxes=0, max_num_boxes=5, **BOX_CFG)),
]


def ref_terrain(c):
    X, Y = c["hf"].shape
    t = terrain_util.SubTerrain(x_dim=X, y_dim=Y, dx=float(c["dxdy"][0]), dy=float(c["dxdy"][1]), min_x=float(c["min_point"][0]),
                                min_y=float(c["min_point"][1]), device="cpu")
    t.hf = gg.t(c["hf"])
    return t


def rand_float(lo, hi):
    return random.random() * (hi - lo) + lo


def replay_box_draws(n, cfg, py_state, th_state):
    """the draws add_boxes_to_hf_at_xy_points made, by restoring the generator states and making the same calls"""
    after = (random.getstate(), torch.get_rng_state())
    random.setstate(py_state)
    torch.set_rng_state(th_state)
    lens, angles, hs = [], [], []
    for _ in range(n):
        lens.append((torch.rand(size=(2,), dtype=torch.float32) * (cfg["max_len"] - cfg["min_len"]) + cfg["min_len"]).numpy())
        angles.append(random.random() * (cfg["max_angle"] - cfg["min_angle"]) + cfg["min_angle"])
        hs.append(random.random() * (cfg["max_h"] - cfg["min_h"]) + cfg["min_h"])
    assert random.getstate() == after[0] and torch.equal(torch.get_rng_state(), after[1]), "the replay consumed other draws than the reference"
    return np.array(lens, np.float32).reshape(n, 2), np.array(angles, np.float64), np.array(hs, np.float64)


def ref_variant(clips, v, box_cfg, out, k):
    """one variant through the reference's functions in the script's order (:147-205); v carries every draw made outside
    add_boxes_to_hf_at_xy_points.  Writes its arrays into out under v<k>_*."""
    c = clips[v["clip"]]
    terrain = ref_terrain(c)
    src_frames = gg.t(c["frames"][v["start"]:v["start"] + v["length"]].copy())
    heading_angle = torch.tensor([v["heading"]], dtype=torch.float32)
    heading_angle = heading_angle * torch.pi / 180.0
    src_frames[..., 0:2] = torch_util.rotate_2d_vec(src_frames[..., 0:2], heading_angle)
    z_axis = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32)
    dq = torch_util.axis_angle_to_quat(z_axis, heading_angle)
    composed = torch_util.quat_multiply(dq, torch_util.exp_map_to_quat(src_frames[..., 3:6]))
    src_frames[..., 3:6] = torch_util.quat_to_exp_map(composed)
    src_frames[..., 0] *= v["sx"]
    src_frames[..., 1] *= v["sy"]
    transformed = src_frames.clone()
    bounds = np.array([transformed[:, 0].min().item(), transformed[:, 1].min().item(), transformed[:, 0].max().item(), transformed[:, 1].max().item()],
                      np.float32)
    if v["pad"] > 0:
        terrain.pad(padding_size=v["pad"])
    grid_min = terrain.min_point.clone()
    padded_min, padded_dims = terrain.min_point.clone(), tuple(terrain.hf.shape)
    if v["slice"]:
        padding = terrain.dxdy[0].item() * 2
        lo = torch.tensor([bounds[0], bounds[1]], dtype=torch.float32) - padding
        hi = torch.tensor([bounds[2], bounds[3]], dtype=torch.float32) + padding
        grid_min = terrain.round_point_to_grid_point(lo)          # what slice_terrain_around_motion derives first (:1691)
        for p in (lo, hi):                                       # precondition 1: no rounding tie within 1e-3
            q = (p.double() - terrain.min_point.double()) / terrain.dxdy.double()
            assert torch.all(torch.abs(q - torch.floor(q) - 0.5) > 1e-3), ("rounding tie", k, q)
        terrain, src_frames = terrain_util.slice_terrain_around_motion(src_frames, terrain, padding=padding)
    boxes = (np.zeros((0, 2), np.float32), np.zeros(0), np.zeros(0))
    frame_inds = np.zeros(0, np.int64)
    if v["mode"] == "HEIGHT_SCALE":
        terrain.hf = v["height_scale"] * terrain.hf
    elif v["mode"] == "BOXES_ALONG_PATH":
        frame_inds = np.asarray(v["frame_inds"], np.int64)
        fi = torch.tensor(frame_inds, dtype=torch.int64)
        box_centers = src_frames[fi, 0:2] - terrain.min_point
        box_centers = box_centers / terrain.dxdy
        states = (random.getstate(), torch.get_rng_state())
        terrain_util.add_boxes_to_hf_at_xy_points(box_centers=box_centers, hf=terrain.hf, min_h=box_cfg["min_h"], max_h=box_cfg["max_h"],
                                                  min_len=box_cfg["min_len"], max_len=box_cfg["max_len"], min_angle=box_cfg["min_angle"],
                                                  max_angle=box_cfg["max_angle"])
        boxes = replay_box_draws(len(frame_inds), box_cfg, *states)
        out["v%d_box_centers" % k] = gg.npy(box_centers).astype(np.float32)
    p = "v%d_" % k
    out[p + "heading_rad"] = gg.npy(heading_angle)[0]
    out[p + "heading_terms"] = np.array([torch.cos(heading_angle)[0].item(), torch.sin(heading_angle)[0].item(), dq[0, 2].item(), dq[0, 3].item()],
                                        np.float32)
    out[p + "composed_w_min"] = np.float32(composed[:, 3].min().item())
    out[p + "transformed"] = gg.npy(transformed)
    out[p + "bounds"] = bounds
    out[p + "frames"] = gg.npy(src_frames)
    out[p + "contacts"] = c["contacts"][v["start"]:v["start"] + v["length"]].copy()
    out[p + "dims"] = np.array(terrain.hf.shape, np.int64)
    out[p + "grid_min"] = gg.npy(grid_min).astype(np.float32)
    out[p + "min_point"] = gg.npy(terrain.min_point).astype(np.float32)
    out[p + "hf"] = gg.npy(terrain.hf).astype(np.float32)
    out[p + "frame_inds"] = frame_inds
    out[p + "box_len"], out[p + "box_angle"], out[p + "box_h"] = boxes
    out[p + "padded_min"], out[p + "padded_dims"] = gg.npy(padded_min).astype(np.float32), np.array(padded_dims, np.int64)
    return transformed, bounds


def drawn_run(clips, run):
    """the script's loop (:132-205) for one config, as a generator of variants: every draw made outside add_boxes_to_hf_at_xy_points, in
    the script's order"""
    cfg = run["cfg"]
    random.seed(run["seed"])
    torch.manual_seed(run["seed"])
    lengths = torch.tensor([c["frames"].shape[0] / FPS for c in clips], dtype=torch.float32)
    weights = lengths if cfg["sample_weight_by_length"] else torch.ones_like(lengths)
    file_indices = torch.multinomial(weights, num_samples=cfg["num_new_motions"], replacement=True)
    for n in range(cfg["num_new_motions"]):
        fi = int(file_indices[n])
        T = clips[fi]["frames"].shape[0]
        max_frames = int(round(FPS * cfg["max_motion_len"]))
        start, length = 0, T
        if T > max_frames:
            start, length = random.randint(0, T - max_frames - 1), max_frames
        v = dict(clip=fi, start=start, length=length, heading=rand_float(cfg["min_heading_angle"], cfg["max_heading_angle"]),
                 sx=rand_float(cfg["x_scale"][0], cfg["x_scale"][1]), sy=rand_float(cfg["y_scale"][0], cfg["y_scale"][1]),
                 pad=cfg["terrain_padding_size"], slice=cfg["slice_terrain"], mode=cfg["terrain_aug_type"])
        if v["mode"] == "HEIGHT_SCALE":
            s, tries = rand_float(cfg["min_h_scale"], cfg["max_h_scale"]), 1
            while cfg["bad_h_range"][0] < s and s < cfg["bad_h_range"][1]:
                s, tries = rand_float(cfg["min_h_scale"], cfg["max_h_scale"]), tries + 1
            v["height_scale"], v["tries"] = s, tries
        elif v["mode"] == "BOXES_ALONG_PATH":
            nb = random.randint(cfg["min_num_boxes"], cfg["max_num_boxes"])
            v["frame_inds"] = torch.randint(0, length, size=[nb], dtype=torch.int64).tolist()
        yield v          # the caller runs the reference's functions now: add_boxes_to_hf_at_xy_points draws from the same generators


def main():
    out_dir = tempfile.mkdtemp(prefix="parc_g31_check_") if "--check" in sys.argv else HERE
    clips = make_clips()
    out = {}
    for i, c in enumerate(clips):
        for key in ("frames", "contacts", "hf", "min_point", "dxdy"):
            out["c%d_%s" % (i, key)] = c[key]
    variants, runs_meta = [], []
    for v in DESIGNED:
        v = dict(v)
        if "seed" in v:
            random.seed(v["seed"])
            torch.manual_seed(v["seed"])
        ref_variant(clips, v, BOX_CFG, out, len(variants))
        variants.append(v)
    for run in RUNS:
        first = len(variants)
        for v in drawn_run(clips, run):
            ref_variant(clips, v, run["cfg"], out, len(variants))
            variants.append(v)
        runs_meta.append(dict(seed=run["seed"], cfg=run["cfg"], first=first, count=len(variants) - first))
    meta = dict(fps=FPS, clips=len(clips), variants=variants, runs=runs_meta, box_cfg=BOX_CFG)
    out["meta"] = np.array(json.dumps(meta))

    # preconditions 2 and 3 and the coverage the tests rely on, under the float64 restatement of the reference alone
    z = {k: np.asarray(a) for k, a in out.items()}
    any_w_neg, any_clamped, any_outside, rejected = False, False, False, 0
    for k, v in enumerate(variants):
        fr, info, ter = augment_ref.variant64(z, meta, k)
        for i in info:
            assert i["raw"] == 0.0 or (abs(i["in_angle"]) > 1e-5 + 1e-3 and abs(abs(i["in_angle"]) - math.pi) > 1e-3), ("input angle", k, i)
            assert i["out_len"] == 0.0 or i["out_len"] > 1e-5 + 1e-3, ("output angle", k, i)
            assert abs(i["w"]) > 1e-3, ("w near the sign flip", k, i)
            any_w_neg |= i["w"] < 0
        share = ter["unsafe"].mean()
        assert share <= 0.02, ("unsafe share", k, share)
        good = ~ter["unsafe"]
        assert np.allclose(ter["hf"][good], z["v%d_hf" % k][good], rtol=0, atol=2e-6), ("float64 heights", k)
        c = clips[v["clip"]]
        lo = z["v%d_padded_min" % k]
        hi = lo + (z["v%d_padded_dims" % k] - 1) * c["dxdy"]
        b = z["v%d_bounds" % k]
        any_clamped |= bool(v["slice"] and (b[0] < lo[0] - 1 or b[1] < lo[1] - 1 or b[2] > hi[0] + 1 or b[3] > hi[1] + 1))
        if v["mode"] == "BOXES_ALONG_PATH" and len(v["frame_inds"]):
            bc = z["v%d_box_centers" % k]
            # a box centred outside the grid that still reaches into it
            any_outside |= bool((np.any(bc < -0.5) or np.any(bc > z["v%d_dims" % k] - 0.5)) and not v["slice"] and
                                np.any(z["v%d_hf" % k] != np.pad(c["hf"], v["pad"])))
        rejected += v.get("tries", 1) - 1
    assert any_w_neg and any_clamped and any_outside and rejected > 0, (any_w_neg, any_clamped, any_outside, rejected)
    assert np.all(z["v8_frames"][:, 3:6] == 0.0) and not np.any(np.signbit(z["v8_frames"][:, 3:6])), "zero exp-map, heading 0"
    print("e-bar = %.6e" % augment_ref.measure_ebar(z, meta))

    path = os.path.join(out_dir, "g31_augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(variants), "variants")
    if "--check" in sys.argv:
        old = np.load(os.path.join(HERE, "g31_augment.npz"))
        new = np.load(path)
        assert sorted(old.files) == sorted(new.files)
        for key in old.files:
            assert np.array_equal(old[key], new[key], equal_nan=True) if old[key].dtype.kind == "f" else np.array_equal(old[key], new[key]), key
        print("check OK")


if __name__ == "__main__":
    main()
