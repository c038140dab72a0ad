#!/usr/bin/env python3
"""Generate tests/golden/g32_mdm_sampler.npz from the REFERENCE's own MDMHeightfieldContactMotionSampler (CPU, torch) over a small
dataset written to a temporary directory.

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference on
the path.  The dataset holds four clips with reference SubTerrains, bands (hf_maxmin) and per-frame cell lists (hf_mask_inds):
  0  CLAMP, 40 frames, 30 fps, on 20 x 16 at 0.4 m        1  WRAP, 25 frames, 20 fps, on 12 x 14 at (0.4, 0.25) m
  2  CLAMP, exactly 15 frames, on 10 x 10 at 0.4 m         3  CLAMP, 20 frames, on a 1 x 1 terrain
  4  CLAMP, 20 frames, root rotation zero, on 24 x 24 at 0.4 m (only the 31 x 31 case uses it: under a generic heading about four of its
     1922 grid lookups lie within 1e-3 cells of a rounding tie, with heading 0 they share two fractional parts)
with some frames whose cell list is empty.  The fixture holds
  * DESIGNED cases: each augmentation mode x both z styles on a 9 x 7 local grid (a transposed axis shows), a 1 x 1 local grid with
    S = 1 and one previous state, the shipped 31 x 31 grid once, start times on and between frames (each the
    first of its nominal value + whole frames that meets the preconditions below), windows whose mask frames run past
    the clip's end, local grids partly outside the terrain, pool radius 0 and a radius >= the grid, all six pool orders, all pools on
    and all off, the height change on and off, 0, 1 and max_num_boxes boxes, boxes longer than the grid, future times past the end of
    the CLAMP and of the WRAP clip.  The draws _box_hf_augmentation makes itself come from a script put in place of the sampler
    module's `random`; the draws add_boxes_to_hf2 makes (torch.rand, random.random) come from seeded generators.
  * two DRAWN runs through the trainer's calling sequence (sample_motions, _sample_motion_start_times, sample_motion_data) with seeded
    generators.
A case's seed is the first one, counting up from the listed one, under which the preconditions hold; the fixture records it.
Every draw is recorded by restoring the generator states and replaying the reference's calls in its order; the replay must leave both
generators in the state the reference left them.  Per case: every draw, the five motion tensors, hfs, center_h, the target, and the
pre-augmentation heights and band (from an extra call of get_hfs_from_data that draws nothing).

The generator ASSERTS its preconditions under the float64 restatement (tests/mdm_sampler_ref.py): no grid lookup within 1e-3 cells of a
rounding tie, no start frame within 1e-3 of one, no reference heading within 1e-3 of the atan2 branch, at most 2 % of a sample's cells
within 1e-4 cells of a box edge.  If a seed violates one, pick another seed - do not loosen the bound.

usage:  python tests/golden/gen_mdm_sampler.py            # rewrites tests/golden/g32_mdm_sampler.npz
        python tests/golden/gen_mdm_sampler.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import json
import math
import os
import pickle
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

import anim.motion_lib as motion_lib  # noqa: E402
import util.terrain_util as terrain_util  # noqa: E402
import diffusion.mdm_heightfield_contact_motion_sampler as ref_sampler  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import mdm_sampler_ref as msr  # noqa: E402  (tests/mdm_sampler_ref.py: the float64 restatement)

S15 = 15
POOL_KINDS = {"maxpool_hf": 0, "maxpool_hf_1d_x": 1, "maxpool_hf_1d_y": 2}


# ------------------------------------------------------------------------------------------------------------------- dataset
def make_clips():
    rng = np.random.default_rng(32)
    clips = []

    def clip(T, fps, loop, X, Y, dxdy, p0, p1, rot_z, zero_rot=False):
        f = np.zeros((T, 34), np.float32)
        s = np.linspace(0.0, 1.0, T)
        tt = np.arange(T) / fps
        f[:, 0] = p0[0] + (p1[0] - p0[0]) * s + 0.03 * np.sin(5.0 * tt)
        f[:, 1] = p0[1] + (p1[1] - p0[1]) * s + 0.03 * np.cos(4.0 * tt)
        f[:, 2] = 0.9 + 0.05 * np.sin(7.0 * tt)
        # rotations differ from frame to frame by tenths of a radian: between nearly equal frames the reference's fp32 slerp loses four
        # digits (sqrt(1 - c * c) at c near 1), which would set the unit of every bound of the tests
        f[:, 3:5] = 0.2 * rng.standard_normal((T, 2))
        f[:, 5] = rot_z + 0.3 * np.sin(2.5 * tt) + 0.2 * rng.standard_normal(T)
        if zero_rot:
            f[:, 3:6] = 0.0
        f[:, 6:] = np.where(np.arange(T) % 2 == 0, 1.0, -1.0)[:, None] * rng.uniform(0.25, 0.5, size=(T, 28))      # a hinge turns >= 0.5 rad per frame
        con = (rng.uniform(size=(T, 15)) > 0.6).astype(np.float32)
        hf = np.round(rng.uniform(-1.0, 1.0, size=(X, Y)), 2).astype(np.float32)
        band = np.stack([hf + rng.uniform(0.05, 0.6, size=(X, Y)), hf - rng.uniform(0.05, 0.6, size=(X, Y))], -1).astype(np.float32)
        mp = np.array([-(X - 1) * dxdy[0] / 2 + 0.07, -(Y - 1) * dxdy[1] / 2 - 0.03], np.float32)
        # the cells under and around the root of each frame; every seventh frame has none
        lists = []
        for t in range(T):
            if t % 7 == 3:
                lists.append(np.zeros((0, 2), np.int64))
                continue
            ci = int(np.clip(np.rint((f[t, 0] - mp[0]) / dxdy[0]), 0, X - 1)), int(np.clip(np.rint((f[t, 1] - mp[1]) / dxdy[1]), 0, Y - 1))
            cells = {(min(max(ci[0] + a, 0), X - 1), min(max(ci[1] + b, 0), Y - 1)) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a + b + t) % 3 != 0}
            lists.append(np.array(sorted(cells), np.int64).reshape(-1, 2))
        clips.append(dict(frames=f, contacts=con, fps=fps, loop=loop, hf=hf, band=band, min_point=mp, dxdy=np.array(dxdy, np.float32), lists=lists))

    clip(40, 30, "CLAMP", 20, 16, (0.4, 0.4), (-2.6, -1.9), (2.7, 2.1), 0.7)
    clip(25, 20, "WRAP", 12, 14, (0.4, 0.25), (-1.4, -1.0), (1.5, 0.8), 2.4)
    clip(S15, 30, "CLAMP", 10, 10, (0.4, 0.4), (-0.9, 0.5), (0.8, -0.6), -1.3)
    clip(20, 30, "CLAMP", 1, 1, (0.5, 0.5), (0.1, -0.2), (0.6, 0.3), 0.2)
    # heading exactly 0 for the 31 x 31 grid: under a generic heading about four of its 1922 lookups lie within 1e-3 cells of a tie
    clip(20, 30, "CLAMP", 24, 24, (0.4, 0.4), (-1.1, -0.7), (0.9, 0.8), 0.0, zero_rot=True)
    return clips


def write_dataset(clips, out_dir):
    entries = []
    for i, c in enumerate(clips):
        X, Y = c["hf"].shape
        ter = terrain_util.SubTerrain(x_dim=X, y_dim=Y, dx=float(c["dxdy"][0]), dy=float(c["dxdy"][1]), min_x=float(c["min_point"][0]),
                                      min_y=float(c["min_point"][1]), device="cpu")
        ter.hf = gg.t(c["hf"])
        ter.hf_maxmin = gg.t(c["band"])
        path = os.path.join(out_dir, "clip%d.pkl" % i)
        data = dict(frames=c["frames"], contacts=c["contacts"], fps=c["fps"], loop_mode=c["loop"], terrain=ter,
                    hf_mask_inds=[torch.tensor(a, dtype=torch.int64) for a in c["lists"]])
        with open(path, "wb") as f:
            pickle.dump(data, f)
        entries.append(dict(file=path, weight=0.0 if i == 4 else 1.0))
    ypath = os.path.join(out_dir, "dataset.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(dict(motions=entries), f)
    return ypath


# ------------------------------------------------------------------------------------------------------------------- configurations
def make_cfg(mode="MAXPOOL_AND_BOXES", z_style="RELATIVE_TO_ROOT", grid=(3, 5, 2, 4), dx=0.4, fps=30, S=S15, num_prev=2, max_h=3.0, max_num_boxes=4,
             box_min_len=2, box_max_len=12, maxpool_chance=0.15, max_maxpool=10, change_chance=0.1, fmin=0.4, fmax=1.5, noise_scale=0.05,
             autoregressive=True):
    return dict(mode=mode, z_style=z_style, grid=list(grid), dx=dx, fps=fps, S=S, num_prev=num_prev, max_h=max_h, max_num_boxes=max_num_boxes,
                box_min_len=box_min_len, box_max_len=box_max_len, maxpool_chance=maxpool_chance, max_maxpool=max_maxpool, change_chance=change_chance,
                fmin=fmin, fmax=fmax, noise_scale=noise_scale, autoregressive=autoregressive)


def sampler_cfg(c, mlib):
    """the reference's config keys (:34-121) from a case config"""
    return {"device": "cpu", "char_file": gg.CHAR_FILE, "motion_lib_file": mlib,
            "features": {"canonicalize_samples": True, "frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"]},
            "sequence_fps": c["fps"], "autoregressive": c["autoregressive"], "sequence_duration": (c["S"] - 0.5) / c["fps"],
            "num_prev_states": c["num_prev"], "future_pos_noise_scale": c["noise_scale"], "use_saved_heightmaps": True,
            "relative_z_style": c["z_style"], "hf_augmentation_mode": c["mode"],
            "heightmap": {"horizontal_scale": c["dx"], "max_h": c["max_h"],
                          "local_grid": {"num_x_neg": c["grid"][0], "num_x_pos": c["grid"][1], "num_y_neg": c["grid"][2], "num_y_pos": c["grid"][3]}},
            "use_hf_augmentation": True, "max_num_boxes": c["max_num_boxes"], "box_min_len": c["box_min_len"], "box_max_len": c["box_max_len"],
            "hf_maxpool_chance": c["maxpool_chance"], "hf_max_maxpool_size": c["max_maxpool"], "hf_change_height_chance": c["change_chance"],
            "angle_noise_scale": 0.01, "pos_noise_scale": 0.01, "future_window_min": c["fmin"], "future_window_max": c["fmax"]}


def P(change=None, rolls=(False, False, False), order=(0, 1, 2), radii=(), nboxes=0):
    """one sample's script: change = None or the height draw in [0, 1); order = the pool kinds after the shuffle"""
    return dict(change=change, rolls=list(rolls), order=list(order), radii=list(radii), nboxes=nboxes)


ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
IDS6 = [0, 1, 2, 3, 0, 1]
# on a frame, between frames, mask frames past the clip's end (0: 40 frames at 30 fps; 1: 25 frames at 20 fps, indexed at 30 fps), a local
# grid partly outside the terrain (every sample of clip 2 and 3, and the ends of the others)
STARTS6 = [10 / 30, 0.413, 0.0, 2.2 / 30, 36.4 / 30, 17 / 30]
SCRIPT6 = [P(change=0.8, rolls=(True, True, True), order=ORDERS[0], radii=(0, 1, 10), nboxes=0),
           P(rolls=(True, True, True), order=ORDERS[1], radii=(2, 0, 1), nboxes=1),
           P(rolls=(True, False, True), order=ORDERS[2], radii=(1, 3), nboxes=4),
           P(change=0.1, rolls=(False, True, False), order=ORDERS[3], radii=(10,), nboxes=2),
           P(rolls=(False, False, False), order=ORDERS[4], nboxes=3),
           P(rolls=(True, True, False), order=ORDERS[5], radii=(9, 2), nboxes=4)]

DESIGNED = []
for _mode in ("MAXPOOL_AND_BOXES", "NOISE", "NONE"):
    for _z in ("RELATIVE_TO_ROOT", "RELATIVE_TO_ROOT_FLOOR"):
        DESIGNED.append(dict(cfg=make_cfg(mode=_mode, z_style=_z), ids=IDS6, starts=STARTS6, script=SCRIPT6 if _mode == "MAXPOOL_AND_BOXES" else None,
                             seed=11 + len(DESIGNED)))
DESIGNED += [
    # all pools on, in each of the six orders
    dict(cfg=make_cfg(), ids=IDS6, starts=STARTS6, script=[P(rolls=(True, True, True), order=o, radii=(1, 2, 1), nboxes=0) for o in ORDERS], seed=20),
    # a 1 x 1 local grid, S = 1, one previous state
    dict(cfg=make_cfg(grid=(0, 0, 0, 0), S=1, num_prev=1, z_style="RELATIVE_TO_ROOT_FLOOR"), ids=[0, 1, 3], starts=[0.5, 0.31, 0.1],
         script=[P(rolls=(True, True, True), order=ORDERS[3], radii=(0, 5, 1), nboxes=1), P(change=0.4, nboxes=4), P(nboxes=0)], seed=21),
    # the shipped grid and augmentation values
    dict(cfg=make_cfg(grid=(10, 20, 15, 15), dx=0.2), ids=[4, 4], starts=[0.2, 0.41],
         script=[P(rolls=(True, False, True), order=ORDERS[4], radii=(10, 4), nboxes=4), P(change=0.9, rolls=(True, True, True), order=ORDERS[1],
                                                                                          radii=(3, 0, 7), nboxes=2)], seed=22),
    # boxes longer than the grid
    dict(cfg=make_cfg(box_min_len=12, box_max_len=20, z_style="RELATIVE_TO_ROOT_FLOOR"), ids=[0, 2], starts=[0.6, 0.0],
         script=[P(nboxes=1), P(nboxes=4)], seed=23),
    # future times past the clip's end (CLAMP and WRAP), one previous state
    dict(cfg=make_cfg(mode="NONE", fmin=1.0, fmax=2.0, num_prev=1), ids=[0, 1, 0, 1], starts=[1.1, 1.0, 0.06, 1.13], script=None, seed=24),
]
# clip 4 is not drawn (weight 0 in the dataset file)
RUNS = [dict(seed=301, n=8, cfg=make_cfg(maxpool_chance=0.5, change_chance=0.3)),
        dict(seed=302, n=6, cfg=make_cfg(mode="NOISE", z_style="RELATIVE_TO_ROOT_FLOOR"))]


# ------------------------------------------------------------------------------------------------------------------- scripted `random`
class ScriptedRandom:
    """stands in for the sampler module's `random`: the draws _box_hf_augmentation makes itself, from a per-sample script"""

    def __init__(self, script):
        self.q = []
        for p in script:
            self.q.append(("random", 0.0 if p["change"] is not None else 0.999))
            if p["change"] is not None:
                self.q.append(("random", p["change"]))
            self.q += [("random", 0.0 if r else 0.999) for r in p["rolls"]]
            self.q.append(("shuffle", p["order"]))
            assert len(p["radii"]) == sum(p["rolls"])
            self.q += [("randint", r) for r in p["radii"]]
            self.q.append(("randint", p["nboxes"]))

    def _pop(self, kind):
        k, v = self.q.pop(0)
        assert k == kind, (k, kind)
        return v

    def random(self):
        return self._pop("random")

    def randint(self, a, b):
        v = self._pop("randint")
        assert a <= v <= b, (a, v, b)
        return v

    def shuffle(self, lst):
        order = self._pop("shuffle")
        by_kind = {POOL_KINDS[f.__name__]: f for f in lst}
        lst[:] = [by_kind[k] for k in order]


def replay(c, level_rng, n, dims, lengths, starts):
    """the reference's draws of one sample_motion_data call, made again in its order (:365-411, terrain_util.py:881-909, :199, :210)"""
    X, Y = dims
    max_h, min_h = c["max_h"], -c["max_h"]
    B = c["max_num_boxes"]
    d = dict(change=np.zeros(n, np.int32), new_h=np.zeros(n, np.float32), pool_kind=np.full((n, 3), -1, np.int32), pool_r=np.zeros((n, 3), np.int32),
             nboxes=np.zeros(n, np.int32), boxes=np.zeros((n, B, 6), np.float32), noise=np.zeros((n, X, Y), np.float32))
    for s in range(n):
        if c["mode"] == "NOISE":
            d["noise"][s] = (torch.rand(size=(X, Y), dtype=torch.float32) * (max_h - min_h) + min_h).numpy()
        elif c["mode"] == "MAXPOOL_AND_BOXES":
            if level_rng.random() < c["change_chance"]:
                d["change"][s] = 1
                d["new_h"][s] = np.float32(level_rng.random() * (max_h - min_h) + min_h)
            use = [level_rng.random() < c["maxpool_chance"] for _ in range(3)]

            def maxpool_hf():
                pass

            def maxpool_hf_1d_x():
                pass

            def maxpool_hf_1d_y():
                pass
            fns = [maxpool_hf, maxpool_hf_1d_x, maxpool_hf_1d_y]
            level_rng.shuffle(fns)
            for q in range(3):
                if use[q]:
                    d["pool_r"][s, q] = level_rng.randint(0, c["max_maxpool"])
                    d["pool_kind"][s, q] = POOL_KINDS[fns[q].__name__]
            nb = level_rng.randint(0, B)
            d["nboxes"][s] = nb
            for b in range(nb):
                center = torch.rand(size=(2,), dtype=torch.float32) * torch.tensor([X, Y], dtype=torch.float32)
                length = torch.rand(size=(2,), dtype=torch.float32) * (c["box_max_len"] - c["box_min_len"]) + c["box_min_len"]
                angle = random.random() * (2.0 * torch.pi - 0.0) + 0.0
                h = random.random() * (max_h - min_h) + min_h
                d["boxes"][s, b] = [center[0].item(), center[1].item(), length[0].item(), length[1].item(), np.float32(angle), np.float32(h)]
    st = torch.tensor(starts, dtype=torch.float32)
    remaining = torch.clamp_max(lengths - st, c["fmax"] - c["fmin"])
    d["future_time"] = (torch.rand_like(st) * remaining + st + c["fmin"]).numpy()
    d["future_noise"] = (c["noise_scale"] * torch.randn(size=(n, 3), dtype=torch.float32)).numpy()
    return d


def sample_ok(info, start, fps):
    """the per-sample preconditions that do not depend on a seed; None or the reason"""
    if not info["tie"] > 1e-3:
        return ("grid rounding tie", info["tie"])
    if not abs(abs(info["heading"]) - math.pi) > 1e-3:
        return ("heading at the atan2 branch", info["heading"])
    fr = float(np.float32(start) / np.float32(1.0 / fps))
    if not abs(fr - math.floor(fr) - 0.5) > 1e-3:
        return ("start frame rounding tie", fr)
    return None


def preconditions(z, meta, k, seen):
    """case k under the float64 restatement alone: None, or the first violated precondition; `seen` collects the coverage"""
    model, tables = msr.model_tables(z), msr.clip_tables(z, meta)
    cs = meta["cases"][k]
    o64, infos = msr.case64(z, meta, k, model, tables)
    a = msr.case_arrays(z, k)
    X, Y = len(a["grid_x"]), len(a["grid_y"])
    for s, info in enumerate(infos):
        why = sample_ok(info, a["starts"][s], cs["cfg"]["fps"])
        if why is not None:
            return why + (k, s)
        share = o64["unsafe"][s].mean()
        if share > msr.EDGE_SHARE:
            return ("cells near a box edge", share, k, s)
        if seen is None:
            continue
        seen["outside"] |= info["outside"]
        seen["window_past_end"] |= info["window_past_end"]
        seen["clamp_past" if int(a["ids"][s]) != 1 else "wrap_past"] |= info["future_past_end"]
        if cs["cfg"]["mode"] == "MAXPOOL_AND_BOXES":
            kinds, rs = a["pool_kind"][s], a["pool_r"][s]
            used = kinds >= 0
            seen["all_on"] |= bool(used.all())
            seen["all_off"] |= bool(not used.any())
            seen["r0"] |= bool(np.any(used & (rs == 0)))
            seen["rbig"] |= bool(np.any(used & (rs >= max(X, Y))))
            if used.all():
                seen["orders"].add(tuple(int(v) for v in kinds))
            seen["change"].add(int(a["change"][s]))
            seen["nboxes"].add(int(a["nboxes"][s]))
    good = ~o64["unsafe"]
    assert np.allclose(o64["hfs"][good], a["hfs"][good], rtol=0, atol=1e-5), ("float64 heights", k)
    assert np.allclose(o64["pre"], a["pre"], rtol=0, atol=1e-5), ("float64 pre-augmentation planes", k)
    return None


def resolve_starts(mlib, case, tables_z):
    """each nominal start time moved by whole frames (0, +1, -1, +2, ...) inside its clip to the first that meets the preconditions"""
    c = case["cfg"]
    s = ref_sampler.MDMHeightfieldContactMotionSampler(sampler_cfg(c, mlib))
    tables = msr.clip_tables(tables_z, dict(clips=mlib.num_motions()))
    cfg = dict(dim_x=s._grid_dim_x, dim_y=s._grid_dim_y, seq_len=s._seq_len, dt=np.float32(1.0 / c["fps"]), num_x_neg=c["grid"][0], num_y_neg=c["grid"][2],
               grid_x=gg.npy(s._generic_heightmap[:, 0, 0]), grid_y=gg.npy(s._generic_heightmap[0, :, 1]), z_style=0, mode=2, max_h=c["max_h"],
               min_h=-c["max_h"])
    mt = gg.npy(s._motion_times).astype(np.float32)
    starts = []
    for cid, nominal in zip(case["ids"], case["starts"]):
        clip = tables[cid]
        for j in range(0, 80):
            st = np.float32(nominal + ((j + 1) // 2) * (1 if j % 2 else -1) / c["fps"])
            if st < 0 or st > clip["length"]:
                continue
            ref_pos, ref_q, _ = msr.lookup(clip, float(np.float32(st + mt[s._ref_frame_idx])))
            info = {}
            msr.heightfield(cfg, clip, float(st), ref_pos, ref_q[0], None, 0, info)
            if sample_ok(info, st, c["fps"]) is None:
                starts.append(float(st))
                break
        else:
            raise AssertionError(("no start near", nominal, "meets the preconditions on clip", cid))
    return starts


def run_case(mlib, case, out, k, drawn):
    c = case["cfg"]
    s = ref_sampler.MDMHeightfieldContactMotionSampler(sampler_cfg(c, mlib))
    assert s._seq_len == c["S"], (s._seq_len, c["S"])
    MT = ref_sampler.MDMFrameType
    if drawn:
        random.seed(case["seed"])
        torch.manual_seed(case["seed"])
        ids = s._mlib.sample_motions(case["n"])                                               # the trainer's calling sequence (mdm.py:776-796)
        starts = s._sample_motion_start_times(ids, s._sample_seq_time)
    else:
        ids = torch.tensor(case["ids"], dtype=torch.int64)
        starts = torch.tensor(case["starts"], dtype=torch.float32)
        random.seed(case["seed"])
        torch.manual_seed(case["seed"])
    n = ids.shape[0]
    dims = (s._grid_dim_x, s._grid_dim_y)

    # the pre-augmentation heights and band and center_h: get_hfs_from_data with an augmentation that records and draws nothing
    idx = torch.round(starts / s._timestep).to(dtype=torch.int64).unsqueeze(-1) + torch.arange(0, s._seq_len, dtype=torch.int64).unsqueeze(0)
    rp, rr = s._extract_motion_data(ids, starts, s._motion_times, s._seq_len)[0:2]
    cpos, crot = rp[:, s._ref_frame_idx].clone(), rr[:, s._ref_frame_idx].clone()
    rec = []
    s._hf_augmentation_mode = ref_sampler.HFAugmentationMode.NOISE
    s._noise_hf_augmentation = lambda hf, mm: rec.append(torch.stack([hf.clone(), mm[..., 0].clone(), mm[..., 1].clone()]))
    _, center_h = s.get_hfs_from_data(ids, cpos, crot, cpos[:, 2].clone(), idx)
    del s._noise_hf_augmentation
    s._hf_augmentation_mode = ref_sampler.HFAugmentationMode[c["mode"]]

    states = (random.getstate(), torch.get_rng_state())
    script = None if drawn else case["script"]
    if script is not None:
        ref_sampler.random = ScriptedRandom(script)
    try:
        motion, hfs, target = s.sample_motion_data(motion_ids=ids, motion_start_times=starts)
    finally:
        if script is not None:
            assert not ref_sampler.random.q, "the script was not consumed"
        ref_sampler.random = random
    after = (random.getstate(), torch.get_rng_state())
    random.setstate(states[0])
    torch.set_rng_state(states[1])
    d = replay(c, ScriptedRandom(script) if script is not None else random, n, dims, s._mlib.get_motion_length(ids), gg.npy(starts))
    assert random.getstate() == after[0] and torch.equal(torch.get_rng_state(), after[1]), "the replay consumed other draws than the reference"

    p = "k%d_" % k
    out[p + "ids"], out[p + "starts"] = gg.npy(ids).astype(np.int64), gg.npy(starts).astype(np.float32)
    out[p + "motion_times"] = gg.npy(s._motion_times).astype(np.float32)
    out[p + "grid_x"] = gg.npy(s._generic_heightmap[:, 0, 0]).astype(np.float32)
    out[p + "grid_y"] = gg.npy(s._generic_heightmap[0, :, 1]).astype(np.float32)
    for key, v in d.items():
        out[p + key] = v
    out[p + "root_pos"], out[p + "root_rot"] = gg.npy(motion[MT.ROOT_POS]), gg.npy(motion[MT.ROOT_ROT])
    out[p + "body_pos"], out[p + "joint_rot"], out[p + "contacts"] = gg.npy(motion[MT.JOINT_POS]), gg.npy(motion[MT.JOINT_ROT]), gg.npy(motion[MT.CONTACTS])
    out[p + "hfs"], out[p + "center_h"] = gg.npy(hfs), gg.npy(center_h)
    out[p + "future_pos"], out[p + "future_rot"] = gg.npy(target.future_pos), gg.npy(target.future_rot)
    out[p + "pre"] = gg.npy(torch.stack(rec))
    cfg = dict(c, ref_idx=s._ref_frame_idx)
    return dict(cfg=cfg, drawn=bool(drawn), seed=case["seed"], n=int(n))


def main():
    check = "--check" in sys.argv
    out_dir = tempfile.mkdtemp(prefix="parc_g32_check_") if check else HERE
    data_dir = tempfile.mkdtemp(prefix="parc_g32_data_")
    clips = make_clips()
    ypath = write_dataset(clips, data_dir)
    km = gg.load_char()
    mlib = motion_lib.MotionLib(motion_input=ypath, kin_char_model=km, device="cpu", contact_info=True)
    out = {}
    out["model_parent"] = gg.npy(km._parent_indices).astype(np.int32)
    out["model_local_translation"] = gg.npy(km._local_translation).astype(np.float32)
    out["model_local_rotation"] = gg.npy(km._local_rotation).astype(np.float32)
    for i, c in enumerate(clips):
        a, b = int(mlib._motion_start_idx[i]), int(mlib._motion_start_idx[i]) + int(mlib._motion_num_frames[i])
        pre = "c%d_" % i
        out[pre + "frames"], out[pre + "contacts"] = c["frames"], gg.npy(mlib._frame_contacts[a:b])
        out[pre + "root_pos"], out[pre + "root_rot"] = gg.npy(mlib._frame_root_pos[a:b]), gg.npy(mlib._frame_root_rot[a:b])
        out[pre + "joint_rot"] = gg.npy(mlib._frame_joint_rot[a:b])
        out[pre + "fps"], out[pre + "loop"] = np.float32(c["fps"]), np.int32(int(mlib._motion_loop_modes[i]))
        out[pre + "length"], out[pre + "pos_delta"] = gg.npy(mlib._motion_lengths[i]), gg.npy(mlib._motion_root_pos_delta[i])
        out[pre + "hf"], out[pre + "hf_maxmin"], out[pre + "min_point"], out[pre + "dxdy"] = c["hf"], c["band"], c["min_point"], c["dxdy"]
        Y = c["hf"].shape[1]
        out[pre + "cell_start"] = np.concatenate([[0], np.cumsum([len(a_) for a_ in c["lists"]])]).astype(np.int32)
        out[pre + "cells"] = np.concatenate([a_[:, 0] * Y + a_[:, 1] for a_ in c["lists"]]).astype(np.int32)
    tables_z = {k: np.asarray(a_) for k, a_ in out.items()}
    cases = []
    seen = dict(outside=False, window_past_end=False, clamp_past=False, wrap_past=False, orders=set(), r0=False, rbig=False, all_on=False, all_off=False,
                change=set(), nboxes=set())
    for case, drawn in [(c, False) for c in DESIGNED] + [(r, True) for r in RUNS]:
        k = len(cases)
        case = dict(case)
        if not drawn:
            case["starts"] = resolve_starts(mlib, case, tables_z)
        for attempt in range(400):
            tmp = {}
            info = run_case(mlib, dict(case, seed=case["seed"] + attempt), tmp, k, drawn)
            z = dict(tables_z, **{key: np.asarray(v) for key, v in tmp.items()})
            why = preconditions(z, dict(clips=len(clips), cases=cases + [info]), k, None)
            if why is None:
                break
            assert drawn or why[0] == "cells near a box edge", why     # a designed case's other preconditions do not depend on its seed
        else:
            raise AssertionError(("no seed meets the preconditions", k, why))
        preconditions(z, dict(clips=len(clips), cases=cases + [info]), k, seen)
        out.update(tmp)
        cases.append(info)
    meta = dict(clips=len(clips), cases=cases, S15=S15)
    out["meta"] = np.array(json.dumps(meta))
    z = {k: np.asarray(a_) for k, a_ in out.items()}
    assert seen["outside"] and seen["window_past_end"] and seen["clamp_past"] and seen["wrap_past"] and seen["r0"] and seen["rbig"], seen
    assert seen["all_on"] and seen["all_off"] and seen["change"] == {0, 1} and {0, 1, 4} <= seen["nboxes"] and len(seen["orders"]) == 6, seen
    print("e-bar = %.6e" % msr.measure_ebar(z, meta))

    path = os.path.join(out_dir, "g32_mdm_sampler.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cases), "cases")
    if check:
        old = np.load(os.path.join(HERE, "g32_mdm_sampler.npz"))
        new = np.load(path)
        assert sorted(old.files) == sorted(new.files)
        diffs = 0
        for key in old.files:
            same = np.array_equal(old[key], new[key], equal_nan=True) if old[key].dtype.kind == "f" else np.array_equal(old[key], new[key])
            if not same:
                diffs += 1
                print("differs:", key)
        print("check: %d differences" % diffs)
        assert diffs == 0


if __name__ == "__main__":
    main()
