"""Dataset augmentation before the first tracker is trained: a few seed clips -> many variants, built and optimised in batches.

Mirror of the reference's ``tools/motion_opt/augment_motions.py``.  Every variant is a window of a seed clip (at most ``max_motion_len``
seconds), turned by a random heading and stretched in x and y; the terrain is padded, cut out around the result and both are
re-centred on the first frame; the heights are then scaled (``HEIGHT_SCALE``) or stamped with random rotated boxes under the path
(``BOXES_ALONG_PATH``); the contact optimiser runs on the result, which is written as ``<name>_augNNN.pkl`` with its log.

Config keys are the reference's (:45-122): motions_yaml_path, device, char_model, num_new_motions, output_folder_path, num_iters, step_size,
w_root_pos, w_root_rot, w_joint_rot, w_smoothness, w_penetration, w_contact, w_sliding, use_wandb, max_motion_len, max_heading_angle,
min_heading_angle, terrain_padding_size, slice_terrain, x_scale, y_scale, sample_weight_by_length, terrain_aug_type and its sub-keys
(min_len, max_len, min_angle, max_angle, min_num_boxes, max_num_boxes, min_h, max_h | min_h_scale, max_h_scale, bad_h_range),
char_point_samples{...}; plus ``opt_batch_size`` (variants per descent, default 8), ``w_jerk`` (default 0.0) and ``max_jerk``
(default 1000.0).  NOTE: the reference script as shipped calls ``motion_contact_optimization`` WITHOUT ``w_jerk`` and ``max_jerk`` and so
does not run against its own optimiser (:211-229 against motion_optimization.py:404); the two keys here fill that gap, and the defaults
switch the jerk term off.

What differs is the mechanics.  The reference handles one variant at a time: some thirty small torch ops, half a dozen ``.item()``
reads and then a launch-bound descent.  Here
  * ``draw_variants`` makes ALL draws first, on the host, from Python's ``random`` and torch's CPU generator in exactly the order the
    reference's loop consumes them (so the same seeds give the variants of the reference's functions on the CPU);
  * ``prepare_variants`` builds all variants' frames and terrains on the device in three launches (parc_augment_frames, _terrains,
    _localize: include/parc_augment.h) with one host read - the xy bounds that size the terrain windows;
  * ``augment_dataset`` descends them ``opt_batch_size`` at a time through ``motion_contact_optimization_batch``, whose terrain table
    reads the heights from the pool the kernels wrote.

usage:  python -m parc_amd.tools.motion_opt.augment_motions --config platform_aug.yaml
"""
import ctypes
import enum
import os
import random
import sys
import time

import numpy as np
import torch
import yaml

from ... import _hip_augment, _hip_moopt
from ...util import terrain_util, torch_util


class TerrainAugmentationType(enum.Enum):
    HEIGHT_SCALE = 0
    BOXES_ALONG_PATH = 1
    NONE = 2


_MODE = {TerrainAugmentationType.NONE: _hip_augment.MODE_NONE, TerrainAugmentationType.HEIGHT_SCALE: _hip_augment.MODE_HEIGHT_SCALE,
         TerrainAugmentationType.BOXES_ALONG_PATH: _hip_augment.MODE_BOXES_ALONG_PATH}
DESCENT_BASE_Z = -10.0      # base_z of the optimiser's terrain queries


def rand_float(f_min, f_max):
    return random.random() * (f_max - f_min) + f_min


class SeedClip:
    """One seed motion: frames [T, 34] and contacts [T, C] (float32 CPU tensors), its SubTerrain (CPU) and fps."""

    def __init__(self, name, frames, contacts, terrain, fps):
        self.name = name
        self.frames = torch.as_tensor(np.asarray(frames, np.float32)).contiguous()
        self.contacts = torch.as_tensor(np.asarray(contacts, np.float32)).contiguous()
        assert self.frames.dim() == 2 and self.frames.shape[1] == _hip_augment.FRAME_DIM and self.contacts.shape[0] == self.frames.shape[0]
        terrain = terrain.torch_copy()
        terrain.set_device("cpu")
        self.terrain = terrain
        self.fps = fps


class VariantSpec:
    """Every draw of one variant (draw_variants): the seed clip, the window, heading (degrees), scales, and the terrain mode with its
    height scale or boxes (frame_inds int64 [n], box_len float32 [n, 2], angles and heights as the Python floats that were drawn)."""

    def __init__(self, file_index, name, start, length, heading, sx, sy, mode, height_scale=None, frame_inds=None, box_len=None, box_angle=None, box_h=None):
        self.file_index, self.name, self.start, self.length = int(file_index), name, int(start), int(length)
        self.heading, self.sx, self.sy, self.mode = float(heading), float(sx), float(sy), mode
        self.height_scale = height_scale
        self.frame_inds = frame_inds if frame_inds is not None else torch.zeros(0, dtype=torch.int64)
        self.box_len = box_len if box_len is not None else torch.zeros((0, 2), dtype=torch.float32)
        self.box_angle = list(box_angle) if box_angle is not None else []
        self.box_h = list(box_h) if box_h is not None else []


# ---------------------------------------------------------------------------------------------------------------------
# all draws, on the host, in the reference's order
# ---------------------------------------------------------------------------------------------------------------------
def draw_variants(cfg, clips):
    """-> list of VariantSpec, cfg["num_new_motions"] long.  Order of the draws (reference :136-205): torch.multinomial over the seeds up
    front; then per variant random.randint for the start frame (only when the clip is longer than max_motion_len), random.random for the
    heading, the x scale and the y scale; then either the height scale with its rejection loop, or random.randint for the box count,
    torch.randint for the boxes' frame indices and per box torch.rand(2), random.random (angle), random.random (height)."""
    aug = TerrainAugmentationType[cfg["terrain_aug_type"]]
    lengths = torch.tensor([c.frames.shape[0] / c.fps for c in clips], dtype=torch.float32)
    weights = lengths if cfg["sample_weight_by_length"] else torch.ones_like(lengths)
    n_new = int(cfg["num_new_motions"])
    file_indices = torch.multinomial(weights, num_samples=n_new, replacement=True).tolist() if n_new > 0 else []
    count = [0] * len(clips)
    specs = []
    for fi in file_indices:
        clip = clips[fi]
        count[fi] += 1
        T = int(clip.frames.shape[0])
        max_frames = int(round(clip.fps * cfg["max_motion_len"]))
        start, length = 0, T
        if T > max_frames:
            start, length = random.randint(0, T - max_frames - 1), max_frames
        heading = rand_float(cfg["min_heading_angle"], cfg["max_heading_angle"])
        sx = rand_float(cfg["x_scale"][0], cfg["x_scale"][1])
        sy = rand_float(cfg["y_scale"][0], cfg["y_scale"][1])
        kw = {}
        if aug == TerrainAugmentationType.HEIGHT_SCALE:
            bad = cfg["bad_h_range"]
            s = rand_float(cfg["min_h_scale"], cfg["max_h_scale"])
            while bad[0] < s and s < bad[1]:
                s = rand_float(cfg["min_h_scale"], cfg["max_h_scale"])
            kw["height_scale"] = s
        elif aug == TerrainAugmentationType.BOXES_ALONG_PATH:
            n_boxes = random.randint(cfg["min_num_boxes"], cfg["max_num_boxes"])
            kw["frame_inds"] = torch.randint(0, length, size=[n_boxes], dtype=torch.int64)
            lens, angles, hs = [], [], []
            for _ in range(n_boxes):
                lens.append(torch.rand(size=(2,), dtype=torch.float32) * (cfg["max_len"] - cfg["min_len"]) + cfg["min_len"])
                angles.append(rand_float(cfg["min_angle"], cfg["max_angle"]))
                hs.append(rand_float(cfg["min_h"], cfg["max_h"]))
            kw.update(box_len=torch.stack(lens) if lens else None, box_angle=angles, box_h=hs)
        specs.append(VariantSpec(fi, clip.name + "_aug" + str(count[fi]).zfill(3), start, length, heading, sx, sy, aug, **kw))
    return specs


# ---------------------------------------------------------------------------------------------------------------------
# host-side plans of the three launches (pure host code: numpy, ctypes and the few CPU torch ops whose rounding the reference fixes)
# ---------------------------------------------------------------------------------------------------------------------
def _heading_terms(heading_deg):
    """(cos, sin, qz, qw) of a heading in degrees, by the torch ops the reference applies to its one-element tensor (:164-168)"""
    h = torch.tensor([heading_deg], dtype=torch.float32) * torch.pi / 180.0
    q = torch_util.axis_angle_to_quat(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32), h)
    return float(torch.cos(h)[0]), float(torch.sin(h)[0]), float(q[0, 2]), float(q[0, 3])


class FramesPlan:
    """parc_augment_frames for `specs`: the seed clips packed along the frame axis and one parc_augment_frames_t per variant"""

    def __init__(self, specs, clips):
        self.V = len(specs)
        self.src_frames = np.concatenate([c.frames.numpy() for c in clips], axis=0) if clips else np.zeros((0, _hip_augment.FRAME_DIM), np.float32)
        self.contact_width = int(clips[0].contacts.shape[1]) if clips else 0
        self.src_contacts = np.concatenate([c.contacts.numpy() for c in clips], axis=0) if clips else np.zeros((0, 0), np.float32)
        src_off = np.concatenate([[0], np.cumsum([c.frames.shape[0] for c in clips])]).astype(np.int64)
        assert src_off[-1] < 2 ** 31
        self.table = (_hip_augment.AugFramesS * max(self.V, 1))()
        self.out_off, off = [], 0
        for k, s in enumerate(specs):
            e = self.table[k]
            e.src_off, e.src_len = int(src_off[s.file_index]), int(clips[s.file_index].frames.shape[0])
            e.start, e.length, e.out_off = s.start, s.length, off
            e.cos_h, e.sin_h, e.qz, e.qw = _heading_terms(s.heading)
            e.sx, e.sy = s.sx, s.sy          # (a Python float times a float32 tensor multiplies by the float32 of that float)
            self.out_off.append(off)
            off += s.length
        assert off < 2 ** 31
        self.n_out = off
        self.lengths = [s.length for s in specs]


def _padded_origin(terrain, pad):
    """min point of `terrain` after SubTerrain.pad(pad) (float32 tensor [2])"""
    return terrain.min_point - terrain.dxdy * pad if pad > 0 else terrain.min_point.clone()


class TerrainPlan:
    """parc_augment_terrains / _localize for `specs` once the xy bounds [V, 4] (min x, min y, max x, max y) of their transformed frames
    are known: the sources' table and pool, per variant the output grid - its x and y points are the reference's
    torch.arange(min_grid_point, max_grid_point + dx, step=dx) (util/terrain_util.py:1700-1701), so the shapes are the reference's - and
    the pool that holds, per variant, [heights | HfGrid xs | HfGrid ys] (the layout of terrain_util.HfTable), followed by every
    variant's x and y points."""

    def __init__(self, specs, clips, bounds, frames_plan, padding_size, slice_terrain):
        V = self.V = len(specs)
        bounds = np.asarray(bounds, np.float32).reshape(V, 4)
        for k in range(V):
            if not np.all(np.isfinite(bounds[k])):
                raise ValueError("variant {} ({}): the transformed frames are not finite (xy bounds {})".format(k, specs[k].name, bounds[k].tolist()))
        pad = int(padding_size)
        # sources
        self.src_table = (_hip_augment.AugTerrainS * max(len(clips), 1))()
        parts, off = [], 0
        for k, c in enumerate(clips):
            t = c.terrain
            X, Y = int(t.hf.shape[0]), int(t.hf.shape[1])
            e = self.src_table[k]
            e.off_hf, e.off_x, e.off_y, e.dim_x, e.dim_y = off, 0, 0, X, Y
            e.min_x, e.min_y, e.dx, e.dy = float(t.min_point[0]), float(t.min_point[1]), float(t.dxdy[0]), float(t.dxdy[1])
            parts.append(t.hf.numpy().astype(np.float32).reshape(-1))
            off += X * Y
        self.src_pool = np.concatenate(parts) if parts else np.zeros(0, np.float32)
        # outputs
        self.out_table = (_hip_augment.AugTerrainS * max(V, 1))()
        self.vars = (_hip_augment.AugVariantS * max(V, 1))()
        self.hf_entries = (_hip_moopt.MooptTerrainS * max(V, 1))()
        n_boxes = sum(int(s.frame_inds.shape[0]) for s in specs)
        self.boxes = (_hip_augment.AugBoxS * max(n_boxes, 1))()
        self.n_boxes = n_boxes
        self.shapes, self.grid_min, self.dxdy, grids = [], [], [], []
        out_parts, point_parts, out_off, pt_off, box_off, cells = [], [], 0, 0, 0, [0]
        for k, s in enumerate(specs):
            t = clips[s.file_index].terrain
            origin = _padded_origin(t, pad)
            if slice_terrain:
                padding = t.dxdy[0].item() * 2
                lo = torch.tensor([bounds[k, 0], bounds[k, 1]], dtype=torch.float32) - padding
                hi = torch.tensor([bounds[k, 2], bounds[k, 3]], dtype=torch.float32) + padding
                gmin = torch.round((lo - origin) / t.dxdy) * t.dxdy + origin           # round_point_to_grid_point of the padded terrain
                gmax = torch.round((hi - origin) / t.dxdy) * t.dxdy + origin
                xs = torch.arange(gmin[0], gmax[0] + t.dxdy[0], step=t.dxdy[0])
                ys = torch.arange(gmin[1], gmax[1] + t.dxdy[1], step=t.dxdy[1])
                X, Y = int(xs.shape[0]), int(ys.shape[0])
            else:
                gmin = origin
                X, Y = int(t.hf.shape[0]) + 2 * pad, int(t.hf.shape[1]) + 2 * pad
                xs, ys = torch.zeros(0), torch.zeros(0)
            assert X >= 1 and Y >= 1
            grid = terrain_util.HfGrid(torch.empty((X, Y)), t.dxdy, "cpu")
            o = self.out_table[k]
            o.off_hf, o.off_x, o.off_y, o.dim_x, o.dim_y = out_off, pt_off, pt_off + int(xs.shape[0]), X, Y
            o.min_x, o.min_y, o.dx, o.dy = float(gmin[0]), float(gmin[1]), float(t.dxdy[0]), float(t.dxdy[1])
            h = self.hf_entries[k]
            h.off_hf, h.off_x, h.off_y, h.dim_x, h.dim_y = out_off, out_off + X * Y, out_off + X * Y + X, X, Y
            h.ox, h.oy = o.min_x, o.min_y                   # parc_augment_localize moves them by the first frame's xy
            h.half_x, h.half_y = grid.half
            h.base_z = DESCENT_BASE_Z
            a = self.vars[k]
            a.src, a.pad, a.mode, a.slice = s.file_index, pad, _MODE[s.mode], 1 if slice_terrain else 0
            nb = int(s.frame_inds.shape[0])
            a.box_off, a.box_count = box_off, nb
            a.frame_off, a.frame_len = frames_plan.out_off[k], s.length
            a.scale = float(s.height_scale) if s.height_scale is not None else 1.0
            for b in range(nb):
                e = self.boxes[box_off + b]
                e.frame_ind = int(s.frame_inds[b])
                e.len_x, e.len_y = float(s.box_len[b, 0]), float(s.box_len[b, 1])
                ang = torch.tensor([s.box_angle[b]], dtype=torch.float32)
                e.angle, e.cos_a, e.sin_a = float(ang[0]), float(torch.cos(ang)[0]), float(torch.sin(ang)[0])
                e.h = float(s.box_h[b])
            box_off += nb
            out_parts += [np.zeros(X * Y, np.float32), grid.xs.numpy(), grid.ys.numpy()]
            point_parts += [xs.numpy().astype(np.float32), ys.numpy().astype(np.float32)]
            out_off += X * Y + X + Y
            pt_off += int(xs.shape[0]) + int(ys.shape[0])
            cells.append(cells[-1] + X * Y)
            self.shapes.append((X, Y))
            self.grid_min.append((o.min_x, o.min_y))
            self.dxdy.append((o.dx, o.dy))
        assert out_off + pt_off < 2 ** 31
        self.out_floats, self.points_floats = out_off, pt_off
        self.pool = np.concatenate(out_parts + point_parts) if V else np.zeros(0, np.float32)      # ONE array: one copy to the device
        self.cell_start = np.asarray(cells, np.int64)
        self.n_cells = int(cells[-1])
        self.slice = bool(slice_terrain)
        self.pad = pad


def group_ranges(n, batch):
    """[(first, last + 1)] of the groups of at most `batch` consecutive variants"""
    batch = max(int(batch or 1), 1)
    return [(i, min(i + batch, n)) for i in range(0, n, batch)]


# ---------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------
def _upload(blobs, device):
    """several host arrays -> device tensors that are views of ONE uploaded byte buffer (each 16-byte aligned)"""
    raw, offs = [], []
    at = 0
    for b in blobs:
        data = b.tobytes() if isinstance(b, np.ndarray) else bytes(b)
        pad = (-at) % 16
        raw.append(b"\0" * pad)
        at += pad
        offs.append((at, len(data)))
        raw.append(data)
        at += len(data)
    buf = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()).to(device)
    return [buf[o:o + n] for o, n in offs]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class PreparedVariants:
    """What prepare_variants returns: frames / contacts (lists of [T_v, 34] / [T_v, C] device tensors, views of the packed arrays
    frames_packed / contacts_packed), and the terrains - as `hf_table(first, last)` for the batched optimiser (no host read), or as
    SubTerrain objects through `terrains` (one host read of the pool and of canon, made on first use)."""

    def __init__(self, specs, clips, fplan, tplan, frames_packed, contacts_packed, pool, hf_table_bytes, canon):
        self.specs, self.clips, self.fplan, self.tplan = specs, clips, fplan, tplan
        self.frames_packed, self.contacts_packed, self.pool, self.canon = frames_packed, contacts_packed, pool, canon
        self._hf_table_bytes = hf_table_bytes
        o = fplan.out_off
        self.frames = [frames_packed[o[k]:o[k] + fplan.lengths[k]] for k in range(len(specs))]
        self.contacts = [contacts_packed[o[k]:o[k] + fplan.lengths[k]] for k in range(len(specs))]
        self._terrains = None

    def __iter__(self):          # frames, contacts, terrains = prepare_variants(...)
        return iter((self.frames, self.contacts, self.terrains))

    def hf_table(self, first=0, last=None):
        """terrain_util.HfTable of variants first .. last - 1 over the pool the kernels wrote"""
        last = len(self.specs) if last is None else last
        n = ctypes.sizeof(_hip_moopt.MooptTerrainS)
        return terrain_util.HfTable.from_pool(self.pool, self._hf_table_bytes[first * n:last * n], self.tplan.shapes[first:last], DESCENT_BASE_Z)

    @property
    def terrains(self):
        if self._terrains is None:
            self._terrains = self._make_terrains()
        return self._terrains

    def _make_terrains(self):
        tp = self.tplan
        pool = self.pool[:tp.out_floats].cpu().numpy()
        canon = self.canon.cpu().numpy().astype(np.float64)
        dev = self.pool.device
        out = []
        for k, s in enumerate(self.specs):
            X, Y = tp.shapes[k]
            src = self.clips[s.file_index].terrain
            off = tp.hf_entries[k].off_hf
            # (the reference subtracts the two Python floats, then rounds to float32: the float32 difference)
            mn = (tp.grid_min[k][0] - canon[k, 0], tp.grid_min[k][1] - canon[k, 1]) if tp.slice else tp.grid_min[k]
            t = terrain_util.SubTerrain("terrain", X, Y, tp.dxdy[k][0], tp.dxdy[k][1], mn[0], mn[1], device="cpu")
            t.hf = torch.from_numpy(pool[off:off + X * Y].reshape(X, Y).copy())
            padded = src.torch_copy()
            if tp.pad > 0:
                padded.pad(tp.pad)
            if tp.slice:        # the mask and the height limits follow the cells (util/terrain_util.py:1711-1714)
                o = tp.out_table[k]
                xs = torch.from_numpy(tp.pool[tp.out_floats + o.off_x:tp.out_floats + o.off_x + X].copy())
                ys = torch.from_numpy(tp.pool[tp.out_floats + o.off_y:tp.out_floats + o.off_y + Y].copy())
                gx, gy = torch.meshgrid(xs, ys, indexing="ij")
                g = padded.get_grid_index(torch.stack([gx, gy], dim=-1))
                t.hf_mask, t.hf_maxmin = padded.hf_mask[g[..., 0], g[..., 1]].clone(), padded.hf_maxmin[g[..., 0], g[..., 1]].clone()
            else:
                t.hf_mask, t.hf_maxmin = padded.hf_mask, padded.hf_maxmin
            t.set_device(dev)
            out.append(t)
        return out


def prepare_variants(specs, clips, device, terrain_padding_size=0, slice_terrain=True):
    """Frames, contacts and terrains of all variants, built on `device` -> PreparedVariants (unpacks as frames, contacts, terrains).
    Three launches and ONE host read (the variants' xy bounds [V, 4], which size the terrain windows); reading `.terrains` later reads
    the finished pool and canon [V, 3] back once for the SubTerrain objects.  A variant whose transformed frames are not finite raises
    ValueError naming it before anything is allocated for the terrains."""
    from ... import _hip
    L, dev = _hip.lib(), torch.device(device)
    assert dev.type == "cuda", "the augmentation kernels run on the GPU (no CPU fallback)"
    V = len(specs)
    fp = FramesPlan(specs, clips)
    C = fp.contact_width
    with torch.cuda.device(dev):
        st = _hip.stream()
        src_frames, src_contacts, ftable = _upload([fp.src_frames, fp.src_contacts, fp.table], dev)
        frames = torch.empty((fp.n_out, _hip_augment.FRAME_DIM), dtype=torch.float32, device=dev)
        contacts = torch.empty((fp.n_out, C), dtype=torch.float32, device=dev)
        bounds = torch.empty((V, 4), dtype=torch.float32, device=dev)
        _hip.check(L.parc_augment_frames(st, V, int(fp.src_frames.shape[0]), C, _vp(src_frames), _vp(src_contacts), _vp(ftable), fp.n_out, _vp(frames),
                                         _vp(contacts), _vp(bounds)), "parc_augment_frames")
        tp = TerrainPlan(specs, clips, bounds.cpu().numpy(), fp, terrain_padding_size, slice_terrain)       # the one host read
        pool_b, src_pool, src_table, out_table, vars_t, boxes, cell_start, hf_table = _upload(
            [tp.pool, tp.src_pool, tp.src_table, tp.out_table, tp.vars, tp.boxes, tp.cell_start, tp.hf_entries], dev)
        pool = pool_b.view(torch.float32)
        canon = torch.full((V, 3), float("nan"), dtype=torch.float32, device=dev)
        points = pool[tp.out_floats:]
        _hip.check(L.parc_augment_terrains(st, V, tp.n_cells, _vp(cell_start), _vp(vars_t), len(clips), _vp(src_table), _vp(src_pool),
                                           int(tp.src_pool.size), _vp(out_table), _vp(points) if tp.points_floats else None, tp.points_floats,
                                           _vp(boxes), tp.n_boxes, _vp(frames), fp.n_out, _vp(pool), tp.out_floats, _vp(canon)),
                   "parc_augment_terrains")
        _hip.check(L.parc_augment_localize(st, V, _vp(vars_t), _vp(canon), _vp(frames), fp.n_out, _vp(hf_table)), "parc_augment_localize")
    return PreparedVariants(specs, clips, fp, tp, frames, contacts, pool, hf_table, canon)


def stamp_boxes(hf, box_centers, box_len, angles, heights):
    """terrain_util.add_boxes_to_hf_at_xy_points on a GPU tensor: the drawn boxes stamped into hf [X, Y] in place by ONE launch of
    parc_augment_terrains (the grid itself as the source, the box centres as the "frames" of a grid with origin 0 and cell size 1)."""
    from ... import _hip
    assert hf.is_cuda and hf.dtype == torch.float32 and hf.dim() == 2 and hf.is_contiguous()
    dev, X, Y, n = hf.device, int(hf.shape[0]), int(hf.shape[1]), int(box_centers.shape[0])
    if n == 0 or X * Y == 0:
        return
    grid = (_hip_augment.AugTerrainS * 1)()
    g = grid[0]
    g.off_hf, g.off_x, g.off_y, g.dim_x, g.dim_y, g.min_x, g.min_y, g.dx, g.dy = 0, 0, 0, X, Y, 0.0, 0.0, 1.0, 1.0
    var = (_hip_augment.AugVariantS * 1)()
    a = var[0]
    a.src, a.pad, a.mode, a.slice, a.box_off, a.box_count, a.frame_off, a.frame_len, a.scale = 0, 0, _hip_augment.MODE_BOXES_ALONG_PATH, 0, 0, n, 0, n, 1.0
    boxes = (_hip_augment.AugBoxS * n)()
    for b in range(n):
        e = boxes[b]
        ang = torch.tensor([angles[b]], dtype=torch.float32)
        e.frame_ind, e.len_x, e.len_y = b, float(box_len[b, 0]), float(box_len[b, 1])
        e.angle, e.cos_a, e.sin_a, e.h = float(ang[0]), float(torch.cos(ang)[0]), float(torch.sin(ang)[0]), float(heights[b])
    with torch.cuda.device(dev):
        grid_t, var_t, boxes_t, cells = _upload([grid, var, boxes, np.asarray([0, X * Y], np.int64)], dev)
        rows = torch.zeros((n, _hip_augment.FRAME_DIM), dtype=torch.float32, device=dev)
        rows[:, 0:2] = box_centers.to(device=dev, dtype=torch.float32)
        src = hf.clone()
        canon = torch.empty((1, 3), dtype=torch.float32, device=dev)
        _hip.check(_hip.lib().parc_augment_terrains(_hip.stream(), 1, X * Y, _vp(cells), _vp(var_t), 1, _vp(grid_t), _vp(src), X * Y, _vp(grid_t), None, 0,
                                                    _vp(boxes_t), n, _vp(rows), n, _vp(hf), X * Y, _vp(canon)), "parc_augment_terrains")


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def load_seed_clips(motions_yaml_path):
    """the seed clips of a dataset YAML ({"motions": [{"file": ...}, ...]}), read with the non-executing reader"""
    from ...zmotion_editing_tools import motion_edit_lib
    with open(motions_yaml_path, "r") as f:
        entries = yaml.safe_load(f)["motions"]
    clips = []
    for e in entries:
        md = motion_edit_lib.load_motion_file(e["file"])
        clips.append(SeedClip(os.path.basename(os.path.splitext(e["file"])[0]), md.get_frames().cpu(), md.get_contacts().cpu(), md.get_terrain(),
                              md.get_fps()))
    return clips


def _body_points(cfg, char_model):
    from ...util import geom_util
    ps = cfg["char_point_samples"]
    return geom_util.get_char_point_samples(char_model, sphere_num_subdivisions=ps["sphere_num_subdivisions"], box_num_slices=ps["box_num_slices"],
                                            box_dim_x=ps["box_dim_x"], box_dim_y=ps["box_dim_y"],
                                            capsule_num_circle_points=ps["capsule_num_circle_points"],
                                            capsule_num_sphere_subdivisons=ps["capsule_num_sphere_subdivisions"],
                                            capsule_num_cylinder_slices=ps["capsule_num_cylinder_slices"])


def loss_weights(cfg):
    w = {k: cfg[k] for k in ("w_root_pos", "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding")}
    w["w_body_constraints"] = 0.0            # the reference passes no constraints (:225-226)
    w["w_jerk"] = cfg.get("w_jerk", 0.0)
    return w


def optimize_prepared(prep, cfg, char_model, body_points, log_folder=None, verbose=True, loss_trace=None):
    """descend the prepared variants in groups of cfg["opt_batch_size"] -> list of optimised frames [T_v, 34].
    loss_trace: optional list that receives, per group, ONE [num_iters, group size] device tensor of per-variant totals (tests)."""
    from . import motion_optimization as moopt
    out = []
    for first, last in group_ranges(len(prep.specs), cfg.get("opt_batch_size", 8)):
        names = [s.name for s in prep.specs[first:last]]
        logs = [os.path.join(log_folder, "log_" + n + ".txt") if log_folder is not None else None for n in names]
        if verbose:
            print("AUGMENTING MOTIONS:", ", ".join(names), "{}-{}/{}".format(first, last - 1, len(prep.specs)))
        out += moopt.motion_contact_optimization_batch(src_frames=prep.frames[first:last], contacts=prep.contacts[first:last], body_points=body_points,
                                                       terrains=prep.hf_table(first, last), char_model=char_model, num_iters=cfg["num_iters"],
                                                       step_size=cfg["step_size"], body_constraints=None, max_jerk=cfg.get("max_jerk", 1000.0),
                                                       exp_names=names, use_wandb=False, log_files=logs, verbose=verbose, loss_trace=loss_trace,
                                                       **loss_weights(cfg))
    return out


def augment_dataset(cfg, clips=None, char_model=None, body_points=None, verbose=True, loss_trace=None):
    """The whole script for one config dict -> list of written file paths.  clips / char_model / body_points default to what the config
    names (motions_yaml_path, char_model, char_point_samples)."""
    from ...anim import kin_char_model
    from . import optimize_motions
    t0 = time.time()
    device = cfg["device"]
    if clips is None:
        clips = load_seed_clips(cfg["motions_yaml_path"])
    if char_model is None:
        char_model = kin_char_model.KinCharModel(device)
        char_model.load_char_file(cfg["char_model"])
    if body_points is None:
        body_points = _body_points(cfg, char_model)
    out_folder = cfg["output_folder_path"]
    log_folder = os.path.join(out_folder, "log")
    os.makedirs(log_folder, exist_ok=True)
    specs = draw_variants(cfg, clips)
    prep = prepare_variants(specs, clips, device, cfg["terrain_padding_size"], cfg["slice_terrain"])
    opt = optimize_prepared(prep, cfg, char_model, body_points, log_folder, verbose, loss_trace)
    terrains = prep.terrains
    paths = [optimize_motions._write_clip(out_folder, s.name, opt[k], prep.contacts[k], terrains[k], clips[s.file_index].fps, None)
             for k, s in enumerate(specs)]
    if verbose:
        print("Total augmentation time for", len(specs), "motions:", time.time() - t0, "seconds.")
    return paths


def main(argv):
    cfg_path = argv[2] if len(argv) == 3 and argv[1] == "--config" else "tools/motion_opt/config/platform_aug.yaml"
    print("loading config from", cfg_path)
    with open(cfg_path, "r") as f:
        cfg = yaml.safe_load(f)
    augment_dataset(cfg)


if __name__ == "__main__":
    main(sys.argv)
