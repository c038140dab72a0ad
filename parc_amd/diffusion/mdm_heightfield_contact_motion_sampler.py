"""Training batches for the motion generator from a dataset with terrains (reference diffusion/mdm_heightfield_contact_motion_sampler.py):
windows of motion canonicalised to a reference frame, the local heightfield under the character with a motion-aware augmentation, and a
target drawn from the clip's future.

Every random number of a batch is drawn first, in the reference's order and from the generators it uses, into a SamplerDraws object;
what follows is deterministic.  Two code paths consume the draws:
  * the loop path - the reference's algorithm on the package's torch functions, one sample at a time.  It is the CPU implementation, and
    on a HIP device the fallback and the baseline of the measurement (tools/bench_mdm_sampler.py);
  * the batch path - build_batch(): parc_mdm_heightfields + parc_mdm_windows (include/parc_mdm_batch.h), two launches and one
    host-to-device copy (the draw table) per batch, whatever its size.
Out of scope: FLOOR_HEIGHTS, generate_hfs, sample_mismatched_prev_states_and_hfs, get_motion_sequences_for_id,
use_saved_heightmaps false.
"""
import enum
import random

import numpy as np
import torch

from .. import _hip, _hip_mdm_batch as mb
from ..util import geom_util, terrain_util, torch_util
from . import batch_tables, diffusion_util
from .motion_sampler import MotionSampler, TorchMotionLib, forward_kinematics_reference_order


class HFAugmentationMode(enum.Enum):
    NOISE = 0
    MAXPOOL_AND_BOXES = 1
    NONE = 2


class SamplerDraws:
    """Every random number of one batch of n samples.  Host arrays (numpy) unless said otherwise.

    MAXPOOL_AND_BOXES (the draws of _box_hf_augmentation and add_boxes_to_hf2, reference :365-407, util/terrain_util.py:881-909):
      change_height [n] int32     1: the whole grid is overwritten with new_height first
      new_height    [n] float32   random() * (max_h - min_h) + min_h
      pool_kind     [n, 3] int32  the three pools in the order they run: 0 the 2-D pool, 1 along x (first index), 2 along y; -1: roll failed
      pool_radius   [n, 3] int32  randint(0, hf_max_maxpool_size) of each pool that runs
      num_boxes     [n] int32     randint(0, max_num_boxes)
      boxes         [n, max_num_boxes, 6] float32   per box: centre x, y and side lengths x, y in cells of the local grid (torch.rand(2)
                                  each, scaled as the reference scales them), angle and height (random() each, as fp32)
    NOISE (reference :409-412):
      noise         [n, X, Y] float32 tensor on the sampler's device: rand * (max_h - min_h) + min_h
    the target (reference :188-216), tensors on the sampler's device:
      future_time   [n]     rand * min(length - start, future_window_max - future_window_min) + start + future_window_min
      future_noise  [n, 3]  future_pos_noise_scale * randn
    Fields a batch does not use are None."""

    FIELDS = ("change_height", "new_height", "pool_kind", "pool_radius", "num_boxes", "boxes", "noise", "future_time", "future_noise")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw.pop(f, None))
        assert not kw, kw


def quat_multiply(q1, q2):
    """reference util/torch_util.py:577-594 (the grouping the canonicalisation uses)"""
    x1, y1, z1, w1 = q1[..., 0], q1[..., 1], q1[..., 2], q1[..., 3]
    x2, y2, z2, w2 = q2[..., 0], q2[..., 1], q2[..., 2], q2[..., 3]
    return torch.stack((w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                        w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2), dim=-1)


class BatchUnsupported(RuntimeError):
    """the kernels answered PARC_EUNSUPPORTED: a size of this batch is over their caps"""


class MDMHeightfieldContactMotionSampler(MotionSampler):
    def __init__(self, cfg, types=None, path=None):
        """types: a namespace with MDMFrameType, RelativeZStyle and TargetInfo that replaces parc_amd.diffusion.diffusion_util (the
        reference's trainer indexes the returned dict with its own enum class: pass its diffusion.diffusion_util).
        path: 'batch' or 'loop'; None picks the batch path on a HIP device and the loop path on the CPU."""
        super().__init__(cfg)
        self._types = types if types is not None else diffusion_util
        MDMFrameType, RelativeZStyle = self._types.MDMFrameType, self._types.RelativeZStyle

        self._canonicalize_samples = cfg['features']['canonicalize_samples']
        self._frame_components = [MDMFrameType[comp] for comp in cfg['features']['frame_components']]
        if MDMFrameType.FLOOR_HEIGHTS in self._frame_components:
            raise NotImplementedError("frame component FLOOR_HEIGHTS is not built (DESIGN.md section 7)")
        self._num_rb = len(self._kin_char_model._body_names)
        self._fps = cfg['sequence_fps']
        self._timestep = 1.0 / self._fps
        self._random_start_times = cfg['autoregressive']
        self._sample_seq_time = cfg['sequence_duration']
        # made on the CPU and copied: torch.arange and torch.linspace round differently on a device, and the reference's CPU values are
        # the ones the fixtures hold (the frame times decide the blend weights, the grid points the cells)
        self._motion_times = torch.arange(start=0.0, end=self._sample_seq_time, step=self._timestep, dtype=torch.float32).to(self._device)
        self._seq_len = self._motion_times.shape[0]
        self._num_prev_states = cfg['num_prev_states']
        self._canon_idx = cfg['num_prev_states'] - 1
        self._future_pos_noise_scale = cfg["future_pos_noise_scale"]
        self._use_saved_heightmaps = cfg["use_saved_heightmaps"]
        if not self._use_saved_heightmaps:
            raise NotImplementedError("use_saved_heightmaps: false is not built (DESIGN.md section 7)")
        self._relative_z_style = RelativeZStyle[cfg["relative_z_style"]]
        self._hf_augmentation_mode = HFAugmentationMode[cfg["hf_augmentation_mode"]]
        hmap_cfg = cfg["heightmap"]
        dx = hmap_cfg["horizontal_scale"]
        self._dx = dx
        grid = hmap_cfg["local_grid"]
        self._num_x_neg, self._num_x_pos, self._num_y_neg, self._num_y_pos = grid["num_x_neg"], grid["num_x_pos"], grid["num_y_neg"], grid["num_y_pos"]
        self._grid_min_point = torch.tensor([-self._num_x_neg, -self._num_y_neg], dtype=torch.float32, device=self._device) * dx
        self._grid_dim_x = self._num_x_neg + 1 + self._num_x_pos
        self._grid_dim_y = self._num_y_neg + 1 + self._num_y_pos
        self._grid_dims = torch.tensor([self._grid_dim_x, self._grid_dim_y], dtype=torch.int64, device=self._device)
        self._num_hf_points = self._grid_dim_x * self._grid_dim_y
        zero = torch.zeros(size=(2,), dtype=torch.float32)
        self._generic_heightmap = geom_util.get_xy_grid_points(zero, dx, dx, self._num_x_neg, self._num_x_pos, self._num_y_neg,
                                                               self._num_y_pos).to(self._device)
        self._max_h = cfg["heightmap"]["max_h"]
        self._min_h = -self._max_h
        self._use_hf_augmentation = cfg["use_hf_augmentation"]
        if self._use_hf_augmentation:
            self._max_num_boxes = cfg["max_num_boxes"]
            self._box_min_len = cfg["box_min_len"]
            self._box_max_len = cfg["box_max_len"]
            self._hf_maxpool_chance = cfg["hf_maxpool_chance"]
            self._hf_max_maxpool_size = cfg["hf_max_maxpool_size"]
            self._hf_change_height_chance = cfg["hf_change_height_chance"]
        assert self._num_prev_states >= 1
        self._ref_frame_idx = self._num_prev_states - 1
        self._angle_noise_scale = cfg["angle_noise_scale"]
        self._pos_noise_scale = cfg["pos_noise_scale"]
        self._future_window_min = cfg["future_window_min"]
        self._future_window_max = cfg["future_window_max"]
        self.check_init()

        self._check_dataset()
        on_device = torch.device(self._device).type != "cpu"
        assert path in (None, "batch", "loop")
        if path == "batch" and not on_device:
            raise ValueError("the batch path runs HIP kernels: cfg['device'] must be a HIP device")
        self._path = path if path is not None else ("batch" if on_device else "loop")
        self._tables = None
        self._fallback_logged = False
        self.last_path = None           # the path the last batch took ('batch' or 'loop')

    # ------------------------------------------------------------------------------------------------------------ the dataset
    def _check_dataset(self):
        """every motion needs a terrain, its band (hf_maxmin) and its per-frame cell lists (hf_mask_inds); the reference fails on a file
        without them with a TypeError at the first batch.  A band that is the constructor's default (1, -1) everywhere counts as missing:
        a file without hf_maxmin loads as that."""
        m = self._mlib
        files = getattr(m, "_motion_files", None) or ["motion %d" % i for i in range(m.num_motions())]
        lists = getattr(m, "_hf_mask_inds", None)
        terrains = getattr(m, "_terrains", None) or []
        for i in range(m.num_motions()):
            ter = terrains[i] if i < len(terrains) else None
            if ter is None:
                raise ValueError("{}: no terrain (the sampler needs a dataset written by create_dataset)".format(files[i]))
            band = getattr(ter, "hf_maxmin", None)
            if band is None or (bool(torch.all(band[..., 0] == 1.0)) and bool(torch.all(band[..., 1] == -1.0))):
                raise ValueError("{}: no height band hf_maxmin (run create_dataset over the file)".format(files[i]))
            if lists is None or i >= len(lists) or lists[i] is None:
                raise ValueError("{}: no per-frame cell lists hf_mask_inds (run create_dataset over the file)".format(files[i]))

    def _device_tables(self):
        """the per-clip terrain and cell-list tables of the kernels, uploaded once"""
        if self._tables is None:
            m = self._mlib
            terrains = [(t.hf.cpu().numpy(), t.hf_maxmin.cpu().numpy(), t.min_point.cpu().numpy(), t.dxdy.cpu().numpy()) for t in m._terrains]
            lists = [[a.cpu().numpy() for a in per_clip] for per_clip in m._hf_mask_inds]
            clips, pool, cell_start, cells, mask_cells = batch_tables.pack_clip_tables(terrains, lists)
            dev = self._device
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
            raw = np.frombuffer(bytes(clips), dtype=np.uint8).copy()
            self._tables = dict(n_clips=len(terrains), clips=up(raw), pool=up(pool), cell_start=up(cell_start), cells=up(cells), mask_cells=mask_cells,
                                n_cell_start=int(cell_start.size), n_cells=int(cells.size), pool_floats=int(pool.size),
                                grid_x=self._generic_heightmap[:, 0, 0].contiguous(), grid_y=self._generic_heightmap[0, :, 1].contiguous())
        return self._tables

    def update_old_sampler(self):
        self._relative_z_style = self._types.RelativeZStyle.RELATIVE_TO_ROOT

    # ------------------------------------------------------------------------------------------------------------ draws
    def _mode(self):
        """the augmentation a batch gets: use_hf_augmentation false is NONE"""
        return self._hf_augmentation_mode if self._use_hf_augmentation else HFAugmentationMode.NONE

    def _draw_heightfields(self, n, d):
        """the draws of get_hfs_from_data, sample by sample in the reference's order"""
        mode = self._mode()
        X, Y = self._grid_dim_x, self._grid_dim_y
        if mode == HFAugmentationMode.NOISE:
            span = self._max_h - self._min_h
            if torch.device(self._device).type == "cpu":
                # one rand_like per sample, as the reference's loop makes them
                d.noise = torch.stack([torch.rand(size=(X, Y), dtype=torch.float32) * span + self._min_h for _ in range(n)]) if n else \
                    torch.zeros((0, X, Y), dtype=torch.float32)
            else:
                d.noise = torch.rand(size=(n, X, Y), dtype=torch.float32, device=self._device) * span + self._min_h
        elif mode == HFAugmentationMode.MAXPOOL_AND_BOXES:
            B = self._max_num_boxes
            d.change_height, d.new_height = np.zeros(n, np.int32), np.zeros(n, np.float32)
            d.pool_kind, d.pool_radius = np.full((n, 3), mb.POOL_UNUSED, np.int32), np.zeros((n, 3), np.int32)
            d.num_boxes, d.boxes = np.zeros(n, np.int32), np.zeros((n, B, 6), np.float32)
            dims = torch.tensor([X, Y], dtype=torch.float32)
            for s in range(n):
                if random.random() < self._hf_change_height_chance:
                    d.change_height[s] = 1
                    d.new_height[s] = random.random() * (self._max_h - self._min_h) + self._min_h
                use = [random.random() < self._hf_maxpool_chance for _ in range(3)]
                kinds = [mb.POOL_2D, mb.POOL_X, mb.POOL_Y]
                random.shuffle(kinds)
                for q in range(3):
                    if use[q]:
                        d.pool_radius[s, q] = random.randint(0, self._hf_max_maxpool_size)
                        d.pool_kind[s, q] = kinds[q]
                nb = random.randint(0, B)
                d.num_boxes[s] = nb
                for b in range(nb):
                    # the per-box torch draws come from the CPU generator on every device: they go up with the rest of the table
                    center = torch.rand(size=(2,), dtype=torch.float32) * dims
                    length = torch.rand(size=(2,), dtype=torch.float32) * (self._box_max_len - self._box_min_len) + self._box_min_len
                    angle = random.random() * (2.0 * torch.pi - 0.0) + 0.0
                    h = random.random() * (self._max_h - self._min_h) + self._min_h
                    d.boxes[s, b] = [center[0].item(), center[1].item(), length[0].item(), length[1].item(), angle, h]

    def _sample_motion_future_times(self, motion_ids, start_times, future_window_min, future_window_max):
        remaining_time = self._mlib.get_motion_length(motion_ids) - start_times
        remaining_time = torch.clamp_max(remaining_time, future_window_max - future_window_min)
        return torch.rand_like(start_times) * remaining_time + start_times + future_window_min

    def make_draws(self, motion_ids, motion_start_times, ret_hf_obs=True, ret_target_info=True):
        d = SamplerDraws()
        n = motion_ids.shape[0]
        if ret_hf_obs:
            self._draw_heightfields(n, d)
        if ret_target_info:
            d.future_time = self._sample_motion_future_times(motion_ids, motion_start_times, self._future_window_min, self._future_window_max)
            d.future_noise = self._future_pos_noise_scale * torch.randn(size=(n, 3), dtype=torch.float32, device=motion_start_times.device)
        return d

    # ------------------------------------------------------------------------------------------------------------ the public call
    def sample_motion_data(self, motion_ids=None, num_samples=None, motion_start_times=None, ret_hf_obs=True, ret_target_info=True):
        if motion_ids is None:
            assert num_samples is not None
            motion_ids = self._mlib.sample_motions(num_samples)
        if motion_start_times is None:
            motion_start_times = self._sample_motion_start_times(motion_ids, self._sample_seq_time)
        draws = self.make_draws(motion_ids, motion_start_times, ret_hf_obs, ret_target_info)
        out = self.run_batch(motion_ids, motion_start_times, draws, ret_hf_obs, ret_target_info)
        return self._assemble(out, ret_hf_obs, ret_target_info)

    def run_batch(self, motion_ids, motion_start_times, draws, ret_hf_obs=True, ret_target_info=True):
        """the batch of these draws on the sampler's path; a batch over the kernels' caps takes the loop path (said once)"""
        if self._path == "batch":
            try:
                out = self.build_batch(motion_ids, motion_start_times, draws, ret_hf_obs, ret_target_info)
                self.last_path = "batch"
                return out
            except BatchUnsupported as e:
                if not self._fallback_logged:
                    print("MDMHeightfieldContactMotionSampler: {}; such batches take the loop path".format(e))
                    self._fallback_logged = True
        self.last_path = "loop"
        return self.loop_batch(motion_ids, motion_start_times, draws, ret_hf_obs, ret_target_info)

    def _assemble(self, out, ret_hf_obs, ret_target_info):
        T = self._types.MDMFrameType
        entries = {T.ROOT_POS: "root_pos", T.ROOT_ROT: "root_rot", T.JOINT_POS: "body_pos", T.JOINT_ROT: "joint_rot", T.CONTACTS: "contacts"}
        motion_ret = dict()
        for frame_type in self._frame_components:          # JOINT_VEL yields no entry, as in the reference
            if frame_type in entries:
                motion_ret[frame_type] = out[entries[frame_type]]
        if not (ret_hf_obs or ret_target_info):
            return motion_ret
        ret = [motion_ret]
        if ret_hf_obs:
            ret.append(out["hfs"])
        if ret_target_info:
            ret.append(self._types.TargetInfo(out["future_pos"], out["future_rot"]))
        return tuple(ret)

    # ------------------------------------------------------------------------------------------------------------ the batch path
    def _cfg_struct(self):
        R = self._types.RelativeZStyle
        z = mb.Z_ROOT_FLOOR if self._relative_z_style == R.RELATIVE_TO_ROOT_FLOOR else mb.Z_ROOT
        mode = {HFAugmentationMode.NOISE: mb.AUG_NOISE, HFAugmentationMode.MAXPOOL_AND_BOXES: mb.AUG_MAXPOOL_AND_BOXES,
                HFAugmentationMode.NONE: mb.AUG_NONE}[self._mode()]
        max_boxes = self._max_num_boxes if mode == mb.AUG_MAXPOOL_AND_BOXES else 0
        return batch_tables.make_cfg(self._seq_len, self._ref_frame_idx, self._num_x_neg, self._num_y_neg, self._grid_dim_x, self._grid_dim_y, z, mode,
                                     max_boxes, self._fps, self._max_h)

    def _alloc(self, shape, dtype=torch.float32):
        """an output of build_batch (the tests put one more row behind it to see that it stays untouched)"""
        return torch.empty(shape, dtype=dtype, device=self._device)

    def build_batch(self, motion_ids, start_times, draws, ret_hf_obs=True, ret_target_info=True, debug=False):
        """Deterministic: the batch of these ids, start times and draws through parc_mdm_heightfields and parc_mdm_windows.  Returns a dict
        of device tensors: root_pos, root_rot, body_pos, joint_rot, contacts[, hfs, center_h][, future_pos, future_rot]; with debug also
        pre [n, 3, X, Y] and cell_code [n, X, Y] (include/parc_mdm_batch.h).  Raises BatchUnsupported for a batch over the kernels' caps."""
        L = _hip.lib()
        dev = self._device
        n, S, B = int(motion_ids.shape[0]), self._seq_len, self._num_rb
        X, Y = self._grid_dim_x, self._grid_dim_y
        cfg = self._cfg_struct()
        ml, km = self._mlib.c_struct(), self._kin_char_model.c_struct()
        ids = motion_ids.to(device=dev, dtype=torch.int64).contiguous()
        starts = start_times.to(device=dev, dtype=torch.float32).contiguous()
        f32 = dict(dtype=torch.float32, device=dev)
        out = {}
        center_h = None
        if ret_hf_obs:
            t = self._device_tables()
            d_draws = d_boxes = None
            if cfg.mode == mb.AUG_MAXPOOL_AND_BOXES:
                raw, box_off = batch_tables.pack_draws(draws.change_height, draws.new_height, draws.pool_kind, draws.pool_radius, draws.num_boxes,
                                                       draws.boxes, cfg.max_boxes)
                table = torch.from_numpy(raw).to(dev, non_blocking=False)           # the one host-to-device copy of the batch
                d_draws = _hip.c_vp(table.data_ptr())
                d_boxes = _hip.c_vp(table.data_ptr() + box_off) if cfg.max_boxes else _hip.c_vp(0)
            noise = draws.noise.to(**f32).contiguous() if cfg.mode == mb.AUG_NOISE else None
            out["hfs"], out["center_h"] = self._alloc((n, X, Y)), self._alloc((n,))
            if debug:
                out["pre"], out["cell_code"] = self._alloc((n, 3, X, Y)), self._alloc((n, X, Y), torch.int32)
            rc = L.parc_mdm_heightfields(_hip.stream(), ml, cfg, n, _hip.ptr(ids), _hip.ptr(starts), _hip.ptr(self._motion_times), _hip.ptr(t["grid_x"]),
                                         _hip.ptr(t["grid_y"]), t["n_clips"], _hip.ptr(t["clips"]), _hip.ptr(t["pool"]), t["pool_floats"],
                                         _hip.ptr(t["cell_start"]), t["n_cell_start"], _hip.ptr(t["cells"]), t["n_cells"], t["mask_cells"], d_draws,
                                         d_boxes, _hip.ptr(noise), _hip.ptr(out["hfs"]), _hip.ptr(out["center_h"]), _hip.ptr(out.get("pre")),
                                         _hip.ptr(out.get("cell_code")))
            if rc == mb.EUNSUPPORTED:
                raise BatchUnsupported("a {} x {} local grid, {} boxes per sample or a terrain of {} cells is over the kernels' caps".format(
                    X, Y, cfg.max_boxes, t["mask_cells"]))
            _hip.check(rc, "parc_mdm_heightfields")
            if self._relative_z_style == self._types.RelativeZStyle.RELATIVE_TO_ROOT_FLOOR:
                center_h = out["center_h"]
        out["root_pos"], out["root_rot"] = self._alloc((n, S, 3)), self._alloc((n, S, 4))
        out["body_pos"], out["joint_rot"] = self._alloc((n, S, B - 1, 3)), self._alloc((n, S, B - 1, 4))
        out["contacts"] = self._alloc((n, S, B))
        ft = fn = None
        if ret_target_info:
            ft, fn = draws.future_time.to(**f32).contiguous(), draws.future_noise.to(**f32).contiguous()
            out["future_pos"], out["future_rot"] = self._alloc((n, 3)), self._alloc((n, 4))
        rc = L.parc_mdm_windows(_hip.stream(), km, ml, cfg, n, _hip.ptr(ids), _hip.ptr(starts), _hip.ptr(self._motion_times), _hip.ptr(center_h),
                                _hip.ptr(ft), _hip.ptr(fn), _hip.ptr(out["root_pos"]), _hip.ptr(out["root_rot"]), _hip.ptr(out["body_pos"]),
                                _hip.ptr(out["joint_rot"]), _hip.ptr(out["contacts"]), _hip.ptr(out.get("future_pos")), _hip.ptr(out.get("future_rot")))
        if rc == mb.EUNSUPPORTED:
            raise BatchUnsupported("a window of {} frames is over the kernels' caps".format(S))
        _hip.check(rc, "parc_mdm_windows")
        return out

    # ------------------------------------------------------------------------------------------------------------ the loop path
    def _extract_motion_data(self, motion_ids, motion_start_times, motion_times, seq_len):
        """all motion data in global coordinates, [num_samples, seq_len, ...] (reference :218-246)"""
        num_samples = motion_ids.shape[0]
        times = (motion_start_times.unsqueeze(-1) + motion_times).flatten()
        ids = motion_ids.unsqueeze(-1).expand(-1, seq_len).flatten()
        root_pos, root_rot, root_vel, root_ang_vel, joint_rot, dof_vel, contacts = self._mlib.calc_motion_frame(ids, motion_times=times)
        shape = lambda x, tail: None if x is None else torch.reshape(x, [num_samples, seq_len] + tail)     # noqa: E731
        return (shape(root_pos, [3]), shape(root_rot, [4]), shape(root_vel, [3]), shape(root_ang_vel, [3]), shape(joint_rot, [-1, 4]), dof_vel,
                shape(contacts, [self._kin_char_model.get_num_joints()]))

    def _extract_root_pos_and_rot(self, motion_ids, times):
        ret = self._mlib.calc_motion_frame(motion_ids, motion_times=times)
        return ret[0], ret[1]

    def _sample_target_info(self, motion_ids, motion_start_times, canon_pos, canon_heading_quat_inv, draws=None):
        """reference :202-216; with draws the future time and noise are taken from them instead of drawn"""
        if draws is None:
            draws = self.make_draws(motion_ids, motion_start_times, ret_hf_obs=False, ret_target_info=True)
        future_pos, future_rot = self._extract_root_pos_and_rot(motion_ids, draws.future_time)
        future_pos = future_pos + draws.future_noise
        future_pos = future_pos - canon_pos
        future_pos = torch_util.quat_rotate(canon_heading_quat_inv, future_pos)
        future_rot = quat_multiply(canon_heading_quat_inv, future_rot)
        return self._types.TargetInfo(future_pos, future_rot)

    def _apply_boxes(self, hf, hf_maxmin, boxes):
        """add_boxes_to_hf2 (util/terrain_util.py:864-917) with its draws given: boxes [k, 6] as in SamplerDraws"""
        dev = hf.device
        x, y = torch.meshgrid(torch.arange(hf.shape[0], device=dev), torch.arange(hf.shape[1], device=dev), indexing="ij")
        xy = torch.stack([x, y], dim=-1).to(dtype=torch.float32)
        for b in range(boxes.shape[0]):
            center, length = boxes[b, 0:2], boxes[b, 2:4]
            angle = boxes[b, 4] * torch.ones_like(xy[:, :, 0])
            rot_xy = torch_util.rotate_2d_vec(xy - center, angle) + center
            in_x = torch.logical_and(rot_xy[..., 0] < center[0] + length[0] / 2, rot_xy[..., 0] > center[0] - length[0] / 2)
            in_y = torch.logical_and(rot_xy[..., 1] < center[1] + length[1] / 2, rot_xy[..., 1] > center[1] - length[1] / 2)
            hf[...] = torch.where(torch.logical_and(in_x, in_y), boxes[b, 5] * torch.ones_like(hf), hf)
        hf[...] = torch.clamp(hf, hf_maxmin[..., 1], hf_maxmin[..., 0])

    @staticmethod
    def _maxpool(hf, hf_maxmin, kind, r):
        """util/terrain_util.py:1595-1621: the pool, then the clamp to the band (also at radius 0)"""
        F = torch.nn.functional
        if kind == mb.POOL_2D:
            new_hf = F.max_pool2d(hf.unsqueeze(0), kernel_size=2 * r + 1, stride=1, padding=r).squeeze(0)
        elif kind == mb.POOL_X:
            new_hf = F.max_pool1d(hf.unsqueeze(0).permute(0, 2, 1), kernel_size=2 * r + 1, stride=1, padding=r).permute(0, 2, 1).squeeze(0)
        else:
            new_hf = F.max_pool1d(hf.unsqueeze(0), kernel_size=2 * r + 1, stride=1, padding=r).squeeze(0)
        hf[...] = torch.clamp(new_hf, hf_maxmin[..., 1], hf_maxmin[..., 0])

    def _augment(self, hf, hf_maxmin, draws, s):
        mode = self._mode()
        if mode == HFAugmentationMode.NOISE:
            # the band's maximum as the lower and its minimum as the upper bound, as the reference has them (:411)
            hf[...] = torch.clamp(draws.noise[s].to(hf.device), hf_maxmin[..., 0], hf_maxmin[..., 1])
        elif mode == HFAugmentationMode.MAXPOOL_AND_BOXES:
            if draws.change_height[s]:
                hf[...] = float(draws.new_height[s])
            for q in range(3):
                if draws.pool_kind[s, q] != mb.POOL_UNUSED:
                    self._maxpool(hf, hf_maxmin, int(draws.pool_kind[s, q]), int(draws.pool_radius[s, q]))
            nb = int(draws.num_boxes[s])
            self._apply_boxes(hf, hf_maxmin, torch.from_numpy(np.ascontiguousarray(draws.boxes[s, :nb])).to(hf.device))

    def get_hfs_from_data_helper(self, motion_ids, xy_points, motion_time_indices):
        hfs, hf_maxmins = [], []
        for i in range(len(motion_ids)):
            mid = int(motion_ids[i])
            ter = self._mlib._terrains[mid]
            hf_inds = ter.get_grid_index(xy_points[i])
            hf = ter.hf[hf_inds[..., 0], hf_inds[..., 1]]
            # python slicing clamps a window that runs past the clip's end
            lists = self._mlib._hf_mask_inds[mid][slice(int(motion_time_indices[i][0]), int(motion_time_indices[i][-1]) + 1)]
            mask = terrain_util.compute_hf_mask_from_inds(ter, lists).unsqueeze(-1).expand(size=[-1, -1, 2])
            band = torch.zeros_like(ter.hf_maxmin)
            band[..., 0] = self._max_h * 2.0
            band[..., -1] = self._min_h * 2.0
            band[mask] = ter.hf_maxmin[mask]
            hfs.append(hf)
            hf_maxmins.append(band[hf_inds[..., 0], hf_inds[..., 1], :])
        return hfs, hf_maxmins

    def get_hfs_from_data(self, motion_ids, ref_root_pos, ref_root_rot, canon_root_z, motion_time_indices, draws=None):
        """reference :449-488 -> (hfs [n, X, Y] before the final clamp, center_h [n]); without draws they are made here"""
        num_samples = ref_root_pos.shape[0]
        if draws is None:
            draws = SamplerDraws()
            self._draw_heightfields(num_samples, draws)
        pts = self._generic_heightmap.clone().unsqueeze(dim=0).expand(num_samples, -1, -1, -1)
        heading = torch_util.calc_heading(ref_root_rot).unsqueeze(-1).unsqueeze(-1).expand(-1, self._grid_dim_x, self._grid_dim_y)
        pts = torch_util.rotate_2d_vec(pts, heading) + ref_root_pos[:, 0:2].unsqueeze(1).unsqueeze(1)
        hfs, hf_maxmins = self.get_hfs_from_data_helper(motion_ids, pts, motion_time_indices)
        hfs, hf_maxmins = torch.stack(hfs, dim=0), torch.stack(hf_maxmins, dim=0)
        center_h = hfs[:, self._num_x_neg, self._num_y_neg].clone()
        R = self._types.RelativeZStyle
        if self._relative_z_style == R.RELATIVE_TO_ROOT_FLOOR:
            sub = center_h
        elif self._relative_z_style == R.RELATIVE_TO_ROOT:
            sub = canon_root_z
        else:
            assert False
        hfs = hfs - sub.unsqueeze(-1).unsqueeze(-1)
        hf_maxmins = hf_maxmins - sub.unsqueeze(-1).unsqueeze(-1).unsqueeze(-1)
        for i in range(hfs.shape[0]):
            self._augment(hfs[i], hf_maxmins[i], draws, i)
        return hfs, center_h

    def loop_batch(self, motion_ids, motion_start_times, draws, ret_hf_obs=True, ret_target_info=True):
        """the reference's sample_motion_data (:270-363) with the draws given; same dict as build_batch"""
        R = self._types.RelativeZStyle
        motion_start_time_indices = torch.round(motion_start_times / self._timestep).to(dtype=torch.int64)
        future_time_indices = torch.arange(start=0, end=self._seq_len, dtype=torch.int64, device=motion_start_times.device).unsqueeze(0)
        motion_time_indices = motion_start_time_indices.unsqueeze(-1) + future_time_indices
        root_pos, root_rot, _, _, joint_rot, _, contacts = self._extract_motion_data(motion_ids, motion_start_times, self._motion_times, self._seq_len)
        canon_root_pos = root_pos[:, self._ref_frame_idx, :].clone()
        canon_root_rot = root_rot[:, self._ref_frame_idx, :].clone()
        canon_root_z = canon_root_pos[:, 2].clone()
        out = {}
        if ret_hf_obs:
            hfs, center_h = self.get_hfs_from_data(motion_ids, canon_root_pos, canon_root_rot, canon_root_z, motion_time_indices.cpu(), draws)
            out["hfs"], out["center_h"] = torch.clamp(hfs, min=self._min_h, max=self._max_h), center_h
            if self._relative_z_style == R.RELATIVE_TO_ROOT_FLOOR:
                root_pos = root_pos.clone()
                root_pos[..., 2] = root_pos[..., 2] - center_h.unsqueeze(-1)
        root_pos = root_pos - canon_root_pos.unsqueeze(1)
        canon_heading_quat_inv = torch_util.calc_heading_quat_inv(canon_root_rot)
        root_rot = quat_multiply(canon_heading_quat_inv.unsqueeze(1), root_rot)
        root_pos = torch_util.quat_rotate(canon_heading_quat_inv.unsqueeze(1), root_pos)
        if isinstance(self._mlib, TorchMotionLib):
            body_pos, _ = forward_kinematics_reference_order(self._kin_char_model, root_pos, root_rot, joint_rot)
        else:
            body_pos, _ = self._kin_char_model.forward_kinematics(root_pos, root_rot, joint_rot)
        out.update(root_pos=root_pos, root_rot=root_rot, body_pos=body_pos[..., 1:, :], joint_rot=joint_rot, contacts=contacts)
        if ret_target_info:
            target = self._sample_target_info(motion_ids, motion_start_times, canon_root_pos, canon_heading_quat_inv, draws)
            out["future_pos"], out["future_rot"] = target.future_pos, target.future_rot
        return out
