"""The motion generator's training loss: MDM.extract_motion_features followed by MDM.motion_difference of the reference
(diffusion/mdm.py:382-478, 617-754, compute_point_hf_sdf :978-1028), per sample of a training batch.

Two paths give the same terms.  The torch path (`extract_motion_features` + `motion_difference`) restates the reference in torch ops;
it runs anywhere and autograd differentiates it.  The device path hands the denoiser's output to parc_mdm_loss_forward
(include/parc_mdm_loss.h): one launch for the 14 terms of every sample, one more for `predicted_x_0.grad`, no dense
[points, columns] distance tensor.  `MDMMotionLoss._path` says which one an instance takes and `._path_reason` why;
`last_path` / `last_path_reason` say what the last call took (data with FLOOR_HEIGHTS, or a window that does not fit a workgroup's
LDS, falls back to the torch path for that call).
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from ..util import geom_util, torch_util
from . import diffusion_util

# rows of the device path's [14, B] output, in the order motion_difference inserts its keys, with the weight each one takes
_TERMS = [("VEL_ROOT_POS_LOSS", "w_vel_root_pos"), ("VEL_ROOT_ROT_LOSS", "w_vel_root_rot"), ("VEL_JOINT_ROT_LOSS", "w_vel_joint_rot"),
          ("SIMPLE_ROOT_POS_LOSS", "w_simple_root_pos"), ("SIMPLE_ROOT_ROT_LOSS", "w_simple_root_rot"),
          ("SIMPLE_JOINT_ROT_LOSS", "w_simple_joint_rot"), ("SIMPLE_CONTACT_LOSS", "w_simple_contacts"),
          ("SIMPLE_BODY_POS_LOSS", "w_simple_body_pos"), ("FK_BODY_POS_LOSS", "w_body_pos"), ("FK_BODY_ROT_LOSS", "w_body_rot"),
          ("BODY_POS_CONSISTENCY_LOSS", "w_body_pos_consistency"), ("VEL_FK_BODY_POS_LOSS", "w_body_vel"), ("HF_COLLISION_LOSS", "w_hf"),
          ("TARGET_LOSS", "w_target")]
_DEVICE_COMPONENTS = ("ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS")
_LOSS_FNS = {"squared_l2": 0, "pseudo_huber": 1, "squared_l2_loss_fn": 0, "pseudo_huber_loss_fn": 1}


def squared_l2_loss_fn(x, y):
    loss = (x - y) ** 2
    return torch.sum(loss.reshape(loss.shape[0], -1), dim=-1)


def pseudo_huber_loss_fn(x, y):
    loss = (x - y) ** 2 + 0.0009
    return torch.sqrt(torch.sum(loss.reshape(loss.shape[0], -1), dim=-1)) - 0.03


def points_hf_sdf_dense(points, hf, hf_min_box_center, hf_dxdy, base_z):
    """The inverted column distance of util/terrain_util.py:1835-1893 in torch ops: points [B, N, 3], hf [B, X, Y] -> [B, N], negative
    inside the ground.  Dense ([B, N, X * Y, 3] temporaries): the torch path's terrain term, which autograd differentiates."""
    B, X, Y = hf.shape
    dev = points.device
    xs = torch.linspace(0.0, (X - 1.0) * hf_dxdy[0].item(), X, device=dev)
    ys = torch.linspace(0.0, (Y - 1.0) * hf_dxdy[1].item(), Y, device=dev)
    x, y = torch.meshgrid(xs, ys, indexing="ij")
    x = x.unsqueeze(0) + hf_min_box_center[:, 0].reshape(B, 1, 1)
    y = y.unsqueeze(0) + hf_min_box_center[:, 1].reshape(B, 1, 1)
    top_z = -base_z
    z, hz = (hf + top_z) / 2.0, (top_z - hf) / 2.0
    centers = torch.stack([x, y, z], dim=-1).reshape(B, 1, X * Y, 3)
    half = torch.cat([(hf_dxdy / 2.0).expand(B, X * Y, 2), hz.reshape(B, X * Y, 1)], dim=-1).unsqueeze(1)
    q = (points.unsqueeze(2) - centers).abs() - half
    sd = torch.linalg.vector_norm(q.clamp(min=0.0), dim=-1) + q.max(dim=-1)[0].clamp(max=0.0)
    return -torch.min(sd, dim=-1)[0]


class MDMMotionLoss:
    def __init__(self, cfg, char_model, feature_mean, feature_std, types=None, path=None):
        """cfg: the generator's configuration (features.frame_components, features.rot_type, sequence_fps, num_prev_states, the w_*
        weights, use_pos_loss, use_hf_collision_loss, use_target_loss, target_type, target_dir_len_eps, heightmap.*, device).
        feature_mean / feature_std [S, D]: the trainer's _mdm_features_mean / _std.  types: a namespace with MDMFrameType and LossType
        that replaces parc_amd.diffusion.diffusion_util (the reference's own modules, for a hand-over).  path: 'device' or 'torch'
        to override the choice."""
        self._types = types
        self.MDMFrameType = getattr(types, "MDMFrameType", diffusion_util.MDMFrameType)
        self.LossType = getattr(types, "LossType", diffusion_util.LossType)
        self._cfg = cfg
        self._char_model = char_model
        self._device = torch.device(cfg.get("device", char_model._device))
        feats = cfg["features"]
        self._rot_type = str(feats.get("rot_type", "DEFAULT"))
        self._component_names = [str(c) for c in feats["frame_components"]]
        self._frame_components = [self.MDMFrameType[c] for c in self._component_names]
        self._sequence_fps = cfg["sequence_fps"]
        self._num_prev_states = int(cfg["num_prev_states"])
        self._w = [float(cfg.get(name, 0.0)) for _, name in _TERMS]
        self._w_floor_height = float(cfg.get("w_floor_height", 0.0))
        self._use_vel_loss = True
        self._use_simple_loss = True
        self._use_pos_loss = bool(cfg["use_pos_loss"])
        self._use_hf_collision_loss = bool(cfg["use_hf_collision_loss"])
        self._use_target_loss = bool(cfg["use_target_loss"])
        self._target_type = str(cfg.get("target_type", "XY_DIR"))
        self._target_dir_len_eps = float(cfg.get("target_dir_len_eps", 0.0))
        hm = cfg["heightmap"]
        grid = hm["local_grid"]
        self._num_x_neg, self._num_y_neg = int(grid["num_x_neg"]), int(grid["num_y_neg"])
        self._grid_dim_x = 1 + self._num_x_neg + int(grid["num_x_pos"])
        self._grid_dim_y = 1 + self._num_y_neg + int(grid["num_y_pos"])
        self._dx = hm["horizontal_scale"]
        self._dxdy = torch.tensor([self._dx, self._dx], dtype=torch.float32, device=self._device)
        self._max_h = hm["max_h"]
        self._min_h = -self._max_h
        self._mdm_features_mean = torch.as_tensor(feature_mean, dtype=torch.float32).to(self._device)
        self._mdm_features_std = torch.as_tensor(feature_std, dtype=torch.float32).to(self._device)
        self._register_mdm_features()
        assert self._mdm_features_mean.shape[-1] == self._motion_frame_dof and self._mdm_features_std.shape == self._mdm_features_mean.shape
        self._char_point_samples = geom_util.get_minimal_char_point_samples(char_model) if self._use_hf_collision_loss else None
        self._device_tables = None
        self._path, self._path_reason = self._choose_path(path)
        self.last_path, self.last_path_reason = None, None

    # ------------------------------------------------------------------ feature layout (reference :329-364)
    def _register_mdm_features(self):
        km, T = self._char_model, self.MDMFrameType
        J = km.get_num_non_root_joints()
        if self._rot_type in ("DEFAULT", "EXP_MAP"):
            root_dim = 3
            joint_dim = km.get_dof_size() if self._rot_type == "DEFAULT" else 3 * J
        elif self._rot_type == "QUAT":
            root_dim, joint_dim = 4, 4 * J
        else:
            raise NotImplementedError("rot_type {} is not restated here (DEFAULT, EXP_MAP and QUAT are)".format(self._rot_type))
        dims = {T.ROOT_POS: 3, T.ROOT_ROT: root_dim, T.JOINT_POS: 3 * J, T.JOINT_ROT: joint_dim, T.JOINT_VEL: 3 * J,
                T.CONTACTS: km.get_num_joints()}
        self._feature_slices = dict()
        idx = 0
        for comp in self._frame_components:
            if comp not in dims:
                raise NameError(comp)
            self._feature_slices[comp] = slice(idx, idx + dims[comp])
            idx += dims[comp]
        self._motion_frame_dof = idx

    def standardize_features(self, mdm_features):
        seq_len = mdm_features.shape[1]
        return (mdm_features - self._mdm_features_mean[:seq_len, :]) / self._mdm_features_std[:seq_len, :]

    def unstandardize_features(self, mdm_features):
        seq_len = mdm_features.shape[1]
        return mdm_features * self._mdm_features_std[:seq_len, :] + self._mdm_features_mean[:seq_len, :]

    def unnormalize_hf(self, hf):
        return hf * self._max_h

    # ------------------------------------------------------------------ rotations of the feature layout
    def _rot_to_dof(self, rot):
        """KinCharModel.rot_to_dof in torch ops (reference anim/kin_char_model.py:79-100, :493-507)."""
        km = self._char_model
        dof = torch.zeros(rot.shape[:-2] + (km.get_dof_size(),), dtype=rot.dtype, device=rot.device)
        for j in range(1, km.get_num_joints()):
            joint = km.get_joint(j)
            n = joint.get_dof_dim()
            if n == 1:
                axis, angle = torch_util.quat_to_axis_angle(rot[..., j - 1, :])
                j_axis = torch.as_tensor(np.asarray(joint.axis.detach().cpu() if torch.is_tensor(joint.axis) else joint.axis),
                                         dtype=rot.dtype, device=rot.device)
                angle = torch.where(torch.sum(j_axis * axis, dim=-1) < 0, -angle, angle)
                dof[..., joint.dof_idx] = angle
            elif n == 3:
                dof[..., joint.dof_idx:joint.dof_idx + 3] = torch_util.quat_to_exp_map(rot[..., j - 1, :])
        return dof

    def _quat_to_rot_type(self, q):
        return q if self._rot_type == "QUAT" else torch_util.quat_to_exp_map(q)

    def _rot_type_to_quat(self, r):
        return r if self._rot_type == "QUAT" else torch_util.exp_map_to_quat(r)

    def assemble_mdm_features(self, ml_component_dict, standardize=True):
        """dictionary of motion components -> [B, S, D] features, in the order of frame_components (reference :382-432)"""
        T = self.MDMFrameType
        parts = []
        for comp in self._frame_components:
            v = ml_component_dict[comp]
            if comp == T.ROOT_ROT:
                v = self._quat_to_rot_type(v)
            elif comp == T.JOINT_POS:
                v = v.reshape(v.shape[0], v.shape[1], -1)
            elif comp == T.JOINT_ROT:
                v = self._rot_to_dof(v) if self._rot_type == "DEFAULT" else self._quat_to_rot_type(v).reshape(v.shape[0], v.shape[1], -1)
            parts.append(v)
        feats = torch.cat(parts, dim=-1)
        return self.standardize_features(feats) if standardize else feats

    def extract_motion_features(self, mdm_features, unstandardize=True):
        """[B, S, D] features -> dictionary of motion components, rotations as quaternions (reference :434-478)"""
        T = self.MDMFrameType
        if unstandardize:
            mdm_features = self.unstandardize_features(mdm_features)
        out = dict()
        for comp in self._frame_components:
            v = mdm_features[..., self._feature_slices[comp]]
            if comp == T.ROOT_ROT:
                v = self._rot_type_to_quat(v)
            elif comp == T.JOINT_POS:
                v = v.reshape(v.shape[0], v.shape[1], self._char_model.get_num_non_root_joints(), 3)
            elif comp == T.JOINT_ROT:
                if self._rot_type == "DEFAULT":
                    v = self._char_model.dof_to_rot_torch(v)
                else:
                    v = self._rot_type_to_quat(v.reshape(v.shape[0], v.shape[1], self._char_model.get_num_non_root_joints(), -1))
            elif comp == T.JOINT_VEL:
                continue
            out[comp] = v
        return out

    # ------------------------------------------------------------------ the torch path (reference :617-754)
    def compute_point_hf_sdf(self, body_pos, body_rot, body_points, hfs, base_z=-10.0):
        B = body_pos.shape[0]
        localized = []
        for b in range(self._char_model.get_num_joints()):
            pts = body_points[b].unsqueeze(0).unsqueeze(0)
            rot = body_rot[..., b, :].unsqueeze(2).expand(body_rot.shape[:2] + (pts.shape[2], 4))
            world = torch_util.quat_rotate(rot, pts.expand(rot.shape[:-1] + (3,))) + body_pos[..., b, :].unsqueeze(2)
            localized.append(world.reshape(B, -1, 3))
        localized = torch.cat(localized, dim=1)
        neg = torch.tensor([self._num_x_neg, self._num_y_neg], dtype=torch.float32, device=self._dxdy.device)
        min_box_center = (-self._dxdy * neg).unsqueeze(0).expand(B, 2)
        if hfs.dim() == 4:
            hfs = hfs.squeeze(1)
        return points_hf_sdf_dense(localized, hfs, min_box_center, self._dxdy, base_z)

    def motion_difference(self, true_motion_data, pred_motion_data, hfs_normalized, target_dir, loss_fn):
        """-> dict LossType -> [B], the reference's keys in its insertion order; loss_fn: 'squared_l2', 'pseudo_huber' or a callable"""
        T, LT, km = self.MDMFrameType, self.LossType, self._char_model
        if isinstance(loss_fn, str):
            loss_fn = {"squared_l2": squared_l2_loss_fn, "pseudo_huber": pseudo_huber_loss_fn}[loss_fn]
        w = dict((name, v) for (name, _), v in zip(_TERMS, self._w))
        dt = 1.0 / self._sequence_fps
        losses = OrderedDict()
        root_pos_true, root_pos_pred = true_motion_data[T.ROOT_POS], pred_motion_data[T.ROOT_POS]
        root_rot_true, root_rot_pred = true_motion_data[T.ROOT_ROT], pred_motion_data[T.ROOT_ROT]
        joint_rot_true, joint_rot_pred = true_motion_data[T.JOINT_ROT], pred_motion_data[T.JOINT_ROT]
        body_pos_pred, body_rot_pred = km.forward_kinematics_torch(root_pos_pred, root_rot_pred, joint_rot_pred)
        body_pos_true, body_rot_true = km.forward_kinematics_torch(root_pos_true, root_rot_true, joint_rot_true)
        ang_vel = lambda q: torch_util.quat_to_exp_map(torch_util.quat_diff(q[:, :-1], q[:, 1:])) / dt
        if self._use_vel_loss:
            losses[LT.VEL_ROOT_POS_LOSS] = w["VEL_ROOT_POS_LOSS"] * loss_fn((root_pos_true[:, 1:] - root_pos_true[:, :-1]) / dt,
                                                                           (root_pos_pred[:, 1:] - root_pos_pred[:, :-1]) / dt)
            losses[LT.VEL_ROOT_ROT_LOSS] = w["VEL_ROOT_ROT_LOSS"] * loss_fn(ang_vel(root_rot_true), ang_vel(root_rot_pred))
            losses[LT.VEL_JOINT_ROT_LOSS] = w["VEL_JOINT_ROT_LOSS"] * loss_fn(ang_vel(joint_rot_true), ang_vel(joint_rot_pred))
        has_joint_pos = T.JOINT_POS in true_motion_data and T.JOINT_POS in pred_motion_data
        if self._use_simple_loss:
            losses[LT.SIMPLE_ROOT_POS_LOSS] = w["SIMPLE_ROOT_POS_LOSS"] * loss_fn(root_pos_true, root_pos_pred)
            losses[LT.SIMPLE_ROOT_ROT_LOSS] = w["SIMPLE_ROOT_ROT_LOSS"] * loss_fn(torch_util.quat_diff_angle(root_rot_true, root_rot_pred), 0.0)
            losses[LT.SIMPLE_JOINT_ROT_LOSS] = w["SIMPLE_JOINT_ROT_LOSS"] * loss_fn(torch_util.quat_diff_angle(joint_rot_true, joint_rot_pred), 0.0)
            if T.CONTACTS in true_motion_data and T.CONTACTS in pred_motion_data:
                losses[LT.SIMPLE_CONTACT_LOSS] = w["SIMPLE_CONTACT_LOSS"] * loss_fn(true_motion_data[T.CONTACTS], pred_motion_data[T.CONTACTS])
            if T.FLOOR_HEIGHTS in true_motion_data:
                losses[LT.SIMPLE_FLOOR_HEIGHT_LOSS] = self._w_floor_height * loss_fn(true_motion_data[T.FLOOR_HEIGHTS],
                                                                                     pred_motion_data[T.FLOOR_HEIGHTS])
            if has_joint_pos:
                simple_body_pos_pred = pred_motion_data[T.JOINT_POS]
                losses[LT.SIMPLE_BODY_POS_LOSS] = w["SIMPLE_BODY_POS_LOSS"] * loss_fn(body_pos_true[..., 1:, :], simple_body_pos_pred)
        if self._use_pos_loss:
            losses[LT.FK_BODY_POS_LOSS] = w["FK_BODY_POS_LOSS"] * loss_fn(body_pos_true, body_pos_pred)
            losses[LT.FK_BODY_ROT_LOSS] = w["FK_BODY_ROT_LOSS"] * loss_fn(torch_util.quat_diff_angle(body_rot_true, body_rot_pred), 0.0)
            if has_joint_pos:
                losses[LT.BODY_POS_CONSISTENCY_LOSS] = w["BODY_POS_CONSISTENCY_LOSS"] * loss_fn(body_pos_pred[..., 1:, :], simple_body_pos_pred)
            if self._use_vel_loss:
                losses[LT.VEL_FK_BODY_POS_LOSS] = w["VEL_FK_BODY_POS_LOSS"] * loss_fn((body_pos_true[:, 1:] - body_pos_true[:, :-1]) / dt,
                                                                                     (body_pos_pred[:, 1:] - body_pos_pred[:, :-1]) / dt)
        if self._use_hf_collision_loss:
            sdf = self.compute_point_hf_sdf(body_pos_pred, body_rot_pred, self._char_point_samples, self.unnormalize_hf(hfs_normalized),
                                            base_z=self._min_h - 5.0)
            losses[LT.HF_COLLISION_LOSS] = w["HF_COLLISION_LOSS"] * (0.5 * torch.sum(torch.square(torch.clamp(sdf, max=0.0)), dim=-1))
        if self._use_target_loss:
            if self._target_type == "XY_DIR":
                td = target_dir.squeeze(1) if target_dir.dim() == 3 else target_dir
                unnorm_pred_dir = root_pos_pred[:, -1, 0:2] - root_pos_pred[:, self._num_prev_states - 1, 0:2]
                target_loss = torch.clamp(torch.sum(-td * unnorm_pred_dir, dim=-1), min=-self._target_dir_len_eps)
                losses[LT.TARGET_LOSS] = target_loss * w["TARGET_LOSS"]
            else:
                losses[LT.TARGET_LOSS] = torch.zeros(root_pos_pred.shape[0], dtype=root_pos_pred.dtype, device=root_pos_pred.device)
        return losses

    # ------------------------------------------------------------------ the device path
    def _choose_path(self, forced):
        if forced == "torch":
            return "torch", "asked for"
        reason = None
        if self._rot_type != "DEFAULT":
            reason = "rot_type {} (the kernels take DEFAULT)".format(self._rot_type)
        elif len(set(self._component_names)) != len(self._component_names) or not set(self._component_names) <= set(_DEVICE_COMPONENTS):
            reason = "frame_components {} (the kernels take each of {} once)".format(self._component_names, list(_DEVICE_COMPONENTS))
        elif not {"ROOT_POS", "ROOT_ROT", "JOINT_ROT"} <= set(self._component_names):
            reason = "frame_components without ROOT_POS, ROOT_ROT or JOINT_ROT"
        elif self._use_target_loss and self._target_type != "XY_DIR":
            reason = "target_type {} (the kernels take XY_DIR)".format(self._target_type)
        elif self._device.type != "cuda":
            reason = "device {} is not a HIP device".format(self._device)
        if reason is None:
            return "device", "HIP device, rot_type DEFAULT, components {}".format(self._component_names)
        if forced == "device":
            raise ValueError("the device path cannot take this configuration: " + reason)
        return "torch", reason

    def _tables(self):
        """What every launch shares: the point table, the grid's cell centres, and the fixed part of parc_mdm_loss_cfg_t."""
        if self._device_tables is None:
            from .. import _hip_mdm_loss as H
            km, dev = self._char_model, self._device
            nb = km.get_num_joints()
            samples = self._char_point_samples if self._char_point_samples is not None else [torch.zeros((0, 3)) for _ in range(nb)]
            points, start, P = diffusion_util.pack_body_points(samples, dev)
            c = H.MdmLossCfgS()
            diffusion_util.set_feature_layout(c, self)
            diffusion_util.set_local_grid(c, self)
            c.ref_idx = self._num_prev_states - 1
            c.dim_x, c.dim_y, c.num_points = self._grid_dim_x, self._grid_dim_y, P
            c.max_h, c.base_z = float(self._max_h), float(self._min_h - 5.0)
            c.dt, c.target_eps = 1.0 / self._sequence_fps, self._target_dir_len_eps
            for t, v in enumerate(self._w):
                c.w[t] = v
            grid_x, grid_y = diffusion_util.local_grid_axes(self)
            self._device_tables = {"cfg": c, "points": points, "start": start, "grid_x": grid_x, "grid_y": grid_y}
        return self._device_tables

    def _enabled_terms(self, true_motion_data):
        """bit t set = term t of _TERMS is computed, as motion_difference decides it"""
        T = self.MDMFrameType
        has_contacts = "CONTACTS" in self._component_names and T.CONTACTS in true_motion_data
        has_joint_pos = "JOINT_POS" in self._component_names and T.JOINT_POS in true_motion_data
        on = [True] * 6 + [has_contacts, has_joint_pos, self._use_pos_loss, self._use_pos_loss, self._use_pos_loss and has_joint_pos,
                           self._use_pos_loss, self._use_hf_collision_loss, self._use_target_loss]
        return sum(1 << t for t, v in enumerate(on) if v)

    def _device_cfg(self, seq_len, loss_fn, enabled):
        """parc_mdm_loss_cfg_t of a call; it depends on (S, loss_fn, enabled terms) alone and is built once for each"""
        return self._device_cfg_entry(seq_len, loss_fn, enabled)[0]

    def _device_cfg_entry(self, seq_len, loss_fn, enabled):
        cache = self._tables().setdefault("cfgs", {})
        key = (seq_len, loss_fn, enabled)
        if key not in cache:
            from .. import _hip_mdm_loss as H
            c = H.MdmLossCfgS()
            ctypes.memmove(ctypes.byref(c), ctypes.byref(self._tables()["cfg"]), ctypes.sizeof(c))
            c.seq_len, c.loss_fn, c.enabled = seq_len, loss_fn, enabled
            # a component whose term is off for this call is still a slice of x: its columns get zero gradient
            cache[key] = [c, None]
        return cache[key]

    def _device_lds_bytes(self, seq_len, loss_fn, enabled):
        """LDS bytes a workgroup needs for that configuration (asked of the library once)"""
        entry = self._device_cfg_entry(seq_len, loss_fn, enabled)
        if entry[1] is None:
            from .. import _hip
            entry[1] = int(_hip.lib().parc_mdm_loss_lds_bytes(self._char_model.c_struct(), entry[0]))
        return entry[1]

    def _device_call_reason(self, true_motion_data, predicted_x_0, loss_fn):
        """None when this call can take the device path, else why not"""
        T = self.MDMFrameType
        if T.FLOOR_HEIGHTS in true_motion_data:
            return "FLOOR_HEIGHTS in the data"
        name = loss_fn if isinstance(loss_fn, str) else getattr(loss_fn, "__name__", "")
        if name not in _LOSS_FNS:
            return "loss_fn {!r} (the kernels take squared_l2 and pseudo_huber)".format(loss_fn)
        if predicted_x_0.dtype != torch.float32 or not predicted_x_0.is_cuda or predicted_x_0.dim() != 3 or \
                predicted_x_0.shape[2] != self._motion_frame_dof:
            return "predicted_x_0 is not a [B, S, {}] float32 device tensor".format(self._motion_frame_dof)
        if predicted_x_0.shape[1] > self._mdm_features_mean.shape[0] or predicted_x_0.shape[1] < self._num_prev_states:
            return "sequence length {}".format(predicted_x_0.shape[1])
        from .. import _hip_mdm_loss as H
        need = self._device_lds_bytes(int(predicted_x_0.shape[1]), _LOSS_FNS[name], self._enabled_terms(true_motion_data))
        if need > H.MAX_LDS:
            return "a window of {} frames needs {} bytes of LDS per workgroup ({} at the most)".format(predicted_x_0.shape[1], need, H.MAX_LDS)
        return None

    def _device_losses(self, true_motion_data, predicted_x_0, hfs_normalized, target_dir, loss_fn):
        T = self.MDMFrameType
        B, S, _ = predicted_x_0.shape
        dev = predicted_x_0.device
        name = loss_fn if isinstance(loss_fn, str) else loss_fn.__name__
        enabled = self._enabled_terms(true_motion_data)
        c = self._device_cfg(int(S), _LOSS_FNS[name], enabled)
        f32 = lambda t, shape: t.detach().to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
        nb = self._char_model.get_num_joints()
        contacts = f32(true_motion_data[T.CONTACTS], (B, S, nb)) if c.off_contacts >= 0 and T.CONTACTS in true_motion_data else \
            (torch.zeros((B, S, nb), dtype=torch.float32, device=dev) if c.off_contacts >= 0 else None)
        X, Y = self._grid_dim_x, self._grid_dim_y
        hfs = f32(hfs_normalized, (B, X, Y)) if self._use_hf_collision_loss else torch.zeros((B, X, Y), dtype=torch.float32, device=dev)
        td = f32(target_dir, (B, 2)) if self._use_target_loss else torch.zeros((B, 2), dtype=torch.float32, device=dev)
        tensors = (self._mdm_features_mean[:S].contiguous(), self._mdm_features_std[:S].contiguous(), f32(true_motion_data[T.ROOT_POS], (B, S, 3)),
                   f32(true_motion_data[T.ROOT_ROT], (B, S, 4)), f32(true_motion_data[T.JOINT_ROT], (B, S, nb - 1, 4)), contacts, hfs, td)
        out = _MDMLossFn.apply(predicted_x_0, self, c, tensors)
        losses = OrderedDict()
        for t, (key, _) in enumerate(_TERMS):
            if (enabled >> t) & 1:
                losses[self.LossType[key]] = out[t]          # a selection of the one [14, B] output: in-place edits reach its cotangent
        return losses

    # ------------------------------------------------------------------ public
    def __call__(self, true_motion_data, predicted_x_0, hfs_normalized, target_dir, loss_fn="squared_l2"):
        """-> OrderedDict LossType -> [B], the reference's keys in its insertion order."""
        reason = None
        if self._path == "device":
            reason = self._device_call_reason(true_motion_data, predicted_x_0, loss_fn)
            if reason is None:
                self.last_path, self.last_path_reason = "device", self._path_reason
                return self._device_losses(true_motion_data, predicted_x_0, hfs_normalized, target_dir, loss_fn)
        self.last_path, self.last_path_reason = "torch", reason if reason is not None else self._path_reason
        pred = self.extract_motion_features(predicted_x_0)
        return self.motion_difference(true_motion_data, pred, hfs_normalized, target_dir, loss_fn)

    def reduce(self, losses, ood_mask=None):
        """The trainer's reduction: zero every term but HF_COLLISION and TARGET for the out-of-distribution samples (in place, reference
        :936-940), then the sum of the terms' batch means in insertion order (:953-958)."""
        LT = self.LossType
        if ood_mask is not None:          # an all-false mask edits nothing: no host read to find out
            for key in losses:
                if key == LT.HF_COLLISION_LOSS or key == LT.TARGET_LOSS:
                    continue
                losses[key][ood_mask] *= 0.0
        loss = 0.0
        for key in losses:
            loss = loss + losses[key].mean()
        return loss


class _MDMLossFn(torch.autograd.Function):
    """losses [14, B] of x [B, S, D]: parc_mdm_loss_forward, and parc_mdm_loss_backward when autograd asks for x.grad"""

    @staticmethod
    def forward(ctx, x, owner, cfg, tensors):
        from .. import _hip, _hip_mdm_loss as H
        xc = x.detach().contiguous()
        B = int(xc.shape[0])
        tab = owner._tables()
        out = torch.empty((H.TERMS, B), dtype=torch.float32, device=xc.device)
        args = [_hip.ptr(t) for t in tensors] + [_hip.ptr(tab["grid_x"]), _hip.ptr(tab["grid_y"]), _hip.ptr(tab["points"]), _hip.ptr(tab["start"])]
        _hip.check(_hip.lib().parc_mdm_loss_forward(_hip.stream(), owner._char_model.c_struct(), cfg, B, _hip.ptr(xc), *args, _hip.ptr(out)),
                   "parc_mdm_loss_forward")
        ctx.owner, ctx.cfg, ctx.tensors = owner, cfg, tensors
        ctx.save_for_backward(xc)
        return out

    @staticmethod
    def backward(ctx, g):
        from .. import _hip
        (xc,) = ctx.saved_tensors
        owner, tab = ctx.owner, ctx.owner._tables()
        B = int(xc.shape[0])
        gc = g.to(torch.float32).contiguous()
        g_x = torch.empty_like(xc)
        args = [_hip.ptr(t) for t in ctx.tensors] + [_hip.ptr(tab["grid_x"]), _hip.ptr(tab["grid_y"]), _hip.ptr(tab["points"]), _hip.ptr(tab["start"])]
        _hip.check(_hip.lib().parc_mdm_loss_backward(_hip.stream(), owner._char_model.c_struct(), ctx.cfg, B, _hip.ptr(xc), *args, _hip.ptr(gc),
                                                     _hip.ptr(g_x)), "parc_mdm_loss_backward")
        return g_x, None, None, None
