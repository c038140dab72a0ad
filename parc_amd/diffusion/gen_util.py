"""The call that drives a motion generator: gen_mdm_motion of the reference (diffusion/gen_util.py) with the head and tail of
MDM.gen_sequence_with_contacts (diffusion/mdm.py:1338-1398), for a whole batch.

For every sample the previous frames are canonicalised about frame num_prev_states - 1 (its root over the origin, its heading along
+x), the rotated local heightfield is read off the terrain, forward kinematics gives the body positions, the target becomes a
direction and the previous-state features are assembled and standardised (`MDMGenIO.encode`); the conditions go to the model's
sampling loop; the returned sample becomes world-frame MotionFrames (`MDMGenIO.decode`).  The denoiser and the sampling loop are the
model's own: this module builds what every generator needs around them.

Two paths give the same values.  The torch path restates the reference in torch ops; it runs anywhere.  The device path is
parc_mdm_gen_encode and parc_mdm_gen_decode (include/parc_mdm_gen.h): one launch each for the whole batch.  `MDMGenIO._path` says which
one an instance takes and `._path_reason` why; `last_path` / `last_path_reason` say what the last encode took (frames or a terrain
that are not on the instance's HIP device fall back to the torch path for that call, and decode follows its encode).

A model with `ddim_inference` and `reverse_diffusion` (a reference MDM, or anything with those two methods) is driven in feature mode:
conds hold standardised features and the normalised heightfield, exactly what the reference's sampling loop receives, and decode takes
the returned [B, S, D].  A model with `gen_sequence_with_contacts` alone is driven in component mode: conds hold the component
dictionary of gen_util.py:139-145 and the returned component dictionary is un-canonicalised in torch ops.

RELATIVE_TO_ROOT_FLOOR: the reference's branch (gen_util.py:104-111) indexes the batch axis in get_hf_val and raises for B != 2; here
it has its evident per-sample meaning (heights relative to the terrain cell under the canonical root).

Not here: in-painting (`input_root_pos`), `_use_feature_vector`, the path-following driver of tools/procgen/mdm_path.py.
"""
import enum
import sys

import torch

from ..util import geom_util, torch_util
from ..util.motion_util import MotionFrames
from . import diffusion_util
from .mdm_guidance import guidance_params_from_settings
from .mdm_loss import MDMMotionLoss
_DEVICE_COMPONENTS = ("ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS")

# the attributes MotionGenDeepMimicEnv reads from its planner
FIELDS = ("_num_prev_states", "_sequence_fps", "_dx", "_dy", "_num_x_neg", "_num_x_pos", "_num_y_neg", "_num_y_pos", "_target_type")


class MDMGenSettings:
    """reference diffusion/gen_util.py:12-33: class attributes as defaults"""
    use_prev_state = True
    use_cfg = True
    cfg_scale = 0.65
    guide_speed = False
    guide_acc = False
    guide_jerk = False
    w_speed = 0.1
    w_acc = 0.1
    w_jerk = 0.1
    max_jerk = 1000.0
    strong_hf_guidance = False
    target_guidance = False
    hf_collision_guidance = False
    prev_state_ind_key = True
    target_condition_key = True
    feature_vector_key = True
    use_ddim = True
    ddim_stride = 10
    guidance_str = 0.1
    input_root_pos = False
    starting_diffusion_timestep = 0


class GenContext:
    """what decode needs of its encode: the heading frame of every sample and the previous state"""

    def __init__(self, path, B, canon_xy, heading_quat, z_ref, heading, frame, prev_state, no_noise, root_pos, root_rot, body_pos, hf_z, target,
                 target_dir):
        self.path, self.B = path, B
        self.canon_xy, self.heading_quat, self.z_ref, self.heading = canon_xy, heading_quat, z_ref, heading      # [B, 2], [B, 4], [B], [B]
        self.frame = frame                                    # [B, 8], the device path's record (None on the torch path)
        self.prev_state, self.no_noise = prev_state, no_noise      # [B, P, D] standardised (None in component mode), [B] bool
        self.root_pos, self.root_rot, self.body_pos = root_pos, root_rot, body_pos          # canonical [B, T, ...]; body_pos without the root
        self.hf_z, self.target, self.target_dir = hf_z, target, target_dir                  # [B, X, Y], [B, 1, 2], [B, 1, 2]


def _same_device(a, b):
    """torch.device("cuda") names the current device: equal to "cuda:<current>" """
    index = lambda d: d.index if d.index is not None or d.type != "cuda" else torch.cuda.current_device()
    return a.type == b.type and index(a) == index(b)


def _flag(value, B, device):
    """a bool or a [B] tensor in the settings -> [B] bool (gen_util.py:162-171)"""
    if isinstance(value, torch.Tensor):
        return value
    return torch.tensor([value], dtype=torch.bool, device=device).expand(B)


class MDMGenIO:
    def __init__(self, cfg, char_model, mean, std, types=None, path=None):
        """cfg, char_model, mean / std [S, D], types, path: as MDMGuidance takes them.  Further keys of cfg, all optional:
        relative_z_style (RELATIVE_TO_ROOT), target_type (XY_DIR), use_heightmap_obs (True), use_target_obs (True),
        use_feature_vector (False)."""
        self._features = MDMMotionLoss(cfg, char_model, mean, std, types=types, path="torch")
        F = self._features
        self._types = types
        self.MDMFrameType = F.MDMFrameType
        self.MDMKeyType = getattr(types, "MDMKeyType", diffusion_util.MDMKeyType)
        self._char_model = char_model
        self._device = F._device
        self._num_prev_states, self._sequence_fps = F._num_prev_states, F._sequence_fps
        z_style = cfg.get("relative_z_style", "RELATIVE_TO_ROOT")
        self._relative_z_style = str(getattr(z_style, "name", z_style))
        if self._relative_z_style not in ("RELATIVE_TO_ROOT", "RELATIVE_TO_ROOT_FLOOR"):
            raise ValueError("relative_z_style {!r}".format(self._relative_z_style))
        self._target_type = F._target_type
        self._use_heightmap_obs = bool(cfg.get("use_heightmap_obs", True))
        self._use_target_obs = bool(cfg.get("use_target_obs", True))
        self._use_feature_vector = bool(cfg.get("use_feature_vector", False))
        grid = cfg["heightmap"]["local_grid"]
        self._dx = self._dy = F._dx
        self._num_x_neg, self._num_x_pos = int(grid["num_x_neg"]), int(grid["num_x_pos"])
        self._num_y_neg, self._num_y_pos = int(grid["num_y_neg"]), int(grid["num_y_pos"])
        self._local_xy, self._grid, self._terrains = None, None, {}
        self._path, self._path_reason = self._choose_path(path)
        self.last_path, self.last_path_reason = None, None

    @classmethod
    def from_model(cls, model, char_model, types=None, path=None):
        """the instance of a reference MDM object (or a stand-in with its attributes): layout, grid and statistics are read off it"""
        cfg = {"device": model._device, "sequence_fps": model._sequence_fps, "num_prev_states": model._num_prev_states,
               "features": {"frame_components": [getattr(c, "name", str(c)) for c in model._frame_components],
                            "rot_type": getattr(getattr(getattr(model, "_rot_changer", None), "rot_type", None), "name", "DEFAULT")},
               "use_pos_loss": False, "use_hf_collision_loss": False, "use_target_loss": False,
               "target_type": getattr(getattr(model, "_target_type", None), "name", "XY_DIR"),
               "relative_z_style": getattr(model, "_relative_z_style", "RELATIVE_TO_ROOT"),
               "use_heightmap_obs": getattr(model, "_use_heightmap_obs", True), "use_target_obs": getattr(model, "_use_target_obs", True),
               "use_feature_vector": getattr(model, "_use_feature_vector", False),
               "heightmap": {"local_grid": {"num_x_neg": model._num_x_neg, "num_x_pos": model._num_x_pos, "num_y_neg": model._num_y_neg,
                                            "num_y_pos": model._num_y_pos},
                             "horizontal_scale": model._dx, "max_h": model._max_h}}
        assert model._dy == model._dx, "the local grid is square-celled"
        if types is None and len(model._frame_components) and isinstance(model._frame_components[0], enum.Enum):
            # the model's own enums key its conds: the module that defines its MDMFrameType (the reference's diffusion.diffusion_util
            # for a reference MDM) stands in for `types` when it carries MDMKeyType too
            module = sys.modules.get(type(model._frame_components[0]).__module__)
            if hasattr(module, "MDMKeyType") and hasattr(module, "MDMFrameType"):
                types = module
        return cls(cfg, char_model, model._mdm_features_mean, model._mdm_features_std, types=types, path=path)

    # ------------------------------------------------------------------ which path
    def _choose_path(self, forced):
        F = self._features
        if forced == "torch":
            return "torch", "asked for"
        names = F._component_names
        reason = None
        if F._rot_type != "DEFAULT":
            reason = "rot_type {} (the kernels take DEFAULT)".format(F._rot_type)
        elif len(set(names)) != len(names) or not set(names) <= set(_DEVICE_COMPONENTS):
            reason = "frame_components {} (the kernels take each of {} once)".format(names, list(_DEVICE_COMPONENTS))
        elif not {"ROOT_POS", "ROOT_ROT", "JOINT_ROT"} <= set(names):
            reason = "frame_components without ROOT_POS, ROOT_ROT or JOINT_ROT"
        elif self._target_type != "XY_DIR":
            reason = "target_type {} (the kernels take XY_DIR)".format(self._target_type)
        elif self._device.type != "cuda":
            reason = "device {} is not a HIP device".format(self._device)
        if reason is None:
            return "device", "HIP device, rot_type DEFAULT, components {}".format(names)
        if forced == "device":
            raise ValueError("the device path cannot take this configuration: " + reason)
        return "torch", reason

    def _device_call_reason(self, target_world_pos, prev_frames, terrain):
        """None when this call can take the device path, else why not"""
        dev = self._device
        for name, t in (("root_pos", prev_frames.root_pos), ("root_rot", prev_frames.root_rot), ("joint_rot", prev_frames.joint_rot),
                        ("contacts", prev_frames.contacts), ("terrain.hf", terrain.hf), ("target", target_world_pos)):
            if t is None:
                if name == "contacts" and "CONTACTS" not in self._features._component_names:
                    continue
                return "prev_frames.{} is missing".format(name)
            if not _same_device(t.device, dev) or (name != "target" and t.dtype != torch.float32):
                return "{} is not a float32 tensor on {}".format(name, dev)
        return None

    # ------------------------------------------------------------------ shared pieces
    def _check_settings(self, settings):
        if getattr(settings, "input_root_pos", False):
            raise NotImplementedError("input_root_pos (in-painting of the future root positions) is not restated here")
        if self._use_feature_vector:
            raise NotImplementedError("_use_feature_vector: the reference's gen_mdm_motion never sets FEATURE_VECTOR_KEY; not restated here")
        if self._target_type != "XY_DIR":
            raise NotImplementedError("target_type {} (gen_mdm_motion asserts XY_DIR)".format(self._target_type))

    def local_xy_points(self):
        """[X, Y, 2] local grid, coordinates from the host's linspace (geom_util.get_xy_grid_points)"""
        if self._local_xy is None:
            self._local_xy = geom_util.get_xy_grid_points(torch.zeros(2), self._dx, self._dy, self._num_x_neg, self._num_x_pos, self._num_y_neg,
                                                          self._num_y_pos).to(self._device)
        return self._local_xy

    def _grid_points(self):
        if self._grid is None:
            xy = self.local_xy_points()
            self._grid = (xy[:, 0, 0].contiguous(), xy[0, :, 1].contiguous())
        return self._grid

    def device_cfg(self, T, S):
        """parc_mdm_gen_cfg_t of a call with T previous frames (encode) / S sample frames (decode)"""
        from .. import _hip_mdm_gen as H
        F = self._features
        c = H.MdmGenCfgS()
        diffusion_util.set_feature_layout(c, F)
        c.num_frames, c.seq_len, c.num_prev_states = int(T), int(S), self._num_prev_states
        c.dim_x, c.dim_y = F._grid_dim_x, F._grid_dim_y
        c.z_style = H.Z_ROOT_FLOOR if self._relative_z_style == "RELATIVE_TO_ROOT_FLOOR" else H.Z_ROOT
        c.rot_type = {"DEFAULT": H.ROT_DEFAULT, "EXP_MAP": H.ROT_EXP_MAP, "QUAT": H.ROT_QUAT}[F._rot_type]
        c.min_h, c.max_h = float(F._min_h), float(F._max_h)
        return c

    def _conds(self, ctx, settings, obs, prev_state, char_model=None):
        """the dictionary the sampling loop receives (gen_util.py:136-199)"""
        K, B, dev = self.MDMKeyType, ctx.B, self._device
        conds = dict()
        conds[K.OBS_KEY] = obs
        conds[K.OBS_FLAG_KEY] = _flag(True, B, dev)
        conds[K.PREV_STATE_KEY] = prev_state
        conds[K.PREV_STATE_NOISE_IND_KEY] = _flag(settings.use_prev_state, B, dev)
        conds[K.TARGET_KEY] = ctx.target_dir
        conds[K.TARGET_FLAG_KEY] = _flag(settings.target_condition_key, B, dev)
        conds[K.PREV_STATE_FLAG_KEY] = _flag(settings.prev_state_ind_key, B, dev)
        params, attach = guidance_params_from_settings(settings, ctx.target, char_model if char_model is not None else self._char_model, self._types)
        if attach:
            conds[K.GUIDANCE_PARAMS] = params
        return conds

    # ------------------------------------------------------------------ the torch path
    def _encode_torch(self, target_world_pos, prev_frames, terrain):
        F, km, P = self._features, self._char_model, self._num_prev_states
        c = P - 1
        B, T = prev_frames.root_pos.shape[0], prev_frames.root_pos.shape[1]
        canon_xy = prev_frames.root_pos[:, c:c + 1, 0:2]
        rr_c = prev_frames.root_rot[:, c:c + 1]
        heading = torch_util.calc_heading(rr_c)                                       # [B, 1]
        hq, hq_inv = torch_util.calc_heading_quat(rr_c), torch_util.calc_heading_quat_inv(rr_c)
        root_pos = prev_frames.root_pos.clone()
        root_pos[..., 0:2] -= canon_xy
        root_pos = torch_util.quat_rotate(hq_inv.expand(B, T, 4), root_pos)
        root_rot = torch_util.quat_mul(hq_inv.expand(B, T, 4), prev_frames.root_rot)
        local = self.local_xy_points().to(canon_xy.device)
        pts = torch_util.rotate_2d_vec(local, heading.unsqueeze(1)) + canon_xy.unsqueeze(1)
        hf_z = terrain.get_hf_val_from_points(pts)
        if self._relative_z_style == "RELATIVE_TO_ROOT_FLOOR":
            z_ref = terrain.get_hf_val_from_points(canon_xy)                          # [B, 1]: the cell under every sample's own root
        else:
            z_ref = prev_frames.root_pos[:, c:c + 1, 2]
        root_pos[..., 2] -= z_ref
        hf_z = hf_z - z_ref.unsqueeze(-1)
        body_pos, _ = km.forward_kinematics_torch(root_pos, root_rot, prev_frames.joint_rot)
        target = target_world_pos[:, 0:2].to(dtype=torch.float32).unsqueeze(1) - canon_xy
        target = torch_util.rotate_2d_vec(target, -heading)
        target_dir = torch.nn.functional.normalize(target, dim=-1)
        return GenContext("torch", B, canon_xy[:, 0], hq[:, 0], z_ref[:, 0], heading[:, 0], None, None, None, root_pos, root_rot,
                          body_pos[..., 1:, :], hf_z, target, target_dir)

    def _components(self, ctx, prev_frames, n):
        """the component dictionary of the first n canonical frames (gen_util.py:139-145)"""
        T = self.MDMFrameType
        d = {T.ROOT_POS: ctx.root_pos[:, :n], T.ROOT_ROT: ctx.root_rot[:, :n], T.JOINT_POS: ctx.body_pos[:, :n], T.JOINT_ROT: prev_frames.joint_rot[:, :n]}
        if prev_frames.contacts is not None:
            d[T.CONTACTS] = prev_frames.contacts[:, :n]
        return d

    def _uncanonicalize(self, ctx, root_pos, root_rot):
        """gen_util.py:211-218"""
        B, S = root_pos.shape[0], root_pos.shape[1]
        hq = ctx.heading_quat.unsqueeze(1).expand(B, S, 4)
        new_rot = torch_util.quat_mul(hq, root_rot)
        new_pos = torch_util.quat_rotate(hq, root_pos)
        new_pos[..., 0:2] = new_pos[..., 0:2] + ctx.canon_xy.unsqueeze(1)
        new_pos[..., 2] += ctx.z_ref.unsqueeze(1)
        return new_pos, new_rot

    def mlib_rows(self, root_pos, root_rot, joint_rot):
        """[..., 6 + dofs] = root position, root exponential map, joint dofs in torch ops: the rows a MotionLib takes"""
        return torch.cat([root_pos, torch_util.quat_to_exp_map(root_rot), self._features._rot_to_dof(joint_rot)], dim=-1)

    def _decode_torch(self, ctx, out):
        F, T, P = self._features, self.MDMFrameType, self._num_prev_states
        if ctx.prev_state is not None:
            keep = ctx.no_noise.to(out.device).unsqueeze(-1).unsqueeze(-1)
            out = torch.cat([torch.where(keep, ctx.prev_state, out[:, 0:P]), out[:, P:, :]], dim=1)
        feats = F.extract_motion_features(out)
        root_pos, root_rot = self._uncanonicalize(ctx, feats[T.ROOT_POS], feats[T.ROOT_ROT])
        ret = MotionFrames(root_pos=root_pos, root_rot=root_rot, joint_rot=feats[T.JOINT_ROT], contacts=feats.get(T.CONTACTS))
        ret.frames = self.mlib_rows(root_pos, root_rot, feats[T.JOINT_ROT])
        return ret

    # ------------------------------------------------------------------ the device path
    def _terrain_struct(self, terrain):
        """parc_terrain_t of a terrain.  min_point and dxdy are read to the host once per terrain object and height array (the one
        read-back of this module); a terrain whose min_point or dxdy are changed in place afterwards needs a new MDMGenIO."""
        from .. import _hip
        hit = self._terrains.get(id(terrain))
        if hit is None or hit[0] is not terrain or hit[1].data_ptr() != terrain.hf.data_ptr() or hit[1].shape != terrain.hf.shape:
            hf = terrain.hf if terrain.hf.is_contiguous() else terrain.hf.contiguous()
            hit = (terrain, hf, _hip.terrain_struct(hf, terrain.min_point.tolist(), terrain.dxdy.tolist()))
            self._terrains = {id(terrain): hit}          # the last terrain only: nothing else is kept alive
        return hit[2]

    def _encode_device(self, target_world_pos, prev_frames, terrain, with_features):
        from .. import _hip
        F, km, P, dev = self._features, self._char_model, self._num_prev_states, self._device
        B, T = int(prev_frames.root_pos.shape[0]), int(prev_frames.root_pos.shape[1])
        J, D, X, Y = km.get_num_joints() - 1, F._motion_frame_dof, F._grid_dim_x, F._grid_dim_y
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        frame, rp, rr, bp = new(B, 8), new(B, T, 3), new(B, T, 4), new(B, T, J, 3)
        hf_z, target, target_dir = new(B, X, Y), new(B, 1, 2), new(B, 1, 2)
        prev_state, obs = (new(B, P, D), new(B, 1, X, Y)) if with_features else (None, None)
        gx, gy = self._grid_points()
        ter = self._terrain_struct(terrain)
        cont = prev_frames.contacts.contiguous() if (with_features and "CONTACTS" in F._component_names) else None
        tw = target_world_pos[:, 0:2].to(dtype=torch.float32).contiguous()
        p = _hip.ptr
        _hip.check(_hip.lib().parc_mdm_gen_encode(
            _hip.stream(), km.c_struct(), self.device_cfg(T, T), ter, B, p(prev_frames.root_pos.contiguous()), p(prev_frames.root_rot.contiguous()),
            p(prev_frames.joint_rot.contiguous()), p(cont), p(tw), p(gx), p(gy), p(F._mdm_features_mean), p(F._mdm_features_std), p(frame), p(rp),
            p(rr), p(bp), p(hf_z), p(target), p(target_dir), p(prev_state), p(obs)), "parc_mdm_gen_encode")
        ctx = GenContext("device", B, frame[:, 0:2], frame[:, 2:6], frame[:, 6], frame[:, 7], frame, prev_state, None, rp, rr, bp, hf_z, target,
                         target_dir)
        return ctx, obs

    def _decode_device(self, ctx, out):
        from .. import _hip
        F, km, dev = self._features, self._char_model, self._device
        B, S, D = out.shape
        J, nb, dofs = km.get_num_joints() - 1, km.get_num_joints(), km.get_dof_size()
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        rp, rr, jr, frames = new(B, S, 3), new(B, S, 4), new(B, S, J, 4), new(B, S, 6 + dofs)
        contacts = new(B, S, nb) if "CONTACTS" in F._component_names else None
        keep = ctx.no_noise.to(device=dev, dtype=torch.bool).contiguous().view(torch.uint8) if ctx.prev_state is not None else None
        x = out if out.is_contiguous() else out.contiguous()
        p = _hip.ptr
        _hip.check(_hip.lib().parc_mdm_gen_decode(
            _hip.stream(), km.c_struct(), self.device_cfg(S, S), B, p(x), p(ctx.prev_state), p(keep), p(F._mdm_features_mean[:S]),
            p(F._mdm_features_std[:S]), p(ctx.frame), p(rp), p(rr), p(jr), p(contacts), p(frames)), "parc_mdm_gen_decode")
        ret = MotionFrames(root_pos=rp, root_rot=rr, joint_rot=jr, contacts=contacts)
        ret.frames = frames
        return ret

    # ------------------------------------------------------------------ public
    def encode(self, target_world_pos, prev_frames, terrain, settings, components=False, char_model=None):
        """-> (conds, ctx).  conds: the keys and shapes the reference's sampling loop receives (feature mode), or, with components=True,
        what MDM.gen_sequence_with_contacts receives (component mode).  Nothing is read back or waited for."""
        self._check_settings(settings)
        P = self._num_prev_states
        T = prev_frames.root_pos.shape[1]
        if not 1 <= P <= T:
            raise ValueError("num_prev_states {} with {} previous frames".format(P, T))
        reason = None
        if self._path == "device":
            reason = self._device_call_reason(target_world_pos, prev_frames, terrain)
        if self._path == "device" and reason is None:
            self.last_path, self.last_path_reason = "device", self._path_reason
            ctx, obs = self._encode_device(target_world_pos, prev_frames, terrain, not components)
            prev_state = ctx.prev_state
        else:
            self.last_path, self.last_path_reason = "torch", reason if reason is not None else self._path_reason
            ctx = self._encode_torch(target_world_pos, prev_frames, terrain)
            obs = prev_state = None
            if not components:
                F = self._features
                obs = torch.clamp(ctx.hf_z.unsqueeze(dim=1), min=F._min_h, max=F._max_h) / F._max_h
                prev_state = ctx.prev_state = F.assemble_mdm_features(self._components(ctx, prev_frames, P))
        dev = self._device
        if components:
            conds = self._conds(ctx, settings, ctx.hf_z.to(dev), {k: v.to(dev) for k, v in self._components(ctx, prev_frames, P).items()}, char_model)
        else:
            conds = self._conds(ctx, settings, (obs if self._use_heightmap_obs else ctx.hf_z).to(dev), prev_state.to(dev), char_model)
        ctx.no_noise = conds[self.MDMKeyType.PREV_STATE_NOISE_IND_KEY]
        return conds, ctx

    def decode(self, ctx, out):
        """the sampler's standardised [B, S, D] -> world-frame MotionFrames (body_pos / body_rot None, as the reference returns them),
        with the attribute `frames` [B, S, 6 + dofs]: the rows a MotionLib takes"""
        if ctx.path == "device" and out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and \
                self._num_prev_states <= out.shape[1] <= self._features._mdm_features_mean.shape[0]:
            return self._decode_device(ctx, out)
        return self._decode_torch(ctx, out.to(ctx.root_pos.device))

    def decode_components(self, ctx, mdm_ret, device):
        """component mode's tail (gen_util.py:205-225): the model's component dictionary, un-canonicalised in torch ops"""
        T = self.MDMFrameType
        root_pos, root_rot = self._uncanonicalize(ctx, mdm_ret[T.ROOT_POS].to(device), mdm_ret[T.ROOT_ROT].to(device))
        contacts = mdm_ret[T.CONTACTS].to(device) if T.CONTACTS in mdm_ret else None
        return MotionFrames(root_pos=root_pos, root_rot=root_rot, joint_rot=mdm_ret[T.JOINT_ROT].to(device), contacts=contacts)


def gen_mdm_motion(target_world_pos, prev_frames, terrain, mdm_model, char_model, mdm_settings, verbose=True, io=None):
    """The reference's gen_mdm_motion (same arguments; it prints nothing).  io: the MDMGenIO of mdm_model, built from the model's
    attributes when not given (MDMGenerator builds it once)."""
    assert mdm_model is not None, "MDM not loaded"
    input_device = prev_frames.root_pos.device
    assert terrain.hf.device == input_device and target_world_pos.device == input_device
    if io is None:
        io = MDMGenIO.from_model(mdm_model, char_model)
    if hasattr(mdm_model, "ddim_inference") and hasattr(mdm_model, "reverse_diffusion"):
        conds, ctx = io.encode(target_world_pos, prev_frames, terrain, mdm_settings, char_model=char_model)
        denoiser = getattr(mdm_model, "_denoise_model", None)
        if hasattr(denoiser, "eval"):
            denoiser.eval()
        # the dispatch of mdm.py:1381-1390
        if mdm_settings.use_ddim:
            assert mdm_settings.ddim_stride is not None
            sample = mdm_model.ddim_inference(conds=conds, stride=mdm_settings.ddim_stride)
        else:
            timesteps = mdm_model._diffusion_timesteps if "timesteps" not in conds else conds["timesteps"]
            sample = mdm_model.reverse_diffusion(conds=conds, start_timestep=timesteps)
        return io.decode(ctx, sample)
    if hasattr(mdm_model, "gen_sequence_with_contacts"):
        conds, ctx = io.encode(target_world_pos, prev_frames, terrain, mdm_settings, components=True, char_model=char_model)
        modes = getattr(io._types, "GenerationMode", diffusion_util.GenerationMode)
        mode = modes.MODE_DDIM if mdm_settings.use_ddim else modes.MODE_REVERSE_DIFFUSION
        return io.decode_components(ctx, mdm_model.gen_sequence_with_contacts(conds, mdm_settings.ddim_stride, mode=mode), input_device)
    raise TypeError("mdm_model has neither ddim_inference / reverse_diffusion nor gen_sequence_with_contacts")


class MDMGenerator:
    """The callable MotionGenDeepMimicEnv wants, around a model the user has loaded: (target_xy, prev_frames, terrain, char_model,
    settings) -> MotionFrames, with the attributes the env reads from its planner (FIELDS).  It opens no file."""

    def __init__(self, model, io=None):
        self._model = model
        self._io = io
        for name in FIELDS:
            if hasattr(model, name):
                setattr(self, name, getattr(model, name))

    def __call__(self, target_xy, prev_frames, terrain, char_model, settings):
        if self._io is None:
            self._io = MDMGenIO.from_model(self._model, char_model)
        s = MDMGenSettings()          # every field the env sets is carried over (cfg_scale included)
        for k in vars(type(settings)).keys() | vars(settings).keys():
            if not k.startswith("_") and hasattr(s, k):
                setattr(s, k, getattr(settings, k))
        return gen_mdm_motion(target_xy, prev_frames, terrain, self._model, char_model, s, verbose=False, io=self._io)
