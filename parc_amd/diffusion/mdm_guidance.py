"""The motion generator's guidance step: MDM.apply_guidance of the reference (diffusion/mdm.py:1444-1542), for a whole batch.

After a denoising step the predicted clean motion is moved down the gradient of a guidance loss of up to five terms (distance of the
root to a target, penetration of the character's surface points into the local heightfield, hinges on the first, second and third
differences of the body positions): x <- x - guidance_str * dL/dx.  The loss is a sum over the batch, so every sample gets what the
reference gives for that sample alone.

Two paths give the same update.  The torch path restates the reference in torch ops and differentiates with autograd; it runs anywhere.
The device path hands x to parc_mdm_guide_step (include/parc_mdm_guide.h): loss, gradient and update of every sample in one launch, in
place.  `MDMGuidance._path` says which one an instance takes and `._path_reason` why; `last_path` / `last_path_reason` say what the
last call took (a window that does not fit a workgroup's LDS, or a target that differs from frame to frame, falls back to the torch
path for that call).

The difference terms follow the reference as written: `body_pos[..., 1:, :] - body_pos[..., :-1, :]` on body_pos [B, S, bodies, 3]
runs over the bodies of a frame, not over frames.

Hand-over to a reference MDM object `mdm_model`:

    guide = MDMGuidance(cfg, char_model, mdm_model._mdm_features_mean, mdm_model._mdm_features_std, types=diffusion.diffusion_util)
    mdm_model.apply_guidance = guide.apply_guidance
"""
import torch

from . import diffusion_util
from .mdm_loss import MDMMotionLoss

TERM_NAMES = ("target", "hf", "speed", "acc", "jerk")      # rows of the [5, B] terms, in the order the reference adds them
_DEVICE_COMPONENTS = ("ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS")
_BASE_Z = -10.0          # compute_point_hf_sdf's default, which apply_guidance takes


def guidance_params_from_settings(settings, target, char_model, types=None):
    """The guidance parameters gen_mdm_motion builds from its MDMGenSettings (reference diffusion/gen_util.py:173-199).
    target: the canonicalised target [B, 1, 2].  -> (params, attach): attach says whether gen_util puts them into conds at all."""
    from ..util import geom_util
    params = getattr(types, "MDMCustomGuidance", diffusion_util.MDMCustomGuidance)()
    if settings.use_cfg:
        params.obs_cfg_scale = settings.cfg_scale
    if settings.target_guidance:
        params.guidance_str = settings.guidance_str
        params.target_xy = target
    if settings.hf_collision_guidance:
        params.guidance_str = settings.guidance_str
        params.body_points = geom_util.get_char_point_samples(char_model)
    attach = bool(settings.use_cfg or settings.target_guidance or settings.hf_collision_guidance or settings.strong_hf_guidance)
    if attach:
        params.strong_hf_guidance = settings.strong_hf_guidance
    params.guide_speed, params.guide_acc, params.guide_jerk = settings.guide_speed, settings.guide_acc, settings.guide_jerk
    params.w_speed, params.w_acc, params.w_jerk = settings.w_speed, settings.w_acc, settings.w_jerk
    params.max_jerk = settings.max_jerk
    return params, attach


class MDMGuidance:
    def __init__(self, cfg, char_model, feature_mean, feature_std, types=None, path=None):
        """cfg, char_model, feature_mean / feature_std [S, D], types, path: as MDMMotionLoss takes them (types may also carry
        MDMKeyType).  path: 'device' or 'torch' to override the choice."""
        self._features = MDMMotionLoss(cfg, char_model, feature_mean, feature_std, types=types, path="torch")
        self.MDMFrameType = self._features.MDMFrameType
        self.MDMKeyType = getattr(types, "MDMKeyType", diffusion_util.MDMKeyType)
        self._char_model = char_model
        self._device = self._features._device
        self._sequence_fps = self._features._sequence_fps
        self._packed = {}          # id(body_points) -> (body_points, points [P, 3], point_start [nb + 1], P)
        self._lds = {}             # (S, P) -> bytes
        self._grid = None
        self._path, self._path_reason = self._choose_path(path)
        self.last_path, self.last_path_reason = None, None

    # ------------------------------------------------------------------ which terms
    @staticmethod
    def _check_params(gp):
        if getattr(gp, "strong_hf_guidance", False):
            raise NotImplementedError("strong_hf_guidance (predict_x0_hf_guidance) calls the denoiser; MDMGuidance restates apply_guidance alone")

    def _enabled(self, gp, conds):
        """bit t set = term t of TERM_NAMES is part of the loss, as apply_guidance decides it"""
        on = [gp.target_xy is not None, gp.body_points is not None and self.MDMKeyType.OBS_KEY in conds,
              bool(gp.guide_speed), bool(gp.guide_acc), bool(gp.guide_jerk)]
        return sum(1 << t for t, v in enumerate(on) if v)

    @staticmethod
    def _weights(gp):
        return [float(gp.w_target_loss), float(gp.w_hf_loss), float(gp.w_speed), float(gp.w_acc), float(gp.w_jerk)]

    # ------------------------------------------------------------------ the torch path
    def _torch_step(self, x_t, gp, conds, enabled):
        """the reference's algorithm, batch and all -> unweighted terms [5, B]; x_t updated in place"""
        F, T = self._features, self.MDMFrameType
        on = lambda t: (enabled >> t) & 1
        w = self._weights(gp)
        B = x_t.shape[0]
        with torch.enable_grad():
            new_x_t = x_t.detach().clone().requires_grad_(True)
            feats = F.extract_motion_features(new_x_t)
            root_pos, root_rot, joint_rot = feats[T.ROOT_POS], feats[T.ROOT_ROT], feats[T.JOINT_ROT]
            terms = [torch.zeros(B, dtype=x_t.dtype, device=x_t.device) for _ in TERM_NAMES]
            if on(0):
                target = torch.as_tensor(gp.target_xy, dtype=x_t.dtype, device=x_t.device)
                terms[0] = 0.5 * torch.sum(torch.square(target - root_pos[..., 0:2]).reshape(B, -1), dim=-1)
            if enabled >> 1:
                body_pos, body_rot = self._char_model.forward_kinematics_torch(root_pos, root_rot, joint_rot)
                if on(1):
                    hfs = F.unnormalize_hf(conds[self.MDMKeyType.OBS_KEY])
                    sdf = F.compute_point_hf_sdf(body_pos, body_rot, gp.body_points, hfs, base_z=_BASE_Z)
                    terms[1] = 0.5 * torch.sum(torch.square(torch.clamp(sdf, max=0.0)), dim=-1)
                dt = 1.0 / self._sequence_fps
                diff = body_pos
                for k, rate in ((1, gp.max_speed), (2, gp.max_acc), (3, gp.max_jerk)):
                    diff = diff[..., 1:, :] - diff[..., :-1, :]          # the second-to-last axis of [B, S, bodies, 3]: as the reference has it
                    if on(1 + k):
                        mag = torch.norm(diff, dim=-1)
                        terms[1 + k] = torch.sum(torch.clamp(mag - rate * dt ** k, min=0.0).reshape(B, -1), dim=-1)
            loss = 0.0
            for t in range(len(TERM_NAMES)):
                if on(t):
                    loss = loss + torch.sum(terms[t]) * w[t]
            grad = torch.autograd.grad(loss, new_x_t)[0]
        x_t[...] = (new_x_t.detach() - grad * gp.guidance_str)
        return torch.stack([t.detach() for t in terms])

    # ------------------------------------------------------------------ the device path
    def _choose_path(self, forced):
        F = self._features
        if forced == "torch":
            return "torch", "asked for"
        names = F._component_names
        reason = None
        if F._rot_type != "DEFAULT":
            reason = "rot_type {} (the kernel takes DEFAULT)".format(F._rot_type)
        elif len(set(names)) != len(names) or not set(names) <= set(_DEVICE_COMPONENTS):
            reason = "frame_components {} (the kernel takes each of {} once)".format(names, list(_DEVICE_COMPONENTS))
        elif not {"ROOT_POS", "ROOT_ROT", "JOINT_ROT"} <= set(names):
            reason = "frame_components without ROOT_POS, ROOT_ROT or JOINT_ROT"
        elif self._device.type != "cuda":
            reason = "device {} is not a HIP device".format(self._device)
        if reason is None:
            return "device", "HIP device, rot_type DEFAULT, components {}".format(names)
        if forced == "device":
            raise ValueError("the device path cannot take this configuration: " + reason)
        return "torch", reason

    def pack_points(self, body_points):
        """per-body list -> (points [max(P, 1), 3], point_start [nb + 1] int32, P) on the device; packed once per distinct list"""
        key = id(body_points)
        hit = self._packed.get(key)
        if hit is None or hit[0] is not body_points:
            assert len(body_points) == self._char_model.get_num_joints()
            hit = (body_points,) + diffusion_util.pack_body_points(body_points, self._device)
            self._packed[key] = hit
        return hit[1:]

    def device_cfg(self, S, gp, enabled, P):
        """parc_mdm_guide_cfg_t of a call"""
        from .. import _hip_mdm_guide as H
        F = self._features
        c = H.MdmGuideCfgS()
        diffusion_util.set_feature_layout(c, F)
        diffusion_util.set_local_grid(c, F)
        c.seq_len = int(S)
        c.dim_x, c.dim_y, c.enabled, c.num_points = F._grid_dim_x, F._grid_dim_y, enabled, int(P)
        c.max_h, c.base_z = float(F._max_h), _BASE_Z
        c.guidance_str = float(gp.guidance_str)
        for t, v in enumerate(self._weights(gp)):
            c.w[t] = v
        c.dt = 1.0 / self._sequence_fps
        c.max_rate[0], c.max_rate[1], c.max_rate[2] = float(gp.max_speed), float(gp.max_acc), float(gp.max_jerk)
        return c

    def _grid_points(self):
        if self._grid is None:
            self._grid = diffusion_util.local_grid_axes(self._features)
        return self._grid

    def _lds_bytes(self, c):
        key = (c.seq_len, c.num_points)
        if key not in self._lds:
            from .. import _hip
            self._lds[key] = int(_hip.lib().parc_mdm_guide_lds_bytes(self._char_model.c_struct(), c))
        return self._lds[key]

    def _device_call(self, x_t, gp, conds, enabled):
        """-> (None, launch arguments) when this call can take the device path, else (why not, None)"""
        from .. import _hip_mdm_guide as H
        F = self._features
        D = F._motion_frame_dof
        if x_t.dtype != torch.float32 or not x_t.is_cuda or x_t.dim() != 3 or x_t.shape[2] != D:
            return "x_t is not a [B, S, {}] float32 device tensor".format(D), None
        B, S, _ = x_t.shape
        if S > F._mdm_features_mean.shape[0]:
            return "sequence length {}".format(S), None
        target = None
        if enabled & 1:
            target = torch.as_tensor(gp.target_xy, dtype=torch.float32, device=x_t.device)
            if target.dim() == 3 and target.shape[1] != 1:
                return "a target per frame (the kernel takes one per sample)", None
            target = target.reshape(-1, 2).expand(B, 2).contiguous()
        points, start, P = self.pack_points(gp.body_points) if enabled & 2 else (None, None, 0)
        c = self.device_cfg(S, gp, enabled, P)
        need = self._lds_bytes(c)
        if need > H.MAX_LDS:
            return "a window of {} frames with {} points needs {} bytes of LDS per workgroup ({} at the most)".format(S, P, need, H.MAX_LDS), None
        hfs = None
        if enabled & 2:
            hfs = conds[self.MDMKeyType.OBS_KEY].detach().to(device=x_t.device, dtype=torch.float32).reshape(B, c.dim_x, c.dim_y).contiguous()
        return None, (c, target, hfs, points, start)

    def _device_step(self, x_t, args):
        from .. import _hip, _hip_mdm_guide as H
        c, target, hfs, points, start = args
        B, S, _ = x_t.shape
        F = self._features
        gx, gy = self._grid_points() if hfs is not None else (None, None)
        xc = x_t if x_t.is_contiguous() else x_t.contiguous()
        terms = torch.empty((H.TERMS, B), dtype=torch.float32, device=x_t.device)
        p = _hip.ptr
        _hip.check(_hip.lib().parc_mdm_guide_step(_hip.stream(), self._char_model.c_struct(), c, int(B), p(xc), p(F._mdm_features_mean[:S].contiguous()),
                                                  p(F._mdm_features_std[:S].contiguous()), p(hfs), p(target), p(gx), p(gy), p(points), p(start), p(xc),
                                                  p(terms)), "parc_mdm_guide_step")
        if xc is not x_t:
            x_t.copy_(xc)
        return terms

    # ------------------------------------------------------------------ public
    def guidance_step(self, x_t, guidance_params, conds):
        """One guidance step on x_t [B, S, D], in place -> the unweighted per-sample terms [5, B] (rows TERM_NAMES), or None when no
        guidance is enabled (x_t is then untouched).  Nothing is read back or waited for."""
        self._check_params(guidance_params)
        enabled = self._enabled(guidance_params, conds)
        if not enabled:
            return None
        reason = None
        if self._path == "device":
            reason, args = self._device_call(x_t, guidance_params, conds, enabled)
            if reason is None:
                self.last_path, self.last_path_reason = "device", self._path_reason
                return self._device_step(x_t, args)
        self.last_path, self.last_path_reason = "torch", reason if reason is not None else self._path_reason
        return self._torch_step(x_t, guidance_params, conds, enabled)

    def apply_guidance(self, x_t, conds):
        """MDM.apply_guidance: reads conds[GUIDANCE_PARAMS] (and conds[OBS_KEY] for the terrain term), updates x_t in place, returns
        None.  With guidance_params.verbose (the reference's default) it prints the reference's lines, summed over the batch: the one
        host read of this module."""
        gp = conds[self.MDMKeyType.GUIDANCE_PARAMS]
        terms = self.guidance_step(x_t, gp, conds)
        if terms is None or not gp.verbose:
            return
        enabled, w = self._enabled(gp, conds), self._weights(gp)
        totals = terms.sum(dim=1).tolist()
        labels = (("target_loss:", "scaled target loss:"), ("hf_loss:", "scaled hf_loss:"), ("speed_loss:", "scaled speed_loss:"),
                  ("acc_loss:", "scaled acc_loss:"), ("jerk_loss:", "scaled jerk_loss:"))
        for t, (plain, scaled) in enumerate(labels):
            if (enabled >> t) & 1:
                print(plain, totals[t])
                print(scaled, totals[t] * w[t])
        return
