"""Base of the generator's samplers (reference diffusion/motion_sampler.py:69-128): the clip database, the character, and the start-time
rule.  On a HIP device the database is parc_amd.anim.motion_lib.MotionLib (frames in HBM, sampled by kernels); with cfg['device'] = 'cpu'
it is TorchMotionLib below - the same files and tables, the lookup written with torch ops - so the sampler's loop path runs without a GPU."""
import numpy as np
import torch

from ..anim import kin_char_model, motion_lib
from ..anim.motion_lib import LoopMode
from ..util import torch_util


class TorchMotionLib(motion_lib.MotionLib):
    """MotionLib for a CPU device: reads the same files into the same per-clip tables, keeps the per-frame arrays the reference keeps
    (_frame_root_pos, _frame_root_rot, _frame_joint_rot, _frame_contacts) and restates calc_motion_frame (reference :80-112, :443-475,
    :528-538) with torch ops.  It serves the sampler: the three velocity entries of calc_motion_frame are None (nothing here derives
    them), and there is no C struct."""

    def _build(self, clips):
        km, dev = self._kin_char_model, self._device
        nf = np.array([c["frames"].shape[0] for c in clips], dtype=np.int64)
        fps = np.array([c["fps"] for c in clips], dtype=np.float64)
        w = torch.tensor([c["weight"] for c in clips], dtype=torch.float32, device=dev)
        self._motion_weights = w / w.sum()
        self._motion_fps = torch.tensor(fps, dtype=torch.float32, device=dev)
        self._motion_dt = torch.tensor(1.0 / fps, dtype=torch.float32, device=dev)
        self._motion_num_frames = torch.tensor(nf, dtype=torch.long, device=dev)
        self._motion_lengths = torch.tensor(1.0 / fps * (nf - 1), dtype=torch.float32, device=dev)
        self._motion_loop_modes = torch.tensor([c["loop"] for c in clips], dtype=torch.int, device=dev)
        self._motion_start_idx = torch.tensor(np.concatenate([[0], np.cumsum(nf)[:-1]]), dtype=torch.long, device=dev)
        self._motion_ids = torch.arange(len(clips), dtype=torch.long, device=dev)
        frames = torch.tensor(np.concatenate([c["frames"] for c in clips], axis=0), dtype=torch.float32, device=dev)
        self._motion_frames = frames
        delta = np.stack([c["frames"][-1, 0:3] - c["frames"][0, 0:3] for c in clips]).astype(np.float32)
        delta[:, 2] = 0.0
        self._motion_root_pos_delta = torch.tensor(delta, dtype=torch.float32, device=dev)
        self._frames_root_pos = frames[:, 0:3].contiguous()
        self._frames_root_rot = torch_util.exp_map_to_quat(frames[:, 3:6])
        self._frames_joint_rot = km.dof_to_rot_torch(frames[:, 6:])
        B = km.get_num_joints()
        self._frames_contacts = torch.tensor(np.concatenate([c["contacts"] if c["contacts"] is not None else np.zeros((c["frames"].shape[0], B), np.float32)
                                                             for c in clips], axis=0), dtype=torch.float32, device=dev)

    _frame_root_pos = property(lambda self: self._frames_root_pos)
    _frame_root_rot = property(lambda self: self._frames_root_rot)
    _frame_joint_rot = property(lambda self: self._frames_joint_rot)
    _frame_contacts = property(lambda self: self._frames_contacts)

    def c_struct(self):
        raise RuntimeError("TorchMotionLib has no device tables: the HIP kernels need parc_amd.anim.motion_lib.MotionLib on a HIP device")

    def _calc_frame_blend(self, motion_ids, times):
        num_frames = self._motion_num_frames[motion_ids]
        phase = self.calc_motion_phase(motion_ids, times)
        frame_idx0 = (phase * (num_frames - 1)).long()
        frame_idx1 = torch.min(frame_idx0 + 1, num_frames - 1)
        blend = phase * (num_frames - 1) - frame_idx0
        start = self._motion_start_idx[motion_ids]
        return frame_idx0 + start, frame_idx1 + start, blend

    def calc_motion_frame(self, motion_ids, motion_times):
        i0, i1, blend = self._calc_frame_blend(motion_ids, motion_times)
        b = blend.unsqueeze(-1)
        root_pos = (1.0 - b) * self._frames_root_pos[i0] + b * self._frames_root_pos[i1]
        root_rot = torch_util.slerp(self._frames_root_rot[i0], self._frames_root_rot[i1], blend)
        joint_rot = torch_util.slerp(self._frames_joint_rot[i0], self._frames_joint_rot[i1], b)
        wrap = (self._motion_loop_modes[motion_ids] == LoopMode.WRAP.value).unsqueeze(-1)
        offset = torch.floor(motion_times / self._motion_lengths[motion_ids]).unsqueeze(-1) * self._motion_root_pos_delta[motion_ids]
        root_pos = root_pos + torch.where(wrap, offset, torch.zeros_like(offset))
        ret = [root_pos, root_rot, None, None, joint_rot, None]
        if self._contact_info:
            ret.append((1.0 - b) * self._frames_contacts[i0] + b * self._frames_contacts[i1])
        return tuple(ret)


def forward_kinematics_reference_order(km, root_pos, root_rot, joint_rot):
    """anim/kin_char_model.py:509-541 body by body with the reference's quat_mul: the CPU loop path's FK (on a HIP device the kernel is)"""
    B = km.get_num_joints()
    parents = km._parent_indices.cpu().tolist()
    body_pos, body_rot = [root_pos], [root_rot]
    for j in range(1, B):
        ppos, prot = body_pos[parents[j]], body_rot[parents[j]]
        lt = torch.broadcast_to(km._local_translation[j], ppos.shape)
        lr = torch.broadcast_to(km._local_rotation[j], prot.shape)
        body_pos.append(ppos + torch_util.quat_rotate(prot, lt))
        body_rot.append(torch_util.quat_mul(prot, torch_util.quat_mul(lr, joint_rot[..., j - 1, :])))
    return torch.stack(body_pos, dim=-2), torch.stack(body_rot, dim=-2)


class MotionSampler:
    def __init__(self, cfg):
        self._device = cfg['device']
        self._seq_len = None
        self._fps = None
        self._kin_char_model = kin_char_model.KinCharModel(self._device)
        self._kin_char_model.load_char_file(cfg['char_file'])
        self._motion_lib_file = cfg['motion_lib_file']
        if isinstance(self._motion_lib_file, str):
            cls = TorchMotionLib if torch.device(self._device).type == "cpu" else motion_lib.MotionLib
            self._mlib = cls(self._motion_lib_file, self._kin_char_model, self._device, contact_info=True)
        elif isinstance(self._motion_lib_file, motion_lib.MotionLib):
            self._mlib = self._motion_lib_file
        else:
            raise TypeError("cfg['motion_lib_file'] is a path or a MotionLib, not {}".format(type(self._motion_lib_file).__name__))
        print("num_motions =", self._mlib.num_motions())

    def check_init(self):
        assert self._seq_len is not None
        assert self._fps is not None

    def get_seq_len(self):
        return self._seq_len

    def _sample_motion_start_times(self, motion_ids, seq_duration):
        """reference :114-128: WRAP clips start anywhere, CLAMP clips leave seq_duration before their end; both draws are always made"""
        motion_full_lengths = self._mlib.get_motion_length(motion_ids)
        if self._random_start_times:
            loop = torch.rand_like(motion_full_lengths) * motion_full_lengths
            clamp = torch.rand_like(motion_full_lengths) * (motion_full_lengths - seq_duration)
            modes = self._mlib.get_motion_loop_mode(motion_ids)
            return torch.where(modes == LoopMode.WRAP.value, loop, clamp)
        return torch.zeros_like(motion_full_lengths)
