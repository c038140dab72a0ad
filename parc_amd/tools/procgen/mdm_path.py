"""Ranking of generated motions against the terrain.

Mirror of the scoring half of the reference's ``tools/procgen/mdm_path.py``: ``MDMPathSettings`` (:19-29), ``compute_motion_loss``
(:31-127) and the tail of ``generate_frames_until_end_of_path`` (:324-376) as ``rank_motions`` for frames that already exist.  The
functions that drive the motion generator itself are not part of this package: they raise and name the planner callable of the
``mgdm`` sub-env instead.

Mechanics: the reference loops over the candidates in Python, and per candidate over the 15 bodies with two ``points_hf_sdf`` calls
each.  Here all candidates go through ``parc_motion_score`` (include/parc_score.h): forward kinematics, sample points, both signed
distances and every reduction in two launches, with no host read - the call can sit in a captured step.  Checked against fixture G28.
"""
import weakref

import torch

from ... import _hip
from ...util import terrain_util
from ...util.motion_util import MotionFrames      # noqa: F401  (the reference's module exports it too)


class MDMPathSettings:
    next_node_lookahead = 7
    rewind_num_frames = 5
    end_of_path_buffer = 2
    max_motion_length = 10.0
    path_batch_size = 16
    mdm_batch_size = 32
    top_k = 4
    w_target = 2.0
    w_contact = 0.1
    w_pen = 0.1


class MotionScore:
    """What one scoring call returns: total / contact / pen [B], the per-frame terms [B, F, 2] = (pen_f, contact_f) and, when the
    jerk figures were asked for, mean_jerk / frac_over [B] (NaN for candidates with fewer than 4 counted frames)."""

    def __init__(self, losses, frame_terms, jerk):
        self.total_loss, self.contact_loss, self.pen_loss = losses[:, 0], losses[:, 1], losses[:, 2]
        self.frame_terms = frame_terms
        self.mean_jerk = None if jerk is None else jerk[:, 0]
        self.frac_over = None if jerk is None else jerk[:, 1]

    def losses(self):
        return {"total_loss": self.total_loss, "contact_loss": self.contact_loss, "pen_loss": self.pen_loss}


class MotionScorer:
    """Scores candidate motions of one character on one terrain.  Construction flattens the per-body point lists, and computes
    min(hf) - 10 (the floor of the columns, mdm_path.py:77) and the column grid once; ``score`` reads nothing back from the device."""

    def __init__(self, char_model, body_points, terrain):
        from ... import _hip_score
        dev = terrain.hf.device
        assert dev.type == "cuda", "the motion scorer runs on the device (no CPU fallback)"
        assert len(body_points) == char_model.get_num_joints()
        self._model = char_model
        self._num_bodies = char_model.get_num_joints()
        self._points = terrain_util.BodyPoints(body_points, dev)
        assert self._points.num_points > 0
        self._hf = terrain.hf.detach().to(torch.float32).contiguous()
        self._grid = terrain_util.HfGrid(self._hf, terrain.dxdy, dev)
        mp, dxdy = terrain.min_point.detach().to(torch.float32).cpu(), terrain.dxdy.detach().to(torch.float32).cpu()
        self.base_z = float(self._hf.min().item()) - 10.0
        self._terrain = _hip_score.ScoreTerrainS(_hip.ptr(self._hf), int(self._hf.shape[0]), int(self._hf.shape[1]), float(mp[0]), float(mp[1]),
                                                 float(dxdy[0]), float(dxdy[1]), _hip.ptr(self._grid.xs), _hip.ptr(self._grid.ys))
        self._key = (terrain.hf.data_ptr(), tuple(terrain.hf.shape), int(terrain.hf._version), id(char_model), id(body_points))

    def matches(self, char_model, body_points, terrain):
        return self._key == (terrain.hf.data_ptr(), tuple(terrain.hf.shape), int(terrain.hf._version), id(char_model), id(body_points))

    def score(self, motion_frames, w_contact, w_pen, num_frames=None, dt=1.0 / 30.0, max_jerk=None, jerk=False):
        """motion_frames: MotionFrames with root_pos [B,F,3], root_rot [B,F,4], joint_rot [B,F,J,4], contacts [B,F,Bd].  num_frames: int32
        tensor [B] of counted frames per candidate (None = all F).  jerk=True (or a max_jerk) also returns the jerk figures."""
        dev = self._hf.device

        def prep(x):
            return x.detach().to(device=dev, dtype=torch.float32).contiguous()
        root_pos, root_rot, joint_rot, contacts = prep(motion_frames.root_pos), prep(motion_frames.root_rot), prep(motion_frames.joint_rot), \
            prep(motion_frames.contacts)
        assert root_pos.dim() == 3
        B, F, Bd = int(root_pos.shape[0]), int(root_pos.shape[1]), self._num_bodies
        assert root_rot.shape == (B, F, 4) and joint_rot.shape == (B, F, Bd - 1, 4) and contacts.shape == (B, F, Bd)
        nf = None
        if num_frames is not None:
            nf = num_frames.detach().to(device=dev, dtype=torch.int32).contiguous()
            assert nf.shape == (B,)
        want_jerk = jerk or max_jerk is not None
        frame_terms = torch.zeros((B, F, 2), dtype=torch.float32, device=dev)
        losses = torch.empty((B, 3), dtype=torch.float32, device=dev)
        jerk_out = torch.empty((B, 2), dtype=torch.float32, device=dev) if want_jerk else None
        ws = torch.empty((B, F, Bd, 3), dtype=torch.float32, device=dev) if want_jerk else None
        bp = self._points
        _hip.check(_hip.lib().parc_motion_score(_hip.stream(), self._model.c_struct(), B, F, _hip.ptr(nf), _hip.ptr(root_pos), _hip.ptr(root_rot),
                                                _hip.ptr(joint_rot), _hip.ptr(contacts), bp.num_points, _hip.ptr(bp.local), _hip.ptr(bp.start32),
                                                self._terrain, self.base_z, float(w_contact), float(w_pen), float(dt),
                                                float("inf") if max_jerk is None else float(max_jerk), _hip.ptr(ws), _hip.ptr(frame_terms),
                                                _hip.ptr(losses), _hip.ptr(jerk_out)), "parc_motion_score")
        return MotionScore(losses, frame_terms, jerk_out)


# one scorer per terrain object, kept beside it and not in it: copies and pickles of a terrain (motion files) stay what they were
_scorers = weakref.WeakKeyDictionary()


def _scorer_for(terrain, char_model, body_points):
    """the scorer cached for the terrain object (rebuilt when the heightfield was written to, or for another character / point set)"""
    s = _scorers.get(terrain)
    if s is None or not s.matches(char_model, body_points, terrain):
        s = MotionScorer(char_model, body_points, terrain)
        _scorers[terrain] = s
    return s


def compute_motion_loss(motion_frames, path_nodes, terrain, char_model, body_points, w_contact, w_pen, w_path, verbose=True):
    """mdm_path.py:31-127: {"total_loss", "contact_loss", "pen_loss"}, each [B] (path_nodes and w_path are unused there too)."""
    return _scorer_for(terrain, char_model, body_points).score(motion_frames, w_contact, w_pen).losses()


def rank_motions(full_motion_frames, final_frame, final_frame_found, terrain, char_model, body_points, w_contact, w_pen,
                 not_finished_penalty=100.0, add_noise_to_loss=False):
    """mdm_path.py:324-376 for frames that already exist: every candidate b is scored over its first final_frame[b] frames in one
    call, the unfinished ones (final_frame_found[b] false) get the penalty, and the candidates are sorted by loss.  Returns the sliced
    MotionFrames [1, final_frame[b], ...] in sorted order, one terrain copy per candidate, and info with "losses", "contact_losses",
    "pen_losses" in that order."""
    dev = terrain.hf.device
    final_frame = torch.as_tensor(final_frame).to(device=dev)
    found = torch.as_tensor(final_frame_found).to(device=dev, dtype=torch.bool)
    sc = _scorer_for(terrain, char_model, body_points).score(full_motion_frames, w_contact, w_pen, num_frames=final_frame.to(torch.int32))
    all_losses = sc.total_loss + (~found).to(torch.float32) * float(not_finished_penalty)
    if add_noise_to_loss:
        all_losses = all_losses + torch.randn_like(all_losses)
    sorted_losses, sorted_ids = torch.sort(all_losses)
    ids, lens = sorted_ids.tolist(), final_frame.tolist()
    frames = [full_motion_frames.get_idx(i).unsqueeze(0).get_slice(slice(0, int(lens[i]))) for i in ids]
    terrains = [terrain.torch_copy() for _ in ids]
    info = {"losses": sorted_losses.squeeze(), "contact_losses": sc.contact_loss[sorted_ids.squeeze()], "pen_losses": sc.pen_loss[sorted_ids.squeeze()]}
    return frames, terrains, info


_NEEDS_GENERATOR = ("{} drives the motion generator (the reference's MDM), which this package does not contain: hand the `mgdm` sub-env a "
                    "planner callable (envs/ig_parkour/mgdm_env.py, `mgdm.generator`) and rank what it produces with rank_motions()")


def gen_mdm_motion_at_path_start(*args, **kwargs):
    raise NotImplementedError(_NEEDS_GENERATOR.format("gen_mdm_motion_at_path_start"))


def generate_frames_until_end_of_path(*args, **kwargs):
    raise NotImplementedError(_NEEDS_GENERATOR.format("generate_frames_until_end_of_path"))


def generate_frames_along_path(*args, **kwargs):
    raise NotImplementedError(_NEEDS_GENERATOR.format("generate_frames_along_path"))
