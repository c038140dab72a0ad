"""Stage 2's contact-aware motion optimiser on MI355X.

Mirror of the reference's ``tools/motion_opt/motion_optimization.py``: ``LossType``, ``BodyConstraint``,
``compute_approx_body_constraints`` (:34-181), ``motion_terrain_contact_loss`` (:183-395) and ``motion_contact_optimization``
(:404-500) with the same arguments, loss definitions and Adam descent, so ``parc_2_kin_gen.py:445`` / ``optimize_motions.py:157``
call it unchanged.  What differs is the mechanics:

* all 15 bodies' sample points go through the terrain query together: two launches of ``parc_points_hf_sdf`` per evaluation (inside /
  outside distance) over ``[frames x points]`` instead of 30 calls that each materialise ``[points, cells, 3]`` temporaries; the
  kernel reports the arg-min column, and autograd sees the distance to that one column only (terrain_util.points_hf_sdf);
* the pose chain (exponential maps -> quaternions -> forward kinematics) and its adjoint are one HIP launch each
  (KinCharModel.pose_chain: parc_pose_chain_forward / _backward) instead of ~190 autograd nodes per evaluation;
* nothing in an iteration reads the device back (the reference takes nine ``.item()`` per iteration for its loss dict); the terms
  are read at the logging stride only, so a whole iteration (forward, backward, Adam) is captured ONCE in a hipGraph and replayed.

``motion_contact_optimization_batch`` / ``compute_approx_body_constraints_batch`` do the same for M motions, each on its own terrain, in
one descent.  The single and the batch path share everything around the loss evaluation: the constraint row tables
(``pack_constraint_rows``, ``_ProblemTables``), the source poses (``_source_poses``), the contact runs (``_contact_runs``) and the descent
driver with its capture protocol and logs (``_descend``).  The two ``evaluate`` bodies are separate on purpose: their reductions differ.

Checked against fixture G20 (the reference's loss terms, gradient, body constraints and a 40-iteration descent).
"""
import enum
import sys
import time

import numpy as np
import torch

from ...util import geom_util, terrain_util, torch_util
from ...util import logger as logger_mod
from ...anim import kin_char_model


class LossType(enum.Enum):
    ROOT_POS_LOSS = 0
    ROOT_ROT_LOSS = 1
    JOINT_ROT_LOSS = 2
    SMOOTHNESS_LOSS = 3
    PENETRATION_LOSS = 4
    CONTACT_LOSS = 5
    SLIDING_LOSS = 6
    BODY_CONSTRAINT_LOSS = 7
    JERK_LOSS = 8
    LOOPING_LOSS = 9


# order of the stacked term tensor the loss evaluation returns (= the keys of the reference's loss dict, in its insertion order)
_TERM_ORDER = (LossType.ROOT_POS_LOSS, LossType.ROOT_ROT_LOSS, LossType.JOINT_ROT_LOSS, LossType.SMOOTHNESS_LOSS, LossType.PENETRATION_LOSS,
               LossType.CONTACT_LOSS, LossType.SLIDING_LOSS, LossType.JERK_LOSS, LossType.BODY_CONSTRAINT_LOSS)


class BodyConstraint:
    """A body (its sole / its sphere) should touch `constraint_point` over frames [start_frame_idx, end_frame_idx]."""
    start_frame_idx = 0
    end_frame_idx = 0
    constraint_point = None      # 3D torch vector


# motion files carry these objects under the key "opt:body_constraints" (optimize_motions.py:189-190); the reference's pickle.load
# resolves the class by this path
REFERENCE_MODULE = "tools.motion_opt.motion_optimization"
BodyConstraint.__module__ = REFERENCE_MODULE
terrain_util.register_reference_pickle_module(REFERENCE_MODULE, sys.modules[__name__])


def _f32(x, device):
    if torch.is_tensor(x):
        return x.detach().to(device=device, dtype=torch.float32)
    return torch.as_tensor(np.asarray(x), dtype=torch.float32).to(device)


# ---------------------------------------------------------------------------------------------------------------------
# approximate contact constraints from the contact labels (reference :34-181)
# ---------------------------------------------------------------------------------------------------------------------
def _consecutive_true_runs(flags):
    """index tensors of the maximal runs of True in a 1-D bool tensor (reference extract_consecutive_trues :43-73, including its
    rule that a trailing run of ONE frame after another run is dropped)"""
    idx = torch.nonzero(flags.flatten(), as_tuple=True)[0]
    if idx.numel() == 0:
        return []
    breaks = [0] + (torch.nonzero(idx[1:] - idx[:-1] > 1, as_tuple=True)[0] + 1).tolist()
    runs = [idx[breaks[i]:breaks[i + 1]].clone() for i in range(len(breaks) - 1)]
    if breaks[-1] < idx.shape[0] - 1:
        runs.append(idx[breaks[-1]:].clone())
    return runs


def _project_points_to_surface(points, terrain, num_iters=1000, lr=0.01):
    """Every point descends 0.5 * d(sd^2) for `num_iters` SGD steps, sd = distance to the terrain's column set (reference
    optimize_contact_points :93-115, one point at a time there; all points of a body advance together here - the objective is
    a sum of independent terms, so each point follows the same trajectory)."""
    if points.shape[0] == 0:
        return points
    base_z = terrain.hf.min().item() - 10.0
    hf, mp = terrain.hf.unsqueeze(0), terrain.min_point.unsqueeze(0)
    grid = terrain_util.HfGrid(hf, terrain.dxdy, points.device)
    p = points.clone().requires_grad_(True)
    for _ in range(num_iters):
        sd = terrain_util.points_hf_sdf(p.unsqueeze(0), hf, mp, terrain.dxdy, base_z=base_z, inverted=False, grid=grid)
        g, = torch.autograd.grad(torch.sum(torch.square(sd)), p)
        with torch.no_grad():
            p -= lr * g
    return p.detach()


def _contact_runs(root_pos, root_rot, joint_rot, contacts, char_model):
    """the (body, frame run, mean body position) triples compute_approx_body_constraints projects, for one motion"""
    body_pos, body_rot = char_model.forward_kinematics(root_pos, root_rot, joint_rot)
    ids = {n: char_model.get_body_id(n) for n in ("left_foot", "right_foot", "left_hand", "right_hand")}
    pos = {}
    for n, b in ids.items():
        pos[n] = body_pos[:, b]
        if n.endswith("foot"):       # the centre of the foot box, not the ankle (:136-142)
            off = _f32(char_model.get_geoms(b)[0]._offset, body_pos.device)
            pos[n] = pos[n] + torch_util.quat_rotate(body_rot[:, b], off.unsqueeze(0).expand(body_pos.shape[0], 3))
    return [(b, r, pos[n][r].mean(dim=0)) for n, b in ids.items() for r in _consecutive_true_runs(contacts[:, b] > 0.9)]


def _add_constraint(per_body, body, start, end, point):
    c = BodyConstraint()
    c.start_frame_idx, c.end_frame_idx, c.constraint_point = int(start), int(end), point
    per_body[body].append(c)


def compute_approx_body_constraints(root_pos, root_rot, joint_rot, contacts, char_model, terrain):
    """Per body a list of BodyConstraint: for feet and hands, every run of frames labelled "in contact" (> 0.9) becomes one
    constraint at the run's mean body position, projected onto the terrain surface."""
    out = [[] for _ in range(char_model.get_num_joints())]
    # every run of every body becomes one point; all of them descend together (independent terms of one objective)
    todo = _contact_runs(root_pos, root_rot, joint_rot, contacts, char_model)
    if todo:
        pts = _project_points_to_surface(torch.stack([p for _, _, p in todo]), terrain)
        for k, (b, r, _) in enumerate(todo):
            _add_constraint(out, b, r[0].item(), r[-1].item(), pts[k].clone())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the tables of a problem: motions packed along the frame axis (one motion is the case M = 1)
# ---------------------------------------------------------------------------------------------------------------------
def pack_segments(lengths):
    """-> (seg_start [M + 1], seg_of_frame [sum T]) as Python lists: motion m owns packed frames seg_start[m] .. seg_start[m + 1] - 1"""
    seg_start, seg_of_frame = [0], []
    for m, t in enumerate(lengths):
        t = int(t)
        assert t >= 0
        seg_start.append(seg_start[-1] + t)
        seg_of_frame += [m] * t
    return seg_start, seg_of_frame


def pack_constraint_rows(char_model, body_constraints, lengths, point_start, point_counts):
    """Body constraints of M motions as flat row tables, one row per (constraint, frame[, sole point]): frame index (offset by the motion's
    seg_start), body / point index, constraint point, radius[, geom offset].  Pure Python, no device: -> (sph, box, keep, sph_seg, box_seg).
    sph / box: dicts of lists (f, b | p, pt, r[, off]) in motion order, so that motion m owns rows sph_seg[m] .. sph_seg[m + 1] - 1
    (box_seg likewise); keep: [sum T][B] nested list, 0 where a constraint covers (frame, body) - those pairs are exempt from the sliding
    term (:328-333) - within the motion's own rows only."""
    B = char_model.get_num_joints()
    seg_start, _ = pack_segments(lengths)
    sph = {"f": [], "b": [], "pt": [], "r": [], "off": []}
    box = {"f": [], "p": [], "pt": [], "r": []}
    keep = [[1.0] * B for _ in range(seg_start[-1])]
    sph_seg, box_seg = [0], [0]
    for m, T in enumerate(lengths):
        T, o = int(T), seg_start[m]
        bc = body_constraints[m] if body_constraints is not None else None
        if bc is not None:
            for b in range(B):
                for c in bc[b]:
                    geom = char_model.get_geoms(b)[0]
                    s, e = int(c.start_frame_idx), int(c.end_frame_idx)
                    point = _f32(c.constraint_point, "cpu").reshape(3).tolist()
                    fr = [o + f for f in range(s, min(e, T - 1) + 1)]
                    if geom._shape_type == kin_char_model.GeomType.SPHERE:
                        radius = float(_f32(geom._dims, "cpu").reshape(-1)[0])
                        off = _f32(geom._offset, "cpu").reshape(3).tolist()
                        sph["f"] += fr
                        sph["b"] += [b] * len(fr)
                        sph["pt"] += [point] * len(fr)
                        sph["r"] += [radius] * len(fr)
                        sph["off"] += [off] * len(fr)
                    elif geom._shape_type == kin_char_model.GeomType.BOX:
                        radius = float(torch.linalg.vector_norm(_f32(geom._dims, "cpu"))) * 1.25
                        assert point_counts[b] >= 18, "the sole of a box body is its first 18 sample points"
                        for f in fr:
                            box["f"] += [f] * 18
                            box["p"] += list(range(point_start[b], point_start[b] + 18))
                        box["pt"] += [point] * (18 * len(fr))
                        box["r"] += [radius] * (18 * len(fr))
                    else:
                        continue
                    for f in range(max(s, 0), min(e + 1, T)):       # never beyond the motion's own rows
                        keep[o + f][b] = 0.0
        sph_seg.append(len(sph["f"]))
        box_seg.append(len(box["f"]))
    return sph, box, keep, sph_seg, box_seg


class _ProblemTables:
    """What an optimisation problem of one motion and one of M packed motions lay out alike, once, on the device: the sample points of all
    bodies as one [P, 3] table with their owner, each body's point range padded to one width, and the body constraints as row tables."""

    def _build_tables(self, char_model, body_points, body_constraints, lengths, dev):
        """body_constraints: per motion a constraint list or None -> (sph_seg, box_seg) of pack_constraint_rows"""
        B = char_model.get_num_joints()
        self.km = char_model
        self.points = terrain_util.BodyPoints(body_points, dev)
        counts, start = self.points.counts, self.points.start[:B]
        assert len(body_points) == B and min(counts) > 0, "every body needs at least one sample point"
        # per-body closest point: the bodies' point ranges padded to one width (a repeated point does not change a minimum)
        self.body_pts = torch.tensor([[start[b] + min(k, counts[b] - 1) for k in range(max(counts))] for b in range(B)], dtype=torch.int64, device=dev)
        sph, box, keep, sph_seg, box_seg = pack_constraint_rows(char_model, body_constraints, lengths, start, counts)
        i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        f32 = lambda v, w_: torch.tensor(v, dtype=torch.float32, device=dev).reshape(-1, w_) if w_ else torch.tensor(v, dtype=torch.float32, device=dev)
        self.sph = (i64(sph["f"]), i64(sph["b"]), f32(sph["pt"], 3), f32(sph["r"], 0), f32(sph["off"], 3)) if sph["f"] else None
        self.box = (i64(box["f"]), i64(box["p"]), f32(box["pt"], 3), f32(box["r"], 0)) if box["f"] else None
        self.pair_keep = torch.tensor(keep, dtype=torch.float32, device=dev).reshape(sum(lengths), B)
        return sph_seg, box_seg


# ---------------------------------------------------------------------------------------------------------------------
# the loss (reference :183-395)
# ---------------------------------------------------------------------------------------------------------------------
class _Problem(_ProblemTables):
    """Everything of one optimisation problem that does not change between evaluations, laid out once on the device: the tables of
    _ProblemTables, the heightfield grid and the contact weights.  evaluate() touches the device only through launches (capturable)."""

    def __init__(self, src_root_pos, src_root_rot_quat, src_joint_rot, src_body_vels, src_body_rot_vels, contacts, terrain, body_points,
                 char_model, body_constraints):
        dev = src_root_pos.device
        self.src = (src_root_pos, src_root_rot_quat, src_joint_rot, src_body_vels, src_body_rot_vels)
        self.contacts = contacts
        T = int(src_root_pos.shape[0])
        self._build_tables(char_model, body_points, [body_constraints], [T], dev)
        self.pair_keep = self.pair_keep[:T - 1]          # one row per frame pair
        self.local = self.points.local
        self.hf = terrain.hf.to(dev, torch.float32).unsqueeze(0)
        self.min_point = terrain.min_point.to(dev, torch.float32).unsqueeze(0)
        self.dxdy = terrain.dxdy
        self.grid = terrain_util.HfGrid(self.hf, terrain.dxdy, dev)
        # contact present in both frames of a pair, negative labels (generator artefacts) clipped (:232-234)
        self.pair_contact = torch.clamp(torch.minimum(contacts[1:], contacts[:-1]), min=0.0)

    def evaluate(self, tgt_root_pos, tgt_root_rot, tgt_joint_dof, w, max_jerk):
        """-> (weighted total, the nine terms stacked in _TERM_ORDER)"""
        km = self.km
        s_rp, s_rq, s_jr, s_bv, s_brv = self.src
        zero = tgt_root_pos.new_zeros(())
        root_pos_loss = torch.sum(torch.square(tgt_root_pos - s_rp))
        # root quaternion, joint rotations and every body's pose in one launch, with a one-launch adjoint (KinCharModel.pose_chain)
        tgt_rq, tgt_jr, body_pos, body_rot = km.pose_chain(tgt_root_pos, tgt_root_rot, tgt_joint_dof)
        root_rot_loss = torch.sum(torch.square(_diff_angle(tgt_rq, s_rq)))
        joint_rot_loss = torch.sum(torch.square(_diff_angle(tgt_jr, s_jr)))
        rot_vel_err_sq = torch.square(_diff_angle(body_rot[1:], body_rot[:-1]) - s_brv)
        dt = 1.0 / 30.0                 # the reference hard-codes the frame time (:360)
        fused_terms = body_pos.is_cuda and int(body_pos.shape[0]) >= 4
        if fused_terms:
            # smoothness, sliding and jerk sums of the frame-to-frame errors: one launch + one reduction (and one launch back)
            tt = _TemporalTerms.apply(body_pos, rot_vel_err_sq, s_bv.contiguous(), self.pair_keep, self.pair_contact, max_jerk * dt ** 3)
            smoothness_loss = tt[0]
        else:
            body_vels = body_pos[1:] - body_pos[:-1]
            vel_err_sq = torch.square(body_vels - s_bv)
            smoothness_loss = torch.sum(vel_err_sq) + torch.sum(rot_vel_err_sq)

        T, P = int(tgt_root_pos.shape[0]), int(self.local.shape[0])
        world = self.points.world(body_pos, body_rot)                      # [T, P, 3], one launch (and one for its adjoint)
        flat = world.reshape(1, T * P, 3)
        inside = terrain_util.points_hf_sdf(flat, self.hf, self.min_point, self.dxdy, base_z=-10.0, inverted=True, grid=self.grid)
        penetration_loss = torch.sum(-torch.clamp(inside, max=0.0))
        if w["w_contact"] != 0.0:
            outside = terrain_util.points_hf_sdf(flat, self.hf, self.min_point, self.dxdy, base_z=-10.0, inverted=False, grid=self.grid)
            outside = torch.clamp(outside, min=0.0).reshape(T, P)
            closest = outside[:, self.body_pts].min(dim=-1)[0]                     # [T, B]: per body its closest sample point
            contact_loss = torch.sum(closest * self.contacts)
        else:
            contact_loss = zero
        body_constraint_loss = zero
        if self.sph is not None:        # sphere bodies: |distance of the constraint point to the sphere| (:295-304)
            f, b, pt, r, off = self.sph
            centre = torch_util.quat_rotate(body_rot[f, b], off) + body_pos[f, b]
            body_constraint_loss = body_constraint_loss + torch.sum(torch.abs(geom_util.sdSphere(pt, centre, r)))
        if self.box is not None:        # box bodies (feet): every sole point within 1.25 box diagonals of the point (:306-322)
            f, p, pt, r = self.box
            body_constraint_loss = body_constraint_loss + torch.sum(torch.clamp(geom_util.sdSphere(pt, world[f, p], r), min=0.0))
        if fused_terms:
            sliding_loss = tt[1] if w["w_sliding"] != 0.0 else zero
            jerk_loss = tt[2]
        else:
            if w["w_sliding"] != 0.0:
                c, c2 = 0.03, 0.0009        # pseudo-Huber
                k = self.pair_keep
                sliding_loss = torch.sum((torch.sqrt(torch.sum(vel_err_sq * k.unsqueeze(-1), dim=-1) + c2) - c) * self.pair_contact) \
                    + torch.sum((torch.sqrt(rot_vel_err_sq * k + c2) - c) * self.pair_contact)
            else:
                sliding_loss = zero
            acc = body_vels[1:] - body_vels[:-1]
            jerk = torch.linalg.vector_norm(acc[1:] - acc[:-1], dim=-1)
            jerk_loss = torch.sum(torch.clamp(jerk - max_jerk * dt ** 3, min=0.0))

        terms = torch.stack([root_pos_loss, root_rot_loss, joint_rot_loss, smoothness_loss, penetration_loss, contact_loss, sliding_loss, jerk_loss,
                             body_constraint_loss])
        loss = w["w_root_pos"] * root_pos_loss + w["w_root_rot"] * root_rot_loss + w["w_joint_rot"] * joint_rot_loss \
            + w["w_smoothness"] * smoothness_loss + w["w_penetration"] * penetration_loss + w["w_contact"] * contact_loss \
            + w["w_sliding"] * sliding_loss + w["w_body_constraints"] * body_constraint_loss + w["w_jerk"] * jerk_loss
        return loss, terms


class _TemporalTerms(torch.autograd.Function):
    """(smoothness, sliding, jerk) sums of the frame-to-frame errors: per-(frame, body) partials in one launch + one reduction, the adjoint
    in one launch (parc_temporal_terms / _grad).  rot_err_sq carries its own gradient (it comes from the rotation-angle kernel)."""

    @staticmethod
    def forward(ctx, body_pos, rot_err_sq, src_vel, keep, pair_contact, jerk_limit):
        from ... import _hip
        T, B = int(body_pos.shape[0]), int(body_pos.shape[1])
        pos = body_pos.detach().to(torch.float32).contiguous()
        r = rot_err_sq.detach().to(torch.float32).contiguous()
        partial = torch.empty((3, T, B), dtype=torch.float32, device=pos.device)
        ctx.args = (T, B, 0.03, 0.0009, float(jerk_limit))          # pseudo-Huber constants of the reference (:349-350)
        _hip.check(_hip.lib().parc_temporal_terms(_hip.stream(), T, B, _hip.ptr(pos), _hip.ptr(r), _hip.ptr(src_vel), _hip.ptr(keep),
                                                  _hip.ptr(pair_contact), ctx.args[2], ctx.args[3], ctx.args[4], _hip.ptr(partial)), "parc_temporal_terms")
        ctx.save_for_backward(pos, r, src_vel, keep, pair_contact)
        return partial.sum(dim=(1, 2))

    @staticmethod
    def backward(ctx, g):
        from ... import _hip
        pos, r, src_vel, keep, pair_contact = ctx.saved_tensors
        T, B, c, c2, lim = ctx.args
        g_pos, g_r = torch.empty_like(pos), torch.empty_like(r)
        gg = g.to(torch.float32).contiguous()
        _hip.check(_hip.lib().parc_temporal_terms_grad(_hip.stream(), T, B, _hip.ptr(pos), _hip.ptr(r), _hip.ptr(src_vel), _hip.ptr(keep),
                                                       _hip.ptr(pair_contact), c, c2, lim, _hip.ptr(gg), _hip.ptr(g_pos), _hip.ptr(g_r)),
                   "parc_temporal_terms_grad")
        return g_pos, g_r, None, None, None, None


def _diff_angle(q0, q1):
    """torch_util.quat_diff_angle: one launch (and one for its adjoint) on the GPU, torch ops elsewhere"""
    if q0.is_cuda:
        return torch_util.quat_diff_angle_fused(q0, q1)
    return torch_util.quat_to_axis_angle(torch_util.quat_mul_compact(q1, torch_util.quat_conjugate(q0)))[1]


def _weights(**kw):
    names = ("w_root_pos", "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding", "w_body_constraints", "w_jerk")
    return {n: float(kw[n]) for n in names}


def motion_terrain_contact_loss(tgt_root_pos, tgt_root_rot, tgt_joint_dof, src_root_pos, src_root_rot_quat, src_joint_rot, src_body_vels,
                                src_body_rot_vels, contacts, terrain, body_points, char_model, w_root_pos, w_root_rot, w_joint_rot, w_smoothness,
                                w_penetration, w_contact, w_sliding, w_body_constraints, w_jerk, body_constraints, max_jerk):
    """-> (weighted loss tensor, {LossType: float}).  One read-back for the whole dict."""
    prob = _Problem(src_root_pos, src_root_rot_quat, src_joint_rot, src_body_vels, src_body_rot_vels, contacts, terrain, body_points, char_model,
                    body_constraints)
    w = _weights(w_root_pos=w_root_pos, w_root_rot=w_root_rot, w_joint_rot=w_joint_rot, w_smoothness=w_smoothness, w_penetration=w_penetration,
                 w_contact=w_contact, w_sliding=w_sliding, w_body_constraints=w_body_constraints, w_jerk=w_jerk)
    loss, terms = prob.evaluate(tgt_root_pos, tgt_root_rot, tgt_joint_dof, w, max_jerk)
    return loss, dict(zip(_TERM_ORDER, terms.detach().tolist()))


# ---------------------------------------------------------------------------------------------------------------------
# the descent (reference :404-500)
# ---------------------------------------------------------------------------------------------------------------------
def build_logger(log_file, exp_name=None, use_wandb=True):
    """Text logger with the reference's keys (its wandb upload has no counterpart: there is no network on the target)."""
    log = logger_mod.Logger()
    log.set_step_key("Iteration")
    if log_file is not None:
        log.configure_output_file(str(log_file))
    return log


def _source_poses(char_model, frames):
    """frames [n, 34] -> (root pos, root quat, joint rot, body pos, body rot) of the source frames"""
    root_pos = frames[:, 0:3].contiguous()
    root_quat = torch_util.exp_map_to_quat(frames[:, 3:6])
    joint_rot = char_model.dof_to_rot(frames[:, 6:34].contiguous())
    body_pos, body_rot = char_model.forward_kinematics(root_pos, root_quat, joint_rot)
    return root_pos, root_quat, joint_rot, body_pos, body_rot


def _descend(iteration, num_iters, use_graph, record, loggers, verbose, start_time, trace=None, loss_trace=None):
    """Run `iteration` num_iters times: eagerly, or (use_graph) three times on a side stream, then captured once in a hipGraph and
    replayed.  `iteration` leaves its results in the fixed buffer `record` [1 + nine terms, len(loggers)] (row 0 the total, then
    _TERM_ORDER; one column per logger); every 25 iterations the record is read back once and each column goes to its logger.  Closes
    the loggers' files and hands trace[:num_iters] to loss_trace.  Adds no launch, copy or synchronise to the iterations."""
    graph = None
    warm, log_iter_stride = 3, 25
    for it in range(num_iters):
        if use_graph and it == warm:
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                iteration()
            # capture records, it does not run: this iteration is the first replay below
        if graph is not None:
            graph.replay()
        elif use_graph:
            # warm-up iterations of the capture protocol run on a side stream (they are ordinary iterations of the descent)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                iteration()
            torch.cuda.current_stream().wait_stream(side)
        else:
            iteration()
        if it % log_iter_stride == 0:
            vals = record.t().tolist()          # the one read-back of the stride
            for logger, v in zip(loggers, vals):
                logger.log("Iteration", it)
                logger.log("Time (min)", (time.time() - start_time) / 60.0)
                logger.log("TOTAL WEIGHTED LOSS", v[0])
                for key, val in zip(_TERM_ORDER, v[1:]):
                    logger.log(key.name, val)
                if verbose:
                    logger.print_log()
                logger.write_log()
    for logger in loggers:
        if getattr(logger, "_file", None) is not None:
            logger._file.close()
            logger._file = None
    if loss_trace is not None:
        loss_trace.append(trace[:num_iters].clone())


def motion_contact_optimization(src_frames, contacts, body_points, terrain, char_model, num_iters, step_size, w_root_pos, w_root_rot, w_joint_rot,
                                w_smoothness, w_penetration, w_contact, w_sliding, w_body_constraints, w_jerk, body_constraints, max_jerk, exp_name,
                                use_wandb, log_file, use_graph=None, verbose=True, loss_trace=None):
    """Adam on (root position, root exponential map, joint dofs) of every frame; returns the optimised frames [T, 34].
    use_graph (default: on a GPU): capture one iteration in a hipGraph after three eager ones and replay it.
    loss_trace: optional list that receives the total loss of every iteration as ONE device tensor at the end (tests)."""
    start_time = time.time()
    dev = src_frames.device
    src_frames = src_frames.to(torch.float32)
    contacts = contacts.to(torch.float32)
    with torch.no_grad():
        src_root_pos, src_root_rot_quat, src_joint_rot, src_body_pos, src_body_rot = _source_poses(char_model, src_frames)
        src_body_vels = src_body_pos[1:] - src_body_pos[:-1]
        src_body_rot_vels = torch_util.quat_diff_angle(src_body_rot[1:], src_body_rot[:-1])
    prob = _Problem(src_root_pos, src_root_rot_quat, src_joint_rot, src_body_vels, src_body_rot_vels, contacts, terrain, body_points, char_model,
                    body_constraints)
    w = _weights(w_root_pos=w_root_pos, w_root_rot=w_root_rot, w_joint_rot=w_joint_rot, w_smoothness=w_smoothness, w_penetration=w_penetration,
                 w_contact=w_contact, w_sliding=w_sliding, w_body_constraints=w_body_constraints, w_jerk=w_jerk)
    params = [src_frames[:, 0:3].clone().requires_grad_(True), src_frames[:, 3:6].clone().requires_grad_(True),
              src_frames[:, 6:34].clone().requires_grad_(True)]
    on_gpu = src_frames.is_cuda
    use_graph = on_gpu if use_graph is None else use_graph
    # one multi-tensor launch per step on the GPU (same update rule)
    optimizer = torch.optim.Adam(params, lr=step_size, capturable=bool(use_graph), **({"fused": True} if on_gpu else {}))
    logger = build_logger(log_file=log_file, exp_name=exp_name, use_wandb=use_wandb)
    # the iteration's outputs live in fixed buffers: [total, nine terms]
    record = torch.zeros(1 + len(_TERM_ORDER), dtype=torch.float32, device=dev)
    trace = torch.zeros(max(num_iters, 1), dtype=torch.float32, device=dev) if loss_trace is not None else None
    it_idx = torch.zeros((), dtype=torch.int64, device=dev)

    def iteration():
        optimizer.zero_grad(set_to_none=True)
        loss, terms = prob.evaluate(params[0], params[1], params[2], w, max_jerk)
        loss.backward()
        optimizer.step()
        with torch.no_grad():
            record[0] = loss.detach()
            record[1:] = terms.detach()
            if trace is not None:
                trace.index_copy_(0, it_idx.reshape(1), loss.detach().reshape(1))
                it_idx.add_(1)

    _descend(iteration, num_iters, use_graph, record.unsqueeze(1), [logger], verbose, start_time, trace, loss_trace)
    return torch.cat([p.detach() for p in params], dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# M motions on their own terrains in one descent
#
# Every term of the loss is a sum over frames of expressions that touch one motion only, and Adam is element-wise: M motions packed
# along the frame axis follow the trajectories they follow alone, while every launch of an iteration does M times the work.  Two
# things need to know about the packing: the terrain query (a terrain per frame: terrain_util.points_hf_sdf_ragged) and the
# frame-to-frame terms (cut at the seams: parc_temporal_terms_seg).  Per-motion loss terms for the logs come from parc_segment_sums.
# ---------------------------------------------------------------------------------------------------------------------
def segment_sums(values, seg_start, num_segments, out=None):
    """values [n_planes, n_rows, width] -> [n_planes, num_segments]: sums over each segment's rows and all columns, in an order fixed by
    the segment's own layout (parc_segment_sums); seg_start: int32 device tensor [num_segments + 1]"""
    from ... import _hip
    assert values.dim() == 3 and values.dtype == torch.float32 and seg_start.dtype == torch.int32
    v = values.contiguous()
    P, R, W = (int(x) for x in v.shape)
    if out is None:
        out = torch.empty((P, num_segments), dtype=torch.float32, device=v.device)
    assert out.is_contiguous() and out.numel() == P * num_segments
    if W == 0 or R == 0:
        return out.zero_()
    _hip.check(_hip.lib().parc_segment_sums(_hip.stream(), P, R, W, int(num_segments), _hip.ptr(seg_start), _hip.ptr(v), _hip.ptr(out)), "parc_segment_sums")
    return out


class _TemporalTermsSeg(torch.autograd.Function):
    """_TemporalTerms for packed motions -> [3, M]: per-(frame, body) partials cut at the seams, one fold per motion, the adjoint in one
    launch (parc_temporal_terms_seg / parc_segment_sums / parc_temporal_terms_seg_grad).  rot_err_sq may lack the packed last row."""

    @staticmethod
    def forward(ctx, body_pos, rot_err_sq, src_vel, keep, pair_contact, jerk_limit, seg_start, seg_of_frame):
        from ... import _hip
        N, B, M = int(body_pos.shape[0]), int(body_pos.shape[1]), int(seg_start.shape[0]) - 1
        pos = body_pos.detach().to(torch.float32).contiguous()
        r = rot_err_sq.detach().to(torch.float32)
        ctx.r_rows = int(r.shape[0])
        if ctx.r_rows < N:
            r = torch.nn.functional.pad(r, (0, 0, 0, N - ctx.r_rows))
        r = r.contiguous()
        for x in (src_vel, keep, pair_contact):
            assert int(x.shape[0]) == N and int(x.shape[1]) == B
        partial = torch.empty((3, N, B), dtype=torch.float32, device=pos.device)
        ctx.args = (N, B, M, 0.03, 0.0009, float(jerk_limit))
        _hip.check(_hip.lib().parc_temporal_terms_seg(_hip.stream(), N, B, M, _hip.ptr(seg_start), _hip.ptr(seg_of_frame), _hip.ptr(pos), _hip.ptr(r),
                                                      _hip.ptr(src_vel), _hip.ptr(keep), _hip.ptr(pair_contact), 0.03, 0.0009, float(jerk_limit),
                                                      _hip.ptr(partial)), "parc_temporal_terms_seg")
        ctx.save_for_backward(pos, r, src_vel, keep, pair_contact, seg_start, seg_of_frame)
        return segment_sums(partial, seg_start, M)

    @staticmethod
    def backward(ctx, g):
        from ... import _hip
        pos, r, src_vel, keep, pair_contact, seg_start, seg_of_frame = ctx.saved_tensors
        N, B, M, c, c2, lim = ctx.args
        g_pos, g_r = torch.empty_like(pos), torch.empty_like(r)
        gg = g.to(torch.float32).contiguous()
        _hip.check(_hip.lib().parc_temporal_terms_seg_grad(_hip.stream(), N, B, M, _hip.ptr(seg_start), _hip.ptr(seg_of_frame), _hip.ptr(pos), _hip.ptr(r),
                                                           _hip.ptr(src_vel), _hip.ptr(keep), _hip.ptr(pair_contact), c, c2, lim, _hip.ptr(gg),
                                                           _hip.ptr(g_pos), _hip.ptr(g_r)), "parc_temporal_terms_seg_grad")
        return g_pos, g_r[:ctx.r_rows], None, None, None, None, None, None


class _BatchProblem(_ProblemTables):
    """_Problem for M motions packed along the frame axis: the same tables, with frame indices offset by seg_start, one terrain table
    for the ragged query and the segment tables the per-motion sums need.  evaluate() touches the device only through launches, and
    their number does not depend on M."""

    def __init__(self, src_frames, contacts, terrains, body_points, char_model, body_constraints):
        M = len(src_frames)
        assert M >= 1 and len(contacts) == M and len(terrains) == M
        dev = src_frames[0].device
        assert dev.type == "cuda", "the batched optimiser runs on the GPU (its kernels have no CPU fallback)"
        self.M = M
        self.lengths = [int(f.shape[0]) for f in src_frames]
        assert min(self.lengths) >= 1
        seg_start, seg_of_frame = pack_segments(self.lengths)
        N = seg_start[-1]
        self.N, self.seg_start_list = N, seg_start
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
        self.seg_start, self.seg_of_frame = i32(seg_start), i32(seg_of_frame)
        frames = torch.cat([f.to(torch.float32) for f in src_frames], dim=0)
        self.frames = frames
        self.contacts = torch.cat([c.to(torch.float32) for c in contacts], dim=0).contiguous()
        last = torch.zeros(N, dtype=torch.bool, device=dev)
        last[[s - 1 for s in seg_start[1:]]] = True
        with torch.no_grad():
            s_rp, s_rq, s_jr, bp, br = _source_poses(char_model, frames)
            # frame-to-frame sources, one row per packed frame; the last row of every motion is zero (and never read)
            nxt = torch.clamp(torch.arange(N, device=dev) + 1, max=N - 1)
            s_bv = torch.where(last[:, None, None], torch.zeros_like(bp), bp[nxt] - bp).contiguous()
            s_brv = torch.where(last[:, None], torch.zeros_like(br[..., 0]), torch_util.quat_diff_angle(br[nxt], br)).contiguous()
            pc = torch.clamp(torch.minimum(self.contacts[nxt], self.contacts), min=0.0)      # :232-234, per pair
            self.pair_contact = torch.where(last[:, None], torch.zeros_like(pc), pc).contiguous()
        self.src = (s_rp, s_rq, s_jr, s_bv, s_brv)
        # the descent's queries use the base_z of the single path (-10.0) for every terrain
        # (a prepared table - the dataset augmentation writes the heights into its pool on the device - is taken as it is)
        self.table = terrains if isinstance(terrains, terrain_util.HfTable) else terrain_util.HfTable(terrains, base_z=-10.0, device=dev)
        sph_seg, box_seg = self._build_tables(char_model, body_points, body_constraints, self.lengths, dev)
        self.sph_seg, self.box_seg = i32(sph_seg), i32(box_seg)
        self._cot = {}

    def _const(self, key, like, value):
        """a constant cotangent (weight) tensor, made once - before the capture - and reused by every iteration"""
        t = self._cot.get(key)
        if t is None or t.shape != like.shape:
            t = self._cot[key] = torch.full_like(like, float(value))
        return t

    def evaluate(self, tgt_root_pos, tgt_root_rot, tgt_joint_dof, w, max_jerk, terms_out, backward=True):
        """One evaluation of all M losses.  Writes the nine terms of every motion into terms_out [9, M] (_TERM_ORDER) and returns the
        weighted totals [M].  backward=True also accumulates d(sum of totals)/d(parameters) into the parameters' .grad: the weights are
        constants, so the per-element terms receive their weight as cotangent directly and the per-motion sums stay outside the graph."""
        km, M, N = self.km, self.M, self.N
        s_rp, s_rq, s_jr, s_bv, s_brv = self.src
        dt = 1.0 / 30.0
        d_rp = torch.square(tgt_root_pos - s_rp)                                                    # [N, 3]
        tgt_rq, tgt_jr, body_pos, body_rot = km.pose_chain(tgt_root_pos, tgt_root_rot, tgt_joint_dof)
        d_rr = torch.square(_diff_angle(tgt_rq, s_rq))                                              # [N]
        d_jr = torch.square(_diff_angle(tgt_jr, s_jr))                                              # [N, J]
        rot_vel_err_sq = torch.square(_diff_angle(body_rot[1:], body_rot[:-1]) - s_brv[:N - 1])     # [N - 1, B]; seam rows are never read
        tt = _TemporalTermsSeg.apply(body_pos, rot_vel_err_sq, s_bv, self.pair_keep, self.pair_contact, max_jerk * dt ** 3, self.seg_start,
                                     self.seg_of_frame)                                            # [3, M]
        world = self.points.world(body_pos, body_rot)                                               # [N, P, 3]
        inside = terrain_util.points_hf_sdf_ragged(world, self.seg_of_frame, self.table, inverted=True)
        pen = -torch.clamp(inside, max=0.0)                                                         # [N, P]
        heads = [(d_rp, w["w_root_pos"], 0), (d_rr, w["w_root_rot"], 1), (d_jr, w["w_joint_rot"], 2), (pen, w["w_penetration"], 4)]
        con = sph_v = box_v = None
        if w["w_contact"] != 0.0:
            outside = torch.clamp(terrain_util.points_hf_sdf_ragged(world, self.seg_of_frame, self.table, inverted=False), min=0.0)
            closest = outside[:, self.body_pts].min(dim=-1)[0]                                      # [N, B]
            con = closest * self.contacts
            heads.append((con, w["w_contact"], 5))
        if self.sph is not None:
            f, b, pt, r, off = self.sph
            centre = torch_util.quat_rotate(body_rot[f, b], off) + body_pos[f, b]
            sph_v = torch.abs(geom_util.sdSphere(pt, centre, r))
            heads.append((sph_v, w["w_body_constraints"], 8))
        if self.box is not None:
            f, p, pt, r = self.box
            box_v = torch.clamp(geom_util.sdSphere(pt, world[f, p], r), min=0.0)
            heads.append((box_v, w["w_body_constraints"], 8))
        if backward:
            w_tt = self._cot.get("tt")
            if w_tt is None:
                w_tt = self._cot["tt"] = torch.tensor([w["w_smoothness"], w["w_sliding"] if w["w_sliding"] != 0.0 else 0.0, w["w_jerk"]],
                                                      dtype=torch.float32, device=tt.device).reshape(3, 1).expand(3, M).contiguous()
            torch.autograd.backward([h[0] for h in heads] + [tt], [self._const(k, h[0], h[1]) for k, h in enumerate(heads)] + [w_tt])
        with torch.no_grad():
            ss = self.seg_start
            terms_out.zero_()
            segment_sums(d_rp.detach().reshape(1, N, 3), ss, M, out=terms_out[0:1])
            segment_sums(d_rr.detach().reshape(1, N, 1), ss, M, out=terms_out[1:2])
            segment_sums(d_jr.detach().reshape(1, N, -1), ss, M, out=terms_out[2:3])
            terms_out[3] = tt[0].detach()
            segment_sums(pen.detach().reshape(1, N, -1), ss, M, out=terms_out[4:5])
            if con is not None:
                segment_sums(con.detach().reshape(1, N, -1), ss, M, out=terms_out[5:6])
            if w["w_sliding"] != 0.0:
                terms_out[6] = tt[1].detach()
            terms_out[7] = tt[2].detach()
            if sph_v is not None:
                segment_sums(sph_v.detach().reshape(1, -1, 1), self.sph_seg, M, out=terms_out[8:9])
            if box_v is not None:
                bsum = segment_sums(box_v.detach().reshape(1, -1, 1), self.box_seg, M)
                terms_out[8] += bsum[0]
            wv = self._cot.get("wv")
            if wv is None:
                wv = self._cot["wv"] = torch.tensor([w["w_root_pos"], w["w_root_rot"], w["w_joint_rot"], w["w_smoothness"], w["w_penetration"],
                                                     w["w_contact"], w["w_sliding"], w["w_jerk"], w["w_body_constraints"]], dtype=torch.float32,
                                                    device=terms_out.device).reshape(9, 1)
            return (terms_out * wv).sum(dim=0)


def motion_terrain_contact_loss_batch(tgt_frames, src_frames, contacts, terrains, body_points, char_model, w_root_pos, w_root_rot, w_joint_rot,
                                      w_smoothness, w_penetration, w_contact, w_sliding, w_body_constraints, w_jerk, body_constraints, max_jerk):
    """The loss of M motions at tgt_frames (list of [T_m, 34]) -> (totals [M], terms [9, M] in _TERM_ORDER, list of gradients [T_m, 34]
    of each motion's total with respect to its frames).  One evaluation of the batched descent, for inspection and tests."""
    prob = _BatchProblem(src_frames, contacts, terrains, body_points, char_model, body_constraints)
    w = _weights(w_root_pos=w_root_pos, w_root_rot=w_root_rot, w_joint_rot=w_joint_rot, w_smoothness=w_smoothness, w_penetration=w_penetration,
                 w_contact=w_contact, w_sliding=w_sliding, w_body_constraints=w_body_constraints, w_jerk=w_jerk)
    tgt = torch.cat([f.to(torch.float32) for f in tgt_frames], dim=0)
    params = [tgt[:, 0:3].clone().requires_grad_(True), tgt[:, 3:6].clone().requires_grad_(True), tgt[:, 6:34].clone().requires_grad_(True)]
    terms = torch.zeros((len(_TERM_ORDER), prob.M), dtype=torch.float32, device=tgt.device)
    totals = prob.evaluate(params[0], params[1], params[2], w, max_jerk, terms)
    grad = torch.cat([p.grad for p in params], dim=-1)
    s = prob.seg_start_list
    return totals, terms, [grad[s[m]:s[m + 1]] for m in range(prob.M)]


def motion_contact_optimization_batch(src_frames, contacts, body_points, terrains, char_model, num_iters, step_size, w_root_pos, w_root_rot,
                                      w_joint_rot, w_smoothness, w_penetration, w_contact, w_sliding, w_body_constraints, w_jerk,
                                      body_constraints, max_jerk, exp_names, use_wandb, log_files, use_graph=None, verbose=True,
                                      loss_trace=None):
    """motion_contact_optimization for M motions, each on its own terrain, in ONE descent: src_frames, contacts, terrains,
    body_constraints (or None, or with None entries), exp_names and log_files are lists of length M; returns a list of [T_m, 34].
    terrains may also be a terrain_util.HfTable of M entries whose heights already lie on the device (the dataset augmentation).
    One Adam over the three packed parameter tensors; one iteration is captured and replayed as in the single path, and its number of
    launches does not depend on M.  Every 25 iterations each motion's total and nine terms go to that motion's own log.
    loss_trace: optional list that receives ONE [num_iters, M] device tensor of per-motion totals."""
    start_time = time.time()
    M = len(src_frames)
    if body_constraints is None:
        body_constraints = [None] * M
    exp_names = [None] * M if exp_names is None else exp_names
    log_files = [None] * M if log_files is None else log_files
    assert len(contacts) == M and len(terrains) == M and len(body_constraints) == M and len(exp_names) == M and len(log_files) == M
    dev = src_frames[0].device
    prob = _BatchProblem(src_frames, contacts, terrains, body_points, char_model, body_constraints)
    w = _weights(w_root_pos=w_root_pos, w_root_rot=w_root_rot, w_joint_rot=w_joint_rot, w_smoothness=w_smoothness, w_penetration=w_penetration,
                 w_contact=w_contact, w_sliding=w_sliding, w_body_constraints=w_body_constraints, w_jerk=w_jerk)
    frames = prob.frames
    params = [frames[:, 0:3].clone().requires_grad_(True), frames[:, 3:6].clone().requires_grad_(True), frames[:, 6:34].clone().requires_grad_(True)]
    use_graph = True if use_graph is None else use_graph
    optimizer = torch.optim.Adam(params, lr=step_size, capturable=bool(use_graph), fused=True)
    loggers = [build_logger(log_file=log_files[m], exp_name=exp_names[m], use_wandb=use_wandb) for m in range(M)]
    # the iteration's outputs live in fixed buffers: row 0 the totals, rows 1..9 the nine terms, one column per motion
    record = torch.zeros((1 + len(_TERM_ORDER), M), dtype=torch.float32, device=dev)
    trace = torch.zeros((max(num_iters, 1), M), dtype=torch.float32, device=dev) if loss_trace is not None else None
    it_idx = torch.zeros((), dtype=torch.int64, device=dev)

    def iteration():
        optimizer.zero_grad(set_to_none=True)
        totals = prob.evaluate(params[0], params[1], params[2], w, max_jerk, record[1:])
        optimizer.step()
        with torch.no_grad():
            record[0] = totals
            if trace is not None:
                trace.index_copy_(0, it_idx.reshape(1), totals.reshape(1, M))
                it_idx.add_(1)

    _descend(iteration, num_iters, use_graph, record, loggers, verbose, start_time, trace, loss_trace)
    out = torch.cat([p.detach() for p in params], dim=-1)
    s = prob.seg_start_list
    return [out[s[m]:s[m + 1]].clone() for m in range(M)]


def compute_approx_body_constraints_batch(root_pos, root_rot, joint_rot, contacts, char_model, terrains, num_iters=1000, lr=0.01):
    """compute_approx_body_constraints for M motions (lists of length M) -> list of per-motion constraint lists.  The contact runs are
    found per motion as in the single function; the points of ALL motions then descend together through the ragged terrain query,
    each on its own terrain with that terrain's min(hf) - 10 as base_z.  Every point follows the trajectory it follows alone: the
    objective is a sum of independent terms, and each step is the single path's arithmetic (g = 2 sd d(sd)/dp; p -= lr g)."""
    from ... import _hip
    M = len(root_pos)
    assert len(root_rot) == M and len(joint_rot) == M and len(contacts) == M and len(terrains) == M
    todo = [_contact_runs(root_pos[m], root_rot[m], joint_rot[m], contacts[m], char_model) for m in range(M)]
    out = [[[] for _ in range(char_model.get_num_joints())] for _ in range(M)]
    flat = [(m, b, r, p) for m in range(M) for (b, r, p) in todo[m]]
    if not flat:
        return out
    dev = flat[0][3].device
    table = terrain_util.HfTable(terrains, base_z=[t.hf.min().item() - 10.0 for t in terrains], device=dev)
    p = torch.stack([x[3] for x in flat]).to(torch.float32).reshape(-1, 1, 3).contiguous()
    rt = torch.tensor([x[0] for x in flat], dtype=torch.int32, device=dev)
    K = int(p.shape[0])
    sd = torch.empty((K, 1), dtype=torch.float32, device=dev)
    cell = torch.empty((K, 1), dtype=torch.int32, device=dev)
    g = torch.empty_like(p)
    L, st = _hip.lib(), _hip.stream()
    for _ in range(num_iters):
        _hip.check(L.parc_points_hf_sdf_ragged(st, K, 1, _hip.ptr(p), _hip.ptr(rt), M, _hip.ptr(table.table), _hip.ptr(table.pool), 0, 0.0, _hip.ptr(sd),
                                               _hip.ptr(cell)), "parc_points_hf_sdf_ragged")
        g_sd = sd * 2.0                                             # d(sum sd^2)/d(sd)
        _hip.check(L.parc_points_hf_sdf_ragged_grad(st, K, 1, _hip.ptr(p), _hip.ptr(rt), M, _hip.ptr(table.table), _hip.ptr(table.pool), 0, _hip.ptr(cell),
                                                    _hip.ptr(g_sd), _hip.ptr(g)), "parc_points_hf_sdf_ragged_grad")
        p -= lr * g
    pts = p.reshape(-1, 3).cpu()
    ends = [(int(r[0]), int(r[-1])) for r in torch.stack([torch.stack([x[2][0], x[2][-1]]) for x in flat]).cpu().tolist()]
    for k, (m, b, _, _) in enumerate(flat):
        _add_constraint(out[m], b, ends[k][0], ends[k][1], pts[k].clone().to(dev))
    return out
