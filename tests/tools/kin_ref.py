"""Float64 evaluation of what the tracker's kinematics kernels compute through the FAST layer of parc_amd/csrc/parc_math.h (fsincos,
fatan2_q1, facos01, the FMA-grouped quat_mul, exp_map_to_quat, quat_to_axis_angle, slerp, calc_heading_quat_inv_alg and their
two-poses-per-lane copies in parc_math_pk.h) -- TEST INFRASTRUCTURE, touches no GPU.

The yardstick of tests/test_kin_branch_gpu.py: the project's torch ports (util/torch_util.py, KinCharModel.dof_to_rot_torch /
forward_kinematics_torch) and restatements of the reference's Joint.rot_to_dof (anim/kin_char_model.py:79-100), of its clip build
(anim/motion_lib.py:264-290,405-423, kin_char_model.py:543-581), of its frame blend (motion_lib.py:80-112,443-475) and of the root
block of compute_char_obs (envs/ig_char_env.py:582-626).  Every function takes `dtype`: float64 is the yardstick, float32 the figure
e-bar is measured with.  tests/test_kin_ref_cpu.py pins the module against fixture G37 (tests/golden/gen_kin_branch.py: the reference's
own classes on the same inputs) and the C oracle against the module.

Also here: the designed inputs.  Every branch point of the fast layer is visited on both sides, and a float64 guard is asserted on
every input: GUARD around each 1e-5 threshold, FAR_PI around the wrap at pi (the sign rule), SLERP_GUARD around slerp's sin < 1e-3,
MIN_HORIZONTAL for the heading.  A guard that fails raises; no test drops an input.  Random filler is drawn from a recorded seed and
redrawn until it passes the same guards.

Run as a script it prints e-bar, the largest |reference fp32 - reference float64| over G37 per output or bucket; the MEASURED_*
constants are those figures rounded up to 3 digits.  They come from torch code on the CPU, never from the kernels.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import pose_opt_ref as por  # noqa: E402
from pose_opt_ref import CHARS, DEVICE_FACTOR, GUARD, THRESHOLD, f64_model, value_error  # noqa: E402,F401
from parc_amd.anim import kin_char_model  # noqa: E402
from parc_amd.util import torch_util  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "g37_kin_branch.npz")
PI = math.pi
SEEDS = {"hum": 3710, "syn": 3720}
N_POSES = 64
FAR_PI = 1e-3                       # of a spherical map's wrapped angle from the wrap at pi: inside, the two precisions may return q and -q
# pose_opt_ref's angle list, with its two maps next to pi moved from pi -+ 1e-3 to pi -+ 1.01e-3: after the fp32 rounding they are still
# outside FAR_PI, so the sign rule is asserted on them like on every other row
ANGLES = tuple(math.pi - 1.01e-3 if a == por.PI - 1e-3 else math.pi + 1.01e-3 if a == por.PI + 1e-3 else a for a in por.ANGLES)
assert len(ANGLES) == len(por.ANGLES) and sum(a != b for a, b in zip(ANGLES, por.ANGLES)) == 2
SLERP_GUARD = (0.8e-3, 1.25e-3)     # of float64 sin(half angle) between two frames: slerp's "sin < 1e-3 -> average"
MIN_HORIZONTAL = 1e-3               # of the rotated x axis: below it the heading is ill-posed in both precisions (left out by design)
MIN_AXIS_DOT = 1e-3                 # |rotation axis . hinge axis| of a designed hinge quaternion: the sign rule of rot_to_dof
FAR_ANGLE = 16.0                    # raw angles beyond it (50, 100, 300, 600) are held to an e-bar of their own: one ulp of the fp32 angle is >= 1.9e-6 there
ROOT_FAR = np.array([1e3, -1e3, 50.0])
SLERP_DECADES = ((0.0, 1e-3), (1e-3, 5e-3), (5e-3, 5e-2), (5e-2, math.inf))     # of float64 sin(half angle), one decade each, cut between the designed
# half angles (2e-3 | 1e-2 | 0.3 and up) so that one ulp of a stored row cannot move a designed pair into the next bucket; [0, 1e-3) is the average
FPS = (30.0, 120.0)

# e-bar: max |reference fp32 - reference float64| over G37 (python tests/tools/kin_ref.py prints them), rounded up to 3 digits; absolute.
MEASURED_DOF_TO_ROT = {"near": 2.26e-07, "far": 6.57e-06}                 # by raw angle of the joint: <= FAR_ANGLE, beyond
MEASURED_ROT_TO_DOF = 3.01e-07
MEASURED_FK = {"origin": {"body_pos": 5.44e-07, "body_rot": 5.12e-07}, "far": {"body_pos": 9.91e-05, "body_rot": 5.12e-07}}     # root at the origin, at ROOT_FAR
MEASURED_BUILD_ROWS = {"root_rot": 1.01e-07, "joint_rot": 8.95e-08}
MEASURED_BUILD_VEL = {30: {"root_vel": 6.03e-06, "root_ang_vel": 1.27e-05, "dof_vel": 1.7e-05}, 120: {"root_vel": 1.67e-05, "root_ang_vel": 3.93e-05, "dof_vel": 5.47e-05}}
MEASURED_SLERP_DECADE = (2.99e-08, 2.66e-06, 3.91e-05, 4.18e-06)     # pairs whose fp32 cosine is < 1; [0, 1e-3) is the plain average: one rounding
MEASURED_ROOT_POS = 2.34e-06           # the fp32 blend weight is up to half an ulp of the frame number off: 4.8e-7 of a frame step of up to 4
MEASURED_ROOT_BLOCK = 1.27e-06
MEASURED_HEADING_QUAT = 7.54e-08          # calc_heading_quat_inv itself, up to the sign of the quaternion


def load_char(name, device="cpu"):
    """pose_opt_ref.load_char; the model remembers which of CHARS it is (the seeds of the designed inputs are per character)"""
    km = por.load_char(name, device)
    km.kin_ref_name = name
    return km


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def _np(x):
    return x.detach().cpu().numpy()


def model(km, dtype):
    """the CPU model holding tensors of `dtype`: km itself (fp32) or its float64 copy"""
    return km if dtype == torch.float32 else f64_model(km)


# ------------------------------------------------------------------------------------------------------------------ evaluation
def dof_to_rot(km, dof, dtype=torch.float64):
    with torch.no_grad():
        return _np(model(km, dtype).dof_to_rot_torch(_t(dof, dtype)))


def forward_kinematics(km, root_pos, root_rot, joint_rot, dtype=torch.float64):
    with torch.no_grad():
        bp, br = model(km, dtype).forward_kinematics_torch(_t(root_pos, dtype), _t(root_rot, dtype), _t(joint_rot, dtype))
    return _np(bp), _np(br)


def _hinge_axis(km, j, dtype):
    ax = km.get_joint(j).axis
    return torch.as_tensor(np.asarray(ax.detach().cpu().numpy() if torch.is_tensor(ax) else ax, np.float32)).to(dtype)


def _rot_to_dof_t(km, rot):
    """anim/kin_char_model.py:79-100, 493-507 on a tensor [..., J, 4]: hinge = the angle, negated where the rotation axis points against
    the joint axis; spherical = the exponential map; nothing is normalised"""
    dof = torch.zeros(rot.shape[:-2] + (km.get_dof_size(),), dtype=rot.dtype)
    for j in range(1, km.get_num_joints()):
        jt, d = km.get_joint(j), km.get_joint(j).dof_idx
        if jt.get_dof_dim() == 1:
            axis, angle = torch_util.quat_to_axis_angle(rot[..., j - 1, :])
            dot = torch.sum(_hinge_axis(km, j, rot.dtype) * axis, dim=-1)
            dof[..., d] = torch.where(dot < 0, -angle, angle)
        elif jt.get_dof_dim() == 3:
            dof[..., d:d + 3] = torch_util.quat_to_exp_map(rot[..., j - 1, :])
    return dof


def rot_to_dof(km, joint_rot, dtype=torch.float64):
    with torch.no_grad():
        return _np(_rot_to_dof_t(km, _t(joint_rot, dtype)))


def _dof_vel_t(km, jr0, jr1, dt):
    """kin_char_model.py:552-581"""
    drot = torch_util.quat_normalize(torch_util.quat_mul(torch_util.quat_conjugate(jr0), jr1))
    out = torch.zeros(jr0.shape[:-2] + (km.get_dof_size(),), dtype=jr0.dtype)
    for j in range(1, km.get_num_joints()):
        jt, d = km.get_joint(j), km.get_joint(j).dof_idx
        if jt.get_dof_dim() == 1:
            out[..., d] = torch.sum(_hinge_axis(km, j, jr0.dtype) * (torch_util.quat_to_exp_map(drot[..., j - 1, :]) / dt), dim=-1)
        elif jt.get_dof_dim() == 3:
            out[..., d:d + 3] = torch_util.quat_to_exp_map(drot[..., j - 1, :]) / dt
    return out


def clip_build(km, frames, fps, dtype=torch.float64):
    """one clip's rows from its fp32 frames [F, 6 + D] -> dict(root_pos, root_rot, joint_rot, root_vel, root_ang_vel, dof_vel):
    motion_lib.py:405-423 (rows; joint quaternions with w >= 0), :275-290 (finite differences, the last frame repeating the previous
    one's).  A single-frame clip has no difference to repeat (the reference's loader indexes frame -2 and stops): its velocities are
    zero, which is what the device build writes."""
    m = model(km, dtype)
    with torch.no_grad():
        fr = _t(frames, dtype)
        rp = fr[:, 0:3].clone()
        rr = torch_util.exp_map_to_quat(fr[:, 3:6])
        jr = torch_util.quat_pos(m.dof_to_rot_torch(fr[:, 6:]))
        F = fr.shape[0]
        rv, rav = torch.zeros_like(rp), torch.zeros_like(rp)
        dv = torch.zeros((F, km.get_dof_size()), dtype=dtype)
        if F >= 2:
            rv[:-1] = fps * (rp[1:] - rp[:-1])
            rv[-1] = rv[-2]
            rav[:-1] = fps * torch_util.quat_to_exp_map(torch_util.quat_diff(rr[:-1], rr[1:]))
            rav[-1] = rav[-2]
            dv[:-1] = _dof_vel_t(km, jr[:-1], jr[1:], 1.0 / fps)
            dv[-1] = dv[-2]
    return dict(root_pos=_np(rp), root_rot=_np(rr), joint_rot=_np(jr), root_vel=_np(rv), root_ang_vel=_np(rav), dof_vel=_np(dv))


BUILD_KEYS = ("root_pos", "root_rot", "joint_rot", "root_vel", "root_ang_vel", "dof_vel")


def frame_blend(rot0, rot1, pos0, pos1, blend, loop_phase, pos_delta, dtype=torch.float64):
    """motion_lib.py:94-112,458-475 for given frame pairs: rot [Q, 1 + J, 4] (root first) slerped, pos [Q, 3] lerped plus
    loop_phase * pos_delta (zero rows for CLAMP clips) -> (rot [Q, 1 + J, 4], root_pos [Q, 3])"""
    with torch.no_grad():
        t = _t(blend, dtype)
        q = torch_util.slerp(_t(rot0, dtype), _t(rot1, dtype), t.reshape(-1, 1, 1).expand(-1, np.shape(rot0)[1], 1))
        t1 = t.unsqueeze(-1)
        p = (1.0 - t1) * _t(pos0, dtype) + t1 * _t(pos1, dtype) + _t(loop_phase, dtype).unsqueeze(-1) * _t(pos_delta, dtype)
    return _np(q), _np(p)


def root_block(root_rot, root_vel, root_ang_vel, dtype=torch.float64, global_obs=False):
    """columns 0..11 of compute_char_obs: tan_norm(heading_inv(q) (x) q), heading_inv(q) applied to both root velocities; global_obs
    leaves the row in world axes (the heading is the identity)"""
    with torch.no_grad():
        q, v, w = _t(root_rot, dtype), _t(root_vel, dtype), _t(root_ang_vel, dtype)
        if global_obs:
            h = torch.zeros_like(q)
            h[..., 3] = 1.0
        else:
            h = torch_util.calc_heading_quat_inv(q)
        out = torch.cat([torch_util.quat_to_tan_norm(torch_util.quat_mul(h, q)), torch_util.quat_rotate(h, v), torch_util.quat_rotate(h, w)], dim=-1)
    return _np(out)


def heading_quat_inv(root_rot, dtype=torch.float64):
    with torch.no_grad():
        return _np(torch_util.calc_heading_quat_inv(_t(root_rot, dtype)))


# ------------------------------------------------------------------------------------------------------------------ float64 helpers
_unit, _qmul64, _exp64 = por._unit, por._qmul64, por._exp64
_CONJ = np.array([-1.0, -1.0, -1.0, 1.0])


def _log64(q):
    """exponential map of the w >= 0 representative, angle in [0, pi]"""
    q = np.where(q[..., 3:] < 0, -q, q)
    s = np.linalg.norm(q[..., :3], axis=-1, keepdims=True)
    return np.where(s > 0, q[..., :3] / np.maximum(s, 1e-300), 0.0) * 2.0 * np.arctan2(s, q[..., 3:])


def _raw_angles(km, dof):
    """[n, J] float64: every joint's raw angle (|e| of a spherical joint, |theta| of a hinge, 0 of a fixed one)"""
    dof = np.asarray(dof, np.float64)
    out = np.zeros((dof.shape[0], km.get_num_joints() - 1))
    for j in range(1, km.get_num_joints()):
        d, k = km.get_joint_dof_idx(j), km.get_joint_dof_dim(j)
        if k:
            out[:, j - 1] = np.linalg.norm(dof[:, d:d + k], axis=1)
    return out


def sph_conditions(maps):
    """guards of exponential maps [..., 3] (fp32 numbers, judged in float64) -> violations: wrapped angle outside GUARD (an exactly zero
    map excepted) and at least FAR_PI from the wrap at pi"""
    raw = np.linalg.norm(np.asarray(maps, np.float64), axis=-1)
    w = por.wrapped(raw)
    bad = ["map {}: wrapped angle {:.3e} inside the guard band".format(i, w[i]) for i in zip(*np.nonzero((w >= GUARD[0]) & (w <= GUARD[1]) & (raw != 0.0)))]
    bad += ["map {}: raw angle {:.9f} within 1e-3 of the wrap at pi".format(i, raw[i]) for i in zip(*np.nonzero(np.abs(w - PI) < FAR_PI))]
    return bad


def sph_maps(km, dof):
    dof = np.asarray(dof, np.float64)
    return np.stack([dof[:, km.get_joint_dof_idx(j):km.get_joint_dof_idx(j) + 3] for j in por.spherical_joints(km)], axis=1)


# ------------------------------------------------------------------------------------------------------------------ designed dofs
HINGE_EXTRA = (2 * PI - 1e-3, 2 * PI + 1e-3, 4 * PI - 1e-3, 4 * PI + 1e-3, 100.0, 600.0)
SPH_EXTRA = (50.0, 300.0)
N_DOF_DESIGNED = 2 * len(ANGLES) + 1 + 2 * len(HINGE_EXTRA)
DOF_ZERO_ROW = 2 * len(ANGLES)


def designed_dofs(km, n=N_POSES, seed=None):
    """fp32 [n, D].  Rows 0..13: ANGLES[k] on a random axis on every spherical joint, +-ANGLES[k] on the hinges (sign alternating from
    hinge to hinge); rows 14..27: the same angles on other axes with the hinge signs swapped; row 28: all zeros; rows 29..40:
    +-HINGE_EXTRA on the hinges (both sign patterns) with |e| = 50 then 300 on the spherical joints; the rest random filler
    (0.8 N(0, 1)), redrawn row by row until it passes the guards.  n < 41 cuts the list short."""
    rng = np.random.default_rng(SEEDS[_char_name(km)] if seed is None else seed)
    D = km.get_dof_size()
    sph, hin = por.spherical_joints(km), por.hinge_joints(km)
    rows = []

    def row(sph_angle, hinge_angle, flip):
        d = np.zeros(D)
        for j in sph:
            d0 = km.get_joint_dof_idx(j)
            d[d0:d0 + 3] = sph_angle * _unit(rng.standard_normal(3))
        for i, j in enumerate(hin):
            d[km.get_joint_dof_idx(j)] = hinge_angle * (1.0 if (i + flip) % 2 == 0 else -1.0)
        return d

    for flip in (0, 1):
        rows += [row(a, a, flip) for a in ANGLES]
    rows.append(np.zeros(D))
    for k, a in enumerate(HINGE_EXTRA):
        for flip in (0, 1):
            rows.append(row(SPH_EXTRA[(2 * k + flip) // len(HINGE_EXTRA)], a, flip))
    assert len(rows) == N_DOF_DESIGNED
    dof = por.mh.f32(np.stack(rows))
    bad = sph_conditions(sph_maps(km, dof))
    if bad:
        raise ValueError("designed dofs: " + "; ".join(bad))
    while dof.shape[0] < n:
        cand = por.mh.f32(0.8 * rng.standard_normal((1, D)))
        if not sph_conditions(sph_maps(km, cand)):
            dof = np.concatenate([dof, cand])
    return dof[:n]


def _char_name(km):
    return km.kin_ref_name          # set by load_char: a model loaded any other way has no designed inputs


# ------------------------------------------------------------------------------------------------------------------ designed joint quaternions
# |v| of the unit quaternion and the scales it is stored at.  The reference's threshold is on the unnormalised |v|: 0.7e-5 crosses it
# when doubled.  0.5e-5 x 2 and 2e-5 x 0.5 would be the threshold itself, inside GUARD, where the two precisions may take different
# branches: those two products are not formed; 0.35e-5 and 3e-5 carry all three scales next to them.
JOINT_V = ((0.0, (1.0, 0.5, 2.0)), (0.35e-5, (1.0, 0.5, 2.0)), (0.5e-5, (1.0, 0.5)), (0.7e-5, (1.0, 0.5, 2.0)), (2e-5, (1.0, 2.0)),
           (3e-5, (1.0, 0.5, 2.0)), (1e-4, (1.0, 0.5, 2.0)), (1e-2, (1.0, 0.5, 2.0)))
JOINT_ANGLES = (1.0, PI - 1e-4, PI)          # the last one is w = 0 exactly
HINGE_TILT = (0.0, PI, PI / 3.0, 2.0 * PI / 3.0)     # rotation axis against the joint axis: parallel, antiparallel, 60 degrees from either


def designed_joint_rots(km, n=N_POSES, seed=None):
    """fp32 joint quaternions [n, J, 4] and their table [n, 4] (|v| of the unit quaternion or -angle, scale, sign, number of the base
    pose).  A base pose gives every moving joint the same (|v|, w) about an axis of its own: spherical joints a random one, hinge number
    h an axis tilted by HINGE_TILT[(h + base) % 4] from its joint axis; fixed joints hold random unit quaternions (their dofs do not
    exist).  The base pose is then stored at each of its scales and, right behind each, negated (w < 0): scaling by a power of two and
    negation are exact, so those rows are the same quaternion in every bit but exponent and sign.  Filler: random unit quaternions of
    either sign, redrawn until they pass the guards."""
    rng = np.random.default_rng((SEEDS[_char_name(km)] if seed is None else seed) + 1)
    J = km.get_num_joints() - 1
    base = [(v, math.sqrt(1.0 - v * v), v, scales) for v, scales in JOINT_V]
    base += [(math.sin(a / 2), 0.0 if a == PI else math.cos(a / 2), -a, (1.0, 0.5, 2.0)) for a in JOINT_ANGLES]
    rows, table = [], []
    for b, (s, w, tag, scales) in enumerate(base):
        q = np.zeros((J, 4))
        for j in range(1, J + 1):
            k = km.get_joint_dof_dim(j)
            if k == 3:
                u = _unit(rng.standard_normal(3))
            elif k == 1:
                a = _unit(_hinge_axis(km, j, torch.float64).numpy())
                p = _unit(np.cross(a, _unit(rng.standard_normal(3))))
                tilt = HINGE_TILT[(por.hinge_joints(km).index(j) + b) % 4]
                u = math.cos(tilt) * a + math.sin(tilt) * p
            else:
                q[j - 1] = _unit(rng.standard_normal(4))
                continue
            q[j - 1] = np.concatenate([s * u, [w]])
        q = por.mh.f32(q).astype(np.float64)
        for sc in scales:
            for sign in (1.0, -1.0):
                rows.append(sign * sc * q)
                table.append((tag, sc, sign, b))
    rot = por.mh.f32(np.stack(rows))
    bad = joint_rot_conditions(km, rot)
    if bad:
        raise ValueError("designed joint quaternions: " + "; ".join(bad))
    while rot.shape[0] < n:
        cand = por.mh.f32(_unit(rng.standard_normal((1, J, 4))))
        if not joint_rot_conditions(km, cand):
            rot = np.concatenate([rot, cand])
            table.append((math.nan, 1.0, 0.0, -1))
    return rot[:n], np.array(table[:n])


def joint_rot_conditions(km, rot):
    """unnormalised |v| outside GUARD; on hinges with |v| above the threshold |rotation axis . joint axis| >= MIN_AXIS_DOT"""
    rot = np.asarray(rot, np.float64)
    bad = []
    for j in range(1, km.get_num_joints()):
        k = km.get_joint_dof_dim(j)
        if not k:
            continue
        s = np.linalg.norm(rot[:, j - 1, :3], axis=1)
        bad += ["row {} joint {}: |v| {:.3e} inside the guard band".format(i, j, s[i]) for i in np.nonzero((s >= GUARD[0]) & (s <= GUARD[1]))[0]]
        if k == 1:
            dot = np.abs((rot[:, j - 1, :3] / np.maximum(s, 1e-300)[:, None]) @ _hinge_axis(km, j, torch.float64).numpy())
            bad += ["row {} joint {}: axis . joint axis {:.3e}".format(i, j, dot[i]) for i in np.nonzero((s > THRESHOLD) & (dot < MIN_AXIS_DOT))[0]]
    return bad


# ------------------------------------------------------------------------------------------------------------------ forward kinematics inputs
def fk_inputs(km, n=N_POSES):
    """fp32 (root_rot [n, 4], joint_rot [n, J, 4]): the float64 rotations of the designed dofs rounded to fp32, the root turned by the
    angle list along pose_opt_ref.ROOT_AXIS.  Run with the root at the origin and at ROOT_FAR."""
    jr = por.mh.f32(dof_to_rot(km, designed_dofs(km, n)))
    ang = np.array([ANGLES[k % len(ANGLES)] for k in range(n)])
    return por.mh.f32(_exp64(ang[:, None] * por.ROOT_AXIS)), jr


def fk_root_pos(n, where):
    return por.mh.f32(np.tile(ROOT_FAR if where == "far" else np.zeros(3), (n, 1)))


# ------------------------------------------------------------------------------------------------------------------ designed clips
LADDER = (0.0, 2e-4, 5e-4, 2e-3, 1e-2, 0.3, 1.0, PI / 2 - 1e-3)      # half angles between consecutive frames of the 12-frame clip
PAIR_V = (0.5e-5, 2e-5)                                               # |v| of the difference rotation of the two designed pairs
CLIP_NAMES = ("single", "two", "ladder30", "ladder120", "edges30", "edges120")
CLIP_FPS = (30.0, 120.0, 30.0, 120.0, 30.0, 120.0)
CLIP_LOOP = (0, 1, 0, 1, 1, 0)                                        # 0 CLAMP, 1 WRAP: one ladder and one edges clip of each
EDGE_FRAMES = 6


def designed_joints(km):
    """(spherical joint, hinge joint) that carry the designed differences next to the root"""
    return por.spherical_joints(km)[1], por.hinge_joints(km)[-1]


def _random_frame(km, rng):
    return np.concatenate([rng.standard_normal(3), 0.8 * rng.standard_normal(3), 0.6 * rng.standard_normal(km.get_dof_size())])


def _turned(e, half_angle, u):
    """exponential map of exp(2 half_angle u) (x) exp(e), float64"""
    return _log64(_qmul64(_exp64(2.0 * half_angle * u), _exp64(e)))


def _step(km, frame, half_angle, rng):
    """the next frame: root, the designed spherical joint and the designed hinge turned by 2 half_angle (identical at 0), every other
    joint redrawn, the root moved"""
    sj, hj = designed_joints(km)
    nxt = _random_frame(km, rng)
    nxt[0:3] = frame[0:3] + 0.02 * rng.standard_normal(3)
    d0, dh = 6 + km.get_joint_dof_idx(sj), 6 + km.get_joint_dof_idx(hj)
    if half_angle == 0.0:
        nxt[3:6], nxt[d0:d0 + 3], nxt[dh] = frame[3:6], frame[d0:d0 + 3], frame[dh]
    else:
        nxt[3:6] = _turned(frame[3:6], half_angle, _unit(rng.standard_normal(3)))
        nxt[d0:d0 + 3] = _turned(frame[d0:d0 + 3], half_angle, _unit(rng.standard_normal(3)))
        nxt[dh] = frame[dh] + 2.0 * half_angle
    return nxt


def designed_clips(km, seed=None):
    """list of fp32 frame arrays [F, 6 + D], in the order of CLIP_NAMES.
    single: one frame.  two: two random frames.  ladder: 12 frames; frames k, k + 1 (k < 8) differ on the root, on one spherical and on
    one hinge joint by the half angle LADDER[k]; three random frames follow.  edges: frame 1 -> 2 takes the root's exponential map
    from |e| = pi - 1e-2 to pi + 1e-2 along one axis (the stored quaternions have cos < 0) while the two designed joints turn by a
    difference rotation of |v| = 0.5e-5; 2 -> 3 turns root and both joints by |v| = 2e-5; 3 -> 4 turns the root by |v| = 0.5e-5 and
    leaves the joints identical; frames 0 and 5 are random."""
    rng = np.random.default_rng((SEEDS[_char_name(km)] if seed is None else seed) + 2)
    sj, hj = designed_joints(km)
    d0, dh = 6 + km.get_joint_dof_idx(sj), 6 + km.get_joint_dof_idx(hj)
    clips = [np.stack([_random_frame(km, rng)]), np.stack([_random_frame(km, rng), _random_frame(km, rng)])]
    for _ in range(2):
        fr = [_random_frame(km, rng)]
        fr[0][dh] = -1.2                                 # the ladder adds 5.8 rad to the hinge
        for h in LADDER:
            fr.append(_step(km, fr[-1], h, rng))
        fr += [_random_frame(km, rng) for _ in range(12 - len(fr))]
        clips.append(np.stack(fr))
    for _ in range(2):
        u = _unit(rng.standard_normal(3))
        f0, f1 = _random_frame(km, rng), _random_frame(km, rng)
        f1[3:6] = (PI - 1e-2) * u
        f2 = f1.copy()
        f2[3:6] = (PI + 1e-2) * u
        f2[0:3] += 0.01
        f2[d0:d0 + 3] = _turned(f1[d0:d0 + 3], math.asin(PAIR_V[0]), _unit(rng.standard_normal(3)))
        f2[dh] = f1[dh] + 2.0 * math.asin(PAIR_V[0])
        f3 = _step(km, f2, math.asin(PAIR_V[1]), rng)
        keep = [k for k in range(6, 6 + km.get_dof_size()) if k not in (d0, d0 + 1, d0 + 2, dh)]
        f3[keep] = f2[keep]
        f4 = f3.copy()
        f4[3:6] = _turned(f3[3:6], math.asin(PAIR_V[0]), _unit(rng.standard_normal(3)))
        clips.append(np.stack([f0, f1, f2, f3, f4, _random_frame(km, rng)]))
    clips = [por.mh.f32(c) for c in clips]
    bad = [b for c in clips for b in clip_conditions(km, c)]
    if bad:
        raise ValueError("designed clips: " + "; ".join(bad))
    return clips


def pair_measures(rot0, rot1):
    """float64, of quaternion pairs [..., 4]: (|v| of normalised conj(q0) (x) q1, sin of slerp's half angle, slerp's cosine)"""
    a, b = np.asarray(rot0, np.float64), np.asarray(rot1, np.float64)
    d = _qmul64(a * _CONJ, b)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    c = (a * b).sum(-1)
    return np.linalg.norm(d[..., :3], axis=-1), np.sqrt(np.maximum(1.0 - c * c, 0.0)), c


def rows_conditions(rot):
    """guards of stored frame rotations [F, 1 + J, 4] (root first): between consecutive frames |v| of the difference rotation outside
    GUARD and slerp's sine outside SLERP_GUARD"""
    rot = np.asarray(rot, np.float64)
    if rot.shape[0] < 2:
        return []
    v, s, _ = pair_measures(rot[:-1], rot[1:])
    bad = ["frames {}: |v| {:.3e} of joint {} inside the guard band".format(i, v[i, j], j) for i, j in zip(*np.nonzero((v >= GUARD[0]) & (v <= GUARD[1])))]
    bad += ["frames {}: slerp sine {:.3e} of joint {} inside its guard band".format(i, s[i, j], j) for i, j in zip(*np.nonzero((s >= SLERP_GUARD[0]) & (s <= SLERP_GUARD[1])))]
    return bad


def clip_conditions(km, frames):
    """the maps' own guards (threshold and wrap of exp_map_to_quat), and rows_conditions of the float64 rows"""
    maps = np.concatenate([np.asarray(frames, np.float64)[:, None, 3:6], sph_maps(km, np.asarray(frames)[:, 6:])], axis=1)
    raw = np.linalg.norm(maps, axis=-1)
    w = por.wrapped(raw)
    bad = ["frame {} map {}: wrapped angle {:.3e} inside the guard band".format(i, j, w[i, j]) for i, j in zip(*np.nonzero((w >= GUARD[0]) & (w <= GUARD[1]) & (raw != 0)))]
    bad += ["frame {} map {}: raw angle {:.9f} within 1e-3 of the wrap at pi".format(i, j, raw[i, j]) for i, j in zip(*np.nonzero(np.abs(w - PI) < FAR_PI))]
    b = clip_build(km, frames, 30.0)
    return bad + rows_conditions(np.concatenate([b["root_rot"][:, None], b["joint_rot"]], axis=1))


# ------------------------------------------------------------------------------------------------------------------ queries
BLENDS = (0.0, 2.0 ** -20, 0.25, 0.5, 1.0 - 2.0 ** -20)


def designed_queries(clips):
    """(ids int64 [Q], times fp32 [Q]): every frame pair of every clip at every blend of BLENDS, time = clip length (the blend into the
    clamped last frame; on a WRAP clip the first loop), and on WRAP clips 2.5 lengths"""
    ids, times = [], []
    for c, fr in enumerate(clips):
        F, fps = fr.shape[0], CLIP_FPS[c]
        for i in range(F - 1):
            for b in BLENDS:
                ids.append(c)
                times.append((i + b) / fps)
        ids.append(c)
        times.append((F - 1) / fps)
        if CLIP_LOOP[c] == 1:
            ids.append(c)
            times.append(2.5 * (F - 1) / fps)
    return np.array(ids, np.int64), np.array(times, np.float32)


def frame_pairs(ids, times, num_frames, fps, loop):
    """make_query (parc_motion_query.h; motion_lib.py:443-456,527-538) in fp32, operation by operation -> (i0, i1 frame numbers within
    the clip, blend fp32, loop_phase fp32 (0 on CLAMP clips), blend64).  The index arithmetic has exact tests of its own
    (test_bookkeeping_gpu).  blend64 is the yardstick's blend: the same expressions in float64 from the same fp32 time and clip length,
    taken relative to the fp32 frame pair (so it may leave [0, 1] by a rounding).  The fp32 blend is phase * (frames - 1) rounded, minus
    i0: up to half an ulp of the frame number away from blend64, which a fused multiply-subtract on the device does not share; float64
    rows blended at the fp32 blend would charge that rounding to the kernel."""
    f32 = np.float32
    nf = np.asarray(num_frames)[ids]
    length = (1.0 / np.asarray(fps, np.float64)[ids] * (nf - 1)).astype(f32)
    wrap = np.asarray(loop)[ids] == 1
    with np.errstate(divide="ignore", invalid="ignore"):
        phase = (np.asarray(times, f32) / length).astype(f32)
        phase64 = np.asarray(times, f32).astype(np.float64) / length.astype(np.float64)
    loop_phase = np.floor(phase).astype(f32)
    phase = np.where(wrap, (phase - loop_phase).astype(f32), phase)
    phase = np.fmin(np.fmax(phase, f32(0)), f32(1)).astype(f32)
    fp = (phase * (nf - 1).astype(f32)).astype(f32)
    i0 = fp.astype(np.int64)
    i1 = np.minimum(i0 + 1, nf - 1)
    phase64 = np.where(wrap, phase64 - np.floor(phase64), phase64)
    phase64 = np.fmin(np.fmax(phase64, 0.0), 1.0)
    blend64 = np.where(nf > 1, phase64 * (nf - 1) - i0, 0.0)
    assert np.array_equal(np.floor(np.where(nf > 1, np.asarray(times, f32).astype(np.float64) / np.maximum(length, f32(1e-30)).astype(np.float64), 0.0))[wrap],
                          loop_phase[wrap].astype(np.float64)), "a designed time sits on a loop boundary"
    return i0, i1, (fp - i0.astype(f32)).astype(f32), np.where(wrap, loop_phase, f32(0)).astype(f32), blend64


def slerp_decade(s):
    s = np.asarray(s)
    out = np.full(s.shape, -1)
    for k, (lo, hi) in enumerate(SLERP_DECADES):
        out[(s >= lo) & (s < hi)] = k
    return out


def cosine_fp32(rot0, rot1):
    """slerp's |cosine| as fp32 evaluates it: the four rounded products summed left to right (torch's sum over four elements, the C
    oracle and the device's dot4_unfused all do).  Where it is >= 1 fp32 returns q0, bit for bit, whatever float64 says: those pairs
    are held to the exact branch and belong to no bucket."""
    p = np.asarray(rot0, np.float32) * np.asarray(rot1, np.float32)
    return np.abs(((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])


def slerp_error_by_decade(got, ref64, s, one):
    """[4]: largest |got - ref64| per decade of the pair's float64 sin(half angle), over the pairs whose fp32 cosine is below 1 (`one`
    marks the others); got, ref64 [..., 4], s, one [...]"""
    err = np.abs(np.asarray(got, np.float64) - ref64).max(axis=-1)
    dec = np.where(one, -1, slerp_decade(s))
    return np.array([float(err[dec == k].max()) if (dec == k).any() else 0.0 for k in range(len(SLERP_DECADES))])


# ------------------------------------------------------------------------------------------------------------------ designed root rotations
HEADINGS = (0.0, PI / 2 - 1e-3, PI / 2 + 1e-3, -(PI / 2 - 1e-3), -(PI / 2 + 1e-3), PI - 1e-3, PI + 1e-3, -(PI - 1e-3), -(PI + 1e-3))
TILTS = (("pitch", 0.0), ("pitch", 0.7), ("roll", 0.5))
N_HEADING_DESIGNED = len(HEADINGS) * len(TILTS) + 2


def designed_root_rots(n=N_POSES, seed=3730):
    """fp32 [n, 4]: every heading of HEADINGS (both sides of cos h = 0 and of h = +-pi, the two branch switches of
    calc_heading_quat_inv_alg) at pitch 0, pitch 0.7 and roll 0.5; the identity; the half turn about z (0, 0, 1, 0); random unit
    quaternions, redrawn until the rotated x axis has horizontal length >= MIN_HORIZONTAL"""
    rng = np.random.default_rng(seed)
    rows = []
    for h in HEADINGS:
        for kind, a in TILTS:
            tilt = _exp64(a * np.array([0.0, 1.0, 0.0] if kind == "pitch" else [1.0, 0.0, 0.0]))
            rows.append(_qmul64(_exp64(h * np.array([0.0, 0.0, 1.0])), tilt))
    rows += [np.array([0.0, 0.0, 0.0, 1.0]), np.array([0.0, 0.0, 1.0, 0.0])]
    q = por.mh.f32(np.stack(rows))
    if heading_conditions(q):
        raise ValueError("designed root rotations: " + "; ".join(heading_conditions(q)))
    while q.shape[0] < n:
        cand = por.mh.f32(_unit(rng.standard_normal((1, 4))))
        if not heading_conditions(cand):
            q = np.concatenate([q, cand])
    return q[:n]


def horizontal_length(q):
    q = np.asarray(q, np.float64)
    a = 1.0 - 2.0 * (q[..., 1] ** 2 + q[..., 2] ** 2)
    b = 2.0 * (q[..., 3] * q[..., 2] + q[..., 0] * q[..., 1])
    return np.hypot(a, b)


def heading_conditions(q):
    r = horizontal_length(q)
    return ["rotation {}: horizontal length {:.3e} of the rotated x axis".format(i, r[i]) for i in np.nonzero(r < MIN_HORIZONTAL)[0]]


def root_velocities(n):
    """fp32 (root velocity, root angular velocity) [n, 3]: those of the G6 state (tests/golden/g6_step.npz), which the GPU heading test
    keeps while it replaces the root rotations"""
    g6 = np.load(os.path.join(REPO, "tests", "golden", "g6_step.npz"))
    assert g6["char_root_vel"].shape[0] >= n
    return por.mh.f32(g6["char_root_vel"][:n]), por.mh.f32(g6["char_root_ang_vel"][:n])


# ------------------------------------------------------------------------------------------------------------------ e-bar
def signless_error(got, ref64):
    """largest |got - ref64| after giving every quaternion of `got` the sign of its float64 partner (q and -q are one rotation)"""
    got = np.asarray(got, np.float64)
    return value_error(got * np.where((got * ref64).sum(-1, keepdims=True) < 0, -1.0, 1.0), ref64)


def far_joints(km, dof):
    return _raw_angles(km, dof) > FAR_ANGLE


def _round_up(x):
    return por._round_up(float(x))


def measure(z):
    """the e-bars of fixture G37 (an open npz): |reference fp32 - reference float64|"""
    m = dict(dof_to_rot={"near": 0.0, "far": 0.0}, rot_to_dof=0.0, fk={w: {"body_pos": 0.0, "body_rot": 0.0} for w in ("origin", "far")},
             build_rows={"root_rot": 0.0, "joint_rot": 0.0}, build_vel={int(f): {"root_vel": 0.0, "root_ang_vel": 0.0, "dof_vel": 0.0} for f in FPS},
             slerp=np.zeros(len(SLERP_DECADES)), root_pos=0.0, root_block=0.0)
    for c in CHARS:
        km = load_char(c)
        far = far_joints(km, z[c + "_dof"])
        err = np.abs(z[c + "_f32_joint_rot"].astype(np.float64) - z[c + "_f64_joint_rot"]).max(axis=-1)
        m["dof_to_rot"]["near"] = max(m["dof_to_rot"]["near"], float(err[~far].max()))
        m["dof_to_rot"]["far"] = max(m["dof_to_rot"]["far"], float(err[far].max()))
        m["rot_to_dof"] = max(m["rot_to_dof"], value_error(z[c + "_f32_dof_back"], z[c + "_f64_dof_back"]))
        for w in ("origin", "far"):
            for k in ("body_pos", "body_rot"):        # body rotations do not see the root position: recorded once, at the origin
                w_ = "origin" if k == "body_rot" else w
                m["fk"][w][k] = max(m["fk"][w][k], value_error(z["{}_f32_{}_{}".format(c, w_, k)], z["{}_f64_{}_{}".format(c, w_, k)]))
        for i, name in enumerate(CLIP_NAMES):
            for k in m["build_rows"]:
                m["build_rows"][k] = max(m["build_rows"][k], value_error(z["{}_{}_f32_{}".format(c, name, k)], z["{}_{}_f64_{}".format(c, name, k)]))
            for k in m["build_vel"][int(CLIP_FPS[i])]:
                m["build_vel"][int(CLIP_FPS[i])][k] = max(m["build_vel"][int(CLIP_FPS[i])][k],
                                                          value_error(z["{}_{}_f32_{}".format(c, name, k)], z["{}_{}_f64_{}".format(c, name, k)]))
        m["slerp"] = np.maximum(m["slerp"], slerp_error_by_decade(z[c + "_q_f32_rot"], z[c + "_q_f64_rot"], z[c + "_q_sine"], z[c + "_q_one"]))
        m["root_pos"] = max(m["root_pos"], value_error(z[c + "_q_f32_root_pos"], z[c + "_q_f64_root_pos"]))
    m["root_block"] = value_error(z["head_f32_block"], z["head_f64_block"])
    m["heading_quat"] = signless_error(z["head_f32_hinv"], z["head_f64_hinv"])
    return m


def main():
    m = measure(np.load(FIXTURE))
    print("e-bar over G37: |reference fp32 - reference float64|")
    print("MEASURED_DOF_TO_ROT = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["dof_to_rot"].items()))
    print("MEASURED_ROT_TO_DOF = %.3g" % _round_up(m["rot_to_dof"]))
    print("MEASURED_FK = {%s}" % ", ".join("\"%s\": {%s}" % (w, ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in d.items())) for w, d in m["fk"].items()))
    print("MEASURED_BUILD_ROWS = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["build_rows"].items()))
    print("MEASURED_BUILD_VEL = {%s}" % ", ".join("%d: {%s}" % (f, ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in d.items())) for f, d in m["build_vel"].items()))
    print("MEASURED_SLERP_DECADE = (%s)" % ", ".join("%.3g" % _round_up(v) for v in m["slerp"]))
    print("MEASURED_ROOT_POS = %.3g" % _round_up(m["root_pos"]))
    print("MEASURED_ROOT_BLOCK = %.3g" % _round_up(m["root_block"]))
    print("MEASURED_HEADING_QUAT = %.3g" % _round_up(m["heading_quat"]))


if __name__ == "__main__":
    main()
