"""Float64 evaluation of the motion optimiser's four differentiable primitives (parc_amd/csrc/parc_pose_opt.hip: pose chain, angle
between rotations, body sample points, frame-to-frame terms) -- TEST INFRASTRUCTURE, touches no GPU.

The yardstick of tests/test_pose_opt_gpu.py where fixture G34 does not reach (the shape sweep): the project's torch ports
(util/torch_util.py, KinCharModel.dof_to_rot_torch / forward_kinematics_torch) run in float64 with autograd on a float64 copy of the
character model, and moopt_host.TtCase.float64 for the frame-to-frame terms.  tests/test_pose_opt_ref_cpu.py pins this module against
the float64 record in G34 (the reference's own for three primitives, a torch restatement for the frame-to-frame terms) and against
central differences.

Also here: the designed inputs (every branch point of the kernels visited on both sides, tests/golden/gen_pose_opt.py stores them in
G34), the synthetic 16-body character, the error measures and the measured e-bars.

Run as a script it prints e-bar, the largest |reference fp32 - reference float64| over G34 per primitive; the MEASURED_* constants
below are those figures rounded up.  They come from torch code on the CPU (the reference's; for the frame-to-frame terms the
restatement temporal_terms_torch below, which the generator runs in both precisions), never from the kernels.
"""
import copy
import math
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from parc_amd.anim import kin_char_model  # noqa: E402
from parc_amd.util import torch_util  # noqa: E402
import moopt_host as mh  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "g34_pose_opt.npz")
CHARS = ("hum", "syn")
OUTS = ("root_quat", "joint_rot", "body_pos", "body_rot")
INS = ("root_pos", "root_exp", "dof")
# cotangent runs of the pose chain: all four outputs, then one output alone
RUNS = ("all",) + OUTS
PI = math.pi
# the angle list of the designed frames: both sides of the 1e-5 threshold, of the wrap at pi and of the wrap back to zero at 2 pi
ANGLES = (5e-6, 2e-5, 1e-4, 1e-2, 1.0, PI - 1e-3, PI + 1e-3, 4.0, 2 * PI - 1e-2, 2 * PI - 1e-4, 2 * PI - 2e-5, 2 * PI + 2e-5, 2 * PI + 1e-2, 9.0)
ZERO_FRAME = len(ANGLES)            # the frame whose root exponential map is exactly zero
N_DESIGNED = ZERO_FRAME + 1
THRESHOLD = 1e-5                    # of exp_map_to_quat (wrapped angle) and quat_diff_angle (|v| of the difference)
GUARD = (0.8e-5, 1.25e-5)           # no designed or random input may fall here in float64: the two precisions could disagree on the branch
# difference angles of the pairs; |v| of the difference is about a / 2
PAIR_ANGLES = (0.0, 0.5e-5, 2e-5 * 2, 1e-4 * 2, 1e-3, 1e-2, 1.0, PI - 1e-2, PI - 1e-4)
DECADES = ((GUARD[1], 1e-4), (1e-4, 1e-3), (1e-3, 1e-2), (1e-2, math.inf))      # of float64 |v|, for the angle gradient's e-bar

# e-bar: max |reference fp32 - reference float64| over G34 (python tests/tools/pose_opt_ref.py prints them), rounded up to 3 digits.
# values: absolute; gradients: relative to the per-frame (per-pair) maximum of the float64 gradient of that input tensor.
MEASURED_POSE_VALUE = 9.06e-07              # over the four outputs: e-bar of the primitive, the unit of the torch fp32 path on the device
# per output: the unit the kernels are held to.  (Not the torch path's: at a raw angle next to pi or 2 pi one ulp of the fp32 norm, 2.4e-7 or
# 4.8e-7, moves the quaternion by half of it, and how torch's reduction rounds there differs between the CPU and the device - DESIGN.md.)
MEASURED_POSE_VALUE_BY_OUTPUT = {"root_quat": 1.01e-07, "joint_rot": 9.53e-08, "body_pos": 9.06e-07, "body_rot": 5.88e-07}
MEASURED_POSE_GRAD = {"root_pos": 2.51e-07, "root_exp": 5.14e-06, "dof": 5.56e-07}      # over the run with cotangents on all four outputs
MEASURED_ANGLE_VALUE = 2.76e-07
MEASURED_ANGLE_GRAD_DECADE = (0.00411, 0.000836, 2.1e-05, 4.22e-07)     # |v| in [1.25e-5, 1e-4), [1e-4, 1e-3), [1e-3, 1e-2), [1e-2, ..): goes as 1 / |v|
MEASURED_POINTS_VALUE = 1.23e-07
MEASURED_POINTS_GRAD = {"body_pos": 8.37e-08, "body_rot": 1.21e-07}
MEASURED_TT_VALUE = 4.73e-05
MEASURED_TT_GRAD = {"g_pos": 2.77e-07, "g_r": 9.07e-08}
DEVICE_FACTOR, TORCH_FACTOR = 4.0, 2.0      # bounds of the GPU tests: kernels 4 e-bar, the torch fp32 path on the device 2 e-bar


# ------------------------------------------------------------------------------------------------------------------ characters
_SYN_BODIES = (
    # name, depth, pos, quat (w x y z) or None, joint: "sph" | "fixed" | hinge axis
    ("base", 0, "0 0 0", None, None),
    ("spine", 1, "0.01 0 0.21", "0.980067 0.198669 0 0", "sph"),
    ("chest", 2, "0 0.02 0.25", "0.955336 0 0.295520 0", "0.3 0.5 -0.8"),            # the branching body: neck, both shoulders
    ("neck", 3, "0.01 0 0.2", "0.921061 0 0 0.389418", "fixed"),                     # fixed, inside a chain
    ("head", 4, "0 0.01 0.12", "0.877583 0.276642 -0.276642 0.276642", "sph"),       # ... with a child below it
    ("r_upper", 3, "-0.02 -0.2 0.18", "0.968912 -0.142857 0.142857 0.142857", "sph"),
    ("r_lower", 4, "0.03 -0.27 0", None, "0 2 1"),
    ("r_hand", 5, "0 -0.25 0.02", "0.995004 0 0.099833 0", "fixed"),
    ("l_upper", 3, "-0.02 0.2 0.18", "0.968912 0.142857 0.142857 -0.142857", "sph"),
    ("l_lower", 4, "0.03 0.27 0", "0.980067 0 0 -0.198669", "0.5 0.5 0"),
    ("r_thigh", 1, "0 -0.09 -0.04", "0.995004 0.099833 0 0", "sph"),
    ("r_shin", 2, "0.02 0 -0.42", None, "-0.2 1.3 0.4"),
    ("r_foot", 3, "0 0.01 -0.41", "0.980067 0 -0.198669 0", "1 0 0.5"),
    ("l_thigh", 1, "0 0.09 -0.04", "0.995004 -0.099833 0 0", "sph"),
    ("l_shin", 2, "0.02 0 -0.42", "0.955336 0 0 0.295520", "0.2 1.3 -0.4"),
    ("l_foot", 3, "0 -0.01 -0.41", None, "0 0.7 0.7"),                               # the dof vector ends on a hinge
)


def synthetic_mjcf(extra_leaf=False):
    """MJCF text of a 16-body tree (PARC_MAX_BODIES) that walks what the humanoid does not: a fixed joint inside a chain with a child
    below it, hinges on oblique non-unit axes, spherical joints, a body with three children, non-identity local rotations, a dof vector
    that ends on a hinge.  extra_leaf adds a 17th body."""
    bodies = list(_SYN_BODIES) + ([("l_toe", 4, "0.1 0 0", None, "0 1 0")] if extra_leaf else [])
    lines = ["<mujoco model=\"pose_opt_tree\">", "  <default>", "    <default class=\"body\">", "      <geom type=\"sphere\"/>",
             "      <joint type=\"hinge\" limited=\"true\"/>", "    </default>", "  </default>", "  <worldbody>"]
    open_depths = []
    for name, depth, pos, quat, joint in bodies:
        while open_depths and open_depths[-1] >= depth:
            lines.append("  " * (open_depths.pop() + 2) + "</body>")
        ind = "  " * (depth + 2)
        lines.append("{}<body name=\"{}\" pos=\"{}\"{}{}>".format(ind, name, pos, "" if quat is None else " quat=\"{}\"".format(quat),
                                                                 " childclass=\"body\"" if depth == 0 else ""))
        if joint == "sph":
            for k, ax in enumerate(("1 0 0", "0 1 0", "0 0 1")):
                lines.append("{}  <joint name=\"{}_{}\" type=\"hinge\" axis=\"{}\" range=\"-180 180\"/>".format(ind, name, "xyz"[k], ax))
        elif joint is not None and joint != "fixed":
            lines.append("{}  <joint name=\"{}\" type=\"hinge\" axis=\"{}\" range=\"-180 180\"/>".format(ind, name, joint))
        lines.append("{}  <geom name=\"{}\" type=\"sphere\" pos=\"0 0 0\" size=\"0.05\"/>".format(ind, name))
        open_depths.append(depth)
    while open_depths:
        lines.append("  " * (open_depths.pop() + 2) + "</body>")
    lines += ["  </worldbody>", "</mujoco>", ""]
    return "\n".join(lines)


def write_synthetic(path, extra_leaf=False):
    with open(path, "w") as f:
        f.write(synthetic_mjcf(extra_leaf))
    return path


def load_char(name, device="cpu"):
    """"hum": the shipped humanoid; "syn": the synthetic tree"""
    km = kin_char_model.KinCharModel(device)
    if name == "hum":
        km.load_char_file(kin_char_model.default_char_file())
    else:
        assert name == "syn", name
        with tempfile.TemporaryDirectory() as d:
            km.load_char_file(write_synthetic(os.path.join(d, "pose_opt_tree.xml")))
    return km


def f64_model(km):
    """a float64 copy on the CPU of what dof_to_rot_torch / forward_kinematics_torch read: local translations and rotations and the
    hinge axes, each the model's fp32 number cast up"""
    m = copy.copy(km)
    m._device = torch.device("cpu")
    m._parent_indices = km._parent_indices.detach().cpu()
    m._local_translation = km._local_translation.detach().cpu().double()
    m._local_rotation = km._local_rotation.detach().cpu().double()
    m._c_struct = None
    m._tt = None
    tables = dict(m._torch_tables())
    tables["axis"] = tables["axis"].double()
    m._tt = tables
    return m


def spherical_joints(km):
    return [j for j in range(1, km.get_num_joints()) if km.get_joint(j).get_dof_dim() == 3]


def hinge_joints(km):
    return [j for j in range(1, km.get_num_joints()) if km.get_joint(j).get_dof_dim() == 1]


# ------------------------------------------------------------------------------------------------------------------ inputs
ROOT_AXIS = np.array([1.0, 2.0, -2.0]) / 3.0            # oblique and unit
JOINT_AXIS = np.array([2.0, -1.0, 2.0]) / 3.0


def pose_chain_inputs(km, n, seed):
    """fp32 (root_pos [n, 3], root_exp [n, 3], dof [n, D]): frame k < len(ANGLES) has the root map ANGLES[k] along ROOT_AXIS, the same
    angle along JOINT_AXIS on one spherical joint (rotating through the joints) and on every hinge; frame ZERO_FRAME has a root map of
    exactly zero; every other entry is random (maps 0.8 N(0, 1), dofs 0.7 N(0, 1)).  n cuts the list short or adds random frames."""
    rng = np.random.default_rng(seed)
    D = km.get_dof_size()
    rp = rng.standard_normal((n, 3))
    re = 0.8 * rng.standard_normal((n, 3))
    dof = 0.7 * rng.standard_normal((n, D))
    sph, hin = spherical_joints(km), hinge_joints(km)
    for k, ang in enumerate(ANGLES[:n]):
        re[k] = ang * ROOT_AXIS
        d0 = km.get_joint_dof_idx(sph[k % len(sph)])
        dof[k, d0:d0 + 3] = ang * JOINT_AXIS
        for j in hin:
            dof[k, km.get_joint_dof_idx(j)] = ang
    if n > ZERO_FRAME:
        re[ZERO_FRAME] = 0.0
    return mh.f32(rp), mh.f32(re), mh.f32(dof)


def pose_chain_cotangents(km, n, seed):
    rng = np.random.default_rng(seed)
    B = km.get_num_joints()
    return {"root_quat": mh.f32(rng.standard_normal((n, 4))), "joint_rot": mh.f32(rng.standard_normal((n, B - 1, 4))),
            "body_pos": mh.f32(rng.standard_normal((n, B, 3))), "body_rot": mh.f32(rng.standard_normal((n, B, 4)))}


def run_cotangents(cots, run):
    """the cotangents of one run: all four, or one output's with zeros on the others"""
    return {k: (v if run in ("all", k) else np.zeros_like(v)) for k, v in cots.items()}


def wrapped(raw):
    return np.abs(np.arctan2(np.sin(raw), np.cos(raw)))


def exp_maps_of(km, root_exp, dof):
    """[n, 1 + S, 3] float64: the root map and every spherical joint's"""
    cols = [np.asarray(root_exp, np.float64)]
    for j in spherical_joints(km):
        d0 = km.get_joint_dof_idx(j)
        cols.append(np.asarray(dof, np.float64)[:, d0:d0 + 3])
    return np.stack(cols, axis=1)


def pose_conditions(km, root_exp, dof):
    """the conditions on the (fp32-rounded) inputs, judged in float64 -> list of violations: no wrapped angle in GUARD (an exactly zero
    map excepted), no raw angle within 1e-5 of the wrap at pi (there the two precisions may return q and -q)"""
    raw = np.linalg.norm(exp_maps_of(km, root_exp, dof), axis=-1)
    w = wrapped(raw)
    bad = []
    for f, s in zip(*np.nonzero((w >= GUARD[0]) & (w <= GUARD[1]) & (raw != 0.0))):
        bad.append("frame {} map {}: wrapped angle {:.3e} inside the guard band".format(f, s, w[f, s]))
    for f, s in zip(*np.nonzero(np.abs(w - PI) < 1e-5)):
        bad.append("frame {} map {}: raw angle {:.9f} within 1e-5 of the wrap at pi".format(f, s, raw[f, s]))
    return bad


def pose_branch_distance(km, root_exp, dof):
    """[n] float64: how far the frame's maps are from a branch point (wrapped angle 1e-5 or pi, or an exactly zero map)"""
    raw = np.linalg.norm(exp_maps_of(km, root_exp, dof), axis=-1)
    w = wrapped(raw)
    return np.minimum(np.abs(w - THRESHOLD), np.abs(w - PI)).min(axis=1) * (raw != 0.0).all(axis=1)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _qmul64(a, b):
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - (av * bv).sum(-1, keepdims=True)], axis=-1)


def _exp64(e):
    ang = np.linalg.norm(e, axis=-1, keepdims=True)
    return np.concatenate([np.where(ang > 0, e / np.maximum(ang, 1e-300), 0.0) * np.sin(ang / 2), np.cos(ang / 2)], axis=-1)


_UNITS = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]])


def angle_pair_inputs(seed=341):
    """fp32 pairs of quat_diff_angle -> dict(q0 [248, 4], q1 [248, 4], bq0 [1, 4], bq1 [72, 4], group [248]): 320 pairs.
    group 0: q1 = exp(a u) (x) q0 for the 9 angles of PAIR_ANGLES, 8 random (q0, u) each; 1: the same kind with q1 negated (d.w < 0);
    2: d.w = 0 exactly (axis-aligned half turns of the signed unit quaternions); 3: the kind of 0 / 1 with both operands scaled to norm
    1 +- 1 %; 4: random pairs.  bq0 / bq1: one q0 broadcast against 72 pairs of the kind of 0 / 1."""
    rng = np.random.default_rng(seed)

    def family(n_each, q0=None):
        a = np.repeat(np.array(PAIR_ANGLES), n_each)
        base = _unit(rng.standard_normal((a.size, 4))) if q0 is None else np.broadcast_to(q0, (a.size, 4))
        u = _unit(rng.standard_normal((a.size, 3)))
        return base, _qmul64(_exp64(a[:, None] * u), base)

    a0, a1 = family(8)
    b0, b1 = family(8)
    b1 = -b1
    c0 = np.concatenate([s * _UNITS for s in (1.0, -1.0)])                                  # 8 signed units
    c0 = np.repeat(c0, 3, axis=0)
    c1 = _qmul64(np.tile(_UNITS[:3], (8, 1)), c0)
    d0, d1 = family(8)
    d1 = d1 * np.where(rng.uniform(size=(d1.shape[0], 1)) < 0.5, -1.0, 1.0)
    d0, d1 = d0 * (1.0 + 0.01 * rng.uniform(-1, 1, size=(d0.shape[0], 1))), d1 * (1.0 + 0.01 * rng.uniform(-1, 1, size=(d1.shape[0], 1)))
    e0, e1 = _unit(rng.standard_normal((8, 4))), _unit(rng.standard_normal((8, 4)))
    bq0 = _unit(rng.standard_normal((1, 4)))
    _, bq1 = family(8, bq0)
    bq1 = bq1 * np.where(np.arange(bq1.shape[0])[:, None] % 2 == 1, -1.0, 1.0)
    group = np.concatenate([np.full(x.shape[0], g) for g, x in enumerate((a0, b0, c0, d0, e0))]).astype(np.int32)
    return dict(q0=mh.f32(np.concatenate([a0, b0, c0, d0, e0])), q1=mh.f32(np.concatenate([a1, b1, c1, d1, e1])), bq0=mh.f32(bq0), bq1=mh.f32(bq1),
                group=group, cot=mh.f32(rng.standard_normal(group.size)), bcot=mh.f32(rng.standard_normal(bq1.shape[0])))


def angle_sweep_inputs(n, seed):
    """n pairs for the shape sweep: the 248 + 72 designed pairs (q0 of the broadcast case expanded) cycled to n"""
    z = angle_pair_inputs()
    q0 = np.concatenate([z["q0"], np.broadcast_to(z["bq0"], z["bq1"].shape)])
    q1 = np.concatenate([z["q1"], z["bq1"]])
    idx = np.arange(n) % q0.shape[0]
    return mh.f32(q0[idx]), mh.f32(q1[idx]), mh.f32(np.random.default_rng(seed).standard_normal(n))


def pair_difference(q0, q1):
    """float64 (|v|, w) of q1 (x) conj(q0)"""
    a, b = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    d = _qmul64(np.broadcast_to(b, np.broadcast_shapes(a.shape, b.shape)), np.broadcast_to(a, np.broadcast_shapes(a.shape, b.shape)) * np.array([-1.0, -1, -1, 1]))
    return np.linalg.norm(d[..., :3], axis=-1), d[..., 3]


def angle_conditions(q0, q1):
    s, _ = pair_difference(q0, q1)
    return ["pair {}: |v| {:.3e} inside the guard band".format(i, s[i]) for i in np.nonzero((s >= GUARD[0]) & (s <= GUARD[1]))[0]]


POINT_COUNTS = (4, 3, 0, 5, 1, 2, 3, 2, 4, 1, 3, 2, 2, 3, 2)          # body 2 owns no point; 37 points in all


def body_points_inputs(seed=342):
    """fp32 dict(local [37, 3], counts [15], pos [2, 4, 15, 3], rot [2, 4, 15, 4] of norm 1 +- 1 %, cot [2, 4, 37, 3]): a leading batch
    dimension, 8 frames x 37 points = 296 threads (more than one workgroup of 256), 8 x 15 in the adjoint"""
    rng = np.random.default_rng(seed)
    B, P = len(POINT_COUNTS), sum(POINT_COUNTS)
    rot = _unit(rng.standard_normal((2, 4, B, 4))) * (1.0 + 0.01 * rng.uniform(-1, 1, size=(2, 4, B, 1)))
    return dict(local=mh.f32(0.2 * rng.standard_normal((P, 3))), counts=np.array(POINT_COUNTS, np.int64), pos=mh.f32(rng.standard_normal((2, 4, B, 3))),
                rot=mh.f32(rot), cot=mh.f32(rng.standard_normal((2, 4, P, 3))))


# ------------------------------------------------------------------------------------------------------------------ evaluation
def _np(x):
    return x.detach().cpu().numpy()


def pose_chain(km, root_pos, root_exp, dof, cots=None, dtype=torch.float64, device="cpu"):
    """the project's torch ports with autograd -> (outputs {name: array}, gradients {name: array} | None).  km must hold tensors of
    `dtype` on `device` (f64_model(km) for float64).  An exactly zero root map gives NaN in g_root_exp (0 / 0 through torch.where, as
    in the reference); expected_root_exp_grad() turns that into the kernels' documented 0."""
    x = [torch.tensor(np.asarray(a), dtype=dtype, device=device).requires_grad_(True) for a in (root_pos, root_exp, dof)]
    rq = torch_util.exp_map_to_quat(x[1])
    jr = km.dof_to_rot_torch(x[2])
    bp, br = km.forward_kinematics_torch(x[0], rq, jr)
    outs = dict(zip(OUTS, (rq, jr, bp, br)))
    if cots is None:
        return {k: _np(v) for k, v in outs.items()}, None
    g = torch.autograd.grad([outs[k] for k in OUTS], x, [torch.tensor(np.asarray(cots[k]), dtype=dtype, device=device) for k in OUTS], allow_unused=True)
    grads = {k: (np.zeros(tuple(a.shape), _np(a).dtype) if v is None else _np(v)) for k, v, a in zip(INS, g, x)}
    return {k: _np(v) for k, v in outs.items()}, grads


def expected_root_exp_grad(g_root_exp, root_exp):
    """the float64 gradient with the documented choice at an exactly zero root map: 0 where autograd (the reference's too) says NaN.
    NaN anywhere else is an error."""
    g = np.array(g_root_exp, dtype=np.float64)
    zero = (np.asarray(root_exp) == 0.0).all(axis=-1)
    assert np.isnan(g[zero]).all() and np.isfinite(g[~zero]).all()
    g[zero] = 0.0
    return g


def pose_chain_frame_sums(km, root_pos, root_exp, dof, cots):
    """[n] float64: sum over the four outputs of cotangent * output, per frame (frames are independent: for central differences)"""
    with torch.no_grad():
        outs, _ = pose_chain(km, root_pos, root_exp, dof)
    return sum((outs[k] * np.asarray(cots[k], np.float64)).reshape(outs[k].shape[0], -1).sum(axis=1) for k in OUTS)


def quat_diff_angle(q0, q1, cot=None, dtype=torch.float64, device="cpu"):
    """torch_util.quat_diff_angle with autograd -> (angle, (g_q0, g_q1) | None); the operands broadcast"""
    a = torch.tensor(np.asarray(q0), dtype=dtype, device=device).requires_grad_(True)
    b = torch.tensor(np.asarray(q1), dtype=dtype, device=device).requires_grad_(True)
    ang = torch_util.quat_diff_angle(a, b)
    if cot is None:
        return _np(ang), None
    ga, gb = torch.autograd.grad(ang, (a, b), torch.tensor(np.asarray(cot), dtype=dtype, device=device))
    return _np(ang), (_np(ga), _np(gb))


def point_tables(counts):
    owner = np.repeat(np.arange(len(counts)), counts)
    return owner, np.concatenate([[0], np.cumsum(counts)])


def body_points_world(pos, rot, local, counts, cot=None, dtype=torch.float64, device="cpu"):
    """pos[owner] + quat_rotate(rot[owner], local) with autograd -> (world, (g_pos, g_rot) | None)"""
    owner = torch.tensor(point_tables(counts)[0], device=device)
    p = torch.tensor(np.asarray(pos), dtype=dtype, device=device).requires_grad_(True)
    r = torch.tensor(np.asarray(rot), dtype=dtype, device=device).requires_grad_(True)
    loc = torch.tensor(np.asarray(local), dtype=dtype, device=device)
    w = torch_util.quat_rotate(r[..., owner, :], loc.expand(r.shape[:-2] + loc.shape)) + p[..., owner, :]
    if cot is None:
        return _np(w), None
    gp, gr = torch.autograd.grad(w, (p, r), torch.tensor(np.asarray(cot), dtype=dtype, device=device))
    return _np(w), (_np(gp), _np(gr))


def temporal_terms(case):
    """moopt_host.TtCase.float64: (sums [3, M], g_pos [N, B, 3], g_r [N, B]) for the cotangents case.w"""
    return case.float64()


def temporal_terms_torch(case, dtype=torch.float64, device="cpu"):
    """the torch expressions of the single path (tools/motion_opt/motion_optimization.py), motion by motion, with autograd: the same
    three arrays as temporal_terms"""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    sums = np.zeros((3, case.M), npdt)
    g_pos, g_r = np.zeros(case.pos.shape, npdt), np.zeros(case.r.shape, npdt)
    for m, T in enumerate(case.lengths):
        sl = slice(int(case.ss[m]), int(case.ss[m]) + T)
        pos = torch.tensor(case.pos[sl], dtype=dtype, device=device).requires_grad_(True)
        r = torch.tensor(case.r[sl][:T - 1], dtype=dtype, device=device).requires_grad_(True)
        s_bv, keep, pc = (torch.tensor(x[sl][:T - 1], dtype=dtype, device=device) for x in (case.sv, case.keep, case.pc))
        v = pos[1:] - pos[:-1]
        e2 = torch.square(v - s_bv)
        smooth = e2.sum() + r.sum()
        slide = ((torch.sqrt((e2 * keep.unsqueeze(-1)).sum(-1) + mh.C2) - mh.C) * pc).sum() + ((torch.sqrt(r * keep + mh.C2) - mh.C) * pc).sum()
        acc = v[1:] - v[:-1]
        jerk = torch.clamp(torch.linalg.vector_norm(acc[1:] - acc[:-1], dim=-1) - case.lim, min=0.0).sum()
        out = torch.stack([smooth, slide, jerk])
        gp, gr = torch.autograd.grad(out, (pos, r), torch.tensor(case.w[:, m], dtype=dtype, device=device), allow_unused=True)
        sums[:, m] = _np(out)
        if gp is not None:
            g_pos[sl] = _np(gp)
        if gr is not None and T > 1:
            g_r[sl][:T - 1] = _np(gr)
    return sums, g_pos, g_r


# ------------------------------------------------------------------------------------------------------------------ error measures
def value_error(got, ref64):
    return float(np.abs(np.asarray(got, np.float64) - ref64).max()) if np.size(ref64) else 0.0


def grad_error(got, ref64):
    """(largest |got - ref64| relative to the frame's (pair's: the leading axis') maximum of |ref64|, the rows where ref64 is all zero):
    on those rows nothing is relative, the caller demands exact zeros"""
    got, ref64 = np.asarray(got, np.float64).reshape(len(ref64), -1), np.asarray(ref64).reshape(len(ref64), -1)
    if ref64.size == 0:
        return 0.0, np.zeros(len(ref64), bool)
    scale = np.abs(ref64).max(axis=1)
    live = scale > 0
    err = np.abs(got - ref64).max(axis=1)
    return (float((err[live] / scale[live]).max()) if live.any() else 0.0), ~live


def decade_of(s):
    """index into DECADES of float64 |v| (an array), -1 below the threshold"""
    s = np.asarray(s)
    out = np.full(s.shape, -1)
    for k, (lo, hi) in enumerate(DECADES):
        out[(s >= lo) & (s < hi)] = k
    return out


def angle_grad_by_decade(got, ref64, s):
    """[4] per decade of |v|: largest |got - ref64| relative to the pair's maximum of |ref64|"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64)
    dec = decade_of(s)
    scale = np.abs(ref64).max(axis=-1)
    err = np.abs(got - ref64).max(axis=-1)
    return np.array([float((err[dec == k] / scale[dec == k]).max()) if (dec == k).any() else 0.0 for k in range(len(DECADES))])


def _round_up(x):
    if x == 0.0:
        return 0.0
    e = math.floor(math.log10(x)) - 2
    return math.ceil(x / 10.0 ** e) * 10.0 ** e


def measure(z):
    """the e-bars of fixture G34 (an open npz): |reference fp32 - reference float64| by the measures above"""
    m = dict(pose_value={k: 0.0 for k in OUTS}, pose_grad={k: 0.0 for k in INS}, angle_grad=np.zeros(len(DECADES)), angle_value=0.0,
             points_value=0.0, points_grad={"body_pos": 0.0, "body_rot": 0.0}, tt_value=0.0, tt_grad={"g_pos": 0.0, "g_r": 0.0})
    for c in CHARS:
        for k in OUTS:
            m["pose_value"][k] = max(m["pose_value"][k], value_error(z["{}_f32_{}".format(c, k)], z["{}_f64_{}".format(c, k)]))
        for run in ("all",):                            # the runs on one output alone are recorded in float64 only
            for k in INS:
                g32, g64 = z["{}_f32_{}_g_{}".format(c, run, k)], z["{}_f64_{}_g_{}".format(c, run, k)]
                if k == "root_exp":
                    zero = (z[c + "_root_exp"] == 0.0).all(axis=-1)
                    g32, g64 = g32[~zero], g64[~zero]                   # the reference's NaN at the zero map, in both precisions
                m["pose_grad"][k] = max(m["pose_grad"][k], grad_error(g32, g64)[0])
    for tag, q0, q1 in (("ang", "ang_q0", "ang_q1"), ("angb", "angb_q0", "angb_q1")):
        s, _ = pair_difference(z[q0], z[q1])
        m["angle_value"] = max(m["angle_value"], value_error(z[tag + "_f32_angle"], z[tag + "_f64_angle"]))
        m["angle_grad"] = np.maximum(m["angle_grad"], angle_grad_by_decade(z[tag + "_f32_g_q1"], z[tag + "_f64_g_q1"], s))
        if tag == "ang":
            m["angle_grad"] = np.maximum(m["angle_grad"], angle_grad_by_decade(z[tag + "_f32_g_q0"], z[tag + "_f64_g_q0"], s))
    m["points_value"] = value_error(z["pts_f32_world"], z["pts_f64_world"])
    for k in ("body_pos", "body_rot"):
        nb = z["pts_f64_g_" + k].shape[-2]
        m["points_grad"][k] = grad_error(z["pts_f32_g_" + k].reshape(-1, nb * z["pts_f64_g_" + k].shape[-1]), z["pts_f64_g_" + k].reshape(-1, nb * z["pts_f64_g_" + k].shape[-1]))[0]
    for name in mh.DESIGNED_TT:
        m["tt_value"] = max(m["tt_value"], value_error(z["tt_{}_f32_sums".format(name)], z["tt_{}_f64_sums".format(name)]))
        for k in ("g_pos", "g_r"):
            m["tt_grad"][k] = max(m["tt_grad"][k], grad_error(z["tt_{}_f32_{}".format(name, k)], z["tt_{}_f64_{}".format(name, k)])[0])
    return m


def main():
    m = measure(np.load(FIXTURE))
    print("e-bar over G34: |reference fp32 - reference float64|")
    print("MEASURED_POSE_VALUE = %.3g" % _round_up(max(m["pose_value"].values())))
    print("MEASURED_POSE_VALUE_BY_OUTPUT = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["pose_value"].items()))
    print("MEASURED_POSE_GRAD = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["pose_grad"].items()))
    print("MEASURED_ANGLE_VALUE = %.3g" % _round_up(m["angle_value"]))
    print("MEASURED_ANGLE_GRAD_DECADE = (%s)" % ", ".join("%.3g" % _round_up(v) for v in m["angle_grad"]))
    print("MEASURED_POINTS_VALUE = %.3g" % _round_up(m["points_value"]))
    print("MEASURED_POINTS_GRAD = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["points_grad"].items()))
    print("MEASURED_TT_VALUE = %.3g" % _round_up(m["tt_value"]))
    print("MEASURED_TT_GRAD = {%s}" % ", ".join("\"%s\": %.3g" % (k, _round_up(v)) for k, v in m["tt_grad"].items()))


if __name__ == "__main__":
    main()
