"""Float64 evaluation of the simulator's joint rotations (parc_amd/csrc/parc_sim_core.h: exp_to_q, q_to_exp, qnormalize, publish_bodies /
store_lane_state, ctl_hold_torque), which on the device run on __builtin_amdgcn_sqrtf / rcpf and the hand-written p_sincos / p_atan2_q1
-- TEST INFRASTRUCTURE: numpy only, no torch, no GPU.

The yardstick of tests/test_sim_rot_gpu.py and tests/test_sim_rot_ref_cpu.py.  It states the simulator's conventions on fp32 inputs cast up:
  exp_to_q / q_to_exp      exponential map <-> quaternion (x, y, z, w); the map of a quaternion has its angle in [0, pi] after w -> |w|;
  chain                    the body chain of publish_bodies, read from the fields of a parc_sim_model_t instance (parent, joint_type,
                           dof_idx, local_translation, local_rotation, joint_axis): positions, world quaternions, linear and angular velocities;
  pd_exp_torque            clip(kp log(conj(q) q_tar) - kd qdot, +-effort), a hinge projected on its axis;
  pd_1d_torque             clip(kp (tar - q) - kd qdot, +-effort): no wrap.
Every function takes `dtype`: float64 is the yardstick, float32 the figure that body velocities' e-bar is measured with (the reference holds
no body velocities: Isaac Gym supplies them).

Also here: the four characters' scenes and the designed inputs of parts A-C, with their guards.  Every guard is asserted in float64 on
every input; a guard that fails raises, no test drops an input.  Seeded values (axes, velocities) come from the recorded SEEDS.

Run as a script it prints e-bar, the largest |reference fp32 - reference float64| over fixture G38 per output group; the MEASURED
constants are those figures rounded up to 3 digits.  They come from the reference's torch code on the CPU (tests/golden/gen_sim_rot.py) and
from this module's fp32 run, never from the kernels.
"""
import copy
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(REPO, "tests", "golden", "g38_sim_rot.npz")
PI = math.pi
F32, F64 = np.float32, np.float64
CHARS = ("hum", "chain", "arm_h", "arm_s", "syn16")
SEEDS = {"hum": 3810, "chain": 3820, "arm_h": 3830, "arm_s": 3840, "syn16": 3850}
N = 48
THRESHOLD = 1e-6                    # of exp_to_q (|e|) and of q_to_exp (|v|)
GUARD = (0.8e-6, 1.25e-6)           # no input may fall here in float64: the two precisions could disagree on the branch
REF_THRESHOLD = 1e-5                # the reference zeroes a map whose angle / vector part is at most this (util/torch_util.py:70-82,395-412)
REF_GUARD = (0.8e-5, 1.25e-5)
FAR_PI = 0.5e-3                     # of a wrapped angle from pi: inside, the two precisions may take the wrap's two sides
FAR_ANGLE = 16.0                    # raw angles beyond it are held to an e-bar of their own: one ulp of the fp32 half angle is >= 9.5e-7 there
CLIP_SIDE = 1e-3                    # the clip rows: float64 kp diff - kd w = effort (1 -+ CLIP_SIDE)
CLIP_GUARD = 1e-4                   # relative, around the clip
ROOT_FAR = np.array([1e3, -1e3, 50.0])
DEVICE_FACTOR, HOST_FACTOR = 4.0, 2.0

TINY = (0.35e-6, 0.7e-6, 1.5e-6, 3e-6, 0.0)                       # on both sides of THRESHOLD, and the zero map
NEAR = (1e-4, 1e-2, 1.0, PI / 2 - 1e-3, PI / 2 + 1e-3, PI - 1.01e-3, PI + 1.01e-3, 3 * PI / 2 - 1e-3, 3 * PI / 2 + 1e-3, 2 * PI - 1e-3,
        2 * PI + 1e-3, 5 * PI / 2 - 1e-3, 5 * PI / 2 + 1e-3)
HINGE_NEAR = NEAR + (4 * PI - 1e-3, 4 * PI + 1e-3)
FAR = (50.0, 300.0)
HINGE_FAR = FAR + (100.0, 600.0)
BAND_ROWS, FAR_ROWS = slice(0, 10), slice(10, 18)                 # rows of part A: every joint below / around THRESHOLD; every joint beyond
NEAR_ROWS = slice(18, N)                                          # FAR_ANGLE; the rest.  e-bar: NEAR_ROWS and FAR_ROWS (the reference zeroes
#                                                                   a spherical map of BAND_ROWS: DESIGN.md, "deviation band")
# relative rotations of part C (angle; negative = about the opposite axis): 0, both sides of 2 THRESHOLD and of 2 REF_THRESHOLD (|v| =
# half the angle), then the seam of p_atan2_q1 (pi / 2), the w < 0 flip (pi) and a full turn
REL_TINY = (0.0, 0.7e-6, 1.4e-6, 3e-6, 6e-6, 0.7e-5, 1.4e-5, 3e-5, 6e-5)
REL_REST = (1e-3, 1.0, PI / 2 - 1e-3, PI / 2 + 1e-3, PI - 1.01e-3, PI + 1.01e-3, -(PI - 1.01e-3), -(PI + 1.01e-3), 2 * PI - 1e-3, 2 * PI + 1e-3,
            -(2 * PI - 1e-3), -(2 * PI + 1e-3))
REL = REL_TINY + REL_REST
STATE_TINY = (0.0, 1e-2, 1.0)             # states under a tiny relative rotation: the target's fp32 rounding stays below 4e-8 of |v|
STATE_NEAR = (0.0, 1.0, 3.0, PI / 2 - 1e-3, PI - 1.01e-3)
STATE_FAR = (50.0,)
C_NEAR_ROWS, C_FAR_ROWS, C_CLIP_ROWS = slice(0, 28), slice(28, 40), slice(40, 48)

# e-bar over G38, rounded up to 3 digits: `python tests/tools/sim_rot_ref.py` prints them, test_sim_rot_ref_cpu.py holds them to the fixture
MEASURED = {
    "joint_quat": {"near": 1.79e-07, "far": 5.06e-06},
    "rt_map": {"near": 5.08e-07, "far": 1.25e-05},
    "body_pos_origin": {"near": 7.54e-07, "far": 6.91e-06},
    "body_pos_far_root": {"near": 0.000105, "far": 0.000103},
    "body_rot": {"near": 3.5e-07, "far": 5.64e-06},
    "body_lin_vel": {"near": 3.49e-06, "far": 1.81e-05},
    "body_ang_vel": {"near": 4.27e-06, "far": 3.96e-05},
    "torque_exp": {"near": 6.08e-07, "far": 4.81e-06},
    "torque_1d": {"near": 3.53e-07, "far": 2.94e-07},
}

JOINT_FIXED, JOINT_HINGE, JOINT_SPHERICAL = 3, 1, 2


# ---------------------------------------------------------------------------------------------------------------------- quaternions
def qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def qconj(q):
    return q * np.array([-1, -1, -1, 1], q.dtype)


def qunit(q):
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def qrot(q, v):
    t = 2 * np.cross(q[..., :3], v)
    return v + q[..., 3:] * t + np.cross(q[..., :3], t)


def exp_to_q(e, dtype=F64):
    e = np.asarray(e, dtype)
    a = np.sqrt((e.astype(F64) ** 2).sum(-1, keepdims=True)).astype(dtype)        # the length correctly rounded: what torch's norm gives in fp32
    safe = np.where(a > 0, a, 1)
    s = np.where(a > 0, np.sin(a / 2) / safe, dtype(0.5))
    return np.concatenate([e * s, np.cos(a / 2)], axis=-1).astype(dtype)


def q_to_exp(q, dtype=F64):
    """the map of |w|'s quaternion: its angle is in [0, pi]"""
    q = np.asarray(q, dtype)
    q = np.where(q[..., 3:] < 0, -q, q)
    l = np.sqrt((q[..., :3] ** 2).sum(-1, keepdims=True))
    k = np.where(l > 0, 2 * np.arctan2(l, q[..., 3:]) / np.where(l > 0, l, 1), dtype(2))
    return (q[..., :3] * k).astype(dtype)


def wrapped(angle):
    """a raw angle as the angle of the quaternion's map: in (-pi, pi]"""
    return angle - 2 * PI * np.ceil((angle - PI) / (2 * PI))


# ---------------------------------------------------------------------------------------------------------------------- model
def model_arrays(s, dtype=F64):
    """the fields of a parc_sim_model_t instance that the chain and the torque read, each fp32 number cast to `dtype`"""
    B, D = int(s.num_bodies), int(s.dof_size)
    f = lambda a, n, k: np.array([[a[i][j] for j in range(k)] for i in range(n)], dtype)  # noqa: E731
    v = lambda a, n: np.array([a[i] for i in range(n)], dtype)  # noqa: E731
    return dict(B=B, D=D, parent=[int(s.parent[b]) for b in range(B)], jt=[int(s.joint_type[b]) for b in range(B)],
                d0=[int(s.dof_idx[b]) for b in range(B)], lt=f(s.local_translation, B, 3), lr=f(s.local_rotation, B, 4), ax=f(s.joint_axis, B, 3),
                kp=v(s.kp, D), kd=v(s.kd, D), effort=v(s.effort, D))


def joint_quats(M, dof_pos, dtype=F64):
    """[n, D] -> [n, B, 4]: a hinge turns by its angle about the stored axis, a spherical joint by its map; the root and fixed joints: identity"""
    dof_pos = np.asarray(dof_pos, dtype)
    q = np.zeros(dof_pos.shape[:-1] + (M["B"], 4), dtype)
    q[..., 3] = 1
    for b in range(1, M["B"]):
        d0 = M["d0"][b]
        if M["jt"][b] == JOINT_SPHERICAL:
            q[..., b, :] = exp_to_q(dof_pos[..., d0:d0 + 3], dtype)
        elif M["jt"][b] == JOINT_HINGE:
            q[..., b, :] = exp_to_q(dof_pos[..., d0:d0 + 1] * M["ax"][b].astype(dtype), dtype)
    return q


def qmat(q):
    x, y, z, w = np.moveaxis(q, -1, 0)
    m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def _mv(m, v):
    return (m * v[..., None, :]).sum(-1)


def _mtv(m, v):
    return (m * v[..., :, None]).sum(-2)


def chain(M, root_state, dof_state, dtype=F64, unit_root=False):
    """publish_bodies as it is written: rigid_body_state [n, B, 13] (position, world quaternion, linear and angular velocity in the world
    frame) of the state rows.  Frames are rotation matrices chained from the root (E = qmat(local_rotation * q), R = R_parent E), the
    world quaternion is normalised at every body, velocities are carried in body coordinates and turned to the world at the end: in
    float64 this is the chain itself, in fp32 it rounds where the simulator rounds.
    unit_root: the reference's forward_kinematics instead (quat_rotate down the chain, nothing normalised, poses only), which is handed a
    unit root quaternion - what the fixture's float64 records are pinned with."""
    rs, ds = np.asarray(root_state, dtype), np.asarray(dof_state, dtype)
    n, B = rs.shape[0], M["B"]
    jq = joint_quats(M, ds[..., 0], dtype)
    out = np.zeros((n, B, 13), dtype)
    lt, lr, ax = M["lt"].astype(dtype), M["lr"].astype(dtype), M["ax"].astype(dtype)
    out[:, 0, 0:3] = rs[:, 0:3]
    if unit_root:
        out[:, 0, 3:7] = rs[:, 3:7]
        for b in range(1, B):
            Pp, Qp = out[:, M["parent"][b], 0:3], out[:, M["parent"][b], 3:7]
            out[:, b, 0:3] = Pp + qrot(Qp, np.broadcast_to(lt[b], (n, 3)))
            out[:, b, 3:7] = qmul(Qp, qmul(np.broadcast_to(lr[b], (n, 4)), jq[:, b]))
        return out
    out[:, 0, 3:7] = qunit(rs[:, 3:7])
    R, va, vl = [None] * B, [None] * B, [None] * B
    R[0] = qmat(out[:, 0, 3:7])
    vl[0], va[0] = _mtv(R[0], rs[:, 7:10]), _mtv(R[0], rs[:, 10:13])             # world -> body coordinates (load_state)
    for b in range(1, B):
        p, d0 = M["parent"][b], M["d0"][b]
        lq = qmul(np.broadcast_to(lr[b], (n, 4)), jq[:, b])
        E = qmat(lq)
        r = np.broadcast_to(lt[b], (n, 3))
        out[:, b, 3:7] = qunit(qmul(out[:, p, 3:7], lq))
        R[b] = np.matmul(R[p], E)
        out[:, b, 0:3] = out[:, p, 0:3] + _mv(R[p], r)
        wj = np.zeros((n, 3), dtype)
        if M["jt"][b] == JOINT_SPHERICAL:
            wj = ds[:, d0:d0 + 3, 1]
        elif M["jt"][b] == JOINT_HINGE:
            wj = ds[:, d0:d0 + 1, 1] * ax[b]
        va[b] = _mtv(E, va[p]) + wj
        vl[b] = _mtv(E, vl[p] + np.cross(va[p], r))
    for b in range(B):
        out[:, b, 7:10], out[:, b, 10:13] = _mv(R[b], vl[b]), _mv(R[b], va[b])
    return out


def _pd_terms(M, dof_state, tar, diff, dtype):
    ds = np.asarray(dof_state, dtype)
    kp, kd, lim = M["kp"].astype(dtype), M["kd"].astype(dtype), M["effort"].astype(dtype)
    raw = kp * diff - kd * ds[..., 1]
    return raw, np.clip(raw, -lim, lim)


def rel_maps(M, dof_pos, tar, dtype=F64):
    """[n, D]: log(conj(q) q_tar) of every joint, a hinge projected on its axis (so it wraps to (-pi, pi]); and [n, B] the length of the
    vector part of the relative quaternion (w >= 0), which the thresholds read"""
    jq, tq = joint_quats(M, dof_pos, dtype), joint_quats(M, tar, dtype)
    rel = qunit(qmul(qconj(jq), tq))
    e = q_to_exp(rel, dtype)
    diff = np.zeros(np.shape(dof_pos), dtype)
    for b in range(1, M["B"]):
        d0 = M["d0"][b]
        if M["jt"][b] == JOINT_SPHERICAL:
            diff[..., d0:d0 + 3] = e[..., b, :]
        elif M["jt"][b] == JOINT_HINGE:
            diff[..., d0] = (e[..., b, :] * M["ax"][b].astype(dtype)).sum(-1)
    return diff, np.sqrt((rel[..., :3] ** 2).sum(-1)), rel[..., 3]


def pd_exp_torque(M, dof_state, tar, dtype=F64):
    """(kp diff - kd qdot before the clip, the torque): IGCharEnv._calc_pd_exp_torque / ctl_hold_torque"""
    diff = rel_maps(M, np.asarray(dof_state, dtype)[..., 0], np.asarray(tar, dtype), dtype)[0]
    return _pd_terms(M, dof_state, tar, diff, dtype)


def pd_1d_torque(M, dof_state, tar, dtype=F64):
    ds = np.asarray(dof_state, dtype)
    return _pd_terms(M, dof_state, tar, np.asarray(tar, dtype) - ds[..., 0], dtype)


def per_dof(M, per_body):
    """[n, B] -> [n, D]: a body's figure on each of its dofs"""
    out = np.zeros(per_body.shape[:-1] + (M["D"],), per_body.dtype)
    for b in range(1, M["B"]):
        k = 3 if M["jt"][b] == JOINT_SPHERICAL else 1 if M["jt"][b] == JOINT_HINGE else 0
        out[..., M["d0"][b]:M["d0"][b] + k] = per_body[..., b:b + 1]
    return out


# ---------------------------------------------------------------------------------------------------------------------- characters
ARM_MJCF = """<mujoco model="arm">
  <default>
    <default class="body">
      <geom type="sphere"/>
      <joint type="hinge" limited="true"/>
    </default>
  </default>
  <worldbody>
    <body name="base" pos="0 0 0" childclass="body">
      <freejoint name="root"/>
      <geom name="base" type="sphere" size="0.1" density="1000"/>
      <body name="link" pos="0 0 0">
{joints}
        <geom name="link" type="capsule" fromto="0 0 0 0 0 -0.6" size="0.03" density="1000"/>
      </body>
    </body>
  </worldbody>
</mujoco>
"""


def arm_mjcf(joint):
    """the kinematics of test_control_modes.make_arm as MJCF, for the reference's KinCharModel (the simulator's arm is built from the struct)"""
    axes = ("0 1 0",) if joint == 1 else ("1 0 0", "0 1 0", "0 0 1")
    return ARM_MJCF.format(joints="\n".join("        <joint name=\"j{}\" type=\"hinge\" axis=\"{}\" range=\"-180 180\"/>".format(k, a)
                                            for k, a in enumerate(axes)))


def syn16_mjcf():
    """pose_opt_ref.synthetic_mjcf with every hinge on the coordinate axis nearest to its oblique one: the simulator turns a hinge about the
    STORED axis (exp_to_q(angle * axis)), the reference about the normalised one, so only unit axes mean the same in both, and no oblique
    fp32 axis is exactly unit.  The local rotations, which that text gives to six digits (up to 1.3e-4 from unit), are written unit to nine:
    the reference's forward_kinematics chains them as they are, the simulator needs unit ones (SimModel normalises what is further than 1e-6
    from unit).  Oblique local rotations, the fixed joints inside the chains and the 16 bodies stay."""
    import pose_opt_ref as por

    def unit(m):
        v = [float(t) for t in m.group(1).split()]
        k = int(np.argmax(np.abs(v)))
        return "axis=\"{}\"".format(" ".join("-1" if (i == k and v[k] < 0) else "1" if i == k else "0" for i in range(3)))
    def unit_quat(m):
        q = np.array([float(t) for t in m.group(1).split()])
        return "quat=\"{}\"".format(" ".join("%.9f" % v for v in q / np.linalg.norm(q)))
    return re.sub(r"quat=\"([^\"]+)\"", unit_quat, re.sub(r"axis=\"([^\"]+)\"", unit, por.synthetic_mjcf()))


def mjcf_text(name):
    if name == "chain":
        return str(np.load(os.path.join(REPO, "tests", "golden", "g27_control_modes.npz"))["hinge_mjcf"])
    return {"arm_h": lambda: arm_mjcf(1), "arm_s": lambda: arm_mjcf(2), "syn16": syn16_mjcf}[name]()


_structs = {}


def _base_struct(name):
    """the character's parc_sim_model_t as SimModel (or make_arm) builds it"""
    if name not in _structs:
        import tempfile
        import sim_ctl
        from parc_amd.anim.kin_char_model import KinCharModel
        from parc_amd.sim_model import SimModel
        if name in ("hum", "arm_h", "arm_s"):
            s = sim_ctl.humanoid_struct()[1].struct
            if name != "hum":
                import test_control_modes as cm
                s = cm.make_arm(s, "core", None, 1 if name == "arm_h" else 2).m
        else:
            km = KinCharModel("cpu")
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, name + ".xml")
                with open(path, "w") as f:
                    f.write(mjcf_text(name))
                km.load_char_file(path)
            s = SimModel(km).struct
        _structs[name] = s
    return copy.deepcopy(_structs[name])


def scene_struct(name, clip=False):
    """The character in a designed scene: gravity 0, angular damping 0, no link-link contact (self_mask 0, capsule radii 0), joint limits at
    -+1e9.  The humanoid and the hinge chain keep their gains; the arms and the 16-body tree, which have none, get kp 40 / 300, kd 3 / 30.
    clip=False: every motor gear that is not 0 is raised to 1e6, so that no designed torque is clipped; clip=True: the character's own gears
    (arms 50, tree 120)."""
    s = _base_struct(name)
    s.gravity, s.angular_damping = 0.0, 0.0
    for b in range(16):
        s.self_mask[b], s.cap_radius[b] = 0, 0.0
    own = {"arm_h": (40.0, 3.0, 50.0), "arm_s": (40.0, 3.0, 50.0), "syn16": (300.0, 30.0, 120.0)}.get(name)
    for d in range(int(s.dof_size)):
        s.limit_lo[d], s.limit_hi[d] = -1e9, 1e9
        if own:
            s.kp[d], s.kd[d], s.effort[d] = own
        if not clip and s.effort[d] != 0.0:
            s.effort[d] = 1e6
    return s


# ---------------------------------------------------------------------------------------------------------------------- designed inputs
def _axes(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


HEADINGS = (0.0, PI / 2 - 1e-3, PI + 1e-3, -2.0)
SCALES = (1.0, -1.0, 0.5, 2.0)


def base_root_quats():
    """identity, (0, 0, 1, 0), and the designed headings at pitch 0.7 and at roll 0.5: 10 unit quaternions (float64)"""
    out = [np.array([0.0, 0, 0, 1]), np.array([0.0, 0, 1, 0])]
    for tilt in (np.array([0, 0.7, 0.0]), np.array([0.5, 0, 0.0])):
        for h in HEADINGS:
            out.append(qmul(exp_to_q(np.array([0, 0, h])), exp_to_q(tilt)))
    return np.stack(out)


def root_quats(n=N):
    """row i: base quaternion i % 10 times SCALES[(i // 10) % 4]: q, -q, 0.5 q, 2 q are one rotation"""
    base = base_root_quats()
    return np.stack([base[i % 10] * SCALES[(i // 10) % 4] for i in range(n)]).astype(F32)


def inputs_a(name, far_root=False):
    """(root_state [N, 13], dof_state [N, D, 2]) of part A, fp32.  Spherical joints: the designed angles on seeded axes; hinges: plus and
    minus the designed angles.  Rows BAND_ROWS hold TINY, FAR_ROWS the angles beyond FAR_ANGLE, NEAR_ROWS the rest, shifted by one from
    joint to joint; odd rows carry seeded root and joint velocities, even rows none."""
    M = model_arrays(scene_struct(name))
    rng = np.random.default_rng(SEEDS[name])
    ds = np.zeros((N, M["D"], 2))
    rs = np.zeros((N, 13))
    rs[:, 3:7] = root_quats()
    rs[:, 0:3] = ROOT_FAR if far_root else 0.0
    ax = _axes(rng, (N, M["B"]))
    for i in range(N):
        for b in range(1, M["B"]):
            d0 = M["d0"][b]
            if i < BAND_ROWS.stop:
                a, sign = TINY[(i + b) % 5], 1.0 if i < 5 else -1.0
            elif i < FAR_ROWS.stop:
                far = HINGE_FAR if M["jt"][b] == JOINT_HINGE else FAR
                k = (i + b) % (2 * len(far))
                a, sign = far[k % len(far)], 1.0 if k < len(far) else -1.0
            else:
                near = HINGE_NEAR if M["jt"][b] == JOINT_HINGE else NEAR
                k = (i + b) % (2 * len(near))
                a, sign = near[k % len(near)], 1.0 if k < len(near) else -1.0
            if M["jt"][b] == JOINT_SPHERICAL:
                ds[i, d0:d0 + 3, 0] = a * ax[i, b] * sign + 0.0          # (+ 0.0: no -0, whose sign bit an added +0 velocity step clears)
            elif M["jt"][b] == JOINT_HINGE:
                ds[i, d0, 0] = a * sign + 0.0
    vel = rng.standard_normal((N, M["D"])) * 2.0
    rvel = rng.standard_normal((N, 6))
    ds[1::2, :, 1] = vel[1::2]
    rs[1::2, 7:13] = rvel[1::2]
    return rs.astype(F32), ds.astype(F32)


def raw_angles(M, dof_pos):
    """[n, B]: the raw angle of every joint's dofs (0 for the root and fixed joints), float64"""
    p = np.asarray(dof_pos, F64)
    out = np.zeros(p.shape[:-1] + (M["B"],))
    for b in range(1, M["B"]):
        d0 = M["d0"][b]
        if M["jt"][b] == JOINT_SPHERICAL:
            out[..., b] = np.linalg.norm(p[..., d0:d0 + 3], axis=-1)
        elif M["jt"][b] == JOINT_HINGE:
            out[..., b] = np.abs(p[..., d0]) * np.linalg.norm(M["ax"][b])
    return out


def _outside(x, band):
    return (x < band[0]) | (x > band[1])


def guards_a(name, dof_state):
    """asserts the guards of part A on fp32 inputs (in float64) and returns the distances met"""
    M = model_arrays(scene_struct(name))
    a = raw_angles(M, dof_state[..., 0])
    dofs = np.array([M["jt"][b] in (JOINT_HINGE, JOINT_SPHERICAL) for b in range(M["B"])])
    a = a[:, dofs]
    assert _outside(a, GUARD).all(), (name, a[~_outside(a, GUARD)])
    w = np.abs(wrapped(a))
    assert (np.abs(w - PI) >= FAR_PI).all(), name
    assert (a[BAND_ROWS] <= 3.1e-6).all() and (a[FAR_ROWS] > FAR_ANGLE).all() and (a[NEAR_ROWS] <= FAR_ANGLE).all() and (a[NEAR_ROWS] >= 0.9e-4).all()
    below, above = a[(a > 0) & (a < THRESHOLD)], a[a > THRESHOLD]
    return {"below_threshold": int(below.size), "closest_below": float(below.max()), "closest_above": float(above.min()),
            "closest_to_pi": float(np.abs(w - PI).min()), "zero_maps": int((a == 0).sum()), "largest": float(a.max())}


def inputs_c(name, clip=False):
    """(dof_state [N, D, 2], target [N, D]) of part C, fp32; root: inputs_a's row quaternions at (0, 0, 5), no root velocity.  Row i, joint b: the
    relative rotation REL[(i + b) % 21] on the state angle STATE_*[(i + 2 b) % ..] (rows C_FAR_ROWS: a state beyond FAR_ANGLE under REL_REST).
    Spherical: state and relative rotation on two seeded axes, target = log(q exp(rel)); hinge: target = state + rel.  Rows C_CLIP_ROWS: the
    zero state and a target such that float64 kp diff - kd w is +-effort (1 -+ CLIP_SIDE) on every dof with a gear (meant for
    scene_struct(name, clip=True); with the gears raised they are plain rows).  Odd rows carry seeded joint velocities."""
    M = model_arrays(scene_struct(name, clip=True))
    rng = np.random.default_rng(SEEDS[name] + 1)
    ds, tar = np.zeros((N, M["D"], 2)), np.zeros((N, M["D"]))
    ax, ux = _axes(rng, (N, M["B"])), _axes(rng, (N, M["B"]))
    vel = rng.standard_normal((N, M["D"])) * 2.0
    ds[1::2, :, 1] = vel[1::2]
    ds = ds.astype(F32).astype(F64)
    for i in range(N):
        for b in range(1, M["B"]):
            d0, jt = M["d0"][b], M["jt"][b]
            if jt not in (JOINT_HINGE, JOINT_SPHERICAL):
                continue
            k = 3 if jt == JOINT_SPHERICAL else 1
            if i >= C_CLIP_ROWS.start:
                j = i - C_CLIP_ROWS.start
                sign, side = (1.0 if j & 1 else -1.0), (1.0 - CLIP_SIDE if j & 2 else 1.0 + CLIP_SIDE)
                sl = slice(d0, d0 + k)
                lim, kp, kd = M["effort"][sl], M["kp"][sl], M["kd"][sl]
                d = np.where(lim > 0, (sign * side * lim + kd * ds[i, sl, 1]) / np.where(kp > 0, kp, 1), 0.3 * sign)
                assert np.linalg.norm(d) < PI - 0.1, (name, b, d)
                tar[i, sl] = d
                continue
            if i < C_NEAR_ROWS.stop:
                rel = REL[(i + b) % len(REL)]
                states = STATE_TINY if abs(rel) < 1e-4 else STATE_NEAR
            else:
                rel, states = REL_REST[(i + b) % len(REL_REST)], STATE_FAR
            st = states[(i + 2 * b) % len(states)]
            if jt == JOINT_HINGE:
                ds[i, d0, 0] = F32(st)
                tar[i, d0] = float(F32(st)) + rel
            else:
                e = (st * ax[i, b]).astype(F32).astype(F64)
                ds[i, d0:d0 + 3, 0] = e
                tar[i, d0:d0 + 3] = q_to_exp(qmul(exp_to_q(e), exp_to_q(rel * ux[i, b])))
    return ds.astype(F32), tar.astype(F32)


def root_c(name):
    rs = np.zeros((N, 13), F32)
    rs[:, 3:7] = root_quats()
    rs[:, 2] = 5.0
    return rs


def masks_c(name, dof_state, tar):
    """per dof [N, D], float64 on the fp32 inputs: `band` = the reference zeroes the relative map (|v| <= REF_THRESHOLD, or a spherical
    target / state map that small); `far` = a state or target beyond FAR_ANGLE; `geared` = the dof has a motor gear"""
    M = model_arrays(scene_struct(name, clip=True))
    _, v, _ = rel_maps(M, dof_state[..., 0], tar)
    sph = np.array([M["jt"][b] == JOINT_SPHERICAL for b in range(M["B"])])
    a_s, a_t = raw_angles(M, dof_state[..., 0]), raw_angles(M, tar)
    small = sph & (((a_s > 0) & (a_s <= REF_GUARD[1])) | ((a_t > 0) & (a_t <= REF_GUARD[1])))
    band = per_dof(M, (v <= REF_THRESHOLD) | small)
    far = per_dof(M, (a_s > FAR_ANGLE) | (a_t > FAR_ANGLE))
    return band, far, np.broadcast_to(M["effort"] != 0, band.shape)


def guards_c(name, dof_state, tar):
    """asserts the guards of part C (in float64, on the fp32 inputs) and returns the distances met"""
    M = model_arrays(scene_struct(name, clip=True))
    diff, v, w = rel_maps(M, dof_state[..., 0], tar)
    dofs = np.array([M["jt"][b] in (JOINT_HINGE, JOINT_SPHERICAL) for b in range(M["B"])])
    v, w = v[:, dofs], w[:, dofs]
    assert _outside(v, GUARD).all() and _outside(v, REF_GUARD).all(), (name, v[~(_outside(v, GUARD) & _outside(v, REF_GUARD))])
    ang = 2 * np.arctan2(v, np.abs(w))
    assert (PI - ang >= FAR_PI).all(), (name, (PI - ang).min())
    raw, _ = pd_exp_torque(M, dof_state, tar)
    lim = M["effort"]
    geared = lim != 0
    ratio = np.abs(raw[C_CLIP_ROWS][:, geared]) / lim[geared]
    assert (np.abs(ratio - 1) >= CLIP_GUARD).all() and (np.abs(ratio - 1) <= 2 * CLIP_SIDE).all(), (name, ratio)
    assert (ratio > 1).any() and (ratio < 1).any()
    return {"below_threshold": int(((v > 0) & (v < THRESHOLD)).sum()), "closest_below": float(v[(v > 0) & (v < THRESHOLD)].max()),
            "closest_above": float(v[v > THRESHOLD].min()), "in_reference_band": int((v <= REF_THRESHOLD).sum()),
            "closest_to_reference_threshold": [float(v[v <= REF_THRESHOLD].max()), float(v[v > REF_THRESHOLD].min())],
            "closest_to_pi": float((PI - ang).min()), "closest_to_clip": float(np.abs(ratio - 1).min())}


# ---------------------------------------------------------------------------------------------------------------------- errors, e-bars
def value_error(got, ref64):
    return float(np.abs(np.asarray(got, F64) - ref64).max()) if np.size(ref64) else 0.0


def signless(got, ref64):
    """`got` with every quaternion given the sign of its float64 partner (q and -q are one rotation)"""
    got = np.asarray(got, F64)
    return got * np.where((got * ref64).sum(-1, keepdims=True) < 0, -1.0, 1.0)


GROUPS = ("joint_quat", "rt_map", "body_pos_origin", "body_pos_far_root", "body_rot", "body_lin_vel", "body_ang_vel", "torque_exp", "torque_1d")


def _round_up(x):
    if x == 0:
        return 0.0
    e = math.floor(math.log10(x)) - 2
    return float("%.3g" % (math.ceil(x / 10 ** e) * 10 ** e))


def measure(z):
    """the e-bars of fixture G38 (an open npz): the largest |fp32 - float64| per group over the characters, {group: {"near", "far"}}"""
    m = {g: {"near": 0.0, "far": 0.0} for g in GROUPS}

    def up(g, where, a, b):
        m[g][where] = max(m[g][where], value_error(a, b))
    for c in CHARS:
        s = scene_struct(c)
        vel = [chain(model_arrays(s, dt), z[c + "_a_root"], z[c + "_a_dof"], dt) for dt in (F32, F64)]
        assert vel[0].dtype == F32
        for where, rows in (("near", NEAR_ROWS), ("far", FAR_ROWS)):
            up("joint_quat", where, z[c + "_f32_joint_quat"][rows], z[c + "_f64_joint_quat"][rows])
            up("rt_map", where, z[c + "_f32_rt_map"][rows], z[c + "_f64_rt_map"][rows])
            for g in ("body_pos_origin", "body_pos_far_root", "body_rot"):
                up(g, where, z["{}_f32_{}".format(c, g)][rows], z["{}_f64_{}".format(c, g)][rows])
            up("body_lin_vel", where, vel[0][rows, :, 7:10], vel[1][rows, :, 7:10])
            up("body_ang_vel", where, vel[0][rows, :, 10:13], vel[1][rows, :, 10:13])
        band, far, geared = masks_c(c, z[c + "_c_dof"], z[c + "_c_tar"])
        for g in ("torque_exp", "torque_1d"):
            if c + "_f32_" + g not in z:
                continue
            kp = np.array([scene_struct(c).kp[d] for d in range(band.shape[1])], F64)
            keep = ~band & geared & (kp > 0)
            keep[C_CLIP_ROWS] = False
            a, b = z["{}_f32_{}".format(c, g)] / np.where(kp > 0, kp, 1), z["{}_f64_{}".format(c, g)] / np.where(kp > 0, kp, 1)
            up(g, "near", a[keep & ~far], b[keep & ~far])
            up(g, "far", a[keep & far], b[keep & far])
    return m


def bound(group, where, factor):
    return factor * MEASURED[group][where]


def main():
    m = measure(np.load(FIXTURE))
    print("e-bar over G38: |reference fp32 - reference float64| (body velocities: this module's fp32 - float64)")
    print("MEASURED = {")
    for g in GROUPS:
        print("    \"%s\": {\"near\": %.3g, \"far\": %.3g}," % (g, _round_up(m[g]["near"]), _round_up(m[g]["far"])))
    print("}")


if __name__ == "__main__":
    main()
