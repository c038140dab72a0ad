"""The tracker's kinematics kernels (parc_amd/csrc/parc_motion.hip and the fused post-step of parc_kin.hip) through their public entry
points, at the branch points of the FAST math layer they are built on (parc_math.h, parc_math_pk.h, parc_pose_lane.h): fsincos,
fatan2_q1, facos01, sin_0_halfpi, normalize_angle, the FMA-grouped quat_mul, exp_map_to_quat, quat_to_axis_angle, slerp with its two
overrides, calc_heading_quat_inv_alg with its two half-angle branches.

Inputs: the designed ones of fixture G37 (tests/golden/gen_kin_branch.py, tests/tools/kin_ref.py), every branch point on both sides,
a float64 guard asserted on each, none left out.  Yardstick: the float64 record of G37 (the reference's own classes) and, where the
device's stored rows are the input, kin_ref's float64 functions (pinned by tests/test_kin_ref_cpu.py).  Bounds: e-bar is
|reference fp32 - reference float64| on the CPU over G37 (kin_ref.MEASURED_*), per output or bucket; the kernels get DEVICE_FACTOR = 4
e-bar.  Values are compared absolutely; quaternions also carry the sign rule dot(got, float64) > 0.99.  Every test prints err / bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from test_hip_parity import DEV, T, close, _core_from_golden, km, mlib  # noqa: F401  (km, mlib: the fixtures of the G6 state)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import kin_ref as kr  # noqa: E402
import pose_opt_ref as por  # noqa: E402

pytestmark = pytest.mark.gpu
K = kr.DEVICE_FACTOR
SIZES = (1, 15, 16, 17, 64)         # a 256-thread block holds 16 poses: a lone pose, an empty tail, a full block, one pose in a second block
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0], np.float32)


@pytest.fixture(scope="module")
def z():
    return golden("g37_kin_branch")


@pytest.fixture(scope="module")
def chars():
    return {c: kr.load_char(c, DEV) for c in kr.CHARS}


@pytest.fixture(scope="module")
def libs(chars):
    """name -> the designed clip library on the device"""
    from parc_amd.anim.motion_lib import MotionLib
    z = golden("g37_kin_branch")
    out = {}
    for c in kr.CHARS:
        B = chars[c].get_num_joints()
        clips = [dict(frames=z["{}_{}_frames".format(c, name)], contacts=np.zeros((z["{}_{}_frames".format(c, name)].shape[0], B), np.float32),
                      fps=kr.CLIP_FPS[i], loop=kr.CLIP_LOOP[i], weight=1.0, name=name) for i, name in enumerate(kr.CLIP_NAMES)]
        out[c] = MotionLib(clips, chars[c], DEV, init_type="clips", contact_info=True)
    return out


def _np(x):
    return x.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(got, ref64, ebar, what, factor=K):
    err = kr.value_error(got, ref64)
    print("{:52s} err {:.3e}  bound {:.3e} ({:g} e-bar)  err / bound {:.3f}".format(what, err, factor * ebar, factor, err / (factor * ebar)))
    assert np.shape(got) == np.shape(ref64) and err <= factor * ebar, (what, err, factor * ebar)


def _sign_rule(got, ref64, what):
    dot = (np.asarray(got, np.float64) * ref64).sum(-1)
    assert (dot > 0.99).all(), (what, float(dot.min()))


# ------------------------------------------------------------------------------------------------------------------ dofs -> rotations
@pytest.mark.parametrize("c", kr.CHARS)
def test_dof_to_rot_at_its_branch_points(z, chars, c):
    km_ = chars[c]
    dof, ref = z[c + "_dof"], z[c + "_f64_joint_rot"]
    assert kr.sph_conditions(kr.sph_maps(km_, dof)) == []
    outs = {n: _np(km_.dof_to_rot(T(dof[:n]))) for n in SIZES}
    got = outs[64]
    far = kr.far_joints(km_, dof)
    err = np.abs(got.astype(np.float64) - ref).max(axis=-1)
    for bucket, rows in (("near", ~far), ("far", far)):
        bound = K * kr.MEASURED_DOF_TO_ROT[bucket]
        print("{:52s} err {:.3e}  bound {:.3e} ({:g} e-bar)  err / bound {:.3f}".format("{} joint_rot {}".format(c, bucket), err[rows].max(), bound, K, err[rows].max() / bound))
        assert err[rows].max() <= bound, (c, bucket, err[rows].max(), bound)
    _sign_rule(got, ref, c)
    # below the threshold and at the zero map: the bits of the identity; above it: not the identity
    sph = [j - 1 for j in por.spherical_joints(km_)]
    w = por.wrapped(kr._raw_angles(km_, dof)[:, sph])
    below = w < kr.THRESHOLD
    assert below[[0, len(kr.ANGLES), kr.DOF_ZERO_ROW]].all() and below.sum() == 3 * len(sph)
    assert np.array_equal(_bits(got[:, sph][below]), np.broadcast_to(_bits(IDENTITY), (below.sum(), 4)))
    assert (np.abs(got[:, sph][~below][:, :3]).max(axis=1) > 5e-6).all()
    hin = [j - 1 for j in por.hinge_joints(km_)]
    # the zero hinge: the identity.  Its vector part is axis * sin(0): a zero that carries the sign of the axis component, in the reference
    # (whose fp32 record holds the same -0) as on the device; the bits of the identity hold for the magnitudes, and for w as it stands
    zero_hinge = got[kr.DOF_ZERO_ROW][hin]
    assert np.array_equal(_bits(np.abs(zero_hinge)), np.broadcast_to(_bits(IDENTITY), (len(hin), 4))) and (_bits(zero_hinge[:, 3]) == _bits(IDENTITY)[3]).all()
    assert np.array_equal(np.abs(z[c + "_f32_joint_rot"][kr.DOF_ZERO_ROW][hin]), np.broadcast_to(IDENTITY, (len(hin), 4)))
    fixed = [j - 1 for j in range(1, km_.get_num_joints()) if km_.get_joint_dof_dim(j) == 0]
    assert np.array_equal(_bits(got[:, fixed]), np.broadcast_to(_bits(IDENTITY), (64, len(fixed), 4)))
    # a pose's result depends neither on the batch size nor on its place in the block
    for n in SIZES:
        assert outs[n].shape == (n,) + got.shape[1:] and np.array_equal(_bits(outs[n]), _bits(got[:n])), n


# ------------------------------------------------------------------------------------------------------------------ rotations -> dofs
@pytest.mark.parametrize("c", kr.CHARS)
def test_rot_to_dof_at_its_branch_points(z, chars, c):
    km_ = chars[c]
    jrot, table, ref = z[c + "_jrot"], z[c + "_jrot_table"], z[c + "_f64_dof_back"]
    assert kr.joint_rot_conditions(km_, jrot) == []
    got = _np(km_.rot_to_dof(T(jrot)))
    _check(got, ref, kr.MEASURED_ROT_TO_DOF, c + " dof")
    designed = ~np.isnan(table[:, 0])
    owner = np.full(km_.get_dof_size(), -1)
    for j in range(1, km_.get_num_joints()):
        owner[km_.get_joint_dof_idx(j):km_.get_joint_dof_idx(j) + km_.get_joint_dof_dim(j)] = j - 1
    assert (owner >= 0).all()                               # every slot has a joint; the fixed joints own none and their quaternions are random
    v = np.linalg.norm(jrot[..., :3].astype(np.float64), axis=-1)[:, owner]           # [n, D]: unnormalised |v| of the slot's joint
    w = jrot[..., 3][:, owner]
    # below the threshold exactly 0, above it not (a hinge's angle, and the largest entry of a spherical joint's map)
    assert (got[v < kr.THRESHOLD] == 0.0).all()
    for j in range(1, km_.get_num_joints()):
        d, k = km_.get_joint_dof_idx(j), km_.get_joint_dof_dim(j)
        if k:
            live = v[:, d] > kr.THRESHOLD
            assert (np.abs(got[live, d:d + k]).max(axis=1) > 0).all(), j
    # q and -q are one rotation: equal bits (w = 0 excepted, where neither precision prefers a representative: quat_pos keeps both)
    plus = np.nonzero(designed & (table[:, 2] > 0))[0]
    assert (table[plus + 1, 2] < 0).all() and np.array_equal(jrot[plus + 1][:, :], -jrot[plus])
    same = (w[plus] != 0.0)
    assert same.sum() > 0.8 * same.size and np.array_equal(_bits(got[plus])[same], _bits(got[plus + 1])[same])
    # q and its scaled copies: equal bits wherever float64 puts both on the same side of the threshold (it is on the unnormalised |v|)
    compared = crossed = 0
    for r in np.nonzero(designed & (table[:, 1] == 1.0))[0]:
        for r2 in np.nonzero(designed & (table[:, 3] == table[r, 3]) & (table[:, 2] == table[r, 2]) & (table[:, 1] != 1.0))[0]:
            assert np.array_equal(jrot[r2], np.float32(table[r2, 1]) * jrot[r])
            side = (v[r] > kr.THRESHOLD) == (v[r2] > kr.THRESHOLD)
            assert np.array_equal(_bits(got[r])[side], _bits(got[r2])[side]), (r, r2)
            compared += int(side.sum())
            crossed += int((~side).sum())
    assert compared >= 36 * km_.get_dof_size() and crossed >= km_.get_dof_size()          # 0.7e-5 doubled crosses the threshold on every joint
    # the hinge sign follows float64 on every designed row
    for j in por.hinge_joints(km_):
        d = km_.get_joint_dof_idx(j)
        rows = designed & (ref[:, d] != 0.0)
        assert rows.sum() >= 30 and (np.sign(got[rows, d]) == np.sign(ref[rows, d])).all(), j
        assert (ref[rows, d] < 0).sum() >= 8 and (ref[rows, d] > 0).sum() >= 8
    # the launcher clears the whole row before the kernel writes what joints own
    from parc_amd import _hip
    out = torch.full((64, km_.get_dof_size()), -7.0, device=DEV)
    _hip.check(_hip.lib().parc_rot_to_dof(_hip.stream(), km_.c_struct(), 64, _hip.ptr(T(jrot)), _hip.ptr(out)), "parc_rot_to_dof")
    assert np.array_equal(_bits(_np(out)), _bits(got))


# ------------------------------------------------------------------------------------------------------------------ forward kinematics
@pytest.mark.parametrize("where", ["origin", "far"])
@pytest.mark.parametrize("c", kr.CHARS)
def test_forward_kinematics_on_both_trees(z, chars, c, where):
    km_ = chars[c]
    rr, jr = z[c + "_fk_root_rot"], z[c + "_fk_joint_rot"]
    rp = kr.fk_root_pos(64, where)
    outs = {n: tuple(_np(x) for x in km_.forward_kinematics(T(rp[:n]), T(rr[:n]), T(jr[:n]))) for n in SIZES}
    bp, br = outs[64]
    _check(bp, z["{}_f64_{}_body_pos".format(c, where)], kr.MEASURED_FK[where]["body_pos"], "{} body_pos, root at {}".format(c, where))
    _check(br, z[c + "_f64_origin_body_rot"], kr.MEASURED_FK[where]["body_rot"], "{} body_rot, root at {}".format(c, where))
    _sign_rule(br, z[c + "_f64_origin_body_rot"], c)
    assert np.array_equal(_bits(bp[:, 0]), _bits(rp)) and np.array_equal(_bits(br[:, 0]), _bits(rr))          # the root passes through
    for n in SIZES:
        assert np.array_equal(_bits(outs[n][0]), _bits(bp[:n])) and np.array_equal(_bits(outs[n][1]), _bits(br[:n])), n


# ------------------------------------------------------------------------------------------------------------------ clip database build
def _stored(lib, c, z):
    """the device's rows per clip: list of dicts of kin_ref.BUILD_KEYS"""
    nf = [z["{}_{}_frames".format(c, name)].shape[0] for name in kr.CLIP_NAMES]
    start = np.concatenate([[0], np.cumsum(nf)])
    cols = dict(root_pos=lib._frame_root_pos, root_rot=lib._frame_root_rot, joint_rot=lib._frame_joint_rot, root_vel=lib._frame_root_vel,
                root_ang_vel=lib._frame_root_ang_vel, dof_vel=lib._frame_dof_vel)
    cols = {k: _np(v) for k, v in cols.items()}
    return [{k: v[start[i]:start[i + 1]] for k, v in cols.items()} for i in range(len(nf))]


@pytest.mark.parametrize("c", kr.CHARS)
def test_motion_lib_build_at_its_branch_points(z, chars, libs, c):
    km_, rows = chars[c], _stored(libs[c], c, z)
    sj, hj = kr.designed_joints(km_)
    ds, dh = km_.get_joint_dof_idx(sj), km_.get_joint_dof_idx(hj)
    for i, name in enumerate(kr.CLIP_NAMES):
        r, fps = rows[i], int(kr.CLIP_FPS[i])
        fr = z["{}_{}_frames".format(c, name)]
        assert kr.clip_conditions(km_, fr) == []
        assert np.array_equal(_bits(r["root_pos"]), _bits(fr[:, 0:3]))
        for k in ("root_rot", "joint_rot"):
            _check(r[k], z["{}_{}_f64_{}".format(c, name, k)], kr.MEASURED_BUILD_ROWS[k], "{} {} {}".format(c, name, k))
            _sign_rule(r[k], z["{}_{}_f64_{}".format(c, name, k)], name)
        assert (r["joint_rot"][..., 3] >= 0).all()                   # stored with w >= 0
        for k in ("root_vel", "root_ang_vel", "dof_vel"):
            _check(r[k], z["{}_{}_f64_{}".format(c, name, k)], kr.MEASURED_BUILD_VEL[fps][k], "{} {} {} ({} fps)".format(c, name, k, fps))
        if fr.shape[0] >= 2:                                         # the last frame repeats the previous difference, bit for bit
            assert all(np.array_equal(_bits(r[k][-1]), _bits(r[k][-2])) for k in ("root_vel", "root_ang_vel", "dof_vel")), name
    single = rows[0]
    assert all((single[k] == 0.0).all() for k in ("root_vel", "root_ang_vel", "dof_vel"))
    for i in (2, 3):                                                 # ladder: frames 0 and 1 are identical on the root and the designed joints
        r = rows[i]
        assert (r["root_ang_vel"][0] == 0.0).all() and (r["dof_vel"][0, ds:ds + 3] == 0.0).all() and r["dof_vel"][0, dh] == 0.0
        assert all(np.abs(r["root_ang_vel"][k]).max() > 0 and np.abs(r["dof_vel"][k, ds:ds + 3]).max() > 0 and r["dof_vel"][k, dh] != 0.0 for k in range(1, 8))
    for i in (4, 5):                                                 # edges
        r, fps = rows[i], kr.CLIP_FPS[i]
        # 1 -> 2: the root's map crosses pi.  Its angular velocity is the small rotation 2e-2 fps, not 2 pi fps; the joints' difference
        # has |v| = 0.5e-5: exactly zero
        speed = np.linalg.norm(r["root_ang_vel"][1].astype(np.float64))
        print("{} {} root angular speed across pi {:.6f} (2e-2 fps = {:.6f}, 2 pi fps = {:.1f})".format(c, kr.CLIP_NAMES[i], speed, 2e-2 * fps, 2 * kr.PI * fps))
        assert abs(speed - 2e-2 * fps) <= 1e-2 * fps                  # (the value itself is held to float64 above)
        assert (r["dof_vel"][1, ds:ds + 3] == 0.0).all() and r["dof_vel"][1, dh] == 0.0
        # 2 -> 3: |v| = 2e-5 on the root and both joints: not zero.  3 -> 4: the root by |v| = 0.5e-5, the joints identical: all zero
        assert np.abs(r["root_ang_vel"][2]).max() > 0 and np.abs(r["dof_vel"][2, ds:ds + 3]).max() > 0 and r["dof_vel"][2, dh] != 0.0
        assert (r["root_ang_vel"][3] == 0.0).all() and (r["dof_vel"][3] == 0.0).all()


# ------------------------------------------------------------------------------------------------------------------ frame query
def _blend_reference(z, c, rows, sel=slice(None)):
    """the float64 blend (at the float64 blend weight of the fp32 query time) on the device's stored fp32 rows -> (rot [Q, 1 + J, 4], root_pos [Q, 3], sine [Q, 1 + J], rot0, dict of row i0's velocities)"""
    ids, i0, i1 = z[c + "_q_ids"][sel], z[c + "_q_i0"][sel], z[c + "_q_i1"][sel]
    rot = [np.concatenate([r["root_rot"][:, None], r["joint_rot"]], axis=1) for r in rows]
    for r in rot:
        assert kr.rows_conditions(r) == []                           # the guards hold on what the device stored
    rot0, rot1 = np.stack([rot[m][a] for m, a in zip(ids, i0)]), np.stack([rot[m][a] for m, a in zip(ids, i1)])
    pos0, pos1 = np.stack([rows[m]["root_pos"][a] for m, a in zip(ids, i0)]), np.stack([rows[m]["root_pos"][a] for m, a in zip(ids, i1)])
    fr = [z["{}_{}_frames".format(c, name)] for name in kr.CLIP_NAMES]
    delta = np.stack([(fr[m][-1, 0:3] - fr[m][0, 0:3]) * np.array([1, 1, 0], np.float32) for m in ids]).astype(np.float32)
    q, p = kr.frame_blend(rot0, rot1, pos0, pos1, z[c + "_q_blend64"][sel], z[c + "_q_loop_phase"][sel], delta)
    _, sine, cosine = kr.pair_measures(rot0, rot1)
    vel = {k: np.stack([rows[m][k][a] for m, a in zip(ids, i0)]) for k in ("root_vel", "root_ang_vel", "dof_vel")}
    return q, p, sine, cosine, rot0, rot1, vel


def _check_blend(got_rot, got_pos, ref, what, min_one=1):
    q, p, sine, cosine, rot0, rot1, _ = ref
    # the exact branch: where the fp32 cosine (four rounded products, summed left to right) is >= 1 slerp returns the bits of q0.  Pairs
    # that are NOT identical are what tells this override from the average (0.5 q0 + 0.5 q0 is q0 as well): the 2e-4 rungs and the
    # 0.5e-5 / 2e-5 pairs, where float64 averages and differs from q0 by up to 2e-4
    one = kr.cosine_fp32(rot0, rot1) >= 1.0
    ident = (_bits(rot0) == _bits(rot1)).all(axis=-1)
    differ = one & ~ident
    assert (sine[one] < kr.SLERP_GUARD[0]).all() and differ.sum() >= min_one, (what, int(differ.sum()))
    assert np.array_equal(_bits(got_rot)[one], _bits(rot0)[one]), what
    if differ.any():
        assert np.abs(q[differ] - rot0[differ]).max() > 1e-5          # ... so q0 there is not what an average or a slerp would return
    # every other pair: within 4 e-bar of float64, per decade of sin(half angle); [0, 1e-3) is the average override, whose e-bar (one
    # rounding of 0.5 q0 + 0.5 q1) separates it from a slerp (|0.5 - t| sine apart) and from q0 (0.5 sine apart)
    err = kr.slerp_error_by_decade(got_rot, q, sine, one)
    bound = K * np.array(kr.MEASURED_SLERP_DECADE)
    print("{:52s} err per decade {}  bounds {}  err / bound {}  (cos >= 1: {} pairs, {} not identical)".format(
        what + " slerp", " ".join("%.3e" % e for e in err), " ".join("%.3e" % b for b in bound), " ".join("%.3f" % r for r in err / bound), int(one.sum()), int(differ.sum())))
    assert got_rot.shape == q.shape and (err <= bound).all(), (what, err, bound)
    _check(got_pos, p, kr.MEASURED_ROOT_POS, what + " root_pos")
    # the short arc: the result keeps the side of q0, also where the stored pair has cos < 0
    assert ((got_rot.astype(np.float64) * rot0).sum(-1) > 0).all() and ((got_rot.astype(np.float64) * q).sum(-1) > 0.99).all()
    return int((cosine < 0).sum()), int((~one & (sine < 1e-3)).sum())


@pytest.mark.parametrize("c", kr.CHARS)
def test_calc_motion_frame_at_slerps_overrides(z, chars, libs, c):
    lib, rows = libs[c], _stored(libs[c], c, z)
    ids, times = z[c + "_q_ids"], z[c + "_q_times"]
    ref = _blend_reference(z, c, rows)
    out = [_np(x) for x in lib.calc_motion_frame(T(ids, torch.int64), T(times))]
    got_rot = np.concatenate([out[1][:, None], out[4]], axis=1)
    negative, averaged = _check_blend(got_rot, out[0], ref, c, min_one=50)
    assert negative >= 5 and averaged >= 20                         # pairs with cos < 0; pairs in the average override at blends other than 0.5
    # the velocities are frame 0's, bit for bit
    for k, col in (("root_vel", 2), ("root_ang_vel", 3), ("dof_vel", 5)):
        assert np.array_equal(_bits(out[col]), _bits(ref[6][k])), k
    assert (out[6] == 0.0).all()
    # a query's result depends neither on the number of queries nor on its place (16 queries fill a block)
    for nq in (1, 16, 17):
        part = [_np(x) for x in lib.calc_motion_frame(T(ids[:nq], torch.int64), T(times[:nq]))]
        assert all(np.array_equal(_bits(a), _bits(b[:nq])) for a, b in zip(part, out)), nq


# ------------------------------------------------------------------------------------------------------------------ fused post-step: the reference pose
def test_post_step_reference_pose_at_slerps_overrides(z, chars, libs):
    """parc_math_pk.h: the fused kernel blends two poses per lane.  The designed hum library behind a TrackerCore of the G6 state; every
    env queries one designed (clip, time); then three envs alone, so that the paired lanes hold an odd pose."""
    from parc_amd import _hip
    c = "hum"
    lib, rows = libs[c], _stored(libs[c], c, z)
    core, _ = _core_from_golden(chars[c], lib)
    N = core.N
    core.motion_xy_offset[:] = 0.0
    core.env_offsets[:] = 0.0
    core.time_buf[:] = 0.0
    ids, times = z[c + "_q_ids"], z[c + "_q_times"]
    Q = ids.shape[0]
    alone = None
    for s in range(0, Q, N):
        sel = np.arange(s, s + N) % Q
        core.motion_ids[:] = T(ids[sel], torch.int64)
        core.motion_time_offsets[:] = T(times[sel])
        core.post_step(_hip.POST_REF)
        torch.cuda.synchronize()
        got_rot = np.concatenate([_np(core.ref_root_rot)[:, None], _np(core.ref_joint_rot)], axis=1)
        ref = _blend_reference(z, c, rows, sel)
        _check_blend(got_rot, _np(core.ref_root_pos), ref, "post_step queries {}..{}".format(s, s + N - 1))
        for k in ("root_vel", "root_ang_vel", "dof_vel"):
            assert np.array_equal(_bits(_np(getattr(core, "ref_" + k))), _bits(ref[6][k])), k
        if s == 0:
            alone = (got_rot[[5, 6, 40]], _np(core.ref_root_pos)[[5, 6, 40]])
    # the same three queries in a launch of their own (an odd number of poses), the other rows untouched
    core.motion_ids[:] = T(ids[np.arange(N) % Q], torch.int64)
    core.motion_time_offsets[:] = T(times[np.arange(N) % Q])
    core.ref_root_rot[:] = -7.0
    core.ref_joint_rot[:] = -7.0
    core.ref_root_pos[:] = -7.0
    env_ids = torch.tensor([5, 6, 40], dtype=torch.int64, device=DEV)
    core.post_step(_hip.POST_REF, env_ids)
    torch.cuda.synchronize()
    got_rot = np.concatenate([_np(core.ref_root_rot)[:, None], _np(core.ref_joint_rot)], axis=1)
    assert np.array_equal(_bits(got_rot[[5, 6, 40]]), _bits(alone[0])) and np.array_equal(_bits(_np(core.ref_root_pos)[[5, 6, 40]]), _bits(alone[1]))
    others = np.ones(N, bool)
    others[[5, 6, 40]] = False
    assert (got_rot[others] == -7.0).all() and (_np(core.ref_root_pos)[others] == -7.0).all()


# ------------------------------------------------------------------------------------------------------------------ headings
@pytest.mark.parametrize("global_obs", [False, True])
def test_heading_branches_in_the_observation(z, km, mlib, oracle, ref_char, ref_mlib, global_obs):  # noqa: F811
    """calc_heading_quat_inv_alg stands in for atan2 / sin / cos wherever the fused post-step needs a heading: the G6 state with the
    designed root rotations (both sides of cos h = 0 and of h = +-pi, pitched and rolled, the identity, the half turn about z)"""
    from parc_amd import _hip
    q = z["head_rot"]
    assert kr.heading_conditions(q) == []
    core, g6 = _core_from_golden(km, mlib, **({"global_obs": True} if global_obs else {}))
    assert core.N == q.shape[0] == 64 and np.array_equal(z["head_vel"], g6["char_root_vel"]) and np.array_equal(z["head_ang_vel"], g6["char_root_ang_vel"])
    core.root_state[:, 3:7] = T(q)
    core.post_step(_hip.POST_OBS)
    torch.cuda.synchronize()
    obs = _np(core.obs)
    want = z["head_f64_block"] if not global_obs else kr.root_block(q, z["head_vel"], z["head_ang_vel"], global_obs=True)
    assert global_obs or kr.value_error(kr.root_block(q, z["head_vel"], z["head_ang_vel"]), want) <= 1e-12
    _check(obs[:, 0:12], want, kr.MEASURED_ROOT_BLOCK, "root block of char_obs, global_obs {}".format(global_obs))
    if global_obs:                                                   # the heading must not leak into the row: it differs from the local one
        assert kr.value_error(want[:kr.N_HEADING_DESIGNED - 2], z["head_f64_block"][:kr.N_HEADING_DESIGNED - 2]) > 0.5
    # the whole row against the C oracle (pinned at these rotations by test_kin_ref_cpu), at test_g6_fused_post_step's own tolerance
    off = g6["motion_offsets"][g6["motion_ids"], 0] - g6["env_offsets"][:, 0:2]
    times = g6["time_buf"] + g6["motion_time_offsets"]
    tar_dt = (g6["tar_obs_steps"].astype(np.float32) * np.float32(1.0 / 30.0)).astype(np.float32)
    o_obs = oracle.compute_obs(ref_char, ref_mlib, tar_dt, g6["key_body_ids"], g6["motion_ids"], times, off, g6["char_root_pos"], q, g6["char_root_vel"],
                               g6["char_root_ang_vel"], g6["char_dof_pos"], g6["char_dof_vel"], g6["contact_forces"], g6["ray_hfs"], global_obs=global_obs)
    print("obs[:, :871] against the oracle: max |d| {:.3e} (atol 3e-5, rtol 1e-5)".format(np.abs(obs[:, :871].astype(np.float64) - o_obs[:, :871]).max()))
    close(obs[:, :871], o_obs[:, :871], atol=3e-5)
