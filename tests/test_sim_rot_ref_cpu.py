"""The simulator's joint rotations at their branch points, on the CPU: tests/tools/sim_rot_ref.py (the float64 yardstick and the designed
inputs) pinned to fixture G38 (tests/golden/gen_sim_rot.py: the reference's own classes in fp32 and float64), its guards, and both host
builds of the simulator sources (the one-env-per-lane core and the body-per-lane kernel under the lane emulation) held to the yardstick
at 2 e-bar on parts A-E of DESIGN.md, "Simulator rotations at their branch points".  The host builds run libm, not the device's
primitives: tests/test_sim_rot_gpu.py runs the same checks (the check_* functions below) on the device at 4 e-bar.

A  pose publication     refresh / publish_bodies on the designed states: positions, world quaternions, both velocities
B  map round trip       one substep in torque mode, action 0, no velocity: dof_state out = log(exp(e))
C  explicit torque      pd_exp / pd_1d, n_sub = hold = 1, from dof_torque; the clip, the zero gear, the hinge's sign
D  implicit PD drive    the default mode at the wrap: spherical error wraps, the hinge's does not
E  cap and limit        the angular-velocity cap and the switch-on of the joint-limit spring
"""
import copy
import math
import os
import sys

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import sim_ctl  # noqa: E402
import sim_rot_ref as sr  # noqa: E402

H = 1.0 / 120.0
F32, F64 = np.float32, np.float64
HF = np.zeros((20, 20), np.float32)
VARIANTS = ["core", "bpl"]
# roundings between a spherical map below 3e-6 and its round trip, one relative 2^-24 each; counted from the expressions, not measured.
# exp_to_q: the length (sum of squares and root, 2), the half-angle sine (polynomial, 2), the reciprocal (1), s / a (1), e s (1);
# qnormalize twice: the norm is exactly 1 at these lengths (0); q_to_exp: the length (2), the arctangent of l / 1 (polynomial, 2), the
# reciprocal (1), 2 atan / l (1), a q (1); below the threshold both branches have fewer.  15, rounded up to a power of two.
SMALL_ULPS = 16.0


def g38():
    return golden("g38_sim_rot")


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return sim_ctl.build_host(str(tmp_path_factory.mktemp("sim_rot")))


def report(tag, ratios):
    """every group's err / bound, printed before anything is asserted"""
    print("{}: ".format(tag) + ", ".join("{} {:.3g}".format(k, v) for k, v in ratios.items()))


def rows_of(where):
    return {"near": sr.NEAR_ROWS, "far": sr.FAR_ROWS, "band": sr.BAND_ROWS}[where]


def held(ratios, name, got, ref64, factor, group, quat=False):
    """err / bound of `got` against the float64 yardstick per row class of part A (the rows below the threshold are held to the `near` e-bar)"""
    for where in ("near", "far", "band"):
        r = rows_of(where)
        g = sr.signless(got[r], ref64[r]) if quat else got[r]
        ratios["{}/{}".format(name, where)] = sr.value_error(g, ref64[r]) / sr.bound(group, "far" if where == "far" else "near", factor)
    if quat:
        assert ((np.asarray(got, F64) * ref64).sum(-1) > 0.99).all(), name


def ctl(struct, n, variant, lib):
    return sim_ctl.CtlSim(copy.deepcopy(struct), n, variant, lib=lib, hf=HF)


def refresh(struct, rs, ds, variant, **kw):
    """rigid_body_state, contact_forces of the state rows through parc_sim_refresh_bodies (device) / the core's publish_bodies (host)"""
    n, B, D = rs.shape[0], int(struct.num_bodies), int(struct.dof_size)
    if variant == "device":
        from device_sim import DeviceSim
        sim = DeviceSim(copy.deepcopy(struct), n, HF, (-4.0, -4.0), (0.4, 0.4), num_bodies=B, dof_size=D)
    else:
        from oracle.sim_host import HostSim
        sim = HostSim(copy.deepcopy(struct), n, HF, (-4.0, -4.0), (0.4, 0.4), num_bodies=B, dof_size=D, variant="core")
    sim.root_state[:], sim.dof_state[:] = rs, ds
    sim.contact_forces[:] = 7.0
    sim.refresh_bodies(**kw)
    return sim.rigid_body_state.copy(), sim.contact_forces.copy()


# ------------------------------------------------------------------------------------------------------------- checks (also run on the device)
def check_a(c, variant, factor):
    """Part A: positions, quaternions and both velocities of every body within the bound of their group, root at the origin and far out."""
    z = g38()
    s = sr.scene_struct(c)
    M = sr.model_arrays(s)
    rs, ds = z[c + "_a_root"], z[c + "_a_dof"]
    ratios = {}
    for where, pos in (("origin", np.zeros(3)), ("far_root", sr.ROOT_FAR)):
        r = rs.copy()
        r[:, 0:3] = pos
        ref = sr.chain(M, r, ds)
        rb, cf = refresh(s, r, ds, variant)
        assert np.all(cf == 0.0)
        held(ratios, "pos_" + where, rb[..., 0:3], ref[..., 0:3], factor, "body_pos_" + where)
        if where == "origin":
            held(ratios, "rot", rb[..., 3:7], ref[..., 3:7], factor, "body_rot", quat=True)
            held(ratios, "lin_vel", rb[..., 7:10], ref[..., 7:10], factor, "body_lin_vel")
            held(ratios, "ang_vel", rb[..., 10:13], ref[..., 10:13], factor, "body_ang_vel")
    report("A {} {}".format(c, variant), ratios)
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


def check_b(c, variant, lib, factor):
    """Part B: one substep in torque mode, action 0, no velocity.  The spherical maps come back as the wrapped map within the bound, the
    hinge angles bit for bit, every velocity +-0, the root quaternion normalised, the published poses those of part A, no contact force."""
    z = g38()
    s = sr.scene_struct(c)
    M = sr.model_arrays(s)
    rs, ds = z[c + "_a_root"].copy(), z[c + "_a_dof"].copy()
    rs[:, 0:3], rs[:, 7:13], ds[..., 1] = (0.0, 0.0, 5.0), 0.0, 0.0
    sim = ctl(s, sr.N, variant, lib)
    sim.root_state[:], sim.dof_state[:] = rs, ds
    tq = sim.step(np.zeros((sr.N, M["D"])), "torque", n_sub=1, h=H, hold=1)
    assert np.all(tq == 0.0) and np.all(sim.contact_forces == 0.0)
    ref = ds[..., 0].astype(F64)
    for b in range(1, M["B"]):
        d0 = M["d0"][b]
        if M["jt"][b] == sr.JOINT_SPHERICAL:
            ref[:, d0:d0 + 3] = sr.q_to_exp(sr.exp_to_q(ref[:, d0:d0 + 3]))
        elif M["jt"][b] == sr.JOINT_HINGE:
            assert np.array_equal(sim.dof_state[:, d0, 0].view(np.uint32), ds[:, d0, 0].view(np.uint32)), (c, b)
    ratios = {}
    held(ratios, "rt_map", sim.dof_state[..., 0], ref, factor, "rt_map")
    # The maps of BAND_ROWS are up to 3e-6 long: an absolute e-bar of 5e-7 would pass a small-angle branch that returns half the map.  They
    # are held RELATIVE to their length instead: SMALL_ULPS roundings of 2^-24 each (DESIGN.md counts them: length, half-angle sine,
    # reciprocal, three products on the way in; length, arctangent, reciprocal, two products on the way out; both normalisations see 1).
    sph = [b for b in range(1, M["B"]) if M["jt"][b] == sr.JOINT_SPHERICAL]
    if sph:
        cols = np.concatenate([np.arange(M["d0"][b], M["d0"][b] + 3) for b in sph])
        e_in = ref[sr.BAND_ROWS][:, cols].reshape(-1, len(sph), 3)
        e_out = sim.dof_state[sr.BAND_ROWS][:, cols, 0].astype(F64).reshape(-1, len(sph), 3)
        length = np.linalg.norm(e_in, axis=-1)
        assert np.array_equal(e_out[length == 0], e_in[length == 0])                    # the zero map comes back as zero
        rel = np.linalg.norm(e_out - e_in, axis=-1)[length > 0] / length[length > 0]
        ratios["rt_map/band_relative"] = rel.max() / (SMALL_ULPS * 2.0 ** -24)
    # every force term is a product with a zero
    assert np.all(sim.dof_state[..., 1] == 0.0) and np.all(sim.root_state[:, 7:13] == 0.0) and np.all(sim.rigid_body_state[..., 7:13] == 0.0)
    assert np.array_equal(sim.root_state[:, 0:3], rs[:, 0:3])
    q0 = sr.qunit(rs[:, 3:7].astype(F64))
    ratios["root_quat"] = sr.value_error(sim.root_state[:, 3:7], q0) / sr.bound("body_rot", "near", factor)
    pose = sr.chain(M, rs, ds)
    held(ratios, "pos", sim.rigid_body_state[..., 0:3] - np.array([0, 0, 5.0]), pose[..., 0:3] - np.array([0, 0, 5.0]), factor, "body_pos_origin")
    held(ratios, "rot", sim.rigid_body_state[..., 3:7], pose[..., 3:7], factor, "body_rot", quat=True)
    report("B {} {}".format(c, variant), ratios)
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


def _torque_ratios(ratios, name, tq, raw64, kp, keep, far, factor, group):
    for where, m in (("near", keep & ~far), ("far", keep & far)):
        if m.any():
            ratios["{}/{}".format(name, where)] = sr.value_error((tq / kp)[m], (raw64 / kp)[m]) / sr.bound(group, where, factor)


def check_c(c, variant, lib, factor):
    """Part C: the explicit torque of one hold.  Gears raised: torque / kp within the bound on every dof, the hinge's sign float64's (the
    short way round, flipping at pi), a zero gear gives exactly 0.  The scene's own gears: the clip rows give the bits of +-effort on the
    dofs float64 clips and stay within the bound on the others.  pd_1d (hinge-only characters) does not wrap."""
    z = g38()
    cd, ct = z[c + "_c_dof"], z[c + "_c_tar"]
    band, far, geared = sr.masks_c(c, cd, ct)
    rs = sr.root_c(c)
    ratios, held_tq = {}, {}
    hinge_only = all(t != sr.JOINT_SPHERICAL for t in sr.model_arrays(sr.scene_struct(c))["jt"])
    for mode, fn, group in (("pd_exp", sr.pd_exp_torque, "torque_exp"), ("pd_1d", sr.pd_1d_torque, "torque_1d")):
        if mode == "pd_1d" and not hinge_only:
            continue
        for clip in (False, True):
            s = sr.scene_struct(c, clip=clip)
            M = sr.model_arrays(s)
            sim = ctl(s, sr.N, variant, lib)
            sim.root_state[:], sim.dof_state[:] = rs, cd
            sim.act_lo[:], sim.act_hi[:] = -0.01, 0.01                     # the explicit modes ignore the bounds
            tq = sim.step(ct, mode, n_sub=1, h=H, hold=1).astype(F64)
            assert np.all(sim.contact_forces == 0.0)
            raw, clipped = fn(M, cd, ct)
            kp, lim = np.where(M["kp"] > 0, M["kp"], 1.0), M["effort"]
            assert np.all(tq[:, lim == 0] == 0.0) and np.all(np.abs(tq) <= lim)
            over = (np.abs(raw) > lim) & (lim > 0)                     # (a zero gear: exactly 0, above)
            name = mode + ("_clip" if clip else "")
            if clip:
                assert over[sr.C_CLIP_ROWS][:, lim > 0].any() and (~over[sr.C_CLIP_ROWS][:, lim > 0]).any()
                assert np.array_equal(tq[over].astype(F32).view(np.uint32), clipped[over].astype(F32).view(np.uint32)), name
            else:
                assert not over[:, lim > 0].any()
            _torque_ratios(ratios, name, tq, raw, kp, ~over & geared, far, factor, group)
            # the sign of every hinge torque that float64 holds clear of zero by the bound of the dof's own group
            for b in range(1, M["B"]):
                d0 = M["d0"][b]
                if M["jt"][b] == sr.JOINT_HINGE and lim[d0] > 0:
                    bnd = np.where(far[:, d0], sr.bound(group, "far", factor), sr.bound(group, "near", factor))
                    clear = np.abs(raw[:, d0] / kp[d0]) > bnd
                    assert np.array_equal(np.sign(tq[clear, d0]), np.sign(raw[clear, d0])), (name, b)
            if mode == "pd_exp" and not clip:
                # The relative rotations around the 1e-6 branch are smaller than the absolute bound: it passes a halved or a zeroed small-angle
                # result.  On a joint whose state map is exactly zero and whose velocity is zero, conj(identity) q_tar is q_tar and the torque
                # is kp times the round trip of the target's map: SMALL_ULPS roundings and the product with kp, relative to |diff|.  (On a
                # turned joint conj(q) q_tar carries an absolute rounding of 1e-7, 30 % of the smallest designed |v|: no relative bound holds.)
                zero = sr.per_dof(M, sr.raw_angles(M, cd[..., 0]) == 0) & (cd[..., 1] == 0)
                for b in range(1, M["B"]):
                    k = 3 if M["jt"][b] == sr.JOINT_SPHERICAL else 1
                    zero[:, M["d0"][b]:M["d0"][b] + k] = zero[:, M["d0"][b]:M["d0"][b] + k].all(axis=1, keepdims=True)
                diff = raw / kp
                small = zero & geared & (np.abs(diff) > 0) & (np.abs(diff) < 1e-4) & (np.arange(sr.N) < sr.C_NEAR_ROWS.stop)[:, None]
                # (per joint: a spherical joint's three components are held to the length of its map)
                length = sr.per_dof(M, np.stack([np.linalg.norm(diff[:, M["d0"][b]:M["d0"][b] + (3 if M["jt"][b] == sr.JOINT_SPHERICAL else 1)], axis=1)
                                                 if M["jt"][b] in (sr.JOINT_HINGE, sr.JOINT_SPHERICAL) else np.zeros(sr.N) for b in range(M["B"])], axis=1))
                assert small.sum() >= 2 and (np.abs(diff[small]) < 2.5e-6).any(), (c, small.sum())
                ratios["pd_exp/small_relative"] = (np.abs(tq / kp - diff)[small] / length[small]).max() / ((SMALL_ULPS + 1) * 2.0 ** -24)
                assert np.array_equal(np.sign(tq[small]), np.sign(raw[small])), name
            held_tq[name] = tq
    if hinge_only:
        # pd_1d does not wrap: between pi and 2 pi from the target the device's pd_1d torque pulls the long way (the sign of target - angle)
        # and its pd_exp torque the short way, the opposite one
        rel = ct.astype(F64) - cd[..., 0]
        M = sr.model_arrays(sr.scene_struct(c))
        beyond = (np.abs(rel) > math.pi + 1e-3) & (np.abs(rel) < 2 * math.pi - 0.5e-3) & (cd[..., 1] == 0) & (M["effort"] > 0)
        assert beyond.sum() >= 4
        assert np.array_equal(np.sign(held_tq["pd_1d"][beyond]), np.sign(rel[beyond]))
        assert np.array_equal(np.sign(held_tq["pd_exp"][beyond]), -np.sign(rel[beyond]))
    report("C {} {}".format(c, variant), ratios)
    assert max(ratios.values()) <= 1.0, ratios
    return ratios


# part D: every relative angle of part C; the tiny ones on the states of part C's tiny rows (0 and 1: the target's fp32 rounding stays clear
# of the guard), the others on 0, 1 and 3
D_THETAS = (0.0, 1.0, 3.0)
D_CASES = tuple((t, d) for t in D_THETAS for d in sr.REL if abs(d) >= 1e-3 or d == 0.0 or t in sr.STATE_TINY)
D_RELATIVE = 5e-4          # of a row's own rate, where the drive's error is exact in fp32: the tolerance below, which holds h kp / I at rates of order 1


def arm_struct(joint, kp=40.0, kd=3.0, armature=0.02, **over):
    s = sr.scene_struct("arm_h" if joint == 1 else "arm_s")
    for d in range(int(s.dof_size)):
        s.kp[d], s.kd[d], s.armature[d], s.effort[d] = kp, kd, armature, 0.0          # effort 0: the pd drive is not limited
    for k, v in over.items():
        setattr(s, k, v)
    return s


def check_d(joint, variant, lib, factor):
    """Part D: the default mode (parc_sim_step) on the arm, state angle theta about x (hinge: its own axis), target theta + delta, delta = every
    relative angle of part C.  The rate after one substep is the implicit-Euler step of
    test_sim_invariants.test_joint_drive_is_the_implicit_euler_spring_damper with err = wrap(delta) for the spherical joint and err = delta
    for the hinge, to that test's 5e-4.  That tolerance is void on the rows around the 1e-6 branch (rates of 1e-6), so where the drive's error
    is exact in fp32 - the hinge (target - angle is an exact difference) and the spherical joint at theta = 0 (conj(identity) q_tar is q_tar:
    the error is the map's round trip, SMALL_ULPS roundings) - the rate is also held to D_RELATIVE of itself: the step is linear in the error
    at zero velocity, rate = c err, and c is what the 5e-4 holds at rates of order 1.  There the sign is float64's on every row and a zero
    error gives exactly 0.  On a turned spherical joint the error carries the absolute rounding of conj(q) q_tar: the sign is float64's
    wherever float64's rate clears c times the e-bar bound of the relative map (torque_exp, near)."""
    kp, kd, arm = 40.0, 3.0, 0.02
    inertia = 0.23 + arm
    cases = list(D_CASES)
    n = len(cases)
    assert n <= 64 and sum(1 for t, d in cases if 0 < abs(d) < 1e-4) == 16
    s = arm_struct(joint, kp, kd, arm)
    sim = ctl(s, n, variant, lib)
    sim.root_state[:, 2] = 5.0
    sim.act_lo[:], sim.act_hi[:] = -100.0, 100.0
    act = np.zeros((n, sim.D), F32)
    for i, (t, d) in enumerate(cases):
        sim.dof_state[i, 0, 0] = t
        act[i, 0] = F32(t) + d if joint == 1 else 0.0
        if joint == 2:
            act[i] = sr.q_to_exp(sr.qmul(sr.exp_to_q(np.array([F32(t), 0, 0], F64)), sr.exp_to_q(np.array([d, 0, 0]))))
    th0 = sim.dof_state[:, 0, 0].astype(F64)
    dl = np.array([d for _, d in cases])
    if joint == 1:
        err = act[:, 0].astype(F64) - th0
        exact = np.ones(n, bool)
    else:
        M = sr.model_arrays(s)
        err, v, _ = sr.rel_maps(M, sim.dof_state[..., 0], act)
        err, v = err[:, 0], v[:, 1]
        assert sr._outside(v, sr.GUARD).all(), v[~sr._outside(v, sr.GUARD)]
        assert ((v > 0) & (v < sr.THRESHOLD)).sum() >= 4 and ((v > sr.THRESHOLD) & (v < 4e-6)).sum() >= 4
        assert np.all(np.abs(err) <= math.pi) and (np.sign(err) == -np.sign(dl))[(np.abs(dl) > math.pi) & (np.abs(dl) < 2 * math.pi)].all()
        exact = th0 == 0.0
    assert np.array_equal(np.sign(err[np.abs(dl) < math.pi]), np.sign(dl[np.abs(dl) < math.pi]))
    if variant == "device":
        from device_sim import DeviceSim
        dev = DeviceSim(s, n, HF, (-4.0, -4.0), (0.4, 0.4), num_bodies=2, dof_size=sim.D)
        dev.root_state[:], dev.dof_state[:], dev.act_lo[:], dev.act_hi[:] = sim.root_state, sim.dof_state, sim.act_lo, sim.act_hi
        dev.step(act, n_sub=1, h=H)
        out, cf = dev.dof_state, dev.contact_forces
    else:
        assert sim.step(act, "pd", n_sub=1, h=H, hold=1) is None
        out, cf = sim.dof_state, sim.contact_forces
    assert np.all(cf == 0.0)
    c = H * kp / (inertia + H * kd + H * H * kp)
    w = c * err
    got = out[:, 0, 1].astype(F64)
    rel = np.abs(got - w)[exact & (w != 0)] / np.abs(w[exact & (w != 0)])
    print("D joint {} {}: largest |rate - float64| {:.3g} of 5e-4; relative, where the error is exact, {:.3g} of {:.3g}".format(
        joint, variant, np.abs(got - w).max(), rel.max(), D_RELATIVE))
    print("D joint {} {}: rates where float64 does not clear the bound: {}".format(joint, variant, got[~exact & (np.abs(w) <= c * sr.bound("torque_exp", "near", factor))]))
    assert np.abs(got - w).max() < 5e-4, (got, w)
    assert rel.max() <= D_RELATIVE, rel
    assert np.all(got[exact & (w == 0)] == 0.0)
    clear = exact | (np.abs(w) > c * sr.bound("torque_exp", "near", factor))
    assert (~clear).sum() <= 8 and np.array_equal(np.sign(got[clear]), np.sign(w[clear]))
    if joint == 2:
        assert np.abs(out[:, 1:, 1]).max() < 1e-5


def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_e_cap(variant, lib):
    """Part E, the angular-velocity cap, torque mode, action 0, one substep: a spin of max_angular_velocity (1 - 2^-10) comes back within 4 ulp
    of itself, one of (1 + 2^-10) within 4 ulp of the cap with its direction kept.  The spherical link spins about its z axis (its centre
    of mass is on it: no gyroscopic term), the hinge about its own axis, the base about its z."""
    wmax = 100.0
    lo, hi = F32(wmax * (1 - 2.0 ** -10)), F32(wmax * (1 + 2.0 ** -10))
    for joint in (1, 2):
        s = arm_struct(joint)
        assert s.max_angular_velocity == wmax
        col = 0 if joint == 1 else 2
        for sign in (1.0, -1.0):
            sim = ctl(s, 4, variant, lib)
            sim.root_state[:, 2] = 5.0
            sim.dof_state[0, col, 1], sim.dof_state[1, col, 1] = sign * lo, sign * hi
            sim.root_state[2, 12], sim.root_state[3, 12] = sign * lo, sign * hi
            sim.step(np.zeros((4, sim.D)), "torque", n_sub=1, h=H, hold=1)
            assert np.all(sim.contact_forces == 0.0)
            got = [sim.dof_state[0, col, 1], sim.dof_state[1, col, 1], sim.root_state[2, 12], sim.root_state[3, 12]]
            want = [sign * lo, sign * F32(wmax), sign * lo, sign * F32(wmax)]
            print("E cap joint {} {} sign {:+.0f}: ulps {}".format(joint, variant, sign, [int(_ulps(g, w)) for g, w in zip(got, want)]))
            assert all(_ulps(g, w) <= 4 for g, w in zip(got, want)), (got, want)
            others = [k for k in range(sim.D) if k != col]
            assert np.abs(sim.dof_state[:2, others, 1]).max(initial=0.0) < 1e-4 and np.abs(sim.root_state[2:, 10:12]).max() < 1e-4


def check_e_limit(variant, lib):
    """Part E, the joint-limit spring, torque mode, action 0, no velocity, one substep: with the angle (spherical: the map's component) exactly
    at limit_hi, or at limit_lo, the rate out is exactly 0; one ulp beyond it is non-zero with the restoring sign, the float64
    one-substep formula of ctl_drive, w = -h limit_kp over / (I + armature + h limit_kd + h^2 limit_kp), to the 5e-4 of the invariants
    suite's one-substep recurrences (and, as that bound is wide for a one-ulp excursion, to 1 % of itself)."""
    inertia, arm, lim = 0.23, 0.02, F32(0.7)
    for joint in (1, 2):
        s = arm_struct(joint)
        col = 0 if joint == 1 else 1
        for d in range(int(s.dof_size)):
            s.limit_lo[d], s.limit_hi[d] = -lim, lim
        ang = np.array([lim, -lim, np.nextafter(lim, F32(1)), np.nextafter(-lim, F32(-1))], F32)
        sim = ctl(s, 4, variant, lib)
        sim.root_state[:, 2] = 5.0
        sim.dof_state[:, col, 0] = ang
        sim.step(np.zeros((4, sim.D)), "torque", n_sub=1, h=H, hold=1)
        assert np.all(sim.contact_forces == 0.0)
        w = sim.dof_state[:, col, 1].astype(F64)
        if joint == 2:
            # the limit reads the component of q_to_exp(exp_to_q(e)): the round trip may move a map at the limit by an ulp either way
            back = sr.q_to_exp(sr.exp_to_q(np.stack([0 * ang, ang, 0 * ang], -1).astype(F64)))[:, 1]
            assert np.abs(back - ang).max() < 1e-15
        over = np.where(np.abs(ang.astype(F64)) > lim, ang.astype(F64) - np.sign(ang) * float(lim), 0.0)
        ref = -H * s.limit_kp * over / (inertia + arm + H * s.limit_kd + H * H * s.limit_kp)
        print("E limit joint {} {}: rate {} float64 {}".format(joint, variant, w, ref))
        if joint == 1:
            assert w[0] == 0.0 and w[1] == 0.0
            assert w[2] < 0.0 and w[3] > 0.0
            assert np.abs(w - ref).max() < 5e-4 and np.abs(w[2:] - ref[2:]).max() <= 0.01 * np.abs(ref[2:]).min()
        else:
            # the spherical joint's component has been through exp_to_q and q_to_exp in fp32: at the limit it is within an ulp of it on
            # either side, so the spring is off or pushes back by at most the one-ulp figure
            step = abs(ref[2])
            assert np.all(np.abs(w) <= 3 * step + 1e-12) and w[2] <= 0.0 and w[3] >= 0.0 and w[0] <= 0.0 and w[1] >= 0.0


# ---------------------------------------------------------------------------------------------------------------------- CPU tests
def test_fixture_inputs_are_the_designed_ones_and_pass_their_guards():
    import json
    z = g38()
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "g38_sim_rot.json")))
    assert meta["share_of_cases_left_out"] == 0.0 and meta["seeds"] == sr.SEEDS and meta["rows"] == sr.N
    for c in sr.CHARS:
        rs, ds = sr.inputs_a(c)
        cd, ct = sr.inputs_c(c)
        for k, v in (("_a_root", rs), ("_a_dof", ds), ("_c_dof", cd), ("_c_tar", ct)):
            assert v.dtype == F32 and np.array_equal(z[c + k].view(np.uint32), v.view(np.uint32)), (c, k)
        assert sr.guards_a(c, z[c + "_a_dof"]) == meta[c + "_a"]
        assert sr.guards_c(c, z[c + "_c_dof"], z[c + "_c_tar"]) == meta[c + "_c"]
        assert meta[c + "_a"]["below_threshold"] > 0 and meta[c + "_a"]["zero_maps"] > 0 and meta[c + "_c"]["below_threshold"] > 0
        assert meta[c + "_c"]["in_reference_band"] > 0
    s = sr.scene_struct("syn16")
    assert int(s.num_bodies) == 16 and sorted(set(int(s.joint_type[b]) for b in range(1, 16))) == [1, 2, 3]
    for b in range(1, 16):
        if s.joint_type[b] == sr.JOINT_HINGE:
            assert sorted(abs(s.joint_axis[b][k]) for k in range(3)) == [0.0, 0.0, 1.0]


def test_measured_e_bars_are_the_fixtures():
    m = sr.measure(g38())
    for g in sr.GROUPS:
        for where in ("near", "far"):
            assert m[g][where] <= sr.MEASURED[g][where] <= 1.01 * m[g][where] + 1e-12, (g, where, m[g][where])


@pytest.mark.parametrize("c", sr.CHARS)
def test_yardstick_is_pinned_to_the_reference_records(c):
    """float64 against the reference's float64 at 1e-12 (positions far out: 1e-9, the size of 1e3 in float64 sums), fp32 against its fp32
    within 2 e-bar; the rows whose spherical maps the reference zeroes (BAND_ROWS, the band of part C) are the yardstick's alone."""
    z = g38()
    M = sr.model_arrays(sr.scene_struct(c))
    hinge_only = all(t != sr.JOINT_SPHERICAL for t in M["jt"])
    rows = slice(0, sr.N) if hinge_only else slice(sr.FAR_ROWS.start, sr.N)
    ds = z[c + "_a_dof"]
    for dt, tag, tol in ((F64, "f64", 1e-12), (F32, "f32", None)):
        Md = sr.model_arrays(sr.scene_struct(c), dt)

        def near(got, key, group, quat=False, atol=tol):
            ref = z["{}_{}_{}".format(c, tag, key)].astype(F64)
            for where, r in (("near", sr.NEAR_ROWS), ("far", sr.FAR_ROWS), ("near", rows if hinge_only else slice(0, 0))):
                g = sr.signless(got[r], ref[r]) if quat else got[r]
                assert sr.value_error(g, ref[r]) <= (atol if atol is not None else sr.bound(group, where, 2.0)), (c, tag, key, where)
        jq = sr.joint_quats(Md, ds[..., 0], dt)
        near(jq[:, 1:], "joint_quat", "joint_quat", quat=True)
        rt = ds[..., 0].astype(dt)
        for b in range(1, M["B"]):
            if M["jt"][b] == sr.JOINT_SPHERICAL:
                d0 = M["d0"][b]
                rt[:, d0:d0 + 3] = sr.q_to_exp(sr.exp_to_q(rt[:, d0:d0 + 3], dt), dt)
        near(rt, "rt_map", "rt_map", atol=None if dt == F32 else 1e-11)
        for where, pos in (("origin", np.zeros(3)), ("far_root", sr.ROOT_FAR)):
            rs = z[c + "_a_root"].copy()
            rs[:, 0:3], rs[:, 3:7] = pos, z[c + "_a_unit_root"]
            rb = sr.chain(Md, rs, ds, dt, unit_root=True)
            near(rb[..., 0:3], "body_pos_" + where, "body_pos_" + where, atol=None if dt == F32 else (1e-12 if where == "origin" else 1e-9))
            if where == "origin":
                near(rb[..., 3:7], "body_rot", "body_rot", quat=True)
        cd, ct = z[c + "_c_dof"], z[c + "_c_tar"]
        band, far, geared = sr.masks_c(c, cd, ct)
        for clip in (False, True):
            Mc = sr.model_arrays(sr.scene_struct(c, clip=clip), dt)
            kp = np.where(Mc["kp"] > 0, Mc["kp"], 1).astype(F64)
            for mode, fn, group in (("exp", sr.pd_exp_torque, "torque_exp"), ("1d", sr.pd_1d_torque, "torque_1d")):
                key = "{}_{}_torque_{}{}".format(c, tag, mode, "_clip" if clip else "")
                if key not in z:
                    continue
                got, ref = fn(Mc, cd, ct, dt)[1].astype(F64), z[key].astype(F64)
                for where, m in (("near", ~band & ~far), ("far", ~band & far)):
                    lim = 1e-12 if dt == F64 else sr.bound(group, where, 2.0)
                    assert sr.value_error((got / kp)[m], (ref / kp)[m]) <= lim, (key, where)


@pytest.mark.parametrize("c", sr.CHARS)
def test_pose_publication_on_the_host_core(c):
    check_a(c, "core", sr.HOST_FACTOR)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", sr.CHARS)
def test_map_round_trip_on_the_host(hostlib, c, variant):
    check_b(c, variant, hostlib, sr.HOST_FACTOR)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("c", sr.CHARS)
def test_explicit_torque_on_the_host(hostlib, c, variant):
    check_c(c, variant, hostlib, sr.HOST_FACTOR)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("joint", [1, 2])
def test_implicit_drive_at_the_wrap_on_the_host(hostlib, joint, variant):
    check_d(joint, variant, hostlib, sr.HOST_FACTOR)


@pytest.mark.parametrize("variant", VARIANTS)
def test_velocity_cap_on_the_host(hostlib, variant):
    check_e_cap(variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_limit_switch_on_the_host(hostlib, variant):
    check_e_limit(variant, hostlib)


def test_sim_model_hands_the_kernels_unit_local_rotations():
    """An MJCF quaternion written to six digits is up to 1.3e-4 from unit (pose_opt_ref's synthetic tree); the kernels build a link's frame
    with qmat(local_rotation * q), which is a rotation only for a unit quaternion.  SimModel normalises such a local rotation and leaves one
    that is unit to fp32 (the humanoid's identities, syn16's nine digits) bit for bit; on the six-digit tree the core's body velocities
    then stay within 2 e-bar of the float64 chain (1e-3 rad/s off without the normalisation)."""
    import pose_opt_ref as por
    from parc_amd.sim_model import SimModel
    km = por.load_char("syn")
    raw = km._local_rotation.cpu().numpy().astype(F64)
    assert np.abs(np.linalg.norm(raw, axis=-1) - 1.0).max() > 1e-4
    s = SimModel(km).struct
    lr = sr.model_arrays(s)["lr"]
    assert np.abs(np.linalg.norm(lr, axis=-1) - 1.0).max() < 1.1e-6          # what is within 1e-6 of unit stays as it is
    hum = sim_ctl.humanoid_struct()[1].struct
    assert all(list(hum.local_rotation[b]) == [0.0, 0.0, 0.0, 1.0] for b in range(15))
    assert np.array_equal(sr.model_arrays(sr.scene_struct("syn16"))["lr"].astype(F32), sr.model_arrays(sr._base_struct("syn16"))["lr"].astype(F32))
    rs, ds = sr.inputs_a("syn16")
    rb, _ = refresh(s, rs, ds, "core")
    ref = sr.chain(sr.model_arrays(s), rs, ds)
    for name, cols, group in (("lin", slice(7, 10), "body_lin_vel"), ("ang", slice(10, 13), "body_ang_vel"), ("pos", slice(0, 3), "body_pos_origin")):
        assert sr.value_error(rb[sr.NEAR_ROWS][..., cols], ref[sr.NEAR_ROWS][..., cols]) <= sr.bound(group, "near", sr.HOST_FACTOR), name
