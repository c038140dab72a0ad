"""The vel / torque / pd_exp / pd_1d control modes of the simulator (envs/ig_char_env.py:20-25,378-420,489-504 of the reference).

The drive laws are pinned to the reference's own torque code (G27, tests/golden/gen_control_modes.py: _calc_pd_exp_torque,
_calc_pd_1d_torque, _apply_action, the action bounds); the dynamics of each mode to closed forms computed here in float64 on a one-link arm,
and to momentum conservation on the humanoid.  Every check runs on both host builds of the simulator sources (the one-env-per-lane core and
the body-per-lane kernel under the lane emulation, tests/tools/sim_ctl.py); tests/test_control_modes_gpu.py runs the same checks on the
device kernel through parc_sim_step_ctl."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import sim_ctl  # noqa: E402

H = 1.0 / 120.0


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return sim_ctl.build_host(str(tmp_path_factory.mktemp("sim_ctl")))


@pytest.fixture(scope="module")
def humanoid():
    return sim_ctl.humanoid_struct()


def g27():
    return golden("g27_control_modes")


def make_sim(struct, n, variant, lib, **over):
    s = copy.deepcopy(struct)
    if over.pop("self_collision", True) is False:
        for b in range(16):
            s.self_mask[b] = 0
    for k, v in over.items():
        setattr(s, k, v)
    return sim_ctl.CtlSim(s, n, variant, lib=lib)


def make_arm(struct, variant, lib, joint, kp=40.0, kd=3.0, armature=0.02, effort=0.0):
    """(after tests/test_sim_invariants.py make_arm) A two-body chain in free space without gravity: a 10^6 kg base (the free root) and one
    link on a hinge about y (joint=1) or a spherical joint (joint=2) at the base's origin; the link: 2 kg, centre of mass 0.3 m below the
    joint, 0.23 kg m^2 about the joint's x and y axes."""
    s = copy.deepcopy(struct)
    D = 1 if joint == 1 else 3
    s.num_bodies, s.dof_size, s.num_spheres = 2, D, 1
    s.parent[0], s.dof_idx[0] = -1, 0
    s.parent[1], s.joint_type[1], s.dof_idx[1] = 0, joint, 0
    for k in range(3):
        s.com[0][k] = 0.0
        s.sph_pos[0][k] = 0.0
        s.local_translation[1][k] = 0.0
        s.joint_axis[1][k] = [0.0, 1.0, 0.0][k]
        s.com[1][k] = [0.0, 0.0, -0.3][k]
    for k in range(4):
        s.local_rotation[1][k] = [0.0, 0.0, 0.0, 1.0][k]
    s.mass[0], s.mass[1] = 1.0e6, 2.0
    for k, v in enumerate([1.0e6, 0.0, 0.0, 1.0e6, 0.0, 1.0e6]):
        s.inertia_o[0][k] = v
    for k, v in enumerate([0.05 + 2.0 * 0.09, 0.0, 0.0, 0.05 + 2.0 * 0.09, 0.0, 0.01]):
        s.inertia_o[1][k] = v
    for d in range(D):
        s.kp[d], s.kd[d], s.armature[d], s.effort[d] = kp, kd, armature, effort
        s.limit_lo[d], s.limit_hi[d] = -10.0, 10.0
    s.sph_body[0], s.sph_radius[0] = 0, 0.01
    for b in range(16):
        s.self_mask[b] = 0
        s.cap_radius[b] = 0.0
    s.angular_damping, s.gravity = 0.0, 0.0
    sim = sim_ctl.CtlSim(s, 1, variant, lib=lib)
    sim.root_state[0, 0:3] = [0.0, 0.0, 5.0]
    return sim


def close(got, ref, kp):
    """|got - ref| <= 1e-5 |ref| + (the float32 resolution of kp * angle): the reference's arithmetic is float32 too"""
    tol = 1e-5 * np.abs(ref) + 4e-7 * np.asarray(kp) * (1.0 + np.pi)
    bad = np.abs(got - ref) > tol
    return not bad.any(), np.argwhere(bad)[:8], (got[bad][:8], ref[bad][:8])


# ---------------------------------------------------------------------------------------------------------- checks (also run on the device)
def check_pd_exp_torque_matches_the_reference(humanoid, variant, lib):
    """dof_torque after a one-hold step from the fixture's states equals the reference's _calc_pd_exp_torque: the relative-rotation
    error of every spherical joint, the axis projection (wrap to (-pi, pi]) of every hinge, the clip at the motor gears."""
    z = g27()
    _, sm = humanoid
    np.testing.assert_array_equal(z["humanoid_kp"], [sm.struct.kp[d] for d in range(28)])
    np.testing.assert_array_equal(z["humanoid_kd"], [sm.struct.kd[d] for d in range(28)])
    np.testing.assert_array_equal(z["humanoid_effort"], [sm.struct.effort[d] for d in range(28)])
    n = z["humanoid_dof_pos"].shape[0]
    sim = make_sim(sm.struct, n, variant, lib, gravity=0.0)
    sim.root_state[:, 2] = 3.0
    sim.dof_state[..., 0], sim.dof_state[..., 1] = z["humanoid_dof_pos"], z["humanoid_dof_vel"]
    sim.act_lo[:], sim.act_hi[:] = -0.01, 0.01                         # pd_exp ignores the bounds: the targets are the raw action
    tq = sim.step(z["humanoid_tar"], "pd_exp", n_sub=2, hold=2)
    ref = z["humanoid_pd_exp_torque"]
    assert (np.abs(ref) == z["humanoid_effort"]).mean() > 0.1 and (np.abs(ref) < 0.5 * z["humanoid_effort"]).mean() > 0.3
    ok, where, vals = close(tq, ref, z["humanoid_kp"])
    assert ok, (where, vals)


def check_hinge_chain_matches_the_reference(variant, lib, tmp_path):
    """pd_exp and pd_1d on a hinge-only character (G27's own MJCF): pd_exp wraps a hinge error to the short way round, pd_1d does not;
    an effort of 0 clips the torque to 0 (the reference's torch.clip, unlike the pd drive's 'effort <= 0 = unlimited')."""
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.sim_model import SimModel
    z = g27()
    path = tmp_path / "hinge_chain.xml"
    path.write_text(str(z["hinge_mjcf"]))
    km = KinCharModel("cpu")
    km.load_char_file(str(path))
    sm = SimModel(km)
    assert sm.struct.dof_size == 3 and [sm.struct.joint_type[b] for b in range(1, 4)] == [1, 1, 1]
    np.testing.assert_array_equal(z["hinge_kp"], [sm.struct.kp[d] for d in range(3)])
    np.testing.assert_array_equal(z["hinge_effort"], [sm.struct.effort[d] for d in range(3)])
    n = z["hinge_dof_pos"].shape[0]
    far = np.abs(z["hinge_tar"] - z["hinge_dof_pos"]) > np.pi
    assert far.sum() > 10
    for mode in ("pd_exp", "pd_1d"):
        sim = make_sim(sm.struct, n, variant, lib, gravity=0.0)
        sim.root_state[:, 2] = 3.0
        sim.dof_state[..., 0], sim.dof_state[..., 1] = z["hinge_dof_pos"], z["hinge_dof_vel"]
        tq = sim.step(z["hinge_tar"], mode, n_sub=2, hold=2)
        ref = z["hinge_{}_torque".format(mode)]
        ok, where, vals = close(tq, ref, z["hinge_kp"])
        assert ok, (mode, where, vals)
        assert np.all(tq[:, 1] == 0.0)                                  # the knee's gear is 0
    ref_exp, ref_1d = z["hinge_pd_exp_torque"], z["hinge_pd_1d_torque"]
    assert (np.sign(ref_exp[far]) != np.sign(ref_1d[far])).sum() > 3    # the fixture does tell the two apart


def check_action_bounds_and_apply_action(humanoid, variant, lib):
    """The action space per mode equals the reference's; _apply_action's semantics: torque and vel use the clipped action, pd_exp /
    pd_1d targets are the raw action."""
    from parc_amd.sim_model import action_bounds
    z = g27()
    km, sm = humanoid
    for mode in ("vel", "torque"):
        lo, hi = action_bounds(km, sm, mode)
        np.testing.assert_array_equal(np.stack([lo, hi]), z["humanoid_bounds_" + mode])
    # the fixture's record of _apply_action
    act, low, high = z["apply_action"], z["apply_low"], z["apply_high"]
    clipped = np.minimum(np.maximum(act, low), high)
    for mode in ("pd", "vel", "torque", "pd_exp", "pd_1d"):
        np.testing.assert_array_equal(z["apply_{}_buffer".format(mode)], clipped)
    np.testing.assert_array_equal(z["apply_pd_exp_tar"], act)
    np.testing.assert_array_equal(z["apply_pd_1d_tar"], act)
    assert str(z["apply_torque_calls"]) == "" and str(z["apply_pd_exp_calls"]) == ""
    n = act.shape[0]
    # torque: the torque applied is the clipped action
    sim = make_sim(sm.struct, n, variant, lib, gravity=0.0)
    sim.root_state[:, 2] = 3.0
    sim.act_lo[:], sim.act_hi[:] = low, high
    tq = sim.step(act, "torque", n_sub=4, hold=2)
    np.testing.assert_array_equal(tq, z["apply_torque_buffer"])
    # pd_exp: the bounds change nothing (unclipped targets)
    res = []
    for lo, hi in ((low, high), (np.full(28, -100.0), np.full(28, 100.0))):
        sim = make_sim(sm.struct, n, variant, lib, gravity=0.0)
        sim.root_state[:, 2] = 3.0
        sim.act_lo[:], sim.act_hi[:] = lo, hi
        res.append((sim.step(act, "pd_exp", n_sub=4, hold=2), sim.dof_state.copy()))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def check_torque_mode_closed_form(humanoid, variant, lib):
    """torque on a hinge, gravity off: the rate and the angle follow semi-implicit Euler for tau / (I + armature); an action beyond the
    bounds (+-effort) is clipped."""
    _, sm = humanoid
    inertia, arm, lim = 0.23, 0.02, 5.0
    sim = make_arm(sm.struct, variant, lib, 1, armature=arm, effort=lim)
    sim.act_lo[:], sim.act_hi[:] = -lim, lim
    th, w = 0.0, 0.0
    for step, a in enumerate([3.0, 3.0, 9.0, -7.0, -2.0]):
        tq = sim.step(np.full((1, 1), a), "torque", n_sub=4, hold=2, h=H)
        tau = float(np.clip(a, -lim, lim))
        assert tq[0, 0] == np.float32(tau)
        for _ in range(4):
            w += H * tau / (inertia + arm)
            th += H * w
        assert abs(sim.dof_state[0, 0, 1] - w) < 2e-4 * max(1.0, abs(w)), (step, sim.dof_state[0, 0], w)
        assert abs(sim.dof_state[0, 0, 0] - th) < 2e-4 * max(1.0, abs(th)), (step, sim.dof_state[0, 0], th)


def check_vel_mode_closed_form(humanoid, variant, lib, joint):
    """vel (hinge, and a spherical joint turning about y), gravity off: every substep is the implicit step of I w' = kd (v* - w),
    w+ = (I_eff w + h kd v*) / (I_eff + h kd) with I_eff = I + armature; the rate converges to v*, kp plays no part."""
    _, sm = humanoid
    inertia, arm, kd, v_tar = 0.23, 0.02, 3.0, 1.5
    sim = make_arm(sm.struct, variant, lib, joint, kp=1.0e4, kd=kd, armature=arm)
    col = 1 if joint == 2 else 0
    act = np.zeros((1, sim.D), np.float32)
    act[0, col] = v_tar
    w = 0.0
    for step in range(40):
        assert sim.step(act, "vel", n_sub=4, hold=2, h=H) is None
        for _ in range(4):
            w = ((inertia + arm) * w + H * kd * v_tar) / (inertia + arm + H * kd)
        assert abs(sim.dof_state[0, col, 1] - w) < 5e-4, (step, sim.dof_state[0, col, 1], w)
    assert abs(w - v_tar) < 0.01 * v_tar
    if joint == 2:
        assert np.abs(sim.dof_state[0, [0, 2], 1]).max() < 1e-4
    # out-of-bound velocity targets are clamped to the bounds
    a = make_arm(sm.struct, variant, lib, joint, kd=kd, armature=arm)
    b = make_arm(sm.struct, variant, lib, joint, kd=kd, armature=arm)
    a.act_lo[:], a.act_hi[:] = -1.0, 1.0
    a.step(act * 5.0, "vel", n_sub=4, hold=2)
    b.step(np.clip(act * 5.0, -1.0, 1.0), "vel", n_sub=4, hold=2)
    np.testing.assert_array_equal(a.dof_state, b.dof_state)


def check_explicit_pd_closed_form(humanoid, variant, lib):
    """pd_exp / pd_1d on a hinge: the torque clip(kp (tar - th) - kd w, +-effort) is computed at the start of every hold and held for
    `hold` substeps of semi-implicit Euler (saturating at first); 3.4 rad from the target, pd_exp drives the short way round (through the
    +-pi wrap) and pd_1d the long way."""
    _, sm = humanoid
    inertia, arm, kp, kd, lim = 0.23, 0.02, 40.0, 3.0, 20.0
    for mode in ("pd_exp", "pd_1d"):
        for hold in (1, 2, 4):
            sim = make_arm(sm.struct, variant, lib, 1, kp=kp, kd=kd, armature=arm, effort=lim)
            tar = 0.5
            th, w = 0.0, 0.0
            for step in range(30):
                tq = sim.step(np.full((1, 1), tar), mode, n_sub=4, hold=hold, h=H)
                for k in range(4):
                    if k % hold == 0:
                        tau = float(np.clip(kp * (tar - th) - kd * w, -lim, lim))
                    w += H * tau / (inertia + arm)
                    th += H * w
                assert abs(float(tq[0, 0]) - tau) < 2e-3 * max(1.0, abs(tau)), (mode, hold, step, tq, tau)
                assert abs(sim.dof_state[0, 0, 0] - th) < 1e-4, (mode, hold, step, sim.dof_state[0, 0], th)
                assert abs(sim.dof_state[0, 0, 1] - w) < 1e-3, (mode, hold, step, sim.dof_state[0, 0], w)
    # 3.4 rad away across the +-pi wrap: state -1.7, target 1.7 -> pd_1d pushes + (diff 3.4), pd_exp - (diff 3.4 - 2 pi = -2.88)
    first = {}
    for mode in ("pd_exp", "pd_1d"):
        sim = make_arm(sm.struct, variant, lib, 1, kp=kp, kd=kd, armature=arm, effort=lim)
        sim.dof_state[0, 0, 0] = -1.7
        tq = sim.step(np.full((1, 1), 1.7), mode, n_sub=4, hold=2)
        first[mode] = float(tq[0, 0])
    assert first["pd_1d"] == pytest.approx(lim) and first["pd_exp"] == pytest.approx(-lim), first


def _rotm(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _momentum(sm, sim, e=0):
    P, L = np.zeros(3), np.zeros(3)
    for b in range(sim.B):
        bs = sim.rigid_body_state[e, b].astype(np.float64)
        R = _rotm(bs[3:7])
        w, v0 = bs[10:13], bs[7:10]
        c = R @ sm.body_com[b]
        vc = v0 + np.cross(w, c)
        P += sm.body_mass[b] * vc
        L += R @ sm.body_inertia_com[b] @ R.T @ w + sm.body_mass[b] * np.cross(bs[0:3] + c, vc)
    return P, L


def check_torque_mode_conserves_momentum(humanoid, variant, lib):
    """Humanoid in free flight, gravity off, random joint torques: internal forces, so total linear and angular momentum stay constant
    (to the integrator's O(h), as in test_sim_invariants.test_momentum_conservation_zero_gravity)."""
    _, sm = humanoid
    rng = np.random.default_rng(3)
    # (no link-link contact: random torques fling the limbs through each other and the contact damping dissipates)
    sim = make_sim(sm.struct, 1, variant, lib, gravity=0.0, angular_damping=0.0, self_collision=False)
    sim.root_state[0, 0:3] = [0.1, -0.3, 2.0]
    sim.root_state[0, 7:13] = rng.standard_normal(6) * 0.5
    sim.dof_state[0, :, 0] = rng.standard_normal(28) * 0.3
    sim.dof_state[0, :, 1] = rng.standard_normal(28) * 2.0
    eff = np.array([sm.struct.effort[d] for d in range(28)], np.float32)
    sim.act_lo[:], sim.act_hi[:] = -eff, eff
    sim.step(np.zeros((1, 28)), "torque", n_sub=1, hold=1, h=1e-6)     # publish the bodies of the start state
    P0, L0 = _momentum(sm, sim)
    for _ in range(30):
        sim.step(rng.uniform(-0.05, 0.05, (1, 28)) * eff, "torque", n_sub=4, hold=2)
    P1, L1 = _momentum(sm, sim)
    assert np.isfinite(sim.dof_state).all()
    assert np.abs(P1 - P0).max() < 0.04 * np.linalg.norm(P0) and np.abs(L1 - L0).max() < 0.15 * np.linalg.norm(L0), (P0, P1, L0, L1)


# ---------------------------------------------------------------------------------------------------------------------- CPU tests
VARIANTS = ["core", "bpl"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_pd_exp_torque_matches_the_reference(humanoid, hostlib, variant):
    check_pd_exp_torque_matches_the_reference(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_hinge_chain_matches_the_reference(hostlib, variant, tmp_path):
    check_hinge_chain_matches_the_reference(variant, hostlib, tmp_path)


@pytest.mark.parametrize("variant", VARIANTS)
def test_action_bounds_and_apply_action(humanoid, hostlib, variant):
    check_action_bounds_and_apply_action(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_torque_mode_closed_form(humanoid, hostlib, variant):
    check_torque_mode_closed_form(humanoid, variant, hostlib)


@pytest.mark.parametrize("joint", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
def test_vel_mode_closed_form(humanoid, hostlib, variant, joint):
    check_vel_mode_closed_form(humanoid, variant, hostlib, joint)


@pytest.mark.parametrize("variant", VARIANTS)
def test_explicit_pd_closed_form(humanoid, hostlib, variant):
    check_explicit_pd_closed_form(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_torque_mode_conserves_momentum(humanoid, hostlib, variant):
    check_torque_mode_conserves_momentum(humanoid, variant, hostlib)


def test_the_two_host_formulations_agree(humanoid, hostlib):
    """core and body-per-lane: the same equations in two layouts, every mode, a perturbed humanoid on flat ground."""
    _, sm = humanoid
    rng = np.random.default_rng(5)
    dof = rng.normal(0.0, 0.2, (4, 28))
    act = rng.normal(0.0, 0.4, (4, 28))
    for mode in sim_ctl.MODES:
        out = []
        for variant in VARIANTS:
            sim = sim_ctl.CtlSim(copy.deepcopy(sm.struct), 4, variant, lib=hostlib, hf=np.zeros((20, 20), np.float32))
            sim.root_state[:, 2] = 0.95
            sim.dof_state[..., 0] = dof
            tq = sim.step(act, mode, n_sub=4, hold=2)
            out.append((sim.dof_state.copy(), tq))
        np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-3, atol=1e-3, err_msg=mode)
        if out[0][1] is not None:
            np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-3, atol=1e-2, err_msg=mode)


def test_pd_1d_refuses_a_character_with_a_spherical_joint(humanoid):
    from parc_amd.sim_model import check_control_mode
    km, _ = humanoid
    with pytest.raises(AssertionError, match="pd_1d only supports 1D joints"):
        check_control_mode(km, "pd_1d")
    with pytest.raises(AssertionError, match="Unsupported control mode"):
        check_control_mode(km, "position")
    for mode in ("pd", "vel", "torque", "pd_exp"):
        check_control_mode(km, mode)


def test_step_ctl_refuses_bad_arguments_before_any_launch():
    """parc_sim_step_ctl answers PARC_EINVAL before any HIP call (so this runs without a GPU): a mode out of range, a substep count that
    is not a multiple of the hold, only one of the clock buffers, a torque output in a mode that has none."""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_sim  # noqa: F401
    L = _hip.lib()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p
    a = P(ctypes.addressof(buf))
    ter = _hip.TerrainS()

    def call(n_sub=4, hold=2, mode=3, torque=None, ts=None, tb=None):
        return L.parc_sim_step_ctl(None, a, ter, 4, a, a, a, a, a, a, a, a, n_sub, H, hold, mode, torque, ts, tb, 0.1)
    EINVAL = -1
    assert call(mode=-1) == EINVAL and call(mode=5) == EINVAL
    assert call(n_sub=4, hold=3) == EINVAL and call(hold=0) == EINVAL and call(n_sub=0) == EINVAL
    assert call(ts=a) == EINVAL and call(tb=a) == EINVAL
    assert call(mode=0, torque=a) == EINVAL and call(mode=1, torque=a) == EINVAL
    # (a null heightfield is refused too, in every mode: the terrain struct above is empty)
    for mode in range(5):
        assert call(mode=mode) == EINVAL


def test_host_builds_of_every_mode_are_clean_under_asan_and_ubsan(tmp_path):
    """The control-mode step of both host formulations built with -fsanitize=address,undefined: one step of every mode runs without a
    report (as tests/test_sim_sanitized.py does for the pd step)."""
    lib = sim_ctl.build_host(str(tmp_path), sanitize=True)
    libasan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    assert os.path.isabs(libasan) and os.path.exists(libasan)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1:clear_shadow_mmap_threshold=1000000000",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "tools", "sim_ctl.py"), "--smoke", lib], capture_output=True, text=True,
                         env=env, cwd=REPO, timeout=600)
    out = res.stdout + res.stderr
    assert res.returncode == 0, out[-4000:]
    assert "smoke ok" in res.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
