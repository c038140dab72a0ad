"""Per-env physics parameters and pushes of the simulator (parc_sim_step_phys, parc_sim_env_params_t).

There is no reference trajectory for these: the yardsticks are bit-equality with the entry points without a table (a neutral table, and
rows that do not see each other) and closed forms computed here in float64 - free fall, Coulomb friction, the penalty spring's rest depth,
the implicit-Euler oscillator of a driven link, the momentum a push delivers.  Every check runs on both host builds of the simulator
sources (tests/tools/sim_phys.py: the one-env-per-lane core and the body-per-lane kernel under the lane emulation);
tests/test_phys_params_gpu.py runs the same checks on the device through the C ABI."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import sim_ctl  # noqa: E402
import sim_phys  # noqa: E402
import test_control_modes as cm  # noqa: E402

H = 1.0 / 120.0
F32 = float(np.finfo(np.float32).eps)          # 2^-23


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return sim_phys.build_host(str(tmp_path_factory.mktemp("sim_phys")))


@pytest.fixture(scope="module")
def humanoid():
    return sim_ctl.humanoid_struct()


def make_body(struct, n, variant, lib, mass=10.0, radius=0.2, com=(0.0, 0.0, 0.0), inertia=None, hf=None):
    """(after tests/test_sim_invariants.py make_ball) n envs of ONE free body with one collision sphere at the body origin: a uniform solid
    sphere unless `inertia` (about the centre, isotropic) is given; flat ground at z = 0 unless hf."""
    s = copy.deepcopy(struct)
    s.num_bodies, s.dof_size, s.num_spheres = 1, 0, 1
    s.parent[0], s.dof_idx[0] = -1, 0
    s.mass[0] = mass
    i_c = 0.4 * mass * radius * radius if inertia is None else inertia
    c = np.asarray(com, np.float64)
    i_o = i_c * np.eye(3) + mass * (c @ c * np.eye(3) - np.outer(c, c))
    for k in range(3):
        s.com[0][k] = float(c[k])
        s.sph_pos[0][k] = 0.0
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        s.inertia_o[0][k] = float(i_o[i, j])
    s.sph_body[0], s.sph_radius[0] = 0, radius
    for b in range(16):
        s.self_mask[b] = 0
        s.cap_radius[b] = 0.0
    s.angular_damping = 0.0
    sim = sim_phys.PhysSim(s, n, variant, lib=lib, hf=np.zeros((60, 20), np.float32) if hf is None else hf)
    sim.root_state[:, 2] = 5.0
    return sim


def make_arm(struct, n, variant, lib, joint=1, **kw):
    """n copies of the one-link arm of tests/test_control_modes.py make_arm, with a table"""
    one = cm.make_arm(struct, "core", None, joint, **kw)
    sim = sim_phys.PhysSim(one.m, n, variant, lib=lib)
    sim.root_state[:, 0:3] = [0.0, 0.0, 5.0]
    return sim


NO_ACT = np.zeros((1, 0), np.float32)


# ---------------------------------------------------------------------------------------------------------- checks (also run on the device)
def check_neutral_table_is_bitwise_the_plain_step(humanoid, variant, lib, n=3, steps=8):
    """A table of the model's own constants, scales 1, no push: parc_sim_step_phys == parc_sim_step (pd) / parc_sim_step_ctl, bit for bit,
    in every mode - perturbed humanoids landing on a terrain of box tops 0 / 6 / 12 cm high (column tops and walls, link contacts, drives
    and limits all active).  The workload of this claim, 4096 envs of boxes_64clips for 32 steps from the reset state, runs on the device
    (tests/test_phys_params_gpu.py); the host builds run this small one, because a reset state needs the env (device only) and the lane
    emulation steps one env in tens of milliseconds: 4096 x 32 x 5 modes x 2 would take hours."""
    _, sm = humanoid
    rng = np.random.default_rng(7)
    boxes = rng.choice([0.0, 0.06, 0.12], size=(20, 20)).astype(np.float32)
    dof = rng.normal(0.0, 0.2, (n, 28)).astype(np.float32)
    acts = rng.normal(0.0, 0.4, (steps, n, 28)).astype(np.float32)
    for mode in sim_ctl.MODES:
        out = []
        for phys in (False, True):
            sim = sim_phys.PhysSim(copy.deepcopy(sm.struct), n, variant, lib=lib, hf=boxes)
            sim.root_state[:, 2] = 0.99
            sim.root_state[:, 0] = 0.37 * np.arange(n)             # over different boxes
            sim.dof_state[..., 0] = dof
            tq = None
            for a in acts:
                tq = (sim.step if phys else sim.step_plain)(a, mode, n_sub=4, hold=2)
            out.append(sim.state() + ([tq] if tq is not None else []))
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b, err_msg=mode)
        assert np.abs(out[0][3]).max() > 1.0, mode              # it did touch the ground


def check_rows_are_independent(humanoid, variant, lib):
    """Two envs with different rows in one launch: each equals, bit for bit, a launch in which every env carries that row."""
    _, sm = humanoid
    rng = np.random.default_rng(8)
    dof = np.repeat(rng.normal(0.0, 0.2, (1, 28)), 2, axis=0).astype(np.float32)
    act = np.repeat(rng.normal(0.0, 0.4, (1, 28)), 2, axis=0).astype(np.float32)
    rows = sim_phys.neutral_rows(sm.struct, 2)
    rows["gravity"], rows["friction_mu"], rows["contact_kn"], rows["contact_cn"], rows["contact_ct"] = [3.7, 12.0], [0.5, 1.5], [1e4, 1.6e5], [500.0, 2e3], [1e3, 6e3]
    rows["mass_scale"], rows["kp_scale"], rows["kd_scale"] = [0.7, 1.4], [0.5, 2.0], [0.3, 2.0]
    rows["push_force"], rows["push_steps_left"] = [[80.0, -40.0, 10.0], [0.0, 30.0, 0.0]], [2, 5]

    def run(table, mode):
        sim = sim_phys.PhysSim(copy.deepcopy(sm.struct), 2, variant, lib=lib, hf=np.zeros((20, 20), np.float32))
        sim.params[:] = table
        sim.root_state[:, 2] = 0.93
        sim.dof_state[..., 0] = dof
        tq = None
        for _ in range(4):
            tq = sim.step(act, mode, n_sub=4, hold=2)
        return sim.state() + ([tq] if tq is not None else []), sim.params.copy()
    for mode in ("pd", "vel", "pd_exp"):         # the gain scales enter the implicit drive, ctl_drive and ctl_hold_torque differently
        mixed, mixed_rows = run(rows, mode)
        for e in range(2):
            same, same_rows = run(rows[[e, e]], mode)
            for a, b in zip(mixed, same):
                np.testing.assert_array_equal(a[e], b[e], err_msg=mode)
            assert mixed_rows[e] == same_rows[e]
        assert not np.array_equal(mixed[0][0], mixed[0][1])
        assert list(mixed_rows["push_steps_left"]) == [0, 1]


def check_free_fall_follows_the_rows_gravity(humanoid, variant, lib):
    """One free body dropped for 1 s: semi-implicit Euler's recursion v -= g h, z += h v for the row's g, in float64.  g = 0: at rest,
    exactly.  mass_scale does not change a free fall.
    Tolerance, from float32: K = 120 substeps; the velocity is rounded once per substep (<= ulp(v_max) / 2, v_max < 16: derived) and the
    solve for a = F / m carries a relative error for which 16 eps is ALLOWED - an allowance set before any run, not a derived bound:
    two 3x3 symmetric inverses, two rotations and the 1-ulp device reciprocal, some tens of operations of <= eps / 2 each - so |dv| <= K ulp(16) / 2 +
    16 eps g K h; the height integrates that (x K h) and adds its own rounding, <= K ulp(8) / 2."""
    _, sm = humanoid
    g = np.array([0.0, 1.62, 3.7, 9.81, 9.81, 24.8])
    sim = make_body(sm.struct, len(g), variant, lib, hf=np.full((20, 20), -100.0, np.float32))       # ground far away
    sim.params["gravity"] = g
    sim.params["mass_scale"] = [1.0, 1.0, 1.0, 1.0, 3.0, 0.5]
    steps, n_sub = 30, 4
    K = steps * n_sub
    for _ in range(steps):
        sim.step(NO_ACT, "pd", n_sub=n_sub, h=H)
    v, z = np.zeros_like(g), np.full_like(g, 5.0)
    for _ in range(K):
        v -= g * H
        z += H * v
    tol_v = K * 16 * F32 / 2 + 16 * F32 * g.max() * K * H
    tol_z = tol_v * K * H + K * 8 * F32 / 2
    assert np.abs(sim.root_state[:, 9] - v).max() < tol_v, (sim.root_state[:, 9], v, tol_v)
    assert np.abs(sim.root_state[:, 2] - z).max() < tol_z, (sim.root_state[:, 2], z, tol_z)
    assert sim.root_state[0, 2] == 5.0 and np.all(sim.root_state[0, 7:13] == 0.0)
    assert z[5] < 0.0 < z[1]                                     # the rows do differ


def check_friction_per_env(humanoid, variant, lib):
    """A sliding block (a body that cannot spin up: 10^4 kg m^2) on flat ground, three mu in one launch: v = v0 - mu g t while it
    slides, then it stops.  Setup and tolerance (1 % of v0 on the slip, 0.3 % of v0 on the end state) of
    tests/test_sim_invariants.py test_sliding_ball_decelerates_at_mu_g_then_rolls_at_five_sevenths."""
    _, sm = humanoid
    mass, r, v0 = 10.0, 0.2, 3.0
    mu = np.array([0.5, 1.0, 1.5])
    sim = make_body(sm.struct, 3, variant, lib, mass, r, inertia=1.0e4)
    g, kn = float(sim.m.gravity), float(sim.m.contact_kn)
    sim.params["friction_mu"] = mu
    sim.root_state[:, 0:3] = [-3.0, 0.0, r - mass * g / kn]
    sim.root_state[:, 7] = v0
    hs = H / 4
    k1 = int(0.5 * v0 / (mu.max() * g) / hs)                     # half of the shortest slide
    for _ in range(k1):
        sim.step(NO_ACT, "pd", n_sub=1, h=hs)
    t1 = k1 * hs
    assert np.abs(sim.root_state[:, 7] - (v0 - mu * g * t1)).max() < 0.01 * v0, (sim.root_state[:, 7], v0 - mu * g * t1)
    f = sim.contact_forces[:, 0]
    assert np.all(f[:, 0] < -0.93 * mu * mass * g) and np.all(f[:, 0] > -1.0005 * mu * mass * g)
    k2 = int(1.5 * v0 / (mu.min() * g) / hs)                     # past the longest slide
    for _ in range(0, k2, 8):
        sim.step(NO_ACT, "pd", n_sub=8, h=hs)
    assert np.abs(sim.root_state[:, 7]).max() < 0.003 * v0, sim.root_state[:, 7]
    x = sim.root_state[:, 0] + 3.0
    assert x[0] > x[1] > x[2] and np.abs(x - v0 * v0 / (2 * mu * g)).max() < 0.03 * (v0 * v0 / (2 * mu.min() * g)), x


def check_rest_depth_per_env(humanoid, variant, lib):
    """A ball at rest on the penalty spring sits m s g / kn deep: kn spaced x2 apart (mass_scale 1), then mass_scale s at the default kn.
    Tolerance 2e-5 m: the one of test_ball_rests_at_the_penalty_springs_closed_form_depth for the default kn."""
    _, sm = humanoid
    mass, r = 10.0, 0.2
    kn = np.array([1e4, 2e4, 4e4, 8e4, 1.6e5, 4e4, 4e4])
    s = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 2.0])
    sim = make_body(sm.struct, len(kn), variant, lib, mass, r)
    g = float(sim.m.gravity)
    sim.params["contact_kn"], sim.params["mass_scale"] = kn, s
    sim.root_state[:, 0:3] = [0.0, 0.0, r + 0.01]
    for _ in range(120):
        sim.step(NO_ACT, "pd", n_sub=4, h=H)
    d = mass * s * g / kn.astype(np.float64)
    assert d.max() < float(sim.m.contact_max_pen)
    assert np.abs(sim.root_state[:, 2] - (r - d)).max() < 2e-5, (sim.root_state[:, 2], r - d)
    assert np.abs(sim.root_state[:, 7:13]).max() < 1e-4
    f = sim.contact_forces[:, 0, 2]
    assert np.abs(f - mass * s * g).max() < 1e-3 * mass * g, f


def check_oscillator_with_scales(humanoid, variant, lib):
    """The driven one-link arm of test_joint_drive_is_the_implicit_euler_spring_damper with a row per env: every substep is the implicit
    Euler step of (s I + armature) th'' = kp' (th* - th) - kd' th', kp' = kp_scale kp, kd' = kd_scale kd, in float64 from the constants
    (mass_scale scales the link's inertia, not the armature).  Its tolerances: 5e-5 rad, 5e-4 rad/s."""
    _, sm = humanoid
    kp, kd, arm, target = 40.0, 3.0, 0.02, 0.5
    s = np.array([1.0, 0.5, 2.0, 1.0, 1.0, 1.0, 1.7])
    ks = np.array([1.0, 1.0, 1.0, 0.5, 2.0, 1.0, 1.3])
    ds = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 2.5])
    for joint in (1, 2):
        sim = make_arm(sm.struct, len(s), variant, lib, joint, kp=kp, kd=kd, armature=arm)
        sim.params["mass_scale"], sim.params["kp_scale"], sim.params["kd_scale"] = s, ks, ds
        col = 1 if joint == 2 else 0
        act = np.zeros((len(s), sim.D), np.float32)
        act[:, col] = target
        inertia = s * 0.23 + arm
        th, w = np.zeros_like(s), np.zeros_like(s)
        spread = 0.0
        for step in range(60):
            sim.step(act, "pd", n_sub=4, h=H)
            for _ in range(4):
                w = (inertia * w + H * ks * kp * (target - th)) / (inertia + H * ds * kd + H * H * ks * kp)
                th = th + H * w
            assert np.abs(sim.dof_state[:, col, 0] - th).max() < 5e-5, (joint, step, sim.dof_state[:, col, 0], th)
            assert np.abs(sim.dof_state[:, col, 1] - w).max() < 5e-4, (joint, step, sim.dof_state[:, col, 1], w)
            spread = max(spread, min(abs(th[1] - th[2]), abs(th[3] - th[4]), abs(th[0] - th[5])))
        assert spread > 0.01                                      # the rows do differ on the way


def check_explicit_pd_and_vel_with_gain_scales(humanoid, variant, lib):
    """pd_exp on the hinge arm: the hold's torque is clip(kp' (tar - th) - kd' w, +-effort) with the scaled gains, then semi-implicit
    Euler on s I + armature (check_explicit_pd_closed_form's recursion and tolerances).  vel: the implicit step of
    I_eff w' = kd' (v* - w) (check_vel_mode_closed_form's), kp_scale plays no part."""
    _, sm = humanoid
    arm, kp, kd, lim, tar = 0.02, 40.0, 3.0, 20.0, 0.5
    s = np.array([1.0, 2.0, 1.0, 1.0])
    ks = np.array([1.0, 1.0, 0.5, 2.0])
    ds = np.array([1.0, 1.0, 2.0, 0.5])
    n = len(s)
    sim = make_arm(sm.struct, n, variant, lib, 1, kp=kp, kd=kd, armature=arm, effort=lim)
    sim.params["mass_scale"], sim.params["kp_scale"], sim.params["kd_scale"] = s, ks, ds
    inertia = s * 0.23 + arm
    th, w = np.zeros(n), np.zeros(n)
    for step in range(30):
        tq = sim.step(np.full((n, 1), tar), "pd_exp", n_sub=4, hold=2, h=H)
        for k in range(4):
            if k % 2 == 0:
                tau = np.clip(ks * kp * (tar - th) - ds * kd * w, -lim, lim)
            w = w + H * tau / inertia
            th = th + H * w
        assert np.all(np.abs(tq[:, 0] - tau) < 2e-3 * np.maximum(1.0, np.abs(tau))), (step, tq[:, 0], tau)
        assert np.abs(sim.dof_state[:, 0, 0] - th).max() < 1e-4, (step, sim.dof_state[:, 0, 0], th)
        assert np.abs(sim.dof_state[:, 0, 1] - w).max() < 1e-3, (step, sim.dof_state[:, 0, 1], w)
    v_tar = 1.5
    sim = make_arm(sm.struct, n, variant, lib, 1, kp=1.0e4, kd=kd, armature=arm)
    sim.params["mass_scale"], sim.params["kp_scale"], sim.params["kd_scale"] = s, ks, ds
    w = np.zeros(n)
    spread = 0.0
    for step in range(40):
        sim.step(np.full((n, 1), v_tar), "vel", n_sub=4, hold=2, h=H)
        for _ in range(4):
            w = (inertia * w + H * ds * kd * v_tar) / (inertia + H * ds * kd)
        assert np.abs(sim.dof_state[:, 0, 1] - w).max() < 5e-4, (step, sim.dof_state[:, 0, 1], w)
        spread = max(spread, abs(w[2] - w[3]))
    assert spread > 0.05


def check_push_delivers_its_momentum(humanoid, variant, lib):
    """g = 0, no contact: a push of F for k control steps changes the linear momentum of a free body by F k dt (dt = n_sub h), the counter
    runs down to 0 and the force then stops exactly; the force acts at the CENTRE OF MASS (0.1 m off the body origin here), so the body
    does not start to turn; the env next to it, not pushed, stays bit for bit where it was.  (v_max is taken after the push.)
    Tolerance, from float32: the body does not rotate, so every substep adds dv = h F / m to the world velocity: one rounding of v
    (<= ulp(v_max) / 2: derived) and the relative error of the solve (16 eps allowed - the allowance of the free-fall check, not a
    derived bound) per substep, K = k n_sub
    substeps: |dP| <= m K ulp(v_max) / 2 + 16 eps |F| k dt."""
    _, sm = humanoid
    mass, k, n_sub = 10.0, 5, 4
    F = np.array([30.0, -20.0, 12.0])
    sim = make_body(sm.struct, 2, variant, lib, mass, com=(0.1, 0.0, 0.0))
    sim.params["gravity"] = 0.0
    sim.params["push_force"][0], sim.params["push_steps_left"][0] = F, k
    before = sim.state()
    left = []
    for step in range(k + 3):
        sim.step(NO_ACT, "pd", n_sub=n_sub, h=H)
        left.append(int(sim.params["push_steps_left"][0]))
        if step == k - 1:
            # a twin that takes over the state at the push's end and never had a push in its table
            twin = make_body(sm.struct, 2, variant, lib, mass, com=(0.1, 0.0, 0.0))
            twin.params["gravity"] = 0.0
            for a, b in zip((twin.root_state, twin.dof_state, twin.rigid_body_state, twin.contact_forces), sim.state()):
                a[:] = b
        elif step >= k:
            twin.step(NO_ACT, "pd", n_sub=n_sub, h=H)
    assert left == [4, 3, 2, 1, 0, 0, 0, 0]
    dt = n_sub * H
    dP = F * k * dt
    v_max = np.abs(dP).max() / mass
    ulp = F32 * 2.0 ** np.floor(np.log2(v_max))
    tol = mass * k * n_sub * ulp / 2 + 16 * F32 * np.linalg.norm(F) * k * dt
    rs = sim.root_state[0].astype(np.float64)
    c_w = cm._rotm(rs[3:7]) @ np.array([0.1, 0.0, 0.0])
    P = mass * (rs[7:10] + np.cross(rs[10:13], c_w))
    assert np.abs(P - dP).max() < tol, (P, dP, tol)
    # no turning: a force of |F| at the body origin instead would give the 10 kg, 0.16 kg m^2 body ~ |F| 0.1 k dt / I = 3.6 rad/s
    assert np.abs(rs[10:13]).max() < 16 * F32 * np.linalg.norm(F) * 0.1 * k * dt / (0.4 * mass * 0.04), rs[10:13]
    # the force stopped exactly: the three steps after the push are, bit for bit, those of the twin
    for a, b in zip(sim.state(), twin.state()):
        np.testing.assert_array_equal(a, b)
    assert np.abs(sim.root_state[0, 7:10] - dP / mass).max() < 1e-5
    # the neighbour never moved
    np.testing.assert_array_equal(sim.root_state[1], before[0][1])
    np.testing.assert_array_equal(sim.rigid_body_state[1, 0], before[0][1])       # (published by the step: the same 13 numbers)


def check_push_on_the_humanoid(humanoid, variant, lib):
    """The same identity on the articulated character, at rest, drives holding its pose, g = 0: total linear momentum F k dt, angular
    momentum about the world origin = sum over the substeps of h x_c x F with x_c the root link's centre of mass (the force's point of
    attack) - to the integrator's O(h) momentum error, i.e. the bounds of check_torque_mode_conserves_momentum (4 % / 15 %), relative
    to the delivered momentum."""
    km, sm = humanoid
    F, k = np.array([120.0, 60.0, 0.0]), 3
    sim = sim_phys.PhysSim(copy.deepcopy(sm.struct), 2, variant, lib=lib)
    sim.m.angular_damping = 0.0
    for b in range(16):
        sim.m.self_mask[b] = 0
    sim.params["gravity"] = 0.0
    sim.root_state[:, 0:3] = [0.1, -0.3, 2.0]
    sim.params["push_force"][0], sim.params["push_steps_left"][0] = F, 10 ** 6
    act = np.zeros((2, 28), np.float32)
    sim.step(act, "pd", n_sub=1, h=1e-6)                       # publish the bodies of the start state
    dL = np.zeros(3)
    for _ in range(4 * k):                                       # substep by substep, to see the point of attack move
        b0 = sim.rigid_body_state[0, 0].astype(np.float64)
        x_c = b0[0:3] + cm._rotm(b0[3:7]) @ sm.body_com[0]
        dL += H * np.cross(x_c, F)
        sim.step(act, "pd", n_sub=1, h=H)
    P, L = cm._momentum(sm, sim, 0)
    dP = F * (4 * k * H + 1e-6)
    assert np.abs(P - dP).max() < 0.04 * np.linalg.norm(dP), (P, dP)
    assert np.abs(L - dL).max() < 0.15 * np.linalg.norm(dL), (L, dL)
    P1, L1 = cm._momentum(sm, sim, 1)
    assert np.abs(P1).max() < 1e-4 and np.abs(L1).max() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------- CPU tests
VARIANTS = ["core", "bpl"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_neutral_table_is_bitwise_the_plain_step(humanoid, hostlib, variant):
    check_neutral_table_is_bitwise_the_plain_step(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_rows_are_independent(humanoid, hostlib, variant):
    check_rows_are_independent(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_free_fall_follows_the_rows_gravity(humanoid, hostlib, variant):
    check_free_fall_follows_the_rows_gravity(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_friction_per_env(humanoid, hostlib, variant):
    check_friction_per_env(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_rest_depth_per_env(humanoid, hostlib, variant):
    check_rest_depth_per_env(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_oscillator_with_scales(humanoid, hostlib, variant):
    check_oscillator_with_scales(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_explicit_pd_and_vel_with_gain_scales(humanoid, hostlib, variant):
    check_explicit_pd_and_vel_with_gain_scales(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_push_delivers_its_momentum(humanoid, hostlib, variant):
    check_push_delivers_its_momentum(humanoid, variant, hostlib)


@pytest.mark.parametrize("variant", VARIANTS)
def test_push_on_the_humanoid(humanoid, hostlib, variant):
    check_push_on_the_humanoid(humanoid, variant, hostlib)


def test_the_two_host_formulations_agree_with_a_table(humanoid, hostlib):
    """core and body-per-lane with the same non-neutral rows: the same equations in two layouts"""
    _, sm = humanoid
    rng = np.random.default_rng(5)
    dof = rng.normal(0.0, 0.2, (2, 28))
    act = rng.normal(0.0, 0.4, (2, 28))
    out = []
    for variant in VARIANTS:
        sim = sim_phys.PhysSim(copy.deepcopy(sm.struct), 2, variant, lib=hostlib, hf=np.zeros((20, 20), np.float32))
        sim.params["gravity"], sim.params["contact_kn"], sim.params["mass_scale"] = [3.7, 12.0], [1e4, 1.6e5], [0.7, 1.4]
        sim.params["kp_scale"], sim.params["push_force"], sim.params["push_steps_left"] = [0.5, 2.0], [[80.0, 0.0, 0.0], [0.0, 30.0, 0.0]], [1, 1]
        sim.root_state[:, 2] = 0.95
        sim.dof_state[..., 0] = dof
        sim.step(act, "pd", n_sub=4, hold=2)
        out.append(sim.dof_state.copy())
    np.testing.assert_allclose(out[0], out[1], rtol=1e-3, atol=1e-3)


BAD_ROWS = [("mass_scale", 0.0), ("mass_scale", -1.0), ("mass_scale", np.nan), ("mass_scale", np.inf), ("contact_kn", 0.0),
            ("contact_kn", np.nan), ("contact_kn", np.inf), ("kp_scale", 0.0), ("kp_scale", -2.0), ("kp_scale", np.nan), ("friction_mu", -0.1),
            ("contact_cn", -1.0), ("contact_ct", -1.0), ("kd_scale", -0.5), ("push_steps_left", -1)]


@pytest.mark.parametrize("variant", VARIANTS)
def test_host_builds_refuse_bad_rows(humanoid, hostlib, variant):
    """every rule of the table (include/parc_sim.h) on the host builds: PARC_EINVAL, and nothing stepped"""
    _, sm = humanoid
    for field, val in BAD_ROWS:
        sim = make_body(sm.struct, 3, variant, hostlib)
        sim.params[field][1] = val
        before = sim.state()
        sim.step(NO_ACT, "pd", expect=-1)
        for a, b in zip(sim.state(), before):
            np.testing.assert_array_equal(a, b)
    sim = make_body(sm.struct, 3, variant, hostlib)
    sim.params["friction_mu"], sim.params["contact_cn"], sim.params["contact_ct"], sim.params["kd_scale"] = 0.0, 0.0, 0.0, 0.0
    sim.step(NO_ACT, "pd")                                        # zero is allowed where the rule says non-negative
    L = sim_phys.phys_lib(hostlib)
    assert L.sim_phys_host_check(None, 3) == -1


def test_step_phys_refuses_bad_arguments_before_any_launch():
    """parc_sim_step_phys answers PARC_EINVAL before any HIP call (so this runs without a GPU): a null table, and what parc_sim_step_ctl
    refuses; parc_phys_rand: null pointers and ranges that break their rules."""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_sim
    L = _hip.lib()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p
    a = P(ctypes.addressof(buf))
    ter = _hip.TerrainS()

    def call(n_sub=4, hold=2, mode=3, table=a, torque=None, ts=None, tb=None):
        return L.parc_sim_step_phys(None, a, ter, 4, a, a, a, a, a, a, a, a, n_sub, H, hold, table, mode, torque, ts, tb, 0.1)
    EINVAL = -1
    assert call(table=None) == EINVAL
    assert call(mode=-1) == EINVAL and call(mode=5) == EINVAL
    assert call(n_sub=4, hold=3) == EINVAL and call(hold=0) == EINVAL and call(n_sub=0) == EINVAL
    assert call(ts=a) == EINVAL and call(tb=a) == EINVAL
    assert call(mode=0, torque=a) == EINVAL and call(mode=1, torque=a) == EINVAL
    for mode in range(5):
        assert call(mode=mode) == EINVAL                        # the empty terrain struct
    assert L.parc_sim_env_params_check(None, None, 4) == EINVAL

    def rand(rg, state=a, table=a):
        return L.parc_phys_rand(None, 0, None, rg, 1, state, table)
    ok = _hip_sim.PhysRangesS()
    assert rand(ok) == 0 and rand(None) == EINVAL and rand(ok, state=None) == EINVAL and rand(ok, table=None) == EINVAL
    for field, lohi, bit in (("contact_kn", (0.0, 1.0), 4), ("contact_kn", (2.0, 1.0), 4), ("mass_scale", (-1.0, 1.0), 32),
                             ("gravity", (float("nan"), 1.0), 1), ("friction_mu", (-0.5, 1.0), 2), ("kd_scale", (-0.5, 1.0), 128),
                             ("kp_scale", (0.0, 1.0), 64)):
        rg = _hip_sim.PhysRangesS()
        getattr(rg, field)[0], getattr(rg, field)[1] = lohi
        assert rand(rg) == 0                                     # not selected by field_mask: not looked at
        rg.field_mask = bit
        assert rand(rg) == EINVAL, field
    rg = _hip_sim.PhysRangesS()
    rg.field_mask = 1 << 8
    assert rand(rg) == EINVAL
    rg = _hip_sim.PhysRangesS()
    rg.push_interval[0], rg.push_interval[1], rg.push_duration[0], rg.push_duration[1] = 0, 5, 1, 2
    assert rand(rg) == EINVAL
    rg.push_interval[0], rg.push_duration[0] = 2, 0
    assert rand(rg) == EINVAL
    rg.push_duration[0] = 1
    assert rand(rg) == 0


def test_row_layout_matches_the_header():
    """the ctypes mirror, the numpy mirror and the C struct agree on the 64-byte row (field order of the issue: gravity, friction_mu,
    contact_kn / cn / ct, mass_scale, kp_scale, kd_scale, push_force[3], push_steps_left)"""
    from parc_amd import _hip_sim
    assert ctypes.sizeof(_hip_sim.EnvParamsS) == 64 == sim_phys.ROW.itemsize
    names = [f[0] for f in _hip_sim.EnvParamsS._fields_]
    assert names[:10] == ["gravity", "friction_mu", "contact_kn", "contact_cn", "contact_ct", "mass_scale", "kp_scale", "kd_scale",
                          "push_force", "push_steps_left"]
    for f in names:
        assert getattr(_hip_sim.EnvParamsS, f).offset == sim_phys.ROW.fields[f][1], f
    hdr = open(os.path.join(REPO, "include", "parc_sim.h")).read()
    body = hdr[hdr.index("typedef struct {\n    float gravity;"):hdr.index("} parc_sim_env_params_t;")]
    order = [body.index(f) for f in ("gravity", "friction_mu", "contact_kn", "contact_cn", "contact_ct", "mass_scale", "kp_scale", "kd_scale",
                                     "push_force[3]", "push_steps_left")]
    assert order == sorted(order)


def test_host_builds_with_a_table_are_clean_under_asan_and_ubsan(tmp_path):
    """Both host formulations of the step with a table built with -fsanitize=address,undefined: one pushed, randomised step of every mode
    runs without a report (as test_control_modes.test_host_builds_of_every_mode_are_clean_under_asan_and_ubsan does without one)."""
    lib = sim_phys.build_host(str(tmp_path), sanitize=True)
    libasan = subprocess.check_output(["g++", "-print-file-name=libasan.so"], text=True).strip()
    assert os.path.isabs(libasan) and os.path.exists(libasan)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1:clear_shadow_mmap_threshold=1000000000",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "tools", "sim_phys.py"), "--smoke", lib], capture_output=True, text=True,
                         env=env, cwd=REPO, timeout=600)
    out = res.stdout + res.stderr
    assert res.returncode == 0, out[-4000:]
    assert "smoke ok" in res.stdout and "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
