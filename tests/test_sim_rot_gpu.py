"""The simulator's joint rotations on the DEVICE at their branch points: the checks of tests/test_sim_rot_ref_cpu.py (parts A-E of DESIGN.md,
"Simulator rotations at their branch points") on the product kernels through parc_sim_refresh_bodies, parc_sim_refresh_bodies_masked,
parc_sim_step and parc_sim_step_ctl, held to the float64 yardstick of tests/tools/sim_rot_ref.py at 4 e-bar of fixture G38, plus the exact
assertions: root quaternions q, -q, 0.5 q and 2 q publish the same bits, the index-list and the masked refresh write the bits of the
all-envs one and nothing else, a row does not depend on the batch it is launched in, a zero map is the fixed joint.  Every check prints
its err / bound ratios before it asserts."""
import copy
import os
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import sim_rot_ref as sr  # noqa: E402
import test_sim_rot_ref_cpu as rc  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-777.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("c", sr.CHARS)
def test_pose_publication(c):
    rc.check_a(c, "device", sr.DEVICE_FACTOR)


@pytest.mark.parametrize("c", sr.CHARS)
def test_map_round_trip(c):
    rc.check_b(c, "device", None, sr.DEVICE_FACTOR)


@pytest.mark.parametrize("c", sr.CHARS)
def test_explicit_torque(c):
    rc.check_c(c, "device", None, sr.DEVICE_FACTOR)


@pytest.mark.parametrize("joint", [1, 2])
def test_implicit_drive_at_the_wrap(joint):
    rc.check_d(joint, "device", None, sr.DEVICE_FACTOR)


def test_velocity_cap():
    rc.check_e_cap("device", None)


def test_limit_switch():
    rc.check_e_limit("device", None)


@pytest.mark.parametrize("c", sr.CHARS)
def test_one_rotation_one_result_whatever_the_root_quaternion_is_scaled_by(c):
    """q, -q, 0.5 q and 2 q at the root are one rotation: positions and velocities of every body come out bit-equal, the world quaternions
    bit-equal up to the sign that -q carries down the chain (and up to the sign of an exact zero)."""
    z = rc.g38()
    s = sr.scene_struct(c)
    rs, ds = z[c + "_a_root"][:40].copy(), z[c + "_a_dof"][:40].copy()
    base = sr.base_root_quats()
    for k in range(40):
        assert np.array_equal(rs[k, 3:7], (base[k % 10] * sr.SCALES[k // 10]).astype(np.float32))
        rs[k, 7:13], ds[k] = rs[k % 10 + 30, 7:13], z[c + "_a_dof"][k % 10 + sr.NEAR_ROWS.start]
    rb, _ = rc.refresh(s, rs, ds, "device")
    for block, sign in ((1, -1.0), (2, 1.0), (3, 1.0)):
        a, b = rb[0:10], rb[10 * block:10 * block + 10]
        # (compared as values: equal floats are equal bits except that an exact zero may carry either sign, (-0) (-0) = +0)
        assert np.isfinite(b).all() and np.array_equal(a[..., 0:3], b[..., 0:3]) and np.array_equal(a[..., 7:13], b[..., 7:13]), (c, block)
        assert np.array_equal(a[..., 3:7], sign * b[..., 3:7]), (c, block)


@pytest.mark.parametrize("c", sr.CHARS)
def test_listed_and_masked_refresh_write_the_selected_rows_and_nothing_else(c):
    """The index-list entry with a permuted list and the masked entry write the bits of the all-envs entry on the selected rows and leave the
    bytes of the other rows (a sentinel) as they were."""
    from device_sim import DeviceSim
    z = rc.g38()
    s = sr.scene_struct(c)
    n, B, D = 13, int(s.num_bodies), int(s.dof_size)
    rows = np.arange(n) * 3 + 5
    rs, ds = z[c + "_a_root"][rows], z[c + "_a_dof"][rows]
    full, _ = rc.refresh(s, rs, ds, "device")
    ids = [7, 2, 12, 0, 5, 9]
    for how in ("ids", "mask"):
        sim = DeviceSim(copy.deepcopy(s), n, rc.HF, (-4.0, -4.0), (0.4, 0.4), num_bodies=B, dof_size=D)
        sim.root_state[:], sim.dof_state[:] = rs, ds
        sim.rigid_body_state[:], sim.contact_forces[:] = SENTINEL, SENTINEL
        if how == "ids":
            sim.refresh_bodies(env_ids=ids)
        else:
            sim.refresh_bodies(mask=[int(e in ids) for e in range(n)])
        others = [e for e in range(n) if e not in ids]
        assert np.array_equal(bits(sim.rigid_body_state[ids]), bits(full[ids])) and np.all(sim.contact_forces[ids] == 0.0), (c, how)
        assert np.all(sim.rigid_body_state[others] == SENTINEL) and np.all(sim.contact_forces[others] == SENTINEL), (c, how)


@pytest.mark.parametrize("c", sr.CHARS)
def test_a_row_does_not_depend_on_its_batch(c):
    """Four envs share a 64-lane workgroup: the rows of a launch of 1, 3, 4 and 5 envs are bit-equal to the same rows of a launch of 64."""
    z = rc.g38()
    s = sr.scene_struct(c)
    pick = (np.arange(64) * 7 + 20) % sr.N
    rs, ds = z[c + "_a_root"][pick], z[c + "_a_dof"][pick]
    full, _ = rc.refresh(s, rs, ds, "device")
    for n in (1, 3, 4, 5):
        part, cf = rc.refresh(s, rs[:n], ds[:n], "device")
        assert np.array_equal(bits(part), bits(full[:n])) and np.all(cf == 0.0), (c, n)


@pytest.mark.parametrize("c", sr.CHARS)
def test_a_zero_map_is_the_fixed_joint(c):
    """A joint whose dofs are all zero is the identity exactly: with every dof zero the character publishes the bits of the same tree with
    every joint fixed (the parent chain alone), under every designed root quaternion and root velocity."""
    z = rc.g38()
    s = sr.scene_struct(c)
    rs = z[c + "_a_root"]
    ds = np.zeros_like(z[c + "_a_dof"])
    fixed = copy.deepcopy(s)
    for b in range(1, int(s.num_bodies)):
        fixed.joint_type[b] = sr.JOINT_FIXED
    a, _ = rc.refresh(s, rs, ds, "device")
    b, _ = rc.refresh(fixed, rs, ds, "device")
    assert np.array_equal(bits(a), bits(b)), c
