#!/usr/bin/env python3
"""Generate tests/golden/g27_control_modes.npz from the REFERENCE's own control-mode code (CPU, torch).

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the same stub modules (isaacgym, gym, ...)
and puts the reference on the path; this script then calls the reference's IGCharEnv methods on a bare instance that carries only the
attributes those methods read:
  * _calc_pd_exp_torque / _calc_pd_1d_torque   (envs/ig_char_env.py:399-420) on seeded dof states, velocities and targets;
  * _apply_action for every mode               (:489-504) with a recording stub of the gym handle;
  * _build_action_bounds_vel / _torque          (:350-363), the stub handing out the MJCF motor gears as actuator efforts.
kp / kd are what Isaac Gym reads from the MJCF joints (stiffness / damping), the efforts its motor gears (dof order = joint order).
pd_1d also runs on a small hinge-only character written by this script (stored in the fixture as text).

usage:  python tests/golden/gen_control_modes.py            # rewrites tests/golden/g27_control_modes.npz
        python tests/golden/gen_control_modes.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import os
import sys
import tempfile
import types
import xml.etree.ElementTree as ET

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import anim.kin_char_model as kin_char_model  # noqa: E402
import envs.ig_char_env as ig_char_env  # noqa: E402

N = 64

HINGE_MJCF = """<mujoco model="hinge_chain">
  <default>
    <motor ctrlrange="-1 1" ctrllimited="true"/>
    <default class="body">
      <geom type="capsule" condim="1" friction="1.0 0.05 0.05"/>
      <joint type="hinge" damping="0.1" stiffness="5" armature=".007" limited="true"/>
    </default>
  </default>
  <worldbody>
    <body name="pelvis" pos="0 0 1" childclass="body">
      <freejoint name="root"/>
      <geom name="pelvis" type="sphere" size="0.09" density="1000"/>
      <body name="upper" pos="0 0 -0.1">
        <joint name="hip" type="hinge" axis="0 1 0" range="-120 60" stiffness="500" damping="50" armature=".02"/>
        <geom name="upper" type="capsule" fromto="0 0 0 0 0 -0.3" size="0.05" density="1000"/>
        <body name="lower" pos="0 0 -0.4">
          <joint name="knee" type="hinge" axis="0 1 0" range="0 160" stiffness="300" damping="30" armature=".01"/>
          <geom name="lower" type="capsule" fromto="0 0 0 0 0 -0.3" size="0.04" density="1000"/>
          <body name="foot" pos="0 0 -0.35">
            <joint name="ankle" type="hinge" axis="1 0 0" range="-40 40" stiffness="100" damping="10" armature=".01"/>
            <geom name="foot" type="box" size="0.08 0.04 0.02" density="1000"/>
          </body>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="hip" gear="150" joint="hip"/>
    <motor name="knee" gear="0" joint="knee"/>
    <motor name="ankle" gear="40" joint="ankle"/>
  </actuator>
</mujoco>
"""


def mjcf_drive(path):
    """(kp, kd, gears) per dof in joint order: what Isaac Gym's asset / actuator properties hold for an MJCF character."""
    root = ET.parse(path).getroot()
    kp, kd = [], []
    for j in root.find("worldbody").iter("joint"):
        if j.get("type", "hinge") == "hinge":
            kp.append(float(j.get("stiffness", 0.0)))
            kd.append(float(j.get("damping", 0.0)))
    gears = [float(m.get("gear")) for m in root.find("actuator").iter("motor")]
    assert len(gears) == len(kp)
    return np.array(kp, np.float32), np.array(kd, np.float32), np.array(gears, np.float32)


class _RecordingGym:
    def __init__(self, gears):
        self.calls, self._gears = [], gears

    def _rec(self, name):
        def f(*args):
            self.calls.append(name)
            return None
        return f

    def __getattr__(self, name):
        if name.startswith("set_") or name.startswith("refresh_"):
            return self._rec(name)
        raise AttributeError(name)

    def get_actor_actuator_properties(self, env, actor):
        return [types.SimpleNamespace(motor_effort=float(g)) for g in self._gears]


def bare_env(km, kp, kd, gears, dof_pos, dof_vel, mode):
    e = ig_char_env.IGCharEnv.__new__(ig_char_env.IGCharEnv)
    e._kin_char_model = km
    e._char_dof_pos, e._char_dof_vel = gg.t(dof_pos), gg.t(dof_vel)
    e._pd_exp_kp, e._pd_exp_kd, e._pd_exp_torque_lim = gg.t(kp), gg.t(kd), gg.t(gears)
    e._pd_exp_tar = torch.zeros_like(e._char_dof_pos)
    e._gym = _RecordingGym(gears)
    e._sim, e._envs, e._char_handles = None, [None], [0]
    e._char_control_mode = ig_char_env.ControlMode[mode]
    e._action_buffer = torch.zeros_like(e._char_dof_pos)
    e._char_action_buffer = e._action_buffer[..., :]
    return e


def dof_dims(km):
    return [km.get_joint(j).get_dof_dim() for j in range(1, km.get_num_joints())]


def gen_char(tag, km, mjcf_path, rng, modes):
    kp, kd, gears = mjcf_drive(mjcf_path)
    D = km.get_dof_size()
    dims = dof_dims(km)
    hinge = np.zeros(D, bool)
    d = 0
    for dd in dims:
        hinge[d:d + dd] = dd == 1
        d += dd
    # per-env scale of the state / target spread: small (unsaturated drives) to large (clipped, hinge targets more than pi away)
    scale = np.geomspace(0.002, 2.0, N).astype(np.float32)[:, None]
    dof_pos = (rng.uniform(-1.0, 1.0, (N, D)) * scale * 1.5).astype(np.float32)
    dof_vel = (rng.normal(0.0, 1.0, (N, D)) * scale * 2.0).astype(np.float32)
    tar = (dof_pos + rng.uniform(-1.0, 1.0, (N, D)) * scale * 2.0).astype(np.float32)
    far = rng.uniform(np.pi + 0.2, 2.0 * np.pi - 0.2, (N, D)) * np.sign(rng.uniform(-1, 1, (N, D)))
    sel = (np.arange(N) % 4 == 3)[:, None] & hinge[None, :]
    tar = np.where(sel, dof_pos + far, tar).astype(np.float32)       # every 4th env: hinge targets more than pi from the state
    arrs = {tag + "_kp": kp, tag + "_kd": kd, tag + "_effort": gears, tag + "_dof_pos": dof_pos, tag + "_dof_vel": dof_vel, tag + "_tar": tar}
    for mode in modes:
        e = bare_env(km, kp, kd, gears, dof_pos, dof_vel, mode)
        e._pd_exp_tar[:] = gg.t(tar)
        fn = ig_char_env.IGCharEnv._calc_pd_exp_torque if mode == "pd_exp" else ig_char_env.IGCharEnv._calc_pd_1d_torque
        arrs["{}_{}_torque".format(tag, mode)] = fn(e)
    e = bare_env(km, kp, kd, gears, dof_pos, dof_vel, "pd")
    arrs[tag + "_bounds_vel"] = np.stack(ig_char_env.IGCharEnv._build_action_bounds_vel(e))
    arrs[tag + "_bounds_torque"] = np.stack(ig_char_env.IGCharEnv._build_action_bounds_torque(e))
    return arrs


def gen_apply_action(km, rng):
    """_apply_action per mode on actions partly outside the bounds: which gym setter runs, the clipped action buffer, the pd_exp target."""
    kp, kd, gears = mjcf_drive(gg.CHAR_FILE)
    D = km.get_dof_size()
    low = -np.linspace(0.5, 2.0, D).astype(np.float32)
    high = np.linspace(0.4, 1.5, D).astype(np.float32)
    act = rng.uniform(-3.0, 3.0, (16, D)).astype(np.float32)
    arrs = {"apply_action": act, "apply_low": low, "apply_high": high}
    for mode in ("pd", "vel", "torque", "pd_exp", "pd_1d"):
        e = bare_env(km, kp, kd, gears, np.zeros((16, D), np.float32), np.zeros((16, D), np.float32), mode)
        e._action_bound_low, e._action_bound_high = gg.t(low), gg.t(high)
        ig_char_env.IGCharEnv._apply_action(e, gg.t(act))
        arrs["apply_{}_buffer".format(mode)] = e._char_action_buffer.clone()
        arrs["apply_{}_tar".format(mode)] = e._pd_exp_tar.clone()
        arrs["apply_{}_calls".format(mode)] = np.array(",".join(e._gym.calls))
    return arrs


def main():
    out = tempfile.mkdtemp(prefix="parc_g27_check_") if "--check" in sys.argv else HERE
    rng = np.random.default_rng(27)
    torch.manual_seed(27)
    sys.modules["isaacgym.gymtorch"].unwrap_tensor = lambda x: x
    km = gg.load_char()
    arrs = gen_char("humanoid", km, gg.CHAR_FILE, rng, ["pd_exp"])
    arrs.update(gen_apply_action(km, rng))
    d = tempfile.mkdtemp(prefix="parc_g27_mjcf_")
    path = os.path.join(d, "hinge_chain.xml")
    with open(path, "w") as f:
        f.write(HINGE_MJCF)
    hk = kin_char_model.KinCharModel("cpu")
    hk.load_char_file(path)
    assert all(dd == 1 for dd in dof_dims(hk))
    arrs.update(gen_char("hinge", hk, path, rng, ["pd_exp", "pd_1d"]))
    arrs["hinge_mjcf"] = np.array(HINGE_MJCF)
    # pd_1d refuses a character with a spherical joint (_build_pd_exp_tensors :246-251)
    arrs["humanoid_dof_dims"] = np.array(dof_dims(km), np.int32)
    dst = os.path.join(out, "g27_control_modes.npz")
    np.savez_compressed(dst, **{k: gg.npy(v) for k, v in arrs.items()})
    print("wrote", dst, os.path.getsize(dst), "bytes")
    if "--check" in sys.argv:
        a, b = np.load(dst), np.load(os.path.join(HERE, "g27_control_modes.npz"))
        bad = 0
        for k in sorted(set(a.files) | set(b.files)):
            same = k in a.files and k in b.files and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
            if not same:
                bad += 1
                print("DIFFERS", k)
        print("check: {} arrays differ from the committed fixture".format(bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
