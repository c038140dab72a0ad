#!/usr/bin/env python3
"""Generate tests/golden/g38_sim_rot.npz (+ .json: seeds, guards and the guard distances met) from the REFERENCE's own Python (CPU, torch),
in fp32 and in float64 from the same fp32 inputs, on the designed inputs of tests/tools/sim_rot_ref.py (every branch point of the
simulator's joint rotations visited on both sides):
  * KinCharModel.dof_to_rot and forward_kinematics (anim/kin_char_model.py:478-541) for joint quaternions, body positions and rotations;
  * util/torch_util.py's exp_map_to_quat and quat_to_exp_map for the round trip of a spherical joint's map;
  * IGCharEnv._calc_pd_exp_torque / _calc_pd_1d_torque (envs/ig_char_env.py:399-420) on a bare instance, as G27 does.
The reference holds no body velocities (Isaac Gym supplies them): their e-bar is sim_rot_ref.chain in fp32 against float64, computed
where it is used, not stored.

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference
on the path.  Per character c of sim_rot_ref.CHARS the fixture holds (data only):
  <c>_a_root, <c>_a_dof                      part A's state rows (root at the origin), <c>_a_unit_root the unit fp32 root quaternions that
                                             the reference's forward_kinematics is handed
  <c>_f32/_f64_joint_quat, .._rt_map          dof_to_rot; quat_to_exp_map(exp_map_to_quat(e)) of every spherical map (a hinge: the angle itself)
  .._body_pos_origin, .._body_pos_far_root, .._body_rot     forward_kinematics with the root at the origin and at ROOT_FAR
  <c>_c_dof, <c>_c_tar                        part C's states and targets
  .._torque_exp, .._torque_exp_clip           _calc_pd_exp_torque with the gears raised (nothing clipped) and with the scene's own gears
  .._torque_1d, .._torque_1d_clip             _calc_pd_1d_torque, hinge-only characters
The guards are checked here in float64, after the fp32 rounding; a violation is an error, no case is left out.

usage:  python tests/golden/gen_sim_rot.py            # rewrites the fixture
        python tests/golden/gen_sim_rot.py --check    # regenerate and compare with the committed fixture
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
sys.path.insert(0, os.path.dirname(HERE))
import mdm_loss_ref as mlr  # noqa: E402  (reference_root)

if not os.path.isdir(mlr.reference_root()):          # decided before any work; every failure after this line is a failure
    print("reference tree not found:", mlr.reference_root())
    sys.exit(3)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import anim.kin_char_model as kin_char_model  # noqa: E402
import envs.ig_char_env as ig_char_env  # noqa: E402
import util.torch_util as torch_util  # noqa: E402

import sim_rot_ref as sr  # noqa: E402

F32, F64 = torch.float32, torch.float64
PRECS = (("f32", F32), ("f64", F64))


def load_ref_char(name, dtype):
    km = kin_char_model.KinCharModel("cpu")
    if name == "hum":
        km.load_char_file(gg.CHAR_FILE)
    else:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, name + ".xml")
            with open(path, "w") as f:
                f.write(sr.mjcf_text(name))
            km.load_char_file(path)
    if dtype == F64:                                            # the fp32 model tensors cast up
        km._local_translation = km._local_translation.double()
        km._local_rotation = km._local_rotation.double()
        for j in km._joints:
            if j.axis is not None:
                j.axis = j.axis.double()
    return km


def same_model(km, M):
    """the reference's character is the one the simulator's struct describes"""
    assert km.get_num_joints() == M["B"] and km.get_dof_size() == M["D"]
    assert [int(p) for p in gg.npy(km._parent_indices)] == M["parent"]
    assert np.array_equal(gg.npy(km._local_translation), M["lt"].astype(np.float32))
    assert np.array_equal(gg.npy(km._local_rotation), M["lr"].astype(np.float32))
    for b in range(1, M["B"]):
        j = km.get_joint(b)
        assert j.get_dof_dim() == {sr.JOINT_HINGE: 1, sr.JOINT_SPHERICAL: 3}.get(M["jt"][b], 0), b
        if j.get_dof_dim() > 0:
            assert int(j.dof_idx) == M["d0"][b]
        if j.get_dof_dim() == 1:
            assert np.array_equal(gg.npy(j.axis), M["ax"][b].astype(np.float32)) and abs(np.linalg.norm(M["ax"][b]) - 1.0) == 0.0, b


def bare_env(km, M, dof_state, tar, dtype):
    e = ig_char_env.IGCharEnv.__new__(ig_char_env.IGCharEnv)
    e._kin_char_model = km
    e._char_dof_pos, e._char_dof_vel = gg.t(dof_state[..., 0], dtype), gg.t(dof_state[..., 1], dtype)
    e._pd_exp_kp, e._pd_exp_kd, e._pd_exp_torque_lim = gg.t(M["kp"], dtype), gg.t(M["kd"], dtype), gg.t(M["effort"], dtype)
    e._pd_exp_tar = gg.t(tar, dtype)
    return e


def gen_char(arrays, meta, c):
    M = sr.model_arrays(sr.scene_struct(c))
    Mclip = sr.model_arrays(sr.scene_struct(c, clip=True))
    rs, ds = sr.inputs_a(c)
    meta[c + "_a"] = sr.guards_a(c, ds)
    unit_root = sr.qunit(rs[:, 3:7].astype(np.float64)).astype(np.float32)
    arrays.update({c + "_a_root": rs, c + "_a_dof": ds, c + "_a_unit_root": unit_root})
    cd, ct = sr.inputs_c(c)
    meta[c + "_c"] = sr.guards_c(c, cd, ct)
    arrays.update({c + "_c_dof": cd, c + "_c_tar": ct})
    hinge_only = all(t != sr.JOINT_SPHERICAL for t in M["jt"])
    for tag, dtype in PRECS:
        km = load_ref_char(c, dtype)
        same_model(km, M)
        with torch.no_grad():
            dof = gg.t(ds[..., 0], dtype)
            jq = km.dof_to_rot(dof)
            arrays["{}_{}_joint_quat".format(c, tag)] = gg.npy(jq)
            rt = dof.clone()
            for b in range(1, M["B"]):
                if M["jt"][b] == sr.JOINT_SPHERICAL:
                    d0 = M["d0"][b]
                    rt[:, d0:d0 + 3] = torch_util.quat_to_exp_map(torch_util.exp_map_to_quat(dof[:, d0:d0 + 3]))
            arrays["{}_{}_rt_map".format(c, tag)] = gg.npy(rt)
            for where, pos in (("origin", np.zeros(3)), ("far_root", sr.ROOT_FAR)):
                bp, br = km.forward_kinematics(gg.t(np.broadcast_to(pos, (sr.N, 3)).copy(), dtype), gg.t(unit_root, dtype), jq)
                arrays["{}_{}_body_pos_{}".format(c, tag, where)] = gg.npy(bp)
                if where == "origin":
                    arrays["{}_{}_body_rot".format(c, tag)] = gg.npy(br)
            for suffix, MM in (("", M), ("_clip", Mclip)):
                arrays["{}_{}_torque_exp{}".format(c, tag, suffix)] = gg.npy(ig_char_env.IGCharEnv._calc_pd_exp_torque(bare_env(km, MM, cd, ct, dtype)))
                if hinge_only:
                    arrays["{}_{}_torque_1d{}".format(c, tag, suffix)] = gg.npy(ig_char_env.IGCharEnv._calc_pd_1d_torque(bare_env(km, MM, cd, ct, dtype)))
    for k, v in arrays.items():
        assert np.isfinite(v).all(), k


def generate():
    torch.manual_seed(0)
    arrays = {}
    meta = dict(seeds=sr.SEEDS, guard=list(sr.GUARD), reference_guard=list(sr.REF_GUARD), far_pi=sr.FAR_PI, far_angle=sr.FAR_ANGLE,
                clip_side=sr.CLIP_SIDE, clip_guard=sr.CLIP_GUARD, rows=sr.N, share_of_cases_left_out=0.0)
    for c in sr.CHARS:
        gen_char(arrays, meta, c)
    s = sr.scene_struct("syn16")
    assert int(s.num_bodies) == 16
    return arrays, meta


def main():
    check = "--check" in sys.argv[1:]
    arrays, meta = generate()
    npz, js = os.path.join(HERE, "g38_sim_rot.npz"), os.path.join(HERE, "g38_sim_rot.json")
    if check:
        old = np.load(npz)
        diffs = 0
        for k in sorted(set(arrays) | set(old.files)):
            if k not in arrays or k not in old.files or arrays[k].shape != old[k].shape or arrays[k].dtype != old[k].dtype \
                    or not np.array_equal(arrays[k], old[k]):
                print("differs:", k)
                diffs += 1
        if json.load(open(js)) != json.loads(json.dumps(meta)):
            print("differs: the json record")
            diffs += 1
        print("%d differing arrays" % diffs)
        sys.exit(1 if diffs else 0)
    np.savez_compressed(npz, **arrays)
    with open(js, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", npz, os.path.getsize(npz), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
