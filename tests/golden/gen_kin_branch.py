#!/usr/bin/env python3
"""Generate tests/golden/g37_kin_branch.npz (+ .json: seeds, guards and the guard distances met) from the REFERENCE's own Python (CPU,
torch): util/torch_util.py, anim/kin_char_model.py (dof_to_rot, rot_to_dof, forward_kinematics, compute_frame_dof_vel) and
anim/motion_lib.py (MotionLib: the clip build and calc_motion_frame), in fp32 and in float64, on the designed inputs of
tests/tools/kin_ref.py (every branch point of the tracker's fast kinematics layer visited on both sides).

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference
on the path.  For every case the fixture holds the inputs as fp32, the reference's outputs in fp32 and the same evaluated in float64
from the same fp32 inputs (inputs and model tensors cast up).  Data only.

  <c>_dof, <c>_f32/_f64_joint_rot            dof_to_rot on kin_ref.designed_dofs, c = hum | syn
  <c>_jrot, <c>_jrot_table, .._dof_back       rot_to_dof on kin_ref.designed_joint_rots
  <c>_fk_root_rot, <c>_fk_joint_rot, .._<origin|far>_body_pos, .._origin_body_rot      forward_kinematics, root at the origin and at ROOT_FAR
  <c>_<clip>_frames, .._<key>                 the six designed clips: rows and finite-difference velocities.  fp32: MotionLib's own
                                              arrays; float64: the loader's expressions, function by function, on tensors cast up
                                              (the loader itself builds fp32 tensors only).  The single-frame clip: the loader indexes
                                              frame -2 and stops, in the reference as it stands; its rows come from
                                              _extract_frame_data and its velocities are recorded as zero.
  <c>_q_*                                     the designed queries: MotionLib.calc_motion_frame in fp32 (root_pos, rot = root and
                                              joint rotations, and the velocities it hands through), and slerp / lerp / loop offset in
                                              float64 on the SAME fp32 rows and frame pair, at blend64 (kin_ref.frame_pairs: the blend in
                                              float64 from the same fp32 time); i0, i1, blend, blend64, loop_phase, sine (float64 sin
                                              of slerp's half angle, the bucket of e-bar) and one (fp32 cosine >= 1: fp32 returns q0)
  head_*                                      the root block of compute_char_obs on kin_ref.designed_root_rots, the heading quaternion

The guards are checked here in float64, after the fp32 rounding; a violation is an error, no case is left out.

usage:  python tests/golden/gen_kin_branch.py            # rewrites the fixture
        python tests/golden/gen_kin_branch.py --check    # regenerate and compare with the committed fixture
"""
import json
import os
import pickle
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
import anim.motion_lib as motion_lib  # noqa: E402
import util.torch_util as torch_util  # noqa: E402

import gen_pose_opt as gpo  # noqa: E402  (load_ref_char)
import kin_ref as kr  # noqa: E402
import pose_opt_ref as por  # noqa: E402

F32, F64 = torch.float32, torch.float64
PRECS = (("f32", F32), ("f64", F64))


def gen_pose(arrays, c, mine, ref):
    dof = kr.designed_dofs(mine)
    jrot, table = kr.designed_joint_rots(mine)
    fk_rr, fk_jr = kr.fk_inputs(mine)
    arrays.update({c + "_dof": dof, c + "_jrot": jrot, c + "_jrot_table": table, c + "_fk_root_rot": fk_rr, c + "_fk_joint_rot": fk_jr})
    for tag, dtype in PRECS:
        km = ref[tag]
        with torch.no_grad():
            arrays["{}_{}_joint_rot".format(c, tag)] = gg.npy(km.dof_to_rot(gg.t(dof, dtype)))
            arrays["{}_{}_dof_back".format(c, tag)] = gg.npy(km.rot_to_dof(gg.t(jrot, dtype)))
            for where in ("origin", "far"):
                bp, br = km.forward_kinematics(gg.t(kr.fk_root_pos(len(fk_rr), where), dtype), gg.t(fk_rr, dtype), gg.t(fk_jr, dtype))
                arrays["{}_{}_{}_body_pos".format(c, tag, where)] = gg.npy(bp)
                if where == "origin":               # body rotations do not see the root position
                    arrays["{}_{}_origin_body_rot".format(c, tag)] = gg.npy(br)
                else:
                    assert np.array_equal(gg.npy(br), arrays["{}_{}_origin_body_rot".format(c, tag)])


def ref_clip_build(km, frames, fps, dtype):
    """motion_lib.py:264-290,405-423 with the reference's own functions on tensors of `dtype`"""
    with torch.no_grad():
        fr = gg.t(frames, dtype)
        root_pos, root_exp, joint_dof = motion_lib.extract_pose_data(fr)
        root_pos = root_pos.clone()
        root_rot = torch_util.exp_map_to_quat(root_exp)
        joint_rot = torch_util.quat_pos(km.dof_to_rot(joint_dof))
        root_vel, root_ang_vel = torch.zeros_like(root_pos), torch.zeros_like(root_pos)
        dof_vel = torch.zeros((fr.shape[0], km.get_dof_size()), dtype=dtype)
        if fr.shape[0] >= 2:
            root_vel[:-1] = fps * (root_pos[1:] - root_pos[:-1])
            root_vel[-1] = root_vel[-2]
            root_ang_vel[:-1] = fps * torch_util.quat_to_exp_map(torch_util.quat_diff(root_rot[:-1], root_rot[1:]))
            root_ang_vel[-1] = root_ang_vel[-2]
            dof_vel = km.compute_frame_dof_vel(joint_rot, 1.0 / fps)
    return dict(zip(kr.BUILD_KEYS, (gg.npy(x) for x in (root_pos, root_rot, joint_rot, root_vel, root_ang_vel, dof_vel))))


def gen_clips(arrays, meta, c, mine, ref):
    clips = kr.designed_clips(mine)
    with tempfile.TemporaryDirectory() as d:
        entries = []
        for name, fr, fps, loop in list(zip(kr.CLIP_NAMES, clips, kr.CLIP_FPS, kr.CLIP_LOOP))[1:]:
            p = os.path.join(d, "{}_{}.pkl".format(c, name))
            with open(p, "wb") as f:
                pickle.dump({"fps": fps, "loop_mode": motion_lib.LoopMode(loop).name, "frames": fr}, f)
            entries.append("- {{file: {}, weight: 1.0}}".format(p))
        yp = os.path.join(d, "motions.yaml")
        with open(yp, "w") as f:
            f.write("motions:\n" + "\n".join(entries) + "\n")
        ml = motion_lib.MotionLib(yp, ref["f32"], "cpu")
    start = ml._motion_start_idx.tolist()
    own = dict(root_pos=ml._frame_root_pos, root_rot=ml._frame_root_rot, joint_rot=ml._frame_joint_rot, root_vel=ml._frame_root_vel,
               root_ang_vel=ml._frame_root_ang_vel, dof_vel=ml._frame_dof_vel)
    for i, (name, fr, fps) in enumerate(zip(kr.CLIP_NAMES, clips, kr.CLIP_FPS)):
        arrays["{}_{}_frames".format(c, name)] = fr
        for tag, dtype in PRECS:
            b = ref_clip_build(ref[tag], fr, fps, dtype)
            if tag == "f32" and i > 0:              # the loader's own arrays, which the expressions above must equal bit for bit
                for k in kr.BUILD_KEYS:
                    mine_k = gg.npy(own[k][start[i - 1]:start[i - 1] + fr.shape[0]])
                    assert np.array_equal(mine_k, b[k]), (c, name, k)
            for k in kr.BUILD_KEYS:
                assert np.isfinite(b[k]).all()
                arrays["{}_{}_{}_{}".format(c, name, tag, k)] = b[k]
    # queries: fp32 from calc_motion_frame, float64 on the same fp32 rows
    ids, times = kr.designed_queries(clips)
    nf = [fr.shape[0] for fr in clips]
    i0, i1, blend, loop_phase, blend64 = kr.frame_pairs(ids, times, nf, kr.CLIP_FPS, kr.CLIP_LOOP)
    rows = [{k: arrays["{}_{}_f32_{}".format(c, name, k)] for k in kr.BUILD_KEYS} for name in kr.CLIP_NAMES]
    rot = [np.concatenate([r["root_rot"][:, None], r["joint_rot"]], axis=1) for r in rows]
    rot0, rot1 = np.stack([rot[m][a] for m, a in zip(ids, i0)]), np.stack([rot[m][a] for m, a in zip(ids, i1)])
    pos0, pos1 = np.stack([rows[m]["root_pos"][a] for m, a in zip(ids, i0)]), np.stack([rows[m]["root_pos"][a] for m, a in zip(ids, i1)])
    delta = np.stack([(clips[m][-1, 0:3] - clips[m][0, 0:3]) * np.array([1, 1, 0], np.float32) for m in ids]).astype(np.float32)
    live = ids > 0
    with torch.no_grad():
        out = ml.calc_motion_frame(torch.tensor(ids[live] - 1), torch.tensor(times[live]))
    a0, a1, ab = ml._calc_frame_blend(torch.tensor(ids[live] - 1), torch.tensor(times[live]))
    st = np.array(start)[ids[live] - 1]
    assert np.array_equal(gg.npy(a0) - st, i0[live]) and np.array_equal(gg.npy(a1) - st, i1[live]) and np.array_equal(gg.npy(ab), blend[live])
    assert np.array_equal(gg.npy(ml._motion_root_pos_delta)[ids[live] - 1], delta[live])
    q32, p32 = kr.frame_blend(rot0, rot1, pos0, pos1, blend, loop_phase, delta, dtype=F32)
    # the single-frame clip's queries are not the loader's (it cannot hold the clip): the restatement stands in, and has to equal the
    # loader on every other query up to the rounding of the project's port (another order of operations in no function used here)
    assert np.array_equal(q32[live][:, 0], gg.npy(out[1])) and np.array_equal(q32[live][:, 1:], gg.npy(out[4])), c
    assert np.array_equal(p32[live], gg.npy(out[0])), c
    for k, col in (("root_vel", 2), ("root_ang_vel", 3), ("dof_vel", 5)):
        assert np.array_equal(gg.npy(out[col]), np.stack([rows[m][k][a] for m, a in zip(ids[live], i0[live])]))
    with torch.no_grad():
        t = gg.t(blend64, F64)
        q64 = gg.npy(torch_util.slerp(gg.t(rot0, F64), gg.t(rot1, F64), t.reshape(-1, 1, 1).expand(-1, rot0.shape[1], 1)))
        off = gg.t(loop_phase, F64).unsqueeze(-1) * gg.t(delta, F64)
        p64 = gg.npy((1.0 - t.unsqueeze(-1)) * gg.t(pos0, F64) + t.unsqueeze(-1) * gg.t(pos1, F64) + off)
    _, sine, cosine = kr.pair_measures(rot0, rot1)
    # the pairs whose fp32 cosine is >= 1: the reference's fp32 returns q0 there, bit for bit, and its own sum gives the same cosine
    one = kr.cosine_fp32(rot0, rot1) >= 1.0
    assert np.array_equal(kr.cosine_fp32(rot0, rot1), np.abs(gg.npy(torch.sum(gg.t(rot0) * gg.t(rot1), dim=-1))))
    assert np.array_equal(q32[one].view(np.uint32), rot0[one].view(np.uint32)) and (sine[one] < kr.SLERP_GUARD[0]).all()
    differ = one & ~(rot0.view(np.uint32) == rot1.view(np.uint32)).all(axis=-1)
    meta[c + "_slerp_pairs_cos_one_not_identical"] = int(differ.sum())
    meta[c + "_slerp_pairs_average"] = int((~one & (sine < 1e-3)).sum())
    assert differ.sum() >= 50 and meta[c + "_slerp_pairs_average"] >= 20
    arrays.update({c + "_q_ids": ids, c + "_q_times": times, c + "_q_i0": i0, c + "_q_i1": i1, c + "_q_blend": blend, c + "_q_blend64": blend64, c + "_q_loop_phase": loop_phase,
                   c + "_q_f32_rot": q32, c + "_q_f64_rot": q64, c + "_q_f32_root_pos": p32, c + "_q_f64_root_pos": p64, c + "_q_sine": sine, c + "_q_one": one})
    dec = np.where(one, -1, kr.slerp_decade(sine))
    meta[c + "_slerp_pairs_per_decade"] = [int((dec == k).sum()) for k in range(len(kr.SLERP_DECADES))]
    meta[c + "_slerp_pairs_cos_negative"] = int((cosine < 0).sum())
    assert all(n >= 10 for n in meta[c + "_slerp_pairs_per_decade"]) and meta[c + "_slerp_pairs_cos_negative"] >= 5
    # guard distances met by the stored fp32 rows
    v = np.concatenate([kr.pair_measures(r[:-1], r[1:])[0].ravel() for r in rot if r.shape[0] > 1])
    s = np.concatenate([kr.pair_measures(r[:-1], r[1:])[1].ravel() for r in rot if r.shape[0] > 1])
    assert not [b for r in rot for b in kr.rows_conditions(r)]
    meta[c + "_pairs_below_threshold"] = int((v < kr.THRESHOLD).sum())
    meta[c + "_closest_to_threshold"] = [float(v[v < kr.THRESHOLD].max()), float(v[v > kr.THRESHOLD].min())]
    meta[c + "_closest_to_slerp_sine"] = [float(s[s < 1e-3].max()), float(s[s > 1e-3].min())]


def gen_heading(arrays, meta):
    q = kr.designed_root_rots()
    vel, ang = kr.root_velocities(len(q))
    assert not kr.heading_conditions(q)
    arrays.update({"head_rot": q, "head_vel": vel, "head_ang_vel": ang})
    for tag, dtype in PRECS:
        with torch.no_grad():
            qt, v, w = gg.t(q, dtype), gg.t(vel, dtype), gg.t(ang, dtype)
            h = torch_util.calc_heading_quat_inv(qt)
            block = torch.cat([torch_util.quat_to_tan_norm(torch_util.quat_mul(h, qt)), torch_util.quat_rotate(h, v), torch_util.quat_rotate(h, w)], dim=-1)
        arrays["head_{}_hinv".format(tag)] = gg.npy(h)
        arrays["head_{}_block".format(tag)] = gg.npy(block)
    meta["heading_min_horizontal_length"] = float(kr.horizontal_length(q).min())


def generate():
    torch.manual_seed(0)
    arrays, meta = {}, dict(seeds=kr.SEEDS, guard=list(kr.GUARD), far_pi=kr.FAR_PI, slerp_guard=list(kr.SLERP_GUARD),
                            min_horizontal=kr.MIN_HORIZONTAL, min_axis_dot=kr.MIN_AXIS_DOT, share_of_cases_left_out=0.0)
    for c in kr.CHARS:
        mine = kr.load_char(c)
        ref = {"f32": gpo.load_ref_char(c, F32), "f64": gpo.load_ref_char(c, F64)}
        assert ref["f32"]._body_names == mine._body_names and np.array_equal(gg.npy(ref["f32"]._local_rotation), gg.npy(mine._local_rotation))
        gen_pose(arrays, c, mine, ref)
        gen_clips(arrays, meta, c, mine, ref)
        w = por.wrapped(np.linalg.norm(kr.sph_maps(mine, arrays[c + "_dof"]), axis=-1))
        meta[c + "_dof_closest_to_pi"] = float(np.abs(w - kr.PI).min())
        meta[c + "_dof_closest_to_threshold"] = [float(w[(w < kr.THRESHOLD)].max()), float(w[w > kr.THRESHOLD].min())]
    gen_heading(arrays, meta)
    return arrays, meta


def main():
    check = "--check" in sys.argv[1:]
    arrays, meta = generate()
    npz, js = os.path.join(HERE, "g37_kin_branch.npz"), os.path.join(HERE, "g37_kin_branch.json")
    if check:
        old = np.load(npz)
        diffs = 0
        for k in sorted(set(arrays) | set(old.files)):
            if k not in arrays or k not in old.files or arrays[k].shape != old[k].shape or arrays[k].dtype != old[k].dtype \
                    or not np.array_equal(arrays[k], old[k], equal_nan=arrays[k].dtype.kind == "f"):
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
