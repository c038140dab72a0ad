"""tests/tools/kin_ref.py pinned without a GPU: it is the yardstick of tests/test_kin_branch_gpu.py, so its float64 functions have to
equal the float64 record of fixture G37 (the reference's own classes), its fp32 run has to reproduce the fixture's fp32 record, its
designed inputs have to be the fixture's and to meet their guards, and its e-bars have to be the fixture's.  The C oracle, which the
GPU heading test leans on through oracle.compute_obs, is held to 2 e-bar of float64 on the same designed inputs."""
import ast
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import kin_ref as kr  # noqa: E402
import pose_opt_ref as por  # noqa: E402

ORACLE_FACTOR = 2.0


@pytest.fixture(scope="module")
def z():
    return golden("g37_kin_branch")


@pytest.fixture(scope="module")
def chars():
    return {c: kr.load_char(c) for c in kr.CHARS}


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == np.float64 and b.dtype == np.float64, what
    err = np.abs(a - b).max() if a.size else 0.0
    tol = 1e-12 * max(1.0, np.abs(b).max() if b.size else 0.0)
    assert err <= tol, (what, err, tol)


def _within(got, ref, bound, what):
    err = kr.value_error(got, np.asarray(ref, np.float64))
    print("{:44s} err {:.3e}  bound {:.3e}".format(what, err, bound))
    assert np.shape(got) == np.shape(ref) and err <= bound, (what, err, bound)


def _rot(z, c, name, tag):
    return np.concatenate([z["{}_{}_{}_root_rot".format(c, name, tag)][:, None], z["{}_{}_{}_joint_rot".format(c, name, tag)]], axis=1)


def _query_pairs(z, c, tag="f32"):
    """the frame pairs of the fixture's queries, taken from its rows of precision `tag`"""
    ids, i0, i1 = z[c + "_q_ids"], z[c + "_q_i0"], z[c + "_q_i1"]
    rot = [_rot(z, c, name, tag) for name in kr.CLIP_NAMES]
    pos = [z["{}_{}_{}_root_pos".format(c, name, tag)] for name in kr.CLIP_NAMES]
    fr = [z["{}_{}_frames".format(c, name)] for name in kr.CLIP_NAMES]
    delta = np.stack([(fr[m][-1, 0:3] - fr[m][0, 0:3]) * np.array([1, 1, 0], np.float32) for m in ids]).astype(np.float32)
    return (np.stack([rot[m][a] for m, a in zip(ids, i0)]), np.stack([rot[m][a] for m, a in zip(ids, i1)]),
            np.stack([pos[m][a] for m, a in zip(ids, i0)]), np.stack([pos[m][a] for m, a in zip(ids, i1)]), delta)


def test_designed_inputs_are_the_fixtures_and_meet_their_guards(z, chars):
    meta = json.load(open(os.path.join(REPO, "tests", "golden", "g37_kin_branch.json")))
    assert meta["share_of_cases_left_out"] == 0.0 and tuple(meta["guard"]) == kr.GUARD and tuple(meta["slerp_guard"]) == kr.SLERP_GUARD
    for c in kr.CHARS:
        km = chars[c]
        dof = kr.designed_dofs(km)
        assert dof.dtype == np.float32 and dof.shape[0] == kr.N_POSES and np.array_equal(dof, z[c + "_dof"])
        assert kr.sph_conditions(kr.sph_maps(km, dof)) == []
        assert np.array_equal(kr.designed_dofs(km, 17), dof[:17])                       # a prefix of the list
        raw = kr._raw_angles(km, dof)
        sph, hin = [j - 1 for j in por.spherical_joints(km)], [j - 1 for j in por.hinge_joints(km)]
        for k, a in enumerate(kr.ANGLES):                                               # every angle on every joint, hinges with both signs
            for r in (k, len(kr.ANGLES) + k):
                assert np.abs(raw[r][sph] - a).max() < 1e-6 and np.abs(raw[r][hin] - a).max() < 1e-6
            hd = np.array([dof[k, km.get_joint_dof_idx(j + 1)] for j in hin])
            hd2 = np.array([dof[len(kr.ANGLES) + k, km.get_joint_dof_idx(j + 1)] for j in hin])
            assert (hd > 0).any() and (hd < 0).any() and np.array_equal(hd, -hd2)
        assert not dof[kr.DOF_ZERO_ROW].any()
        extra = raw[kr.DOF_ZERO_ROW + 1:kr.N_DOF_DESIGNED]
        assert sorted(set(np.round(extra[:, hin[0]], 3))) == sorted(round(a, 3) for a in kr.HINGE_EXTRA)
        assert sorted(set(np.round(extra[:, sph[0]], 2))) == [50.0, 300.0]
        w = por.wrapped(raw[:, sph])
        assert (w < kr.THRESHOLD).sum() >= 2 * len(sph) and ((w > kr.THRESHOLD) & (w < 3e-5)).sum() >= 6 * len(sph)
        assert kr.far_joints(km, dof).sum() == 12 * len(sph) + 4 * len(hin) and (raw[kr.N_DOF_DESIGNED:] < kr.FAR_ANGLE).all()
        # joint quaternions
        jrot, table = kr.designed_joint_rots(km)
        assert np.array_equal(jrot, z[c + "_jrot"]) and np.array_equal(table, z[c + "_jrot_table"], equal_nan=True)
        assert kr.joint_rot_conditions(km, jrot) == []
        designed = ~np.isnan(table[:, 0])
        assert designed.sum() == 62 and (table[designed, 2] < 0).sum() == 31 and {0.5, 1.0, 2.0} == set(table[designed, 1])
        v = np.linalg.norm(jrot[:, sph[0], :3].astype(np.float64), axis=1)
        assert (v[designed] == 0).sum() == 6 and (v < kr.GUARD[0]).sum() >= 20 and (jrot[designed][:, sph[0], 3] == 0).sum() == 6
        # a scale that crosses the threshold: 0.7e-5 at scale 1 lies below it, at scale 2 above
        cross = designed & (table[:, 0] == 0.7e-5)
        assert (v[cross & (table[:, 1] == 1.0)] < kr.THRESHOLD).all() and (v[cross & (table[:, 1] == 2.0)] > kr.THRESHOLD).all()
        for h in hin:                                                                   # every tilt on every hinge, both signs of the dot product
            ax = kr._hinge_axis(km, h + 1, torch.float64).numpy()
            s = np.linalg.norm(jrot[:, h, :3].astype(np.float64), axis=1)
            live = designed & (s > kr.THRESHOLD)
            cosines = (jrot[live][:, h, :3].astype(np.float64) / s[live, None]) @ (ax / np.linalg.norm(ax)) * table[live, 2]
            assert {-1.0, -0.5, 0.5, 1.0} == set(np.round(cosines, 3))
        rr, jr = kr.fk_inputs(km)
        assert np.array_equal(rr, z[c + "_fk_root_rot"]) and np.array_equal(jr, z[c + "_fk_joint_rot"])
        # clips
        clips = kr.designed_clips(km)
        assert len(clips) == len(kr.CLIP_NAMES) == 6 and [f.shape[0] for f in clips] == [1, 2, 12, 12, kr.EDGE_FRAMES, kr.EDGE_FRAMES]
        assert sorted(zip(kr.CLIP_FPS[2:], kr.CLIP_LOOP[2:])) == [(30.0, 0), (30.0, 1), (120.0, 0), (120.0, 1)]
        for name, fr in zip(kr.CLIP_NAMES, clips):
            assert np.array_equal(fr, z["{}_{}_frames".format(c, name)]) and kr.clip_conditions(km, fr) == []
        sj, hj = kr.designed_joints(km)
        for name in ("ladder30", "ladder120"):
            rot = _rot(z, c, name, "f64")
            _, sine, _ = kr.pair_measures(rot[:-1], rot[1:])
            for k, h in enumerate(kr.LADDER):
                assert np.abs(np.arcsin(sine[k, [0, sj, hj]]) - h).max() <= 2e-7, (name, k)
        for name in ("edges30", "edges120"):
            rot = _rot(z, c, name, "f64")
            v, _, cosine = kr.pair_measures(rot[:-1], rot[1:])
            e = np.linalg.norm(z["{}_{}_frames".format(c, name)][:, 3:6].astype(np.float64), axis=1)
            assert abs(e[1] - (kr.PI - 1e-2)) < 1e-6 and abs(e[2] - (kr.PI + 1e-2)) < 1e-6 and cosine[1, 0] < -0.99
            assert np.abs(v[1, [sj, hj]] - 0.5e-5).max() < 2e-7 and np.abs(v[2, [0, sj, hj]] - 2e-5).max() < 2e-7 and abs(v[3, 0] - 0.5e-5) < 2e-7
            assert (v[3, 1:] < 1e-12).all()
        ids, times = kr.designed_queries(clips)
        assert np.array_equal(ids, z[c + "_q_ids"]) and np.array_equal(times, z[c + "_q_times"])
        i0, i1, blend, lp, b64 = kr.frame_pairs(ids, times, [f.shape[0] for f in clips], kr.CLIP_FPS, kr.CLIP_LOOP)
        assert all(np.array_equal(a, z[c + k]) for a, k in ((i0, "_q_i0"), (i1, "_q_i1"), (blend, "_q_blend"), (lp, "_q_loop_phase"), (b64, "_q_blend64")))
        assert np.abs(b64 - blend).max() <= 2.0 ** -20 and np.abs(b64 - blend).max() > 0          # within an ulp of the frame number
        assert (blend == 0).sum() >= 6 and (lp == 1).sum() == 3 and (lp == 2).sum() == 3 and ((i0 == i1) & (ids > 0)).sum() >= 2
        for b in kr.BLENDS[1:]:
            assert (np.abs(blend - b) < 2e-5).sum() >= 20, b
        dec = np.where(z[c + "_q_one"], -1, kr.slerp_decade(z[c + "_q_sine"]))
        assert all((dec == k).sum() >= 10 for k in range(4))
    q = kr.designed_root_rots()
    assert np.array_equal(q, z["head_rot"]) and kr.heading_conditions(q) == [] and q.shape == (64, 4)
    assert np.array_equal(q[kr.N_HEADING_DESIGNED - 1], [0, 0, 1, 0]) and np.array_equal(q[kr.N_HEADING_DESIGNED - 2], [0, 0, 0, 1])
    head = np.arctan2(2.0 * (q[:, 3] * q[:, 2] + q[:, 0] * q[:, 1]).astype(np.float64), 1.0 - 2.0 * (q[:, 1].astype(np.float64) ** 2 + q[:, 2].astype(np.float64) ** 2))
    for k, h in enumerate(kr.HEADINGS):
        want = np.arctan2(np.sin(h), np.cos(h))
        assert np.abs(head[3 * k:3 * k + 3] - want).max() < 1e-6, h
    vel, ang = kr.root_velocities(64)
    assert np.array_equal(vel, z["head_vel"]) and np.array_equal(ang, z["head_ang_vel"])


def test_module_equals_the_references_float64_record(z, chars):
    for c in kr.CHARS:
        km = chars[c]
        _same(kr.dof_to_rot(km, z[c + "_dof"]), z[c + "_f64_joint_rot"], c + " dof_to_rot")
        _same(kr.rot_to_dof(km, z[c + "_jrot"]), z[c + "_f64_dof_back"], c + " rot_to_dof")
        for where in ("origin", "far"):
            bp, br = kr.forward_kinematics(km, kr.fk_root_pos(64, where), z[c + "_fk_root_rot"], z[c + "_fk_joint_rot"])
            _same(bp, z["{}_f64_{}_body_pos".format(c, where)], c + " body_pos " + where)
            _same(br, z[c + "_f64_origin_body_rot"], c + " body_rot " + where)
        for name, fps in zip(kr.CLIP_NAMES, kr.CLIP_FPS):
            b = kr.clip_build(km, z["{}_{}_frames".format(c, name)], fps)
            for k in kr.BUILD_KEYS:
                _same(b[k], z["{}_{}_f64_{}".format(c, name, k)], "{} {} {}".format(c, name, k))
        rot0, rot1, pos0, pos1, delta = _query_pairs(z, c)
        q, p = kr.frame_blend(rot0, rot1, pos0, pos1, z[c + "_q_blend64"], z[c + "_q_loop_phase"], delta)
        _same(q, z[c + "_q_f64_rot"], c + " slerp")
        _same(p, z[c + "_q_f64_root_pos"], c + " root_pos")
        _, sine, _ = kr.pair_measures(rot0, rot1)
        one = kr.cosine_fp32(rot0, rot1) >= 1.0
        assert np.array_equal(sine, z[c + "_q_sine"]) and np.array_equal(one, z[c + "_q_one"])
        # where the fp32 cosine is >= 1 the reference's fp32 returned q0, also on pairs that are not identical (the 2e-4 rungs)
        differ = one & ~(rot0.view(np.uint32) == rot1.view(np.uint32)).all(axis=-1)
        assert differ.sum() >= 50 and np.array_equal(z[c + "_q_f32_rot"][one].view(np.uint32), rot0[one].view(np.uint32))
    _same(kr.root_block(z["head_rot"], z["head_vel"], z["head_ang_vel"]), z["head_f64_block"], "root block")
    _same(kr.heading_quat_inv(z["head_rot"]), z["head_f64_hinv"], "heading quaternion")


def test_fp32_run_reproduces_the_references_fp32_record(z, chars):
    """the ports round in another order than the reference (the 16-product quaternion product, x / 2 for 0.5 x): two fp32 evaluations,
    each e-bar from float64, are within 2 e-bar of each other; the frame blend, where the order is the reference's, reproduces it bit for bit"""
    f32 = torch.float32
    M = lambda d: {k: (M(v) if isinstance(v, dict) else 2.0 * v) for k, v in d.items()}     # noqa: E731
    for c in kr.CHARS:
        km = chars[c]
        got = kr.dof_to_rot(km, z[c + "_dof"], f32)
        far = kr.far_joints(km, z[c + "_dof"])
        err = np.abs(got.astype(np.float64) - z[c + "_f32_joint_rot"]).max(axis=-1)
        assert got.dtype == np.float32 and err[~far].max() <= 2 * kr.MEASURED_DOF_TO_ROT["near"] and err[far].max() <= 2 * kr.MEASURED_DOF_TO_ROT["far"]
        _within(kr.rot_to_dof(km, z[c + "_jrot"], f32), z[c + "_f32_dof_back"], 2 * kr.MEASURED_ROT_TO_DOF, c + " rot_to_dof")
        for where in ("origin", "far"):
            bp, br = kr.forward_kinematics(km, kr.fk_root_pos(64, where), z[c + "_fk_root_rot"], z[c + "_fk_joint_rot"], f32)
            _within(bp, z["{}_f32_{}_body_pos".format(c, where)], M(kr.MEASURED_FK)[where]["body_pos"], c + " body_pos " + where)
            _within(br, z[c + "_f32_origin_body_rot"], M(kr.MEASURED_FK)[where]["body_rot"], c + " body_rot " + where)
        for name, fps in zip(kr.CLIP_NAMES, kr.CLIP_FPS):
            b = kr.clip_build(km, z["{}_{}_frames".format(c, name)], fps, f32)
            assert np.array_equal(b["root_pos"], z["{}_{}_f32_root_pos".format(c, name)])
            for k in ("root_rot", "joint_rot"):
                _within(b[k], z["{}_{}_f32_{}".format(c, name, k)], 2 * kr.MEASURED_BUILD_ROWS[k], "{} {} {}".format(c, name, k))
            for k in ("root_vel", "root_ang_vel", "dof_vel"):
                _within(b[k], z["{}_{}_f32_{}".format(c, name, k)], 2 * kr.MEASURED_BUILD_VEL[int(fps)][k], "{} {} {}".format(c, name, k))
        rot0, rot1, pos0, pos1, delta = _query_pairs(z, c)
        q, p = kr.frame_blend(rot0, rot1, pos0, pos1, z[c + "_q_blend"], z[c + "_q_loop_phase"], delta, f32)
        assert np.array_equal(q, z[c + "_q_f32_rot"]) and np.array_equal(p, z[c + "_q_f32_root_pos"])
    _within(kr.root_block(z["head_rot"], z["head_vel"], z["head_ang_vel"], f32), z["head_f32_block"], 2 * kr.MEASURED_ROOT_BLOCK, "root block")


def _oracle_char(orc, km):
    B = km.get_num_joints()
    axis = np.zeros((B, 3), np.float32)
    for b in range(1, B):
        if km.get_joint(b).axis is not None:
            axis[b] = km.get_joint(b).axis.numpy()
    return orc.Char(km._parent_indices.numpy(), km._local_translation.numpy(), km._local_rotation.numpy(),
                    [km._joints[b].joint_type.value for b in range(B)], axis, [km._joints[b].dof_idx for b in range(B)])


def test_c_oracle_at_the_designed_inputs(z, chars, oracle):
    K = ORACLE_FACTOR
    for c in kr.CHARS:
        km = chars[c]
        oc = _oracle_char(oracle, km)
        got = oracle.dof_to_rot(oc, z[c + "_dof"])
        far = kr.far_joints(km, z[c + "_dof"])
        err = np.abs(got.astype(np.float64) - z[c + "_f64_joint_rot"]).max(axis=-1)
        print("{} oracle dof_to_rot near {:.3e} far {:.3e}".format(c, err[~far].max(), err[far].max()))
        assert err[~far].max() <= K * kr.MEASURED_DOF_TO_ROT["near"] and err[far].max() <= K * kr.MEASURED_DOF_TO_ROT["far"]
        assert ((got.astype(np.float64) * z[c + "_f64_joint_rot"]).sum(-1) > 0.99).all()
        _within(oracle.rot_to_dof(oc, z[c + "_jrot"]), z[c + "_f64_dof_back"], K * kr.MEASURED_ROT_TO_DOF, c + " oracle rot_to_dof")
        for where in ("origin", "far"):
            bp, br = oracle.forward_kinematics(oc, kr.fk_root_pos(64, where), z[c + "_fk_root_rot"], z[c + "_fk_joint_rot"])
            _within(bp, z["{}_f64_{}_body_pos".format(c, where)], K * kr.MEASURED_FK[where]["body_pos"], c + " oracle body_pos " + where)
            _within(br, z[c + "_f64_origin_body_rot"], K * kr.MEASURED_FK[where]["body_rot"], c + " oracle body_rot " + where)
        rot0, rot1, _, _, _ = _query_pairs(z, c)
        Q, B = rot0.shape[:2]
        t = np.repeat(z[c + "_q_blend"], B)
        got = oracle.slerp(rot0.reshape(-1, 4), rot1.reshape(-1, 4), t).reshape(Q, B, 4)
        one = z[c + "_q_one"]
        assert np.array_equal(got[one].view(np.uint32), rot0[one].view(np.uint32))           # the exact branch: the bits of q0
        err = kr.slerp_error_by_decade(got, z[c + "_q_f64_rot"], z[c + "_q_sine"], one)
        print("{} oracle slerp per decade {}".format(c, " ".join("%.3e" % e for e in err)))
        assert (err <= K * np.array(kr.MEASURED_SLERP_DECADE)).all(), err
    got = oracle.calc_heading_quat_inv(z["head_rot"])
    err = kr.signless_error(got, z["head_f64_hinv"])
    print("oracle heading quaternion {:.3e}  bound {:.3e}".format(err, K * kr.MEASURED_HEADING_QUAT))
    assert err <= K * kr.MEASURED_HEADING_QUAT
    # its rotation, which is all the observation takes from it: the root block built on the oracle's heading quaternion
    q64, h64 = z["head_rot"].astype(np.float64), got.astype(np.float64)
    block = np.concatenate([_np64(kr.torch_util.quat_to_tan_norm(kr.torch_util.quat_mul(torch.tensor(h64), torch.tensor(q64)))),
                            _np64(kr.torch_util.quat_rotate(torch.tensor(h64), torch.tensor(z["head_vel"].astype(np.float64)))),
                            _np64(kr.torch_util.quat_rotate(torch.tensor(h64), torch.tensor(z["head_ang_vel"].astype(np.float64))))], axis=-1)
    _within(block, z["head_f64_block"], K * kr.MEASURED_ROOT_BLOCK, "root block on the oracle's heading")


def _np64(x):
    return x.numpy()


def test_measured_e_bars_are_the_fixtures(z):
    m = kr.measure(z)
    pairs = [(m["dof_to_rot"][k], kr.MEASURED_DOF_TO_ROT[k], "dof_to_rot " + k) for k in ("near", "far")]
    pairs += [(m["rot_to_dof"], kr.MEASURED_ROT_TO_DOF, "rot_to_dof"), (m["root_pos"], kr.MEASURED_ROOT_POS, "root_pos"),
              (m["root_block"], kr.MEASURED_ROOT_BLOCK, "root block"), (m["heading_quat"], kr.MEASURED_HEADING_QUAT, "heading quaternion")]
    pairs += [(m["fk"][w][k], kr.MEASURED_FK[w][k], "fk {} {}".format(w, k)) for w in ("origin", "far") for k in ("body_pos", "body_rot")]
    pairs += [(m["build_rows"][k], kr.MEASURED_BUILD_ROWS[k], "build " + k) for k in kr.MEASURED_BUILD_ROWS]
    pairs += [(m["build_vel"][f][k], kr.MEASURED_BUILD_VEL[f][k], "build {} fps {}".format(k, f)) for f in (30, 120) for k in kr.MEASURED_BUILD_VEL[f]]
    pairs += [(m["slerp"][k], kr.MEASURED_SLERP_DECADE[k], "slerp decade %d" % k) for k in range(4)]
    for got, const, what in pairs:
        print("{:32s} measured {:.4e} constant {:.4e}".format(what, got, const))
        assert got > 0 and got <= const <= 1.011 * got, (what, got, const)          # the constant is the figure rounded up to 3 digits
    # what the script prints is what the module holds
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "tools", "kin_ref.py")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    printed = {k.strip(): ast.literal_eval(v.strip()) for k, v in (line.split("=", 1) for line in res.stdout.splitlines() if line.startswith("MEASURED_"))}
    assert len(printed) == 9 and all(getattr(kr, k) == v for k, v in printed.items()), printed


def test_generator_check_regenerates_the_fixture():
    """gen_kin_branch.py --check: the reference's own classes give the committed fixture again, 0 differing arrays.  The generator needs
    the reference's Python; where that tree does not exist the test is skipped and says so - decided here, before the generator runs,
    so that any failure of the generator is a failure of the test."""
    import mdm_loss_ref as mlr
    root = mlr.reference_root()
    if not os.path.isdir(root):
        pytest.skip("the reference tree ({}) is not on this machine: the fixture generator cannot run".format(root))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "gen_kin_branch.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0 and "0 differing arrays" in res.stdout, (res.returncode, res.stdout[-2000:] + res.stderr[-2000:])
    assert os.path.getsize(kr.FIXTURE) < os.path.getsize(os.path.join(REPO, "tests", "golden", "g34_pose_opt.npz"))
