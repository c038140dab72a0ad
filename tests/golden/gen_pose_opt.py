#!/usr/bin/env python3
"""Generate tests/golden/g34_pose_opt.npz from the REFERENCE's own Python (CPU, torch): util/torch_util.py exp_map_to_quat,
quat_diff_angle and quat_rotate, anim/kin_char_model.py dof_to_rot and forward_kinematics with their autograd.

The frame-to-frame terms are the exception: the reference evaluates smoothness, sliding and jerk inside motion_terrain_contact_loss,
where they cannot be called apart from the terrain and contact terms.  The tt_* arrays are therefore NOT the reference's output: they
are the project's restatement pose_opt_ref.temporal_terms_torch (the expressions of the project's single-motion path) run in torch fp32
and float64 with autograd.  What ties those expressions to the reference is fixture G20 (gen_golden.py stage motion-opt), whose nine
terms and gradient the reference's motion_terrain_contact_loss produced.

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference on
the path.  The inputs are the designed ones of tests/tools/pose_opt_ref.py and tests/tools/moopt_host.py (every branch point of the
kernels visited on both sides); for every case the fixture holds the inputs as fp32, the reference's outputs and autograd gradients
evaluated in fp32, the same evaluated in float64 from the same fp32 inputs (inputs and model tensors cast up), and the cotangents.

  hum_*, syn_*   pose chain, 64 frames, on the shipped humanoid and on the synthetic 16-body tree (pose_opt_ref.synthetic_mjcf); runs
                 "all" (cotangents on all four outputs, both precisions) and one per output (the others zero; float64 only).  The frame whose root map is exactly
                 zero has NaN in the reference's g_root_exp, in both precisions; the fixture records it as it is.
  ang_*, angb_*  angle between rotations: 248 pairs, and 72 pairs against one broadcast q0 (the reference's quat_mul wants equal
                 shapes: q0 is expanded before the call, autograd sums its gradient)
  pts_*          body sample points, a leading batch dimension
  tt_<case>_*    frame-to-frame terms on moopt_host.designed_tt(case), motion by motion: the restatement, see above

The conditions on the inputs are checked here in float64, after the fp32 rounding; a violation is an error, no case is left out.

Where the reference tree's directory does not exist the script prints "reference tree not found" and exits with status 3 before it
imports anything else; any later failure is an error.

usage:  python tests/golden/gen_pose_opt.py            # rewrites tests/golden/g34_pose_opt.npz
        python tests/golden/gen_pose_opt.py --check    # regenerate and compare with the committed fixture
"""
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
import util.torch_util as torch_util  # noqa: E402

import moopt_host as mh  # noqa: E402
import pose_opt_ref as por  # noqa: E402

SEEDS = {"hum": 3410, "syn": 3420}
N_FRAMES = 64


def load_ref_char(name, dtype):
    km = kin_char_model.KinCharModel("cpu")
    if name == "hum":
        km.load_char_file(gg.CHAR_FILE)
    else:
        with tempfile.TemporaryDirectory() as d:
            km.load_char_file(por.write_synthetic(os.path.join(d, "pose_opt_tree.xml")))
    if dtype == torch.float64:                                  # the fp32 model tensors cast up
        km._local_translation = km._local_translation.double()
        km._local_rotation = km._local_rotation.double()
        for j in km._joints:
            if j.axis is not None:
                j.axis = j.axis.double()
    return km


def ref_pose_chain(km, rp, re, dof, cots, dtype):
    x = [gg.t(a, dtype).requires_grad_(True) for a in (rp, re, dof)]
    rq = torch_util.exp_map_to_quat(x[1])
    jr = km.dof_to_rot(x[2])
    bp, br = km.forward_kinematics(x[0], rq, jr)
    outs = dict(zip(por.OUTS, (rq, jr, bp, br)))
    grads = {}
    for run in por.RUNS:
        c = por.run_cotangents(cots, run)
        g = torch.autograd.grad([outs[k] for k in por.OUTS], x, [gg.t(c[k], dtype) for k in por.OUTS], retain_graph=True, allow_unused=True)
        grads[run] = {k: (np.zeros(a.shape, gg.npy(a).dtype) if v is None else gg.npy(v)) for k, v, a in zip(por.INS, g, x)}
    return {k: gg.npy(v) for k, v in outs.items()}, grads


def gen_pose(arrays):
    for name in por.CHARS:
        mine = por.load_char(name)
        ref32 = load_ref_char(name, torch.float32)
        # both loaders read the same tree
        assert ref32._body_names == mine._body_names and ref32._parent_indices.tolist() == mine._parent_indices.tolist()
        assert np.array_equal(gg.npy(ref32._local_translation), gg.npy(mine._local_translation))
        assert np.array_equal(gg.npy(ref32._local_rotation), gg.npy(mine._local_rotation)) and ref32.get_dof_size() == mine.get_dof_size()
        for j in range(1, mine.get_num_joints()):
            a, b = ref32.get_joint(j), mine.get_joint(j)
            assert a.dof_idx == b.dof_idx and a.get_dof_dim() == b.get_dof_dim() and a.joint_type.name == b.joint_type.name
            assert (a.axis is None) == (b.axis is None) and (a.axis is None or np.array_equal(gg.npy(a.axis), gg.npy(b.axis)))
        rp, re, dof = por.pose_chain_inputs(mine, N_FRAMES, SEEDS[name])
        bad = por.pose_conditions(mine, re, dof)
        assert not bad, bad
        cots = por.pose_chain_cotangents(mine, N_FRAMES, SEEDS[name] + 1)
        arrays.update({name + "_root_pos": rp, name + "_root_exp": re, name + "_dof": dof})
        arrays.update({"{}_cot_{}".format(name, k): v for k, v in cots.items()})
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            outs, grads = ref_pose_chain(ref32 if tag == "f32" else load_ref_char(name, dtype), rp, re, dof, cots, dtype)
            for k, v in outs.items():
                assert np.isfinite(v).all()
                arrays["{}_{}_{}".format(name, tag, k)] = v
            for run, g in grads.items():
                for k, v in g.items():
                    finite = np.isfinite(v).all(axis=-1)
                    want = np.ones(N_FRAMES, bool)
                    if k == "root_exp":
                        want[por.ZERO_FRAME] = False               # 0 / 0 through torch.where, whatever the cotangent
                    assert np.array_equal(finite, want), (name, tag, run, k, np.nonzero(finite != want))
                    if tag == "f64" or run == "all":            # the runs on one output alone are recorded in float64 only
                        arrays["{}_{}_{}_g_{}".format(name, tag, run, k)] = v
        print("pose chain {}: {} bodies, {} dofs, {} frames".format(name, mine.get_num_joints(), mine.get_dof_size(), N_FRAMES))


def ref_angle(q0, q1, cot, dtype):
    a, b = gg.t(q0, dtype).requires_grad_(True), gg.t(q1, dtype).requires_grad_(True)
    shape = torch.broadcast_shapes(a.shape, b.shape)
    ang = torch_util.quat_diff_angle(a.expand(shape), b.expand(shape))
    ga, gb = torch.autograd.grad(ang, (a, b), gg.t(cot, dtype))
    return gg.npy(ang), gg.npy(ga), gg.npy(gb)


def gen_angle(arrays):
    z = por.angle_pair_inputs()
    for tag, q0, q1, cot in (("ang", z["q0"], z["q1"], z["cot"]), ("angb", z["bq0"], z["bq1"], z["bcot"])):
        bad = por.angle_conditions(q0, q1)
        assert not bad, bad
        arrays.update({tag + "_q0": q0, tag + "_q1": q1, tag + "_cot": cot})
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            ang, ga, gb = ref_angle(q0, q1, cot, dtype)
            assert np.isfinite(ang).all() and np.isfinite(ga).all() and np.isfinite(gb).all()
            arrays.update({"{}_{}_angle".format(tag, prec): ang, "{}_{}_g_q0".format(tag, prec): ga, "{}_{}_g_q1".format(tag, prec): gb})
    arrays["ang_group"] = z["group"]
    s, w = por.pair_difference(z["q0"], z["q1"])
    exact = z["group"] == 2
    assert (w[exact] == 0.0).all() and (w[z["group"] == 1] < 0).all() and (w[z["group"] == 0] > 0).all()
    dec = por.decade_of(np.concatenate([s, por.pair_difference(z["bq0"], z["bq1"])[0]]))
    print("angle: pairs per decade of |v|", [(dec == k).sum() for k in range(-1, 4)])
    assert all((dec == k).sum() >= 16 for k in range(-1, 4))


def gen_points(arrays):
    z = por.body_points_inputs()
    owner, _ = por.point_tables(z["counts"])
    arrays.update({"pts_" + k: v for k, v in z.items()})
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        pos, rot = gg.t(z["pos"], dtype).requires_grad_(True), gg.t(z["rot"], dtype).requires_grad_(True)
        q = rot[..., owner, :]
        world = torch_util.quat_rotate(q, gg.t(z["local"], dtype).expand(q.shape[:-1] + (3,))) + pos[..., owner, :]
        gp, gr = torch.autograd.grad(world, (pos, rot), gg.t(z["cot"], dtype))
        arrays.update({"pts_{}_world".format(prec): gg.npy(world), "pts_{}_g_body_pos".format(prec): gg.npy(gp), "pts_{}_g_body_rot".format(prec): gg.npy(gr)})


def gen_temporal(arrays):
    for name in mh.DESIGNED_TT:
        case = mh.designed_tt(name)
        gaps = case.jerk_gaps()
        assert ((gaps == 0.0) | (gaps >= 1e-4)).all(), (name, gaps.min())
        arrays.update({"tt_{}_{}".format(name, k): v for k, v in (("lengths", np.array(case.lengths, np.int64)), ("pos", case.pos), ("r", case.r), ("sv", case.sv),
                                                                  ("keep", case.keep), ("pc", case.pc), ("w", case.w), ("lim", np.float64(case.lim)))})
        for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            sums, g_pos, g_r = por.temporal_terms_torch(case, dtype)
            assert np.isfinite(sums).all() and np.isfinite(g_pos).all() and np.isfinite(g_r).all(), name
            arrays.update({"tt_{}_{}_sums".format(name, prec): sums, "tt_{}_{}_g_pos".format(name, prec): g_pos, "tt_{}_{}_g_r".format(name, prec): g_r})
    k = mh.designed_tt("kink")
    assert (k.jerk_gaps() == 0.0).sum() >= 2, "the kink case must sit on the kink"
    z = mh.designed_tt("zero")
    assert (z.jerk_gaps() == 0.0).sum() == 4


def generate():
    torch.manual_seed(0)
    arrays = {}
    gen_pose(arrays)
    gen_angle(arrays)
    gen_points(arrays)
    gen_temporal(arrays)
    return arrays


def main():
    check = "--check" in sys.argv[1:]
    arrays = generate()
    npz = os.path.join(HERE, "g34_pose_opt.npz")
    if check:
        old = np.load(npz)
        diffs = 0
        for k in sorted(set(arrays) | set(old.files)):
            if k not in arrays or k not in old.files or arrays[k].shape != old[k].shape or arrays[k].dtype != old[k].dtype \
                    or not np.array_equal(arrays[k], old[k], equal_nan=arrays[k].dtype.kind == "f"):
                print("differs:", k)
                diffs += 1
        print("%d differing arrays" % diffs)
        sys.exit(1 if diffs else 0)
    np.savez_compressed(npz, **arrays)
    print("wrote", npz, os.path.getsize(npz), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
