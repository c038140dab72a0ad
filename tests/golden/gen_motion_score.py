#!/usr/bin/env python3
"""Generate tests/golden/g28_motion_score.npz from the REFERENCE's own tools/procgen/mdm_path.compute_motion_loss (CPU, torch).

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference
on the path.  Inputs: frames 150-155 of the civilization clip over the slice of its terrain around them, and the body sample points of
fixture G20 (308 points).  Candidates: the clip as it is, lowered 4 cm (feet in the ground), raised 10 cm (no penetration at all),
lowered 1 m, shifted 3 cells past the +x edge of the field, and the clip with all contacts 0.  The reference scores one candidate
length per call, so it is called once per candidate and length (6, 3 and 1 frames), at weights 1.

usage:  python tests/golden/gen_motion_score.py            # rewrites tests/golden/g28_motion_score.npz
        python tests/golden/gen_motion_score.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util.motion_util as motion_util  # noqa: E402
import util.terrain_util as terrain_util  # noqa: E402

F0, F1 = 150, 156
LENGTHS = (6, 3, 1)
NAMES = ("as_is", "lowered_4cm", "raised_10cm", "lowered_1m", "off_edge", "no_contacts")


def main():
    for n in ("diffusion", "diffusion.diffusion_util", "diffusion.mdm", "diffusion.gen_util"):      # the generator: imported, never called here
        if n not in sys.modules:
            gg._stub(n)
    sys.modules["diffusion.mdm"].MDM = object
    sys.modules["diffusion.gen_util"].MDMGenSettings = object
    import tools.procgen.mdm_path as mdm_path
    out = tempfile.mkdtemp(prefix="parc_g28_check_") if "--check" in sys.argv else HERE
    torch.manual_seed(28)
    km = gg.load_char()
    g20 = np.load(os.path.join(HERE, "g20_motion_opt.npz"))
    counts = g20["pts_count"].astype(np.int64)
    pts_flat = g20["pts"].astype(np.float32)
    pts = [gg.t(p) for p in np.split(pts_flat, np.cumsum(counts)[:-1])]
    assert len(pts) == km.get_num_joints() and pts_flat.shape[0] == 308
    civ = gg.load_motion_file_safe(os.path.join(gg.REF, "data/terrains/civilization.pkl"))
    frames = gg.t(np.asarray(civ["frames"], np.float32)[F0:F1].copy())
    contacts = np.asarray(civ["contacts"], np.float32)[F0:F1].copy()
    ter, src = terrain_util.slice_terrain_around_motion(frames, gg.ref_terrain_from_dict(civ["terrain"]), padding=0.8)
    X, Y = int(ter.hf.shape[0]), int(ter.hf.shape[1])
    print("terrain slice", X, "x", Y, "dxdy", ter.dxdy.tolist(), "min", ter.min_point.tolist())
    cands, cons = [], []
    for name in NAMES:
        f = src.clone()
        c = contacts.copy()
        if name == "lowered_4cm":
            f[:, 2] -= 0.04
        elif name == "raised_10cm":
            f[:, 2] += 0.10
        elif name == "lowered_1m":
            f[:, 2] -= 1.0
        elif name == "off_edge":
            edge = ter.min_point[0] + (X - 1) * ter.dxdy[0]
            f[:, 0] += (edge + 3.0 * ter.dxdy[0]) - f[:, 0].max()
        elif name == "no_contacts":
            c[:] = 0.0
        cands.append(f)
        cons.append(gg.t(c))
    mfs = [motion_util.motion_frames_from_mlib_format(f, km, contacts=c) for f, c in zip(cands, cons)]
    losses = np.zeros((len(NAMES), len(LENGTHS), 3), np.float32)
    for i, mf in enumerate(mfs):
        for j, n in enumerate(LENGTHS):
            one = mf.get_copy("cpu")
            one = motion_util.MotionFrames(root_pos=one.root_pos[None, :n], root_rot=one.root_rot[None, :n], joint_rot=one.joint_rot[None, :n],
                                           contacts=one.contacts[None, :n])
            r = mdm_path.compute_motion_loss(one, None, ter, km, pts, w_contact=1.0, w_pen=1.0, w_path=1.0, verbose=False)
            losses[i, j] = [float(r["total_loss"]), float(r["contact_loss"]), float(r["pen_loss"])]
        print(NAMES[i], losses[i].tolist())
    arrs = dict(names=np.array(",".join(NAMES)), lengths=np.array(LENGTHS, np.int32), pts=pts_flat, pts_count=counts,
                root_pos=torch.stack([m.root_pos for m in mfs]), root_rot=torch.stack([m.root_rot for m in mfs]),
                joint_rot=torch.stack([m.joint_rot for m in mfs]), contacts=torch.stack(cons), hf=ter.hf, min_point=ter.min_point, dxdy=ter.dxdy,
                losses=losses)
    dst = os.path.join(out, "g28_motion_score.npz")
    np.savez_compressed(dst, **{k: gg.npy(v) for k, v in arrs.items()})
    print("wrote", dst, os.path.getsize(dst), "bytes")
    if "--check" in sys.argv:
        a, b = np.load(dst), np.load(os.path.join(HERE, "g28_motion_score.npz"))
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
