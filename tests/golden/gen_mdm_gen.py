#!/usr/bin/env python3
"""Generate tests/golden/g36_mdm_gen.npz (+ .json) from the REFERENCE's own gen_mdm_motion (diffusion/gen_util.py; CPU, torch fp32,
verbose=False), called on an MDM object made without building the transformer (gen_mdm_loss.make_mdm) whose `ddim_inference` is replaced
by a function that records the `conds` it receives and returns a seeded [B, S, D] sample.  So the fixture holds what the reference hands
to its sampling loop and what it makes of the loop's result: every conds tensor and the final MotionFrames.

Runs ONLY in the build container (needs the reference tree).  The previous frames are windows of the clips committed with fixture G32,
turned about z by a seeded yaw and moved onto a seeded terrain (96 x 80 cells of 0.2 m: steps of 5 cm on a tilted plane, one tower and
one pit beyond max_h so that the normalised heights clamp); the sample is the reference's assemble_mdm_features of a window of the same
clip plus seeded noise; feature statistics are the seeded draws of gen_mdm_loss.  `frames` (the rows a MotionLib takes) is
cat(root_pos, quat_to_exp_map(root_rot), rot_to_dof(joint_rot)) of the returned MotionFrames by the reference's own functions, as its
envs/ig_parkour/mgdm_env.py builds it.

Feature-mode cases (tests/golden/g36_mdm_gen.json holds their configurations):
  shipped      B=3 T=2 P=2 S=16  31 x 31 at 0.2 m   use_prev_state a tensor [True, False, True]; target guidance on (records the target)
  edge_7x9     B=2 T=3 P=2 S=5   7 x 9 at 0.4 m     characters within 1 m of the terrain's corner (part of the grid is clamped); the
                                                    second one faces |heading| > 3
  pair         B=1 T=1 P=1 S=2   7 x 9              the smallest shape
  no_pos_con   B=2 T=2 P=2 S=3   7 x 9              components ROOT_POS, ROOT_ROT, JOINT_ROT.  The reference's gen_mdm_motion reads
                                                    mdm_ret[CONTACTS] unconditionally and raises KeyError for this layout; the generator
                                                    lets extract_motion_features add a zero CONTACTS entry and records no contacts
  zero_target  B=2 T=2 P=2 S=3   7 x 9              the first target equals canon_xy; target guidance on
One component-mode case, over the same object with `gen_sequence_with_contacts` replaced by a function that records its conds (the
component dictionary of gen_util.py:139-145 and the raw heights) and returns seeded components:
  components   B=2 T=2 P=2 S=4   7 x 9

A case's seed is the first one, counting up from the listed one, under which the preconditions hold under the float64 restatement
(tests/mdm_gen_ref.preconditions: every quaternion's vector part and w at least 1e-3 from the exponential map's branch points,
|heading| <= pi - 1e-2, all grid indices below 128 in magnitude, at most 0.5 % of the cells within 2e-4 cells of a rounding boundary);
the fixture records it.  The bounds are not loosened, and 100 tries per case must do.

Where the reference tree's directory does not exist the script prints "reference tree not found" and exits with status 3 before it
imports anything else; any later failure is an error.

usage:  python tests/golden/gen_mdm_gen.py            # rewrites tests/golden/g36_mdm_gen.npz and .json
        python tests/golden/gen_mdm_gen.py --check    # regenerate and compare with the committed fixture
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import mdm_gen_ref as mgn  # noqa: E402  (tests/mdm_gen_ref.py: the float64 restatement)
import mdm_loss_ref as mlr  # noqa: E402

if not os.path.isdir(mlr.reference_root()):          # decided before any work; every failure after this line is a failure
    print("reference tree not found:", mlr.reference_root())
    sys.exit(3)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)
import gen_mdm_loss as gml  # noqa: E402  (make_mdm, draw_inputs, true_dict: the pattern of fixture G33)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import anim.kin_char_model as kin_char_model  # noqa: E402
import diffusion.gen_util as ref_gen  # noqa: E402
import util.terrain_util as terrain_util  # noqa: E402
import util.torch_util as torch_util  # noqa: E402
from diffusion.diffusion_util import MDMFrameType, MDMKeyType, RelativeZStyle  # noqa: E402
from util.motion_util import MotionFrames  # noqa: E402

ALL = gml.ALL
G79 = (3, 3, 4, 4)
TERRAIN = dict(dims=(96, 80), dxdy=0.2, min_point=(-3.1, -2.7), seed=36)


def make_case(name, seed, windows, T, P, S, grid=G79, dx=0.4, components=ALL, mode="feature", use_prev_state=True, target_guidance=False,
              place="inside"):
    return dict(name=name, seed=seed, windows=windows, T=T, num_prev_states=P, S=S, grid=list(grid), dx=dx, components=list(components), fps=30,
                max_h=3.0, noise=0.08, mode=mode, use_prev_state=use_prev_state, target_guidance=target_guidance, place=place,
                z_style="RELATIVE_TO_ROOT")


CASES = [make_case("shipped", 100, [[0, 2], [0, 20], [1, 5]], 2, 2, 16, grid=(10, 20, 15, 15), dx=0.2, use_prev_state=[True, False, True],
                   target_guidance=True),
         make_case("edge_7x9", 200, [[0, 9], [2, 4]], 3, 2, 5, place="corner"),
         make_case("pair", 300, [[1, 12]], 1, 1, 2),
         make_case("no_pos_con", 400, [[0, 30], [3, 2]], 2, 2, 3, components=["ROOT_POS", "ROOT_ROT", "JOINT_ROT"]),
         make_case("zero_target", 500, [[0, 14], [2, 8]], 2, 2, 3, target_guidance=True),
         make_case("components", 600, [[1, 8], [2, 1]], 2, 2, 4, mode="components")]


def make_terrain():
    rng = np.random.default_rng(TERRAIN["seed"])
    X, Y = TERRAIN["dims"]
    gx, gy = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    hf = 0.004 * gx - 0.003 * gy + np.round(rng.uniform(-0.4, 0.4, size=(X, Y)) * 20) / 20
    hf[30:34, 40:44] = 4.5          # above root + max_h and below root - max_h: the normalised heights clamp there
    hf[60:63, 20:24] = -3.5
    return hf.astype(np.float32)


def loss_like(case):
    """the keys gen_mdm_loss.make_mdm and draw_inputs read"""
    c = dict(case)
    c.update(weights={}, target_dir_len_eps=0.0, use_pos_loss=False, use_hf_collision_loss=False, use_target_loss=False, rot_type="DEFAULT")
    return c


def qz(yaw):
    return np.array([0.0, 0.0, math.sin(yaw / 2), math.cos(yaw / 2)])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def draw_prev_frames(case, seed, hf):
    """the previous frames of every sample: T frames of its clip from t0, turned by a seeded yaw and put on a seeded place"""
    rng = np.random.default_rng(seed + 36000)
    z = np.load(mlr.G32)
    T, c = case["T"], case["num_prev_states"] - 1
    X, Y = TERRAIN["dims"]
    d, (mx, my) = TERRAIN["dxdy"], TERRAIN["min_point"]
    out = {k: [] for k in ("root_pos", "root_rot", "joint_rot", "contacts", "target_world")}
    for b, (clip, t0) in enumerate(case["windows"]):
        rp = z["c%d_root_pos" % clip][t0:t0 + T].astype(np.float64)
        rr = z["c%d_root_rot" % clip][t0:t0 + T].astype(np.float64)
        q = rr[c]
        clip_heading = math.atan2(2 * (q[3] * q[2] + q[0] * q[1]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]))
        want = rng.uniform(-3.0, 3.0)
        if case["place"] == "corner" and b == 1:
            want = rng.choice([-1.0, 1.0]) * rng.uniform(3.02, 3.12)
        yaw = want - clip_heading
        if case["place"] == "corner":          # within 1 m of the terrain's far corner (first sample) and near corner (second)
            corner = np.array([mx + (X - 1) * d, my + (Y - 1) * d]) if b == 0 else np.array([mx, my])
            place = corner + rng.uniform(0.1, 0.7, size=2) * (-1.0 if b == 0 else 1.0)
        else:
            place = np.array([mx + rng.uniform(5.0, (X - 1) * d - 5.0), my + rng.uniform(5.0, (Y - 1) * d - 5.0)])
        cs, sn = math.cos(yaw), math.sin(yaw)
        xy = rp[:, :2] - rp[c, :2]
        rp = np.concatenate([np.stack([xy[:, 0] * cs - xy[:, 1] * sn, xy[:, 0] * sn + xy[:, 1] * cs], -1) + place, rp[:, 2:]], -1)
        out["root_pos"].append(rp)
        out["root_rot"].append(qmul(qz(yaw), rr))
        out["joint_rot"].append(z["c%d_joint_rot" % clip][t0:t0 + T])
        out["contacts"].append(z["c%d_contacts" % clip][t0:t0 + T])
        out["target_world"].append(place + rng.uniform(-3.0, 3.0, size=2))
    out = {k: np.stack(v).astype(np.float32) for k, v in out.items()}
    if case["name"] == "zero_target":
        out["target_world"][0] = out["root_pos"][0, c, :2]
    return out


def run_case(km, model, case, seed, hf):
    n = case["name"]
    lc = loss_like(case)
    B, S, P = len(case["windows"]), case["S"], case["num_prev_states"]
    D = gml.make_mdm(km, lc, None, None)._motion_frame_dof
    d = gml.draw_inputs(lc, seed, D)
    m = gml.make_mdm(km, lc, gg.t(d["mean"]), gg.t(d["std"]))
    m._denoise_model = torch.nn.Identity()
    m._use_heightmap_obs, m._use_target_obs, m._use_feature_vector = True, True, False
    m._relative_z_style, m._seq_len = RelativeZStyle.RELATIVE_TO_ROOT, S
    with torch.no_grad():
        x = (m.assemble_mdm_features(gml.true_dict(km, lc)) + gg.t(d["noise"])).clone()
    prev = draw_prev_frames(case, seed, hf)
    ups = np.array(case["use_prev_state"] if isinstance(case["use_prev_state"], list) else [case["use_prev_state"]] * B, dtype=bool)
    out = {n + "_prev_" + k: prev[k] for k in ("root_pos", "root_rot", "joint_rot", "contacts")}
    out.update({n + "_target_world": prev["target_world"], n + "_mean": d["mean"], n + "_std": d["std"], n + "_x": gg.npy(x), n + "_use_prev_state": ups})
    X, Y = TERRAIN["dims"]
    terrain = terrain_util.SubTerrain("g36", X, Y, TERRAIN["dxdy"], TERRAIN["dxdy"], TERRAIN["min_point"][0], TERRAIN["min_point"][1], device="cpu")
    terrain.hf[:] = gg.t(hf)
    settings = ref_gen.MDMGenSettings()
    settings.use_prev_state = gg.t(ups, torch.bool) if isinstance(case["use_prev_state"], list) else case["use_prev_state"]
    settings.target_guidance = case["target_guidance"]
    frames_in = MotionFrames(root_pos=gg.t(prev["root_pos"]), root_rot=gg.t(prev["root_rot"]), joint_rot=gg.t(prev["joint_rot"]),
                             contacts=gg.t(prev["contacts"]))
    rec = {}
    if case["mode"] == "feature":
        def ddim_inference(conds, stride):
            rec.update({k: v for k, v in conds.items()})
            return x.clone()
        m.ddim_inference = ddim_inference
        if "CONTACTS" not in case["components"]:
            extract = m.extract_motion_features

            def with_contacts(feats, **kw):
                r = extract(feats, **kw)
                r.setdefault(MDMFrameType.CONTACTS, torch.zeros(feats.shape[0], feats.shape[1], km.get_num_joints()))
                return r
            m.extract_motion_features = with_contacts
    else:
        def gen_sequence_with_contacts(conds, ddim_stride=None, mode=None):
            rec.update({k: v for k, v in conds.items()})
            return m.extract_motion_features(x.clone())
        m.gen_sequence_with_contacts = gen_sequence_with_contacts
    with torch.no_grad():
        ret = ref_gen.gen_mdm_motion(gg.t(prev["target_world"]), frames_in, terrain, m, km, settings, verbose=False)
        rows = torch.cat([ret.root_pos, torch_util.quat_to_exp_map(ret.root_rot), km.rot_to_dof(ret.joint_rot)], dim=-1)
    K = MDMKeyType
    flags = np.stack([gg.npy(rec[k]).astype(bool) for k in (K.OBS_FLAG_KEY, K.PREV_STATE_NOISE_IND_KEY, K.TARGET_FLAG_KEY, K.PREV_STATE_FLAG_KEY)])
    out.update({n + "_flags": flags, n + "_target_dir": gg.npy(rec[K.TARGET_KEY])})
    if case["mode"] == "feature":
        out.update({n + "_obs": gg.npy(rec[K.OBS_KEY]), n + "_prev_state": gg.npy(rec[K.PREV_STATE_KEY])})
    else:
        ps = rec[K.PREV_STATE_KEY]
        out.update({n + "_hf_z": gg.npy(rec[K.OBS_KEY]), n + "_canon_root_pos": gg.npy(ps[MDMFrameType.ROOT_POS]),
                    n + "_canon_root_rot": gg.npy(ps[MDMFrameType.ROOT_ROT]), n + "_canon_body_pos": gg.npy(ps[MDMFrameType.JOINT_POS])})
    gp = rec.get(K.GUIDANCE_PARAMS)
    assert gp is not None and gp.obs_cfg_scale == settings.cfg_scale
    if case["target_guidance"]:
        out[n + "_target"] = gg.npy(gp.target_xy)
    out.update({n + "_out_root_pos": gg.npy(ret.root_pos), n + "_out_root_rot": gg.npy(ret.root_rot), n + "_out_joint_rot": gg.npy(ret.joint_rot),
                n + "_out_frames": gg.npy(rows)})
    if "CONTACTS" in case["components"]:
        out[n + "_out_contacts"] = gg.npy(ret.contacts)
    assert all(np.isfinite(v).all() for v in out.values()), "non-finite value in case " + n
    diag = {}
    zz = dict(out)
    zz.update(terrain_hf=hf, terrain_min_point=np.array(TERRAIN["min_point"], np.float32), terrain_dxdy=np.array([TERRAIN["dxdy"]] * 2, np.float32))

    class Z(dict):
        files = property(lambda self: list(self.keys()))
    mgn.case_eval(model, case, Z(zz), diag=diag)
    return out, diag


def generate(first_seed=None):
    """first_seed: case name -> the seed to begin with (--check begins with the recorded one: the seeds before it were judged when the
    fixture was written)"""
    torch.manual_seed(0)
    km = kin_char_model.KinCharModel(torch.device("cpu"))
    km.load_char_file(gg.CHAR_FILE)
    nb = km.get_num_joints()
    joints = [None] + [km.get_joint(j) for j in range(1, nb)]
    model = dict(nb=nb, parent=[int(p) for p in km._parent_indices.tolist()],
                 kind=[0] + [{0: 0, 1: mlr.HINGE, 3: mlr.SPHERICAL}[j.get_dof_dim()] for j in joints[1:]],
                 first=[0] + [int(j.dof_idx) for j in joints[1:]],
                 axis=np.stack([np.zeros(3)] + [np.zeros(3) if j.axis is None else j.axis.double().numpy().reshape(3) for j in joints[1:]]),
                 lt=km._local_translation.double().numpy(), lr=km._local_rotation.double().numpy(), dof_size=int(km.get_dof_size()))
    hf = make_terrain()
    arrays = dict(terrain_hf=hf, terrain_min_point=np.array(TERRAIN["min_point"], np.float32), terrain_dxdy=np.array([TERRAIN["dxdy"]] * 2, np.float32))
    meta = dict(cases=[], terrain=dict(TERRAIN, dims=list(TERRAIN["dims"]), min_point=list(TERRAIN["min_point"])))
    for case in CASES:
        seed = case["seed"] if first_seed is None else first_seed[case["name"]]
        while True:
            out, diag = run_case(km, model, case, seed, hf)
            bad = mgn.preconditions(diag, case)
            if not bad:
                break
            print("case %s seed %d: %s" % (case["name"], seed, "; ".join(bad)))
            seed += 1
            assert seed < case["seed"] + 100, "no seed meets the preconditions of case " + case["name"]
        c = dict(case)
        c["seed_used"] = seed
        meta["cases"].append(c)
        arrays.update(out)
        print("case %-12s seed %d  |heading| %.3f  max index %.1f  near a boundary %.4f  min |v| %.1e |w| %.1e" % (
            case["name"], seed, diag["max_abs_heading"], diag["max_abs_index"], diag["near_share"], diag["min_vec"], diag["min_w"]))
    return arrays, meta


def main():
    check = "--check" in sys.argv[1:]
    if check:
        old, old_meta = mgn.load_fixture()
        arrays, meta = generate({c["name"]: c["seed_used"] for c in old_meta["cases"]})
    else:
        arrays, meta = generate()
    if check:
        diffs = 0 if old_meta == json.loads(json.dumps(meta)) else 1
        for k in sorted(set(arrays) | set(old.files)):
            if k not in arrays or k not in old.files or arrays[k].shape != old[k].shape or not np.array_equal(arrays[k], old[k]):
                print("differs:", k)
                diffs += 1
        print("%d differences" % diffs)
        sys.exit(1 if diffs else 0)
    np.savez_compressed(mgn.G36, **arrays)
    with open(mgn.G36_JSON, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", mgn.G36, os.path.getsize(mgn.G36), "bytes")


if __name__ == "__main__":
    main()
