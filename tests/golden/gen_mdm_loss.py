#!/usr/bin/env python3
"""Generate tests/golden/g33_mdm_loss.npz (+ .json) from the REFERENCE's own MDM.assemble_mdm_features, extract_motion_features,
motion_difference and compute_point_hf_sdf (CPU, torch fp32), called on an MDM object made without building the transformer
(object.__new__ plus the attributes those methods read).

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference on
the path.  True windows are frames of the clips committed with fixture G32 (tests/mdm_loss_ref.true_windows); the prediction is
assemble(true) + seeded noise; heightfields, feature statistics, target directions and the ood mask are seeded draws.  Per case the
fixture records the inputs, the standardised true features, the quaternions extract_motion_features gives for the prediction, every loss
term [B], and predicted_x_0.grad of the trainer's reduction (mean over the batch, summed over the terms) without and with the ood mask.

Cases (tests/golden/g33_mdm_loss.json holds their configurations):
  1 l2_7x9       B=5 S=5 num_prev_states 2, grid 7 x 9 (a transposed index shows), squared_l2
  2 huber_7x9    the same with pseudo_huber
  3 shipped      B=3 S=16, the shipped 31 x 31 grid at 0.2 m, the weights of PARC/train_gen_default.yaml
  4 pair         B=1 S=2 num_prev_states 1: one velocity pair, the target term reads frames 0 and 1
  5 no_pos       components ROOT_POS, ROOT_ROT, JOINT_ROT only, use_pos_loss false
  6 no_hf_tgt    use_hf_collision_loss false, use_target_loss false
and, listed apart as "rot_cases" (the torch path alone takes them; e-bar is measured over the six above):
  rot_exp_map    B=2 S=3, rot_type EXP_MAP, squared_l2            rot_quat    B=2 S=3, rot_type QUAT, pseudo_huber

A case's seed is the first one, counting up from the listed one, under which the preconditions hold under the float64 restatement
(tests/mdm_loss_ref.py); the fixture records it.  Preconditions: every quaternion fed to quat_to_axis_angle has vector part >= 1e-3 and
|w| >= 1e-3 (the constant fixed-joint pairs excepted); every predicted exponential-map norm lies in [1e-3, pi - 1e-3]; every sample
point has |sdf| >= 1e-4; for every penetrating point the runner-up column is at least 1e-5 further than the best; in each case with
the terrain term between 10 % and 90 % of the points penetrate; no sample's target term is within 1e-3 of the clamp's kink, and over
the fixture the clamp is active for at least one sample and inactive for at least one.  If a seed violates one, the next seed is tried
- the bounds are not loosened.

Where the reference tree's directory does not exist the script prints "reference tree not found" and exits with status 3 before it
imports anything else; any later failure is an error.

usage:  python tests/golden/gen_mdm_loss.py            # rewrites tests/golden/g33_mdm_loss.npz and .json
        python tests/golden/gen_mdm_loss.py --check    # regenerate and compare with the committed fixture
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

sys.path.insert(0, os.path.dirname(HERE))
import mdm_loss_ref as mlr  # noqa: E402  (tests/mdm_loss_ref.py: the float64 restatement)

if not os.path.isdir(mlr.reference_root()):          # decided before any work; every failure after this line is a failure
    print("reference tree not found:", mlr.reference_root())
    sys.exit(3)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import anim.kin_char_model as kin_char_model  # noqa: E402
import diffusion.mdm as ref_mdm  # noqa: E402
import diffusion.utils.rot_changer as rot_changer  # noqa: E402
import util.geom_util as geom_util  # noqa: E402
from diffusion.diffusion_util import MDMFrameType, MDMKeyType  # noqa: E402

TEST_WEIGHTS = dict(w_simple_root_pos=1.0, w_simple_root_rot=0.9, w_simple_joint_rot=0.5, w_simple_contacts=0.8, w_simple_body_pos=0.6,
                    w_body_pos_consistency=1.1, w_vel_root_pos=0.05, w_vel_root_rot=0.02, w_vel_joint_rot=0.01, w_body_pos=0.7, w_body_rot=0.3,
                    w_body_vel=0.03, w_hf=4.0, w_target=0.5, w_floor_height=5.0, w_foot_contact=0.2)
# PARC/train_gen_default.yaml
DEFAULT_WEIGHTS = dict(w_simple_root_pos=1.0, w_simple_root_rot=1.0, w_simple_joint_rot=0.5, w_simple_contacts=1.0, w_simple_body_pos=0.5,
                       w_body_pos_consistency=1.0, w_vel_root_pos=0.5, w_vel_root_rot=0.02, w_vel_joint_rot=0.01, w_body_pos=0.5, w_body_rot=0.1,
                       w_body_vel=0.03, w_foot_contact=0.2, w_target=0.02, w_hf=15.0, w_floor_height=5.0)
ALL = ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"]


def make_case(name, seed, windows, S, num_prev, grid, dx, loss_fn="squared_l2", weights=TEST_WEIGHTS, components=ALL, use_pos=True, use_hf=True,
              use_tgt=True, rot_type="DEFAULT"):
    return dict(rot_type=rot_type, name=name, seed=seed, windows=windows, S=S, num_prev_states=num_prev, grid=list(grid), dx=dx, loss_fn=loss_fn, weights=dict(weights),
                components=list(components), use_pos_loss=use_pos, use_hf_collision_loss=use_hf, use_target_loss=use_tgt, fps=30, max_h=3.0,
                target_dir_len_eps=0.1, noise=0.08)


W5 = [[0, 3], [0, 21], [1, 8], [2, 6], [3, 11]]
CASES = [make_case("l2_7x9", 100, W5, 5, 2, (3, 3, 4, 4), 0.4),
         make_case("huber_7x9", 200, W5, 5, 2, (3, 3, 4, 4), 0.4, loss_fn="pseudo_huber"),
         make_case("shipped", 300, [[0, 2], [0, 20], [1, 5]], 16, 2, (10, 20, 15, 15), 0.2, weights=DEFAULT_WEIGHTS),
         make_case("pair", 400, [[1, 12]], 2, 1, (3, 3, 4, 4), 0.4),
         make_case("no_pos", 500, [[0, 9], [2, 4]], 5, 2, (3, 3, 4, 4), 0.4, components=["ROOT_POS", "ROOT_ROT", "JOINT_ROT"], use_pos=False),
         make_case("no_hf_tgt", 600, [[0, 30], [3, 2]], 5, 2, (3, 3, 4, 4), 0.4, use_hf=False, use_tgt=False)]


# rot_types the device path does not take: the torch path alone is compared with these (kept apart from CASES: e-bar is CASES')
ROT_CASES = [make_case("rot_exp_map", 700, [[0, 12], [1, 3]], 3, 2, (3, 3, 4, 4), 0.4, rot_type="EXP_MAP"),
             make_case("rot_quat", 800, [[0, 26], [2, 9]], 3, 2, (3, 3, 4, 4), 0.4, loss_fn="pseudo_huber", rot_type="QUAT")]


def load_char():
    km = kin_char_model.KinCharModel("cpu")
    km.load_char_file(gg.CHAR_FILE)
    return km


def make_mdm(km, case, mean, std):
    """an MDM with the attributes assemble / extract / motion_difference / compute_point_hf_sdf read, and no network"""
    m = object.__new__(ref_mdm.MDM)
    m._device = "cpu"
    m._kin_char_model = km
    m._sequence_fps = case["fps"]
    m._num_prev_states = case["num_prev_states"]
    for k, v in case["weights"].items():
        setattr(m, "_" + k, v)
    m._target_dir_len_eps = case["target_dir_len_eps"]
    m._use_simple_loss, m._use_vel_loss = True, True
    m._use_pos_loss, m._use_hf_collision_loss, m._use_target_loss = case["use_pos_loss"], case["use_hf_collision_loss"], case["use_target_loss"]
    m._target_type = ref_mdm.TargetType.XY_DIR
    m._rot_changer = rot_changer.RotChanger(rot_changer.RotationType[case["rot_type"]], km)
    m._register_mdm_features(case["components"])
    xn, xp, yn, yp = case["grid"]
    m._dx = m._dy = case["dx"]
    m._dxdy = torch.tensor([m._dx, m._dy], dtype=torch.float32)
    m._num_x_neg, m._num_x_pos, m._num_y_neg, m._num_y_pos = xn, xp, yn, yp
    m._max_h = case["max_h"]
    m._min_h = -m._max_h
    m._mdm_features_mean, m._mdm_features_std = mean, std
    if m._use_hf_collision_loss:
        m.init_char_point_samples()
    return m


def draw_inputs(case, seed, D):
    """everything seeded of a case: feature statistics, noise, heightfields (normalised), target directions, ood mask"""
    rng = np.random.default_rng(seed)
    B, S = len(case["windows"]), case["S"]
    xn, xp, yn, yp = case["grid"]
    X, Y = 1 + xn + xp, 1 + yn + yp
    mean = (0.2 * rng.standard_normal((S, D))).astype(np.float32)
    std = rng.uniform(0.5, 1.5, size=(S, D)).astype(np.float32)
    # no element closer than 0.03 to the true feature: a hinge whose predicted angle equals the true one is a singular pair
    g = rng.standard_normal((B, S, D))
    noise = (np.sign(g) * (0.03 + case["noise"] * np.abs(g))).astype(np.float32)
    # terrain around the height of the lower body: a tilted plane plus steps, so a good share of the sample points is inside the ground
    gx, gy = np.meshgrid(np.arange(X) - xn, np.arange(Y) - yn, indexing="ij")
    hf = np.stack([0.45 + 0.25 * rng.standard_normal() + case["dx"] * (rng.uniform(-0.5, 0.5) * gx + rng.uniform(-0.5, 0.5) * gy)
                   + np.round(rng.uniform(-0.5, 0.5, size=(X, Y)), 1) for _ in range(B)]).astype(np.float32)
    hfs = (np.clip(hf, -case["max_h"], case["max_h"]) / np.float32(case["max_h"])).astype(np.float32).reshape(B, 1, X, Y)
    ang = rng.uniform(0, 2 * np.pi, size=B)
    td = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32).reshape(B, 1, 2)
    if B > 2:
        td[B - 1] = 0.0            # standing still
    ood = rng.uniform(size=B) < 0.4
    ood[0] = True
    return dict(mean=mean, std=std, noise=noise, hfs=hfs, target_dir=td, ood_mask=ood)


def true_dict(km, case):
    tw = mlr.true_windows(case)
    t = {MDMFrameType.ROOT_POS: gg.t(tw["ROOT_POS"]), MDMFrameType.ROOT_ROT: gg.t(tw["ROOT_ROT"]), MDMFrameType.JOINT_ROT: gg.t(tw["JOINT_ROT"])}
    if "CONTACTS" in case["components"]:
        t[MDMFrameType.CONTACTS] = gg.t(tw["CONTACTS"])
    if "JOINT_POS" in case["components"]:
        bp, _ = km.forward_kinematics(t[MDMFrameType.ROOT_POS], t[MDMFrameType.ROOT_ROT], t[MDMFrameType.JOINT_ROT])
        t[MDMFrameType.JOINT_POS] = bp[..., 1:, :].clone()
    return t


def preconditions(diag, case):
    bad = []
    if not (diag["min_vec"] >= 1e-3 and diag["min_w"] >= 1e-3):
        bad.append("quaternion near a singular input: |v| %.2e |w| %.2e" % (diag["min_vec"], diag["min_w"]))
    lo, hi = diag.get("min_exp", math.inf), diag.get("max_exp", 0.0)          # rot_type QUAT has no exponential map
    if not (lo >= 1e-3 and hi <= math.pi - 1e-3):
        bad.append("exp-map norm outside [1e-3, pi - 1e-3]: %.3e .. %.3e" % (lo, hi))
    if case["use_hf_collision_loss"]:
        if not diag["min_abs_sdf"] >= 1e-4:
            bad.append("|sdf| %.2e" % diag["min_abs_sdf"])
        if not diag.get("min_gap", math.inf) >= 1e-5:
            bad.append("runner-up column %.2e" % diag["min_gap"])
        if not 0.1 <= diag["frac_inside"] <= 0.9:
            bad.append("penetrating share %.2f" % diag["frac_inside"])
    if case["use_target_loss"] and min(abs(v) for v in diag["target_raw_plus_eps"]) < 1e-3:
        bad.append("target term at the kink")
    return bad


def run_case(km, model, case, seed):
    """-> (arrays, diag) of the reference under `seed`"""
    T = MDMFrameType
    true = true_dict(km, case)
    probe = make_mdm(km, case, None, None)
    D = probe._motion_frame_dof
    d = draw_inputs(case, seed, D)
    m = make_mdm(km, case, gg.t(d["mean"]), gg.t(d["std"]))
    loss_fn = {"squared_l2": ref_mdm.squared_l2_loss_fn, "pseudo_huber": ref_mdm.pseudo_huber_loss_fn}[case["loss_fn"]]
    with torch.no_grad():
        x_true = m.assemble_mdm_features(true)
    x = (x_true + gg.t(d["noise"])).clone()
    conds = {MDMKeyType.OBS_KEY: gg.t(d["hfs"]), MDMKeyType.TARGET_KEY: gg.t(d["target_dir"])}
    ood = torch.tensor(d["ood_mask"])
    n = case["name"]
    out = {n + "_" + k: v for k, v in d.items() if k != "noise"}
    out[n + "_x_true"] = gg.npy(x_true)
    out[n + "_x"] = gg.npy(x)
    for tag, mask in (("grad", None), ("grad_ood", ood)):
        xr = x.clone().requires_grad_(True)
        pred = m.extract_motion_features(xr)
        losses = m.motion_difference(true, pred, conds, loss_fn)
        if mask is None:
            out[n + "_keys"] = np.array([k.name for k in losses])
            for k, v in losses.items():
                out[n + "_loss_" + k.name] = gg.npy(v.detach())
            out[n + "_pred_root_rot"] = gg.npy(pred[T.ROOT_ROT].detach())
            out[n + "_pred_joint_rot"] = gg.npy(pred[T.JOINT_ROT].detach())
        else:
            for k in losses:                                    # mdm.py:936-940
                if k == ref_mdm.LossType.HF_COLLISION_LOSS or k == ref_mdm.LossType.TARGET_LOSS:
                    continue
                losses[k][mask] *= 0.0
        total = 0.0
        for k in losses:                                        # mdm.py:953-958
            total += losses[k].mean()
        total.backward()
        out[n + "_" + tag] = gg.npy(xr.grad)
    assert all(np.isfinite(v).all() for k, v in out.items() if v.dtype.kind == "f"), "non-finite value in case " + n
    # the preconditions, judged by the float64 restatement on the same inputs
    diag = {}
    z = dict(out)
    if case["use_hf_collision_loss"]:
        pts = m._char_point_samples
        z["points"], z["point_counts"] = np.concatenate([gg.npy(p) for p in pts]), np.array([p.shape[0] for p in pts])
    else:
        z["points"], z["point_counts"] = np.zeros((0, 3), np.float32), np.zeros(15, np.int64)
    mlr.case_eval(model, case, z, with_grad=False, diag=diag)
    return out, diag


def generate():
    torch.manual_seed(0)
    km = load_char()
    nb = km.get_num_joints()
    joints = [None] + [km.get_joint(j) for j in range(1, nb)]
    model = dict(nb=nb, parent=[int(p) for p in km._parent_indices.tolist()],
                 kind=[0] + [{0: 0, 1: mlr.HINGE, 3: mlr.SPHERICAL}[j.get_dof_dim()] for j in joints[1:]],
                 first=[0] + [int(j.dof_idx) for j in joints[1:]],
                 axis=np.stack([np.zeros(3)] + [np.zeros(3) if j.axis is None else j.axis.double().numpy().reshape(3) for j in joints[1:]]),
                 lt=km._local_translation.double().numpy(), lr=km._local_rotation.double().numpy(), dof_size=int(km.get_dof_size()))
    arrays, meta = {}, dict(cases=[])
    pts = geom_util.get_minimal_char_point_samples(km)
    arrays["points"] = np.concatenate([gg.npy(p) for p in pts]).astype(np.float32)
    arrays["point_counts"] = np.array([p.shape[0] for p in pts], np.int64)
    raws = []
    meta["rot_cases"] = []
    for case in CASES + ROT_CASES:
        seed = case["seed"]
        while True:
            out, diag = run_case(km, model, case, seed)
            bad = preconditions(diag, case)
            if not bad:
                break
            print("case %s seed %d: %s" % (case["name"], seed, "; ".join(bad)))
            seed += 1
            assert seed < case["seed"] + 100, "no seed meets the preconditions of case " + case["name"]
        c = dict(case)
        c["seed_used"] = seed
        meta["rot_cases" if case in ROT_CASES else "cases"].append(c)
        arrays.update(out)
        raws += diag.get("target_raw_plus_eps", [])
        print("case %-10s seed %d  inside %.2f  min|sdf| %.1e  gap %.1e  |v| %.1e  exp %.2f..%.2f" % (
            case["name"], seed, diag.get("frac_inside", float("nan")), diag.get("min_abs_sdf", float("nan")), diag.get("min_gap", float("nan")),
            diag["min_vec"], diag.get("min_exp", float("nan")), diag.get("max_exp", float("nan"))))
    assert any(v < 0 for v in raws) and any(v > 0 for v in raws), "the target clamp must be active for one sample and inactive for another"
    return arrays, meta


def main():
    check = "--check" in sys.argv[1:]
    arrays, meta = generate()
    npz, js = os.path.join(HERE, "g33_mdm_loss.npz"), os.path.join(HERE, "g33_mdm_loss.json")
    if check:
        old = np.load(npz)
        with open(js) as f:
            old_meta = json.load(f)
        diffs = 0 if old_meta == json.loads(json.dumps(meta)) else 1
        for k in sorted(set(arrays) | set(old.files)):
            if k not in arrays or k not in old.files or arrays[k].shape != old[k].shape or not np.array_equal(arrays[k], old[k]):
                print("differs:", k)
                diffs += 1
        print("%d differences" % diffs)
        sys.exit(1 if diffs else 0)
    np.savez_compressed(npz, **arrays)
    with open(js, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", npz, os.path.getsize(npz), "bytes")


if __name__ == "__main__":
    main()
