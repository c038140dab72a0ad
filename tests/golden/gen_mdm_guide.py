#!/usr/bin/env python3
"""Generate tests/golden/g35_mdm_guide.npz (+ .json) from the REFERENCE's own MDM.apply_guidance (diffusion/mdm.py:1444-1542; CPU, torch
fp32, verbose=False), called on an MDM object made without building the transformer (gen_mdm_loss.make_mdm).  The reference guides
batches of one (predict_x0 asks for x_t.shape[0] == 1), so every sample of a case goes through apply_guidance by itself.

Runs ONLY in the build container (needs the reference tree).  True windows are frames of the clips committed with fixture G32; x is the
reference's assemble_mdm_features(true) + seeded noise; feature statistics and heightfields are the seeded draws of gen_mdm_loss (terrain
around the height of the lower body, so that points penetrate); targets are seeded draws.  Per case the fixture records the inputs, the
reference's x_out, and the five unweighted terms [5, B], obtained by evaluating the expressions of apply_guidance with the reference's
own extract_motion_features, forward_kinematics and compute_point_hf_sdf.

Cases (tests/golden/g35_mdm_guide.json holds their configurations):
  all_7x9      B=3 S=5   7 x 9 at 0.4 m    minimal points   all five terms
  shipped      B=2 S=16  31 x 31 at 0.2 m  dense (304)      target + hf, w_target 1, w_hf 10, guidance_str 0.1: the gen_util defaults
  hf_only      B=1 S=5   7 x 9             minimal          hf
  target_only  B=2 S=3   7 x 9             none             target
  dt_only      B=2 S=4   7 x 9             none             speed, acc, jerk
  short        B=1 S=2   7 x 9             none             speed, acc, jerk
  no_pos_con   B=2 S=5   7 x 9             minimal          target + hf + speed; components ROOT_POS, ROOT_ROT, JOINT_ROT only
max_speed, max_acc and max_jerk are set per case so that between 10 % and 90 % of the elements of each enabled difference order lie
above their threshold (the reference differences body_pos along its second-to-last axis: the elements are body-to-body offsets within
a frame, decimetres long, and the reference's defaults would put all of them above).

A case's seed is the first one, counting up from the listed one, under which the preconditions hold under the float64 restatement
(tests/mdm_guide_ref.preconditions); the fixture records it.  If a seed violates one, the next seed is tried - the bounds are not
loosened, and 100 tries per case must do.

Where the reference tree's directory does not exist the script prints "reference tree not found" and exits with status 3 before it
imports anything else; any later failure is an error.

usage:  python tests/golden/gen_mdm_guide.py            # rewrites tests/golden/g35_mdm_guide.npz and .json
        python tests/golden/gen_mdm_guide.py --check    # regenerate and compare with the committed fixture
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import mdm_guide_ref as mgr  # noqa: E402  (tests/mdm_guide_ref.py: the float64 restatement)
import mdm_loss_ref as mlr  # noqa: E402

if not os.path.isdir(mlr.reference_root()):          # decided before any work; every failure after this line is a failure
    print("reference tree not found:", mlr.reference_root())
    sys.exit(3)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)
import gen_mdm_loss as gml  # noqa: E402  (make_mdm, draw_inputs, true_dict: the pattern of fixture G33)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import util.geom_util as geom_util  # noqa: E402
from diffusion.diffusion_util import MDMCustomGuidance, MDMFrameType, MDMKeyType  # noqa: E402

ALL = gml.ALL
G79 = (3, 3, 4, 4)


def make_case(name, seed, windows, S, points, terms, grid=G79, dx=0.4, components=ALL, guidance_str=0.1, w=(0.7, 4.0, 1.0, 0.8, 0.5),
              max_rate=(9.0, 360.0, 18900.0)):
    return dict(name=name, seed=seed, windows=windows, S=S, num_prev_states=1, grid=list(grid), dx=dx, components=list(components), fps=30,
                max_h=3.0, noise=0.08, points=points, terms=list(terms), guidance_str=guidance_str, w=list(w), max_rate=list(max_rate))


CASES = [make_case("all_7x9", 100, [[0, 3], [1, 8], [3, 11]], 5, "minimal", mgr.TERMS),
         make_case("shipped", 200, [[0, 2], [0, 20]], 16, "dense", ["target", "hf"], grid=(10, 20, 15, 15), dx=0.2, w=(1.0, 10.0, 0.0, 0.0, 0.0)),
         make_case("hf_only", 300, [[2, 6]], 5, "minimal", ["hf"]),
         make_case("target_only", 400, [[0, 21], [1, 12]], 3, "none", ["target"]),
         make_case("dt_only", 500, [[0, 9], [2, 4]], 4, "none", ["speed", "acc", "jerk"]),
         make_case("short", 600, [[1, 12]], 2, "none", ["speed", "acc", "jerk"]),
         make_case("no_pos_con", 700, [[0, 30], [3, 2]], 5, "minimal", ["target", "hf", "speed"], components=["ROOT_POS", "ROOT_ROT", "JOINT_ROT"])]


def loss_like(case):
    """the keys gen_mdm_loss.make_mdm and draw_inputs read, for an MDM that only extracts features and measures the terrain"""
    c = dict(case)
    c.update(weights={}, target_dir_len_eps=0.0, use_pos_loss=False, use_hf_collision_loss=False, use_target_loss=False, rot_type="DEFAULT")
    return c


def guidance_params(case, target_xy, body_points):
    gp = MDMCustomGuidance()
    gp.verbose = False
    gp.guidance_str = case["guidance_str"]
    gp.target_xy = target_xy if "target" in case["terms"] else None
    gp.body_points = body_points if "hf" in case["terms"] else None
    gp.w_target_loss, gp.w_hf_loss, gp.w_speed, gp.w_acc, gp.w_jerk = case["w"]
    gp.guide_speed, gp.guide_acc, gp.guide_jerk = "speed" in case["terms"], "acc" in case["terms"], "jerk" in case["terms"]
    gp.max_speed, gp.max_acc, gp.max_jerk = case["max_rate"]
    return gp


def reference_terms(m, case, x, gp, conds):
    """the unweighted terms of one sample, by the expressions of apply_guidance on the reference's own functions"""
    out = np.zeros(5, np.float32)
    with torch.no_grad():
        f = m.extract_motion_features(x)
        root_pos, root_rot, joint_rot = f[MDMFrameType.ROOT_POS], f[MDMFrameType.ROOT_ROT], f[MDMFrameType.JOINT_ROT]
        if gp.target_xy is not None:
            out[0] = (0.5 * torch.sum(torch.square(gp.target_xy - root_pos[..., 0:2]))).item()
        body_pos, body_rot = m._kin_char_model.forward_kinematics(root_pos, root_rot, joint_rot)
        if gp.body_points is not None:
            sdf = m.compute_point_hf_sdf(body_pos, body_rot, gp.body_points, m.unnormalize_hf(conds[MDMKeyType.OBS_KEY]))
            out[1] = (0.5 * torch.sum(torch.square(torch.clamp(sdf, max=0.0)))).item()
        dt = 1.0 / m._sequence_fps
        body_vel = (body_pos[..., 1:, :] - body_pos[..., :-1, :])
        body_acc = (body_vel[..., 1:, :] - body_vel[..., :-1, :])
        body_jerk = (body_acc[..., 1:, :] - body_acc[..., :-1, :])
        if gp.guide_speed:
            out[2] = torch.sum(torch.clamp(torch.norm(body_vel, dim=-1) - gp.max_speed * dt, min=0.0)).item()
        if gp.guide_acc:
            out[3] = torch.sum(torch.clamp(torch.norm(body_acc, dim=-1) - gp.max_acc * (dt ** 2), min=0.0)).item()
        if gp.guide_jerk:
            out[4] = torch.sum(torch.clamp(torch.norm(body_jerk, dim=-1) - gp.max_jerk * (dt ** 3), min=0.0)).item()
    return out


def points_to_move(case, world, hfs, counts):
    """(sample, frame, body) of every point that fails a precondition (with a fifth of margin): |sdf| < 1e-4, or penetrating with
    the runner-up column less than 1e-5 further.  The column distances are those of mdm_loss_ref.points_hf_sdf; `world` lists, body
    after body, the [S, P_b] points of each."""
    xn, xp, yn, yp = case["grid"]
    X, Y, dx, top, S = 1 + xn + xp, 1 + yn + yp, case["dx"], -mgr.BASE_Z, case["S"]
    gx, gy = torch.meshgrid(torch.linspace(0.0, (X - 1.0) * dx, X, dtype=torch.float64), torch.linspace(0.0, (Y - 1.0) * dx, Y, dtype=torch.float64),
                            indexing="ij")
    ends = np.cumsum([S * int(c) for c in counts])
    out = set()
    for b in range(world.shape[0]):
        hf = torch.tensor(hfs[b].reshape(X, Y), dtype=torch.float64) * case["max_h"]
        c = torch.stack([gx - dx * xn, gy - dx * yn, (hf + top) / 2.0], -1).reshape(1, X * Y, 3)
        half = torch.stack([torch.full_like(gx, dx / 2.0), torch.full_like(gy, dx / 2.0), (top - hf) / 2.0], -1).reshape(1, X * Y, 3)
        q = (world[b].unsqueeze(1) - c).abs() - half
        sd = q.clamp(min=0.0).norm(dim=-1) + q.max(dim=-1)[0].clamp(max=0.0)
        val = torch.topk(sd, 2, dim=-1, largest=False)[0]
        bad = (val[:, 0].abs() < 1.2e-4) | ((val[:, 0] > 0) & (val[:, 1] - val[:, 0] < 1.2e-5))
        for n in torch.nonzero(bad).reshape(-1).tolist():
            body = int(np.searchsorted(ends, n, side="right"))
            out.add((b, (n - (ends[body - 1] if body else 0)) // int(counts[body]), body))
    return sorted(out)


def run_case(km, model, case, seed, point_sets, arrays):
    """-> (arrays, diag) of the reference under `seed`.  With the terrain term on, a seed's noise is first adjusted: with thousands of
    sample points per case (9728 in `shipped`) some point lies within 1e-4 of the surface or between two equally near columns
    whatever the seed.  The body that carries such a point is turned a little in that frame - 0.004 more noise on the first
    feature of its joint (of the nearest ancestor with a dof for a fixed joint; the root's height for the root) - and the inputs are
    judged again, up to 12 times.  The preconditions themselves are then judged on the final inputs like any others."""
    if "hf" in case["terms"]:
        sl, _ = mlr.slices_of(model, case["components"])
        counts = [p.shape[0] for p in point_sets[case["points"]]]
        moved = {}
        for _ in range(12):
            out, diag = run_case_once(km, model, case, seed, point_sets, arrays, moved)
            pts = points_to_move(case, diag["world"], out[case["name"] + "_hfs"], counts)
            if not pts:
                break
            for b, f, body in pts:
                while body and model["kind"][body] == 0:
                    body = model["parent"][body]
                col = sl["JOINT_ROT"].start + model["first"][body] if body else sl["ROOT_POS"].start + 2
                moved[(b, f, col)] = moved.get((b, f, col), 0) + 1
        diag["features_moved"] = len(moved)
        diag.pop("world", None)
        return out, diag
    return run_case_once(km, model, case, seed, point_sets, arrays, {})


def run_case_once(km, model, case, seed, point_sets, arrays, moved):
    lc = loss_like(case)
    true = gml.true_dict(km, lc)
    D = gml.make_mdm(km, lc, None, None)._motion_frame_dof
    d = gml.draw_inputs(lc, seed, D)
    for (b, f, col), times in sorted(moved.items()):
        d["noise"][b, f, col] += np.float32(times * 0.004)
    m = gml.make_mdm(km, lc, gg.t(d["mean"]), gg.t(d["std"]))
    with torch.no_grad():
        x_true = m.assemble_mdm_features(true)
    x = (x_true + gg.t(d["noise"])).clone()
    B = x.shape[0]
    target = np.random.default_rng(seed + 7919).uniform(-2.0, 2.0, size=(B, 1, 2)).astype(np.float32)
    n = case["name"]
    out = {n + "_mean": d["mean"], n + "_std": d["std"], n + "_x_true": gg.npy(x_true), n + "_x": gg.npy(x)}
    if "hf" in case["terms"]:
        out[n + "_hfs"] = d["hfs"]
    if "target" in case["terms"]:
        out[n + "_target_xy"] = target
    body_points = point_sets.get(case["points"])
    x_out, terms = [], []
    for b in range(B):
        gp = guidance_params(case, gg.t(target[b:b + 1]), body_points)
        conds = {MDMKeyType.GUIDANCE_PARAMS: gp}
        if "hf" in case["terms"]:
            conds[MDMKeyType.OBS_KEY] = gg.t(d["hfs"][b:b + 1])
        xb = x[b:b + 1].clone()
        terms.append(reference_terms(m, case, xb, gp, conds))
        m.apply_guidance(xb, conds)
        x_out.append(gg.npy(xb)[0])
    out[n + "_x_out"], out[n + "_terms"] = np.stack(x_out), np.stack(terms, 1)
    assert all(np.isfinite(v).all() for v in out.values()), "non-finite value in case " + n
    diag = {}
    z = dict(arrays)
    z.update(out)
    mgr.case_eval(model, case, z, diag=diag, with_grad=False)
    return out, diag


def generate(first_seed=None):
    """first_seed: case name -> the seed to begin with (--check begins with the recorded one: the seeds before it were judged when the
    fixture was written)"""
    torch.manual_seed(0)
    km = gml.load_char()
    nb = km.get_num_joints()
    joints = [None] + [km.get_joint(j) for j in range(1, nb)]
    model = dict(nb=nb, parent=[int(p) for p in km._parent_indices.tolist()],
                 kind=[0] + [{0: 0, 1: mlr.HINGE, 3: mlr.SPHERICAL}[j.get_dof_dim()] for j in joints[1:]],
                 first=[0] + [int(j.dof_idx) for j in joints[1:]],
                 axis=np.stack([np.zeros(3)] + [np.zeros(3) if j.axis is None else j.axis.double().numpy().reshape(3) for j in joints[1:]]),
                 lt=km._local_translation.double().numpy(), lr=km._local_rotation.double().numpy(), dof_size=int(km.get_dof_size()))
    # The body points are an input of apply_guidance.  The dense set is the reference's get_char_point_samples; its sphere geoms ask
    # trimesh (absent here) for an un-subdivided icosphere, which is the 12 icosahedron vertices gen_golden._icosa_points gives.
    keep = geom_util.get_sphere_point_surface_samples
    geom_util.get_sphere_point_surface_samples = lambda r, device, num_subdivisions=0: gg.t(gg._icosa_points(r))
    try:
        dense = geom_util.get_char_point_samples(km)
    finally:
        geom_util.get_sphere_point_surface_samples = keep
    point_sets = dict(minimal=geom_util.get_minimal_char_point_samples(km), dense=dense)
    arrays, meta = {}, dict(cases=[])
    for name, pts in point_sets.items():
        arrays["points_" + name] = np.concatenate([gg.npy(p) for p in pts]).astype(np.float32)
        arrays["counts_" + name] = np.array([p.shape[0] for p in pts], np.int64)
    for case in CASES:
        seed = case["seed"] if first_seed is None else first_seed[case["name"]]
        while True:
            out, diag = run_case(km, model, case, seed, point_sets, arrays)
            bad = mgr.preconditions(diag, case)
            if not bad:
                break
            print("case %s seed %d: %s" % (case["name"], seed, "; ".join(bad)))
            seed += 1
            assert seed < case["seed"] + 100, "no seed meets the preconditions of case " + case["name"]
        c = dict(case)
        c["seed_used"] = seed
        c["features_moved"] = diag.get("features_moved", 0)
        meta["cases"].append(c)
        arrays.update(out)
        print("case %-12s seed %d  inside %.2f  min|sdf| %.1e  gap %.1e  above %s" % (
            case["name"], seed, diag.get("frac_inside", float("nan")), diag.get("min_abs_sdf", float("nan")), diag.get("min_gap", float("nan")),
            " ".join("%s %.2f" % (k, diag[k]["frac_above"]) for k in ("speed", "acc", "jerk") if k in diag)))
    return arrays, meta


def main():
    check = "--check" in sys.argv[1:]
    if check:
        old, old_meta = mgr.load_fixture()
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
    np.savez_compressed(mgr.G35, **arrays)
    with open(mgr.G35_JSON, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", mgr.G35, os.path.getsize(mgr.G35), "bytes")


if __name__ == "__main__":
    main()
