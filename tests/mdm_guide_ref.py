"""Float64 restatement of the motion generator's guidance step (reference diffusion/mdm.py:1444-1542 apply_guidance), written from the
reference's definitions on top of the float64 pieces of tests/mdm_loss_ref.py (feature extraction, forward kinematics, the full column
scan) - it shares no code with parc_amd.diffusion.mdm_guidance or the kernels.  The gradient is float64 autograd of this restatement.

The difference terms are the reference's as written: `body_pos[..., 1:, :] - body_pos[..., :-1, :]` on body_pos [B, S, bodies, 3] runs
over the second-to-last axis, the bodies of one frame in model order.

It is the yardstick of tests/test_mdm_guide.py and tests/test_mdm_guide_gpu.py and the judge of fixture G35's preconditions
(tests/golden/gen_mdm_guide.py).  Run as a script it measures e-bar, the largest |reference fp32 - restatement| over G35, for the terms,
for x_out and for the step x - x_out:

    python tests/mdm_guide_ref.py
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mdm_loss_ref as mlr      # noqa: E402

F64 = torch.float64
G35 = os.path.join(HERE, "golden", "g35_mdm_guide.npz")
G35_JSON = os.path.join(HERE, "golden", "g35_mdm_guide.json")
TERMS = ["target", "hf", "speed", "acc", "jerk"]
BASE_Z = -10.0          # compute_point_hf_sdf's default, which apply_guidance takes


def load_fixture():
    z = np.load(G35)
    with open(G35_JSON) as f:
        return z, json.load(f)


def case_points(case, z):
    """list over the bodies of [P_b, 3] float32 tensors, or None"""
    if case["points"] == "none":
        return None
    pts, out, i = torch.tensor(z["points_" + case["points"]]), [], 0
    for n in z["counts_" + case["points"]]:
        out.append(pts[i:i + int(n)])
        i += int(n)
    return out


def guidance_terms(model, case, x, mean, std, hfs_normalized, target_xy, points, diag=None):
    """-> (terms [5, B] float64, unweighted, 0 where switched off; re-ordering bounds [5, B])"""
    B, S = x.shape[0], x.shape[1]
    pred = mlr.extract(model, case["components"], x, mean, std, diag)
    rp = pred["ROOT_POS"]
    bp, br = mlr.forward_kinematics(model, rp, pred["ROOT_ROT"], pred["JOINT_ROT"])
    terms = [torch.zeros(B, dtype=F64) for _ in TERMS]
    bounds = [torch.zeros(B, dtype=F64) for _ in TERMS]
    on = lambda name: name in case["terms"]
    if on("target"):
        sq = ((target_xy.reshape(B, 1, 2) - rp[..., :2]) ** 2).reshape(B, -1)
        terms[0] = 0.5 * sq.sum(-1)
        bounds[0] = 0.5 * mlr.reorder_bound(sq.shape[1], sq.detach().sum(-1))
    if on("hf"):
        world = []
        for b in range(model["nb"]):
            pts = points[b].to(F64)
            w = mlr.qrot(br[:, :, b, None, :].expand(B, -1, pts.shape[0], 4), pts.expand(B, S, -1, 3)) + bp[:, :, b, None, :]
            world.append(w.reshape(B, -1, 3))
        world = torch.cat(world, 1)
        xn, xp, yn, yp = case["grid"]
        hf = hfs_normalized.reshape(B, 1 + xn + xp, 1 + yn + yp) * case["max_h"]
        sdf = mlr.points_hf_sdf(world, hf, (-case["dx"] * xn, -case["dx"] * yn), (case["dx"], case["dx"]), BASE_Z, diag)
        if diag is not None:
            diag["world"] = world.detach()          # for the fixture generator, which looks at single points
            diag["min_abs_sdf"] = float(sdf.detach().abs().min())
            diag["frac_inside"] = float((sdf.detach() < 0).double().mean())
        neg2 = sdf.clamp(max=0.0) ** 2
        terms[1] = 0.5 * neg2.sum(-1)
        bounds[1] = 0.5 * mlr.reorder_bound(neg2.shape[1], neg2.detach().sum(-1))
    dt = 1.0 / case["fps"]
    d = bp
    for k, name in ((1, "speed"), (2, "acc"), (3, "jerk")):
        d = d[..., 1:, :] - d[..., :-1, :]
        if not on(name) or d.shape[-2] == 0:
            continue
        mag, thr = d.norm(dim=-1), case["max_rate"][k - 1] * dt ** k
        h = (mag - thr).clamp(min=0.0).reshape(B, -1)
        terms[1 + k] = h.sum(-1)
        bounds[1 + k] = mlr.reorder_bound(h.shape[1], h.detach().sum(-1))
        if diag is not None:
            m = mag.detach()
            diag[name] = dict(frac_above=float((m > thr).double().mean()), min_kink=float(((m - thr).abs() / thr).min()), min_len=float(m.min()))
    return torch.stack(terms), torch.stack(bounds)


def case_eval(model, case, z, x=None, diag=None, with_grad=True):
    """float64 terms, bounds, gradient, x_out and step of case `case` of the fixture (x: another [B, S, D] float64 input)"""
    n = case["name"]
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=F64)
    mean, std = t64(z[n + "_mean"]), t64(z[n + "_std"])
    xx = (t64(z[n + "_x"]) if x is None else x).clone().requires_grad_(with_grad)
    hfs = t64(z[n + "_hfs"]) if "hf" in case["terms"] else None
    tgt = t64(z[n + "_target_xy"]) if "target" in case["terms"] else None
    if diag is not None:          # the rotations the fixture's inputs were assembled from, judged as G33's are
        true = {k: t64(v) for k, v in mlr.true_windows(case).items()}
        if "JOINT_POS" in case["components"]:
            true["JOINT_POS"] = mlr.forward_kinematics(model, true["ROOT_POS"], true["ROOT_ROT"], true["JOINT_ROT"])[0][..., 1:, :]
        mlr.assemble(model, case["components"], true, mean, std, diag)
    terms, bounds = guidance_terms(model, case, xx, mean, std, hfs, tgt, case_points(case, z), diag)
    out = dict(terms=terms.detach().numpy(), bounds=bounds.numpy())
    if with_grad:
        w = torch.tensor(case["w"], dtype=F64)
        grad = torch.autograd.grad((terms.sum(-1) * w).sum(), xx)[0]
        out["grad"] = grad.numpy()
        out["step"] = out["grad"] * case["guidance_str"]
        out["x_out"] = xx.detach().numpy() - out["step"]
        out["loss"] = float((terms.detach().sum(-1) * w).sum())
    return out


def preconditions(diag, case):
    bad = []
    if not (diag["min_vec"] >= 1e-3 and diag["min_w"] >= 1e-3):
        bad.append("quaternion near a singular input: |v| %.2e |w| %.2e" % (diag["min_vec"], diag["min_w"]))
    if not (diag["min_exp"] >= 1e-3 and diag["max_exp"] <= math.pi - 1e-3):
        bad.append("exp-map norm outside [1e-3, pi - 1e-3]: %.3e .. %.3e" % (diag["min_exp"], diag["max_exp"]))
    if "hf" in case["terms"]:
        if not diag["min_abs_sdf"] >= 1e-4:
            bad.append("|sdf| %.2e" % diag["min_abs_sdf"])
        if not diag.get("min_gap", math.inf) >= 1e-5:
            bad.append("runner-up column %.2e" % diag["min_gap"])
        if not 0.1 <= diag["frac_inside"] <= 0.9:
            bad.append("penetrating share %.2f" % diag["frac_inside"])
    for name in ("speed", "acc", "jerk"):
        if name in case["terms"]:
            d = diag[name]
            if not 0.1 <= d["frac_above"] <= 0.9:
                bad.append("%s: share above the threshold %.2f" % (name, d["frac_above"]))
            if not d["min_kink"] >= 1e-3:
                bad.append("%s: %.2e of the threshold from the kink" % (name, d["min_kink"]))
            if not d["min_len"] >= 1e-4:
                bad.append("%s: difference vector %.2e long" % (name, d["min_len"]))
    return bad


def default_model():
    from parc_amd.anim import kin_char_model as kcm
    km = kcm.KinCharModel("cpu")
    km.load_char_file(kcm.default_char_file())
    return mlr.model_from_char(km)


def rel_terms(got, want):
    want = np.asarray(want, np.float64)
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(1.0, np.abs(want))


def step_unit(step64):
    """the per-sample max of the float64 step, [B, 1, 1] (1 where the step is 0)"""
    u = np.abs(step64).reshape(step64.shape[0], -1).max(-1).reshape(-1, 1, 1)
    return np.where(u > 0, u, 1.0)


def measure_ebar(model=None, evals=None):
    """(terms, x_out, step): the largest |reference fp32 - restatement| over G35 in the three units (evals: case_eval of every case by
    name, where the caller has them already)"""
    model = default_model() if model is None and evals is None else model
    z, meta = load_fixture()
    e = [0.0, 0.0, 0.0]
    for case in meta["cases"]:
        n = case["name"]
        r = evals[n] if evals is not None else case_eval(model, case, z)
        x32, out32 = z[n + "_x"].astype(np.float64), z[n + "_x_out"].astype(np.float64)
        e[0] = max(e[0], float(rel_terms(z[n + "_terms"], r["terms"]).max()))
        e[1] = max(e[1], float(rel_terms(out32, r["x_out"]).max()))
        e[2] = max(e[2], float((np.abs((x32 - out32) - r["step"]) / step_unit(r["step"])).max()))
    return tuple(e)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    et, ex, es = measure_ebar()
    print("e-bar terms %.3e" % et)
    print("e-bar x_out %.3e" % ex)
    print("e-bar step  %.3e" % es)
