"""Float64 restatement of the motion generator's call (reference diffusion/gen_util.py:81-134, :211-218 gen_mdm_motion; diffusion/mdm.py
:1341-1364, :1392-1396 the head and tail of gen_sequence_with_contacts; util/terrain_util.py:2049-2082 sample_hf_z_on_terrain), written
from the reference's definitions on top of the float64 pieces of tests/mdm_loss_ref.py (rotations, forward kinematics, feature assembly
and extraction) - it shares no code with parc_amd.diffusion.gen_util or the kernels.

RELATIVE_TO_ROOT_FLOOR has its evident per-sample meaning here (heights relative to the terrain cell under each sample's own canonical
root); the reference's branch raises for B != 2, so this file is that style's only yardstick.

It is the yardstick of tests/test_mdm_gen.py and tests/test_mdm_gen_gpu.py and the judge of fixture G36's preconditions
(tests/golden/gen_mdm_gen.py).  Run as a script it measures e-bar, the largest |reference fp32 - restatement| over G36 per output group:

    python tests/mdm_gen_ref.py
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
G36 = os.path.join(HERE, "golden", "g36_mdm_gen.npz")
G36_JSON = os.path.join(HERE, "golden", "g36_mdm_gen.json")
DELTA = 2e-4          # cells: a grid coordinate closer than this to k + 1/2 is "near a boundary"
MAX_NEAR = 0.005      # at most this share of a case's cells may be near a boundary
GROUPS = ("canon", "prev_state", "target", "root_pos", "root_rot", "joint_rot", "frames")


def load_fixture():
    z = np.load(G36)
    with open(G36_JSON) as f:
        return z, json.load(f)


def t64(a):
    return torch.tensor(np.asarray(a), dtype=F64)


def rot2d(v, ang):
    """util/torch_util.py:619-631"""
    c, s = torch.cos(ang), torch.sin(ang)
    return torch.stack([v[..., 0] * c - v[..., 1] * s, v[..., 0] * s + v[..., 1] * c], -1)


def z_quat(ang):
    axis = torch.zeros(ang.shape + (3,), dtype=F64)
    axis[..., 2] = 1.0
    return mlr.axis_angle_to_quat(axis, ang)


def local_grid(case):
    xn, xp, yn, yp = case["grid"]
    dx = case["dx"]
    xs = torch.linspace(-dx * xn, dx * xp, 1 + xn + xp, dtype=F64)
    ys = torch.linspace(-dx * yn, dx * yp, 1 + yn + yp, dtype=F64)
    gx, gy = torch.meshgrid(xs, ys, indexing="ij")
    return torch.stack([gx, gy], -1)


def lookup(terrain, coords):
    """heights at round-half-even(coords), clamped to the grid (util/terrain_util.py:113-130)"""
    hf = terrain["hf"]
    i = torch.round(coords[..., 0]).long().clamp(0, hf.shape[0] - 1)
    j = torch.round(coords[..., 1]).long().clamp(0, hf.shape[1] - 1)
    return hf[i, j]


def fixture_terrain(z):
    return dict(hf=t64(z["terrain_hf"]), min_point=t64(z["terrain_min_point"]), dxdy=t64(z["terrain_dxdy"]))


def encode(model, case, terrain, root_pos, root_rot, joint_rot, contacts, target_world, mean, std, diag=None):
    """float64 tensors [B, T, ...] -> dict of the encode outputs; `coords` [B, X, Y, 2] are the grid coordinates before rounding"""
    P = case["num_prev_states"]
    c = P - 1
    B, T = root_pos.shape[:2]
    canon_xy = root_pos[:, c, 0:2]
    ex = torch.zeros(B, 3, dtype=F64)
    ex[:, 0] = 1.0
    d = mlr.qrot(root_rot[:, c], ex)
    heading = torch.atan2(d[:, 1], d[:, 0])
    hq, hq_inv = z_quat(heading), z_quat(-heading)
    coords = (rot2d(local_grid(case).unsqueeze(0), heading.reshape(B, 1, 1)) + canon_xy.reshape(B, 1, 1, 2) - terrain["min_point"]) / terrain["dxdy"]
    hf_z = lookup(terrain, coords)
    if case["z_style"] == "RELATIVE_TO_ROOT_FLOOR":
        z_ref = lookup(terrain, (canon_xy - terrain["min_point"]) / terrain["dxdy"])
    else:
        z_ref = root_pos[:, c, 2]
    hf_z = hf_z - z_ref.reshape(B, 1, 1)
    rp = root_pos.clone()
    rp[..., 0:2] = rp[..., 0:2] - canon_xy.unsqueeze(1)
    rp = mlr.qrot(hq_inv.unsqueeze(1).expand(B, T, 4), rp)
    rp[..., 2] = rp[..., 2] - z_ref.unsqueeze(1)
    rr = mlr.qmul(hq_inv.unsqueeze(1).expand(B, T, 4), root_rot)
    bp, _ = mlr.forward_kinematics(model, rp, rr, joint_rot)
    target = rot2d(target_world[:, 0:2] - canon_xy, -heading)
    target_dir = target / target.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    comp = {"ROOT_POS": rp[:, :P], "ROOT_ROT": rr[:, :P], "JOINT_POS": bp[:, :P, 1:], "JOINT_ROT": joint_rot[:, :P]}
    if contacts is not None:
        comp["CONTACTS"] = contacts[:, :P]
    prev_state = mlr.assemble(model, case["components"], comp, mean, std, diag)
    obs = hf_z.clamp(-case["max_h"], case["max_h"]) / case["max_h"]
    if diag is not None:
        diag["max_abs_heading"] = max(diag.get("max_abs_heading", 0.0), float(heading.abs().max()))
        diag["max_abs_index"] = max(diag.get("max_abs_index", 0.0), float(coords.abs().max()))
        diag["near_share"] = float(near_boundary(coords).double().mean())
    return dict(canon_xy=canon_xy, heading=heading, heading_quat=hq, z_ref=z_ref, root_pos=rp, root_rot=rr, body_pos=bp[..., 1:, :], hf_z=hf_z, obs=obs,
                target=target, target_dir=target_dir, prev_state=prev_state, coords=coords)


def decode(model, case, enc, x, no_noise, mean, std, diag=None):
    """x [B, S, D] float64 (the sampler's standardised output) -> world-frame root_pos, root_rot, joint_rot, contacts, frames"""
    P = case["num_prev_states"]
    B, S = x.shape[:2]
    if no_noise is not None:
        x = torch.cat([torch.where(no_noise.reshape(B, 1, 1), enc["prev_state"], x[:, :P]), x[:, P:]], 1)
    f = mlr.extract(model, case["components"], x, mean, std, diag)
    hq = enc["heading_quat"].unsqueeze(1).expand(B, S, 4)
    rot = mlr.qmul(hq, f["ROOT_ROT"])
    pos = mlr.qrot(hq, f["ROOT_POS"])
    pos = pos + torch.cat([enc["canon_xy"], enc["z_ref"].unsqueeze(-1)], -1).unsqueeze(1)
    frames = torch.cat([pos, mlr.quat_to_exp_map(rot, diag), mlr.rot_to_dof(model, f["JOINT_ROT"], diag)], -1)
    return dict(root_pos=pos, root_rot=rot, joint_rot=f["JOINT_ROT"], contacts=f.get("CONTACTS"), frames=frames)


def near_boundary(coords, delta=DELTA):
    """[.., 2] grid coordinates -> bool: either coordinate within delta cells of a rounding boundary k + 1/2"""
    frac = coords - torch.floor(coords)
    return ((frac - 0.5).abs() < delta).any(-1)


def adjacent_values(terrain, coords, delta=DELTA):
    """[..., 4]: the heights of the at most four cells a near-boundary coordinate can round to"""
    out = []
    for sx in (-delta, delta):
        for sy in (-delta, delta):
            out.append(lookup(terrain, coords + torch.tensor([sx, sy], dtype=F64)))
    return torch.stack(out, -1)


def case_inputs(case, z):
    n = case["name"]
    con = t64(z[n + "_prev_contacts"])
    return dict(root_pos=t64(z[n + "_prev_root_pos"]), root_rot=t64(z[n + "_prev_root_rot"]), joint_rot=t64(z[n + "_prev_joint_rot"]), contacts=con,
                target_world=t64(z[n + "_target_world"]), mean=t64(z[n + "_mean"]), std=t64(z[n + "_std"]))


def case_eval(model, case, z, diag=None, z_style=None):
    """the float64 encode (and, for a feature-mode case, decode) of a fixture case; z_style overrides the case's"""
    n = case["name"]
    cs = dict(case)
    if z_style is not None:
        cs["z_style"] = z_style
    i = case_inputs(cs, z)
    ter = fixture_terrain(z)
    enc = encode(model, cs, ter, i["root_pos"], i["root_rot"], i["joint_rot"], i["contacts"], i["target_world"], i["mean"], i["std"], diag)
    out = dict(enc=enc)
    if n + "_x" in z.files:
        # component mode returns the model's components as they are: no previous state is put back
        keep = None if case["mode"] == "components" else torch.tensor(np.asarray(z[n + "_use_prev_state"], dtype=bool))
        out["dec"] = decode(model, cs, enc, t64(z[n + "_x"]), keep, i["mean"], i["std"], diag)
    return out


def preconditions(diag, case):
    bad = []
    if not (diag["min_vec"] >= 1e-3 and diag["min_w"] >= 1e-3):
        bad.append("quaternion near a singular input: |v| %.2e |w| %.2e" % (diag["min_vec"], diag["min_w"]))
    lo, hi = diag.get("min_exp", math.inf), diag.get("max_exp", 0.0)
    if not (lo >= 1e-3 and hi <= math.pi - 1e-3):
        bad.append("exp-map norm outside [1e-3, pi - 1e-3]: %.3e .. %.3e" % (lo, hi))
    if not diag["max_abs_heading"] <= math.pi - 1e-2:
        bad.append("|heading| %.4f" % diag["max_abs_heading"])
    if not diag["max_abs_index"] < 128:
        bad.append("grid index %.1f" % diag["max_abs_index"])
    if not diag["near_share"] <= MAX_NEAR:
        bad.append("share of cells near a rounding boundary %.4f" % diag["near_share"])
    return bad


def default_model():
    from parc_amd.anim import kin_char_model as kcm
    km = kcm.KinCharModel("cpu")
    km.load_char_file(kcm.default_char_file())
    return mlr.model_from_char(km)


def group_errors(case, z, r):
    """group -> largest |fixture fp32 - restatement| of a case, for the groups the fixture records of it"""
    n = case["name"]
    err = {}

    def put(group, key, ref):
        if n + key in z.files and ref is not None:
            err[group] = max(err.get(group, 0.0), float(np.abs(z[n + key].astype(np.float64) - np.asarray(ref)).max()))
    enc, P = r["enc"], case["num_prev_states"]
    put("canon", "_canon_root_pos", enc["root_pos"][:, :P])
    put("canon", "_canon_root_rot", enc["root_rot"][:, :P])
    put("canon", "_canon_body_pos", enc["body_pos"][:, :P])
    put("prev_state", "_prev_state", enc["prev_state"])
    put("target", "_target", enc["target"].unsqueeze(1))
    put("target", "_target_dir", enc["target_dir"].unsqueeze(1))
    if "dec" in r:
        for g in ("root_pos", "root_rot", "joint_rot", "frames"):
            put(g, "_out_" + g, r["dec"][g])
    return err


def measure_ebar(model=None, evals=None):
    """group -> e-bar over G36 (evals: case_eval of every case by name, where the caller has them already)"""
    model = default_model() if model is None and evals is None else model
    z, meta = load_fixture()
    e = {g: 0.0 for g in GROUPS}
    for case in meta["cases"]:
        r = evals[case["name"]] if evals is not None else case_eval(model, case, z)
        for g, v in group_errors(case, z, r).items():
            e[g] = max(e[g], v)
    return e


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    for g, v in measure_ebar().items():
        print("e-bar %-10s %.4e" % (g, v))
