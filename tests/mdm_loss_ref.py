"""Float64 restatement of the motion generator's training loss (reference diffusion/mdm.py:382-478 assemble / extract features, :617-754
motion_difference, :978-1028 compute_point_hf_sdf, :936-958 the trainer's reduction), written from the reference's definitions with
explicit loops over joints and bodies - it shares no code with parc_amd.diffusion.mdm_loss or the kernels.  The gradient is float64
autograd of this restatement.

It is the yardstick of tests/test_mdm_loss.py and tests/test_mdm_loss_gpu.py and the judge of fixture G33's preconditions
(tests/golden/gen_mdm_loss.py).  Run as a script it measures e-bar, the largest |reference fp32 - restatement| over G33:

    python tests/mdm_loss_ref.py
"""
import math
import os
from collections import OrderedDict

import numpy as np
import torch

F64 = torch.float64
HERE = os.path.dirname(os.path.abspath(__file__))
G33 = os.path.join(HERE, "golden", "g33_mdm_loss.npz")
G33_JSON = os.path.join(HERE, "golden", "g33_mdm_loss.json")
G32 = os.path.join(HERE, "golden", "g32_mdm_sampler.npz")

HINGE, SPHERICAL = 1, 2
TERM_ORDER = ["VEL_ROOT_POS_LOSS", "VEL_ROOT_ROT_LOSS", "VEL_JOINT_ROT_LOSS", "SIMPLE_ROOT_POS_LOSS", "SIMPLE_ROOT_ROT_LOSS", "SIMPLE_JOINT_ROT_LOSS",
              "SIMPLE_CONTACT_LOSS", "SIMPLE_BODY_POS_LOSS", "FK_BODY_POS_LOSS", "FK_BODY_ROT_LOSS", "BODY_POS_CONSISTENCY_LOSS",
              "VEL_FK_BODY_POS_LOSS", "HF_COLLISION_LOSS", "TARGET_LOSS"]
WEIGHT_OF = {"VEL_ROOT_POS_LOSS": "w_vel_root_pos", "VEL_ROOT_ROT_LOSS": "w_vel_root_rot", "VEL_JOINT_ROT_LOSS": "w_vel_joint_rot",
             "SIMPLE_ROOT_POS_LOSS": "w_simple_root_pos", "SIMPLE_ROOT_ROT_LOSS": "w_simple_root_rot", "SIMPLE_JOINT_ROT_LOSS": "w_simple_joint_rot",
             "SIMPLE_CONTACT_LOSS": "w_simple_contacts", "SIMPLE_BODY_POS_LOSS": "w_simple_body_pos", "FK_BODY_POS_LOSS": "w_body_pos",
             "FK_BODY_ROT_LOSS": "w_body_rot", "BODY_POS_CONSISTENCY_LOSS": "w_body_pos_consistency", "VEL_FK_BODY_POS_LOSS": "w_body_vel",
             "HF_COLLISION_LOSS": "w_hf", "TARGET_LOSS": "w_target"}
UNMASKED = ("HF_COLLISION_LOSS", "TARGET_LOSS")      # the terms the ood mask leaves alone


# ------------------------------------------------------------------------------------------------------------------- the character
def model_from_char(km):
    """plain arrays of a parc_amd KinCharModel: the tree's constants, no arithmetic"""
    nb = km.get_num_joints()
    kind, first, axis = [0] * nb, [0] * nb, np.zeros((nb, 3))
    for j in range(1, nb):
        jt = km.get_joint(j)
        n = jt.get_dof_dim()
        kind[j], first[j] = {0: 0, 1: HINGE, 3: SPHERICAL}[n], int(jt.dof_idx)
        if n == 1:
            axis[j] = np.asarray(jt.axis.detach().cpu() if torch.is_tensor(jt.axis) else jt.axis, dtype=np.float64).reshape(3)
    return dict(nb=nb, parent=[int(p) for p in km._parent_indices.cpu().tolist()], kind=kind, first=first, axis=axis,
                lt=km._local_translation.detach().cpu().numpy().astype(np.float64), lr=km._local_rotation.detach().cpu().numpy().astype(np.float64),
                dof_size=int(km.get_dof_size()))


# ------------------------------------------------------------------------------------------------------------------- rotations
def qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                        aw * bw - ax * bx - ay * by - az * bz], -1)


def qconj(q):
    return q * torch.tensor([-1.0, -1.0, -1.0, 1.0], dtype=q.dtype)


def qrot(q, v):
    u = q[..., :3]
    t = 2.0 * torch.linalg.cross(u, v)
    return v + q[..., 3:] * t + torch.linalg.cross(u, t)


def unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp(min=1e-9)


def quat_to_axis_angle(q, diag=None, skip=None):
    """util/torch_util.py:68-88.  diag collects the smallest vector part and |w| fed in; skip [..] marks the constant pairs."""
    q = torch.where(q[..., 3:] < 0, -q, q)
    length = q[..., :3].norm(dim=-1)
    if diag is not None:
        keep = torch.ones_like(length, dtype=torch.bool) if skip is None else ~skip.expand(length.shape)
        if keep.any():
            diag["min_vec"] = min(diag.get("min_vec", math.inf), float(length[keep].detach().min()))
            diag["min_w"] = min(diag.get("min_w", math.inf), float(q[..., 3][keep].detach().abs().min()))
    ok = length > 1e-5
    safe = torch.where(ok, length, torch.ones_like(length))
    angle = torch.where(ok, 2.0 * torch.atan2(safe, q[..., 3]), torch.zeros_like(length))
    z = torch.zeros_like(q[..., :3])
    z[..., 2] = 1.0
    axis = torch.where(ok.unsqueeze(-1), q[..., :3] / safe.unsqueeze(-1), z)
    return axis, angle


def quat_to_exp_map(q, diag=None, skip=None):
    axis, angle = quat_to_axis_angle(q, diag, skip)
    return axis * angle.unsqueeze(-1)


def axis_angle_to_quat(axis, angle):
    th = (angle / 2).unsqueeze(-1)
    return unit(torch.cat([unit(axis) * th.sin(), th.cos()], -1))


def exp_map_to_quat(e, diag=None):
    raw = e.norm(dim=-1)
    if diag is not None:
        diag["min_exp"] = min(diag.get("min_exp", math.inf), float(raw.detach().min()))
        diag["max_exp"] = max(diag.get("max_exp", 0.0), float(raw.detach().max()))
    angle = torch.atan2(raw.sin(), raw.cos())
    ok = angle.abs() > 1e-5
    safe = torch.where(ok, raw, torch.ones_like(raw))
    z = torch.zeros_like(e)
    z[..., 2] = 1.0
    axis = torch.where(ok.unsqueeze(-1), e / safe.unsqueeze(-1), z)
    return axis_angle_to_quat(axis, torch.where(ok, angle, torch.zeros_like(angle)))


def dof_to_rot(model, dof, diag=None):
    out = []
    for j in range(1, model["nb"]):
        k, f = model["kind"][j], model["first"][j]
        if k == HINGE:
            ax = torch.tensor(model["axis"][j], dtype=F64).expand(dof.shape[:-1] + (3,))
            out.append(axis_angle_to_quat(ax, dof[..., f]))
        elif k == SPHERICAL:
            out.append(exp_map_to_quat(dof[..., f:f + 3], diag))
        else:
            q = torch.zeros(dof.shape[:-1] + (4,), dtype=F64)
            q[..., 3] = 1.0
            out.append(q)
    return torch.stack(out, -2)


def rot_to_dof(model, rot, diag=None):
    dof = torch.zeros(rot.shape[:-2] + (model["dof_size"],), dtype=F64)
    for j in range(1, model["nb"]):
        k, f = model["kind"][j], model["first"][j]
        if k == HINGE:
            axis, angle = quat_to_axis_angle(rot[..., j - 1, :], diag)
            dot = (torch.tensor(model["axis"][j], dtype=F64) * axis).sum(-1)
            dof[..., f] = torch.where(dot < 0, -angle, angle)
        elif k == SPHERICAL:
            dof[..., f:f + 3] = quat_to_exp_map(rot[..., j - 1, :], diag)
    return dof


def fixed_joint_mask(model):
    return torch.tensor([model["kind"][j] == 0 for j in range(1, model["nb"])])


def forward_kinematics(model, root_pos, root_rot, joint_rot):
    pos, rot = [root_pos], [root_rot]
    for j in range(1, model["nb"]):
        p = model["parent"][j]
        lt = torch.tensor(model["lt"][j], dtype=F64).expand(root_pos.shape)
        lr = torch.tensor(model["lr"][j], dtype=F64).expand(root_rot.shape)
        pos.append(pos[p] + qrot(rot[p], lt))
        rot.append(qmul(rot[p], qmul(lr, joint_rot[..., j - 1, :])))
    return torch.stack(pos, -2), torch.stack(rot, -2)


# ------------------------------------------------------------------------------------------------------------------- features
def slices_of(model, components, rot_type="DEFAULT"):
    """rot_type DEFAULT: root exponential map, joint dofs; EXP_MAP: exponential maps throughout; QUAT: quaternions throughout"""
    J = model["nb"] - 1
    root = 4 if rot_type == "QUAT" else 3
    joint = {"DEFAULT": model["dof_size"], "EXP_MAP": 3 * J, "QUAT": 4 * J}[rot_type]
    dims = {"ROOT_POS": 3, "ROOT_ROT": root, "JOINT_POS": 3 * J, "JOINT_ROT": joint, "CONTACTS": model["nb"]}
    out, i = {}, 0
    for c in components:
        out[c] = slice(i, i + dims[c])
        i += dims[c]
    return out, i


def assemble(model, components, true, mean, std, diag=None, rot_type="DEFAULT"):
    parts = []
    for c in components:
        v = true[c]
        if c == "ROOT_ROT":
            v = v if rot_type == "QUAT" else quat_to_exp_map(v, diag)
        elif c == "JOINT_ROT":
            if rot_type == "DEFAULT":
                v = rot_to_dof(model, v, diag)
            elif rot_type == "EXP_MAP":          # the fixed joints' identity rotations are constants
                v = quat_to_exp_map(v, diag, fixed_joint_mask(model)).reshape(v.shape[0], v.shape[1], -1)
            else:
                v = v.reshape(v.shape[0], v.shape[1], -1)
        elif c == "JOINT_POS":
            v = v.reshape(v.shape[0], v.shape[1], -1)
        parts.append(v)
    f = torch.cat(parts, -1)
    return (f - mean[:f.shape[1]]) / std[:f.shape[1]]


def extract(model, components, x, mean, std, diag=None, rot_type="DEFAULT"):
    sl, _ = slices_of(model, components, rot_type)
    f = x * std[:x.shape[1]] + mean[:x.shape[1]]
    out = {}
    for c in components:
        v = f[..., sl[c]]
        if c == "ROOT_ROT":
            v = v if rot_type == "QUAT" else exp_map_to_quat(v, diag)
        elif c == "JOINT_ROT":
            if rot_type == "DEFAULT":
                v = dof_to_rot(model, v, diag)
            else:
                v = v.reshape(v.shape[0], v.shape[1], model["nb"] - 1, -1)
                v = v if rot_type == "QUAT" else exp_map_to_quat(v, diag)
        elif c == "JOINT_POS":
            v = v.reshape(v.shape[0], v.shape[1], model["nb"] - 1, 3)
        out[c] = v
    return out


# ------------------------------------------------------------------------------------------------------------------- terrain
def points_hf_sdf(points, hf, min_center, dxdy, base_z, diag=None):
    """points [B, N, 3], hf [B, X, Y] (heights) -> [B, N], negative inside the ground: the full scan of util/terrain_util.py:1835-1893"""
    B, X, Y = hf.shape
    xs = torch.linspace(0.0, (X - 1.0) * dxdy[0], X, dtype=F64)
    ys = torch.linspace(0.0, (Y - 1.0) * dxdy[1], Y, dtype=F64)
    gx, gy = torch.meshgrid(xs, ys, indexing="ij")
    top = -base_z
    out = []
    for b in range(B):
        c = torch.stack([gx + min_center[0], gy + min_center[1], (hf[b] + top) / 2.0], -1).reshape(1, X * Y, 3)
        half = torch.stack([torch.full_like(gx, dxdy[0] / 2.0), torch.full_like(gy, dxdy[1] / 2.0), (top - hf[b]) / 2.0], -1).reshape(1, X * Y, 3)
        q = (points[b].unsqueeze(1) - c).abs() - half
        sd = q.clamp(min=0.0).norm(dim=-1) + q.max(dim=-1)[0].clamp(max=0.0)
        best = sd.min(dim=-1)[0]
        if diag is not None and X * Y > 1:
            two = torch.topk(sd.detach(), 2, dim=-1, largest=False)[0]
            inside = best.detach() > 0                    # sdf = -best < 0
            if inside.any():
                diag["min_gap"] = min(diag.get("min_gap", math.inf), float((two[:, 1] - two[:, 0])[inside].min()))
        out.append(-best)
    return torch.stack(out, 0)


# ------------------------------------------------------------------------------------------------------------------- the loss
def reorder_bound(n, abs_sum):
    """the textbook bound on what re-ordering an fp32 sum of n terms can change: ceil(log2 n) * 2^-24 * sum |summand|"""
    return math.ceil(math.log2(max(n, 2))) * 2.0 ** -24 * abs_sum


def motion_loss(model, cfg, true, x, mean, std, hfs_normalized, target_dir, points, loss_fn, diag=None):
    """-> (OrderedDict name -> [B] float64 in the reference's insertion order, dict name -> [B] re-ordering bound).
    cfg: the case configuration (tests/golden/g33_mdm_loss.json); true: dict of float64 tensors; x [B, S, D] float64 (may require grad);
    points: list over bodies of [P_b, 3]."""
    comps = cfg["components"]
    dt = 1.0 / cfg["fps"]
    huber = loss_fn == "pseudo_huber"
    bounds = {}

    def lf(name, a, b):
        d2 = (a - b) ** 2
        if huber:
            d2 = d2 + 0.0009
        flat = d2.reshape(d2.shape[0], -1)
        s = flat.sum(-1)
        rb = reorder_bound(flat.shape[1], flat.detach().abs().sum(-1))
        w = cfg["weights"][WEIGHT_OF[name]]
        bounds[name] = abs(w) * (rb / (2.0 * s.detach().sqrt()) if huber else rb)
        return w * ((s.sqrt() - 0.03) if huber else s)

    pred = extract(model, comps, x, mean, std, diag, cfg.get("rot_type", "DEFAULT"))
    rpT, rpP, rrT, rrP, jrT, jrP = true["ROOT_POS"], pred["ROOT_POS"], true["ROOT_ROT"], pred["ROOT_ROT"], true["JOINT_ROT"], pred["JOINT_ROT"]
    bpP, brP = forward_kinematics(model, rpP, rrP, jrP)
    bpT, brT = forward_kinematics(model, rpT, rrT, jrT)
    fixed = fixed_joint_mask(model)
    zero = torch.zeros((), dtype=F64)

    def ang_vel(q, skip=None):
        return quat_to_exp_map(qmul(q[:, 1:], qconj(q[:, :-1])), diag, skip) / dt

    def diff_angle(q0, q1, skip=None):
        return quat_to_axis_angle(qmul(q1, qconj(q0)), diag, skip)[1]

    L = OrderedDict()
    L["VEL_ROOT_POS_LOSS"] = lf("VEL_ROOT_POS_LOSS", (rpT[:, 1:] - rpT[:, :-1]) / dt, (rpP[:, 1:] - rpP[:, :-1]) / dt)
    L["VEL_ROOT_ROT_LOSS"] = lf("VEL_ROOT_ROT_LOSS", ang_vel(rrT), ang_vel(rrP))
    L["VEL_JOINT_ROT_LOSS"] = lf("VEL_JOINT_ROT_LOSS", ang_vel(jrT, fixed), ang_vel(jrP, fixed))
    L["SIMPLE_ROOT_POS_LOSS"] = lf("SIMPLE_ROOT_POS_LOSS", rpT, rpP)
    L["SIMPLE_ROOT_ROT_LOSS"] = lf("SIMPLE_ROOT_ROT_LOSS", diff_angle(rrT, rrP), zero)
    L["SIMPLE_JOINT_ROT_LOSS"] = lf("SIMPLE_JOINT_ROT_LOSS", diff_angle(jrT, jrP, fixed), zero)
    if "CONTACTS" in comps:
        L["SIMPLE_CONTACT_LOSS"] = lf("SIMPLE_CONTACT_LOSS", true["CONTACTS"], pred["CONTACTS"])
    if "JOINT_POS" in comps:
        L["SIMPLE_BODY_POS_LOSS"] = lf("SIMPLE_BODY_POS_LOSS", bpT[..., 1:, :], pred["JOINT_POS"])
    if cfg["use_pos_loss"]:
        L["FK_BODY_POS_LOSS"] = lf("FK_BODY_POS_LOSS", bpT, bpP)
        L["FK_BODY_ROT_LOSS"] = lf("FK_BODY_ROT_LOSS", diff_angle(brT, brP), zero)
        if "JOINT_POS" in comps:
            L["BODY_POS_CONSISTENCY_LOSS"] = lf("BODY_POS_CONSISTENCY_LOSS", bpP[..., 1:, :], pred["JOINT_POS"])
        L["VEL_FK_BODY_POS_LOSS"] = lf("VEL_FK_BODY_POS_LOSS", (bpT[:, 1:] - bpT[:, :-1]) / dt, (bpP[:, 1:] - bpP[:, :-1]) / dt)
    if cfg["use_hf_collision_loss"]:
        B = x.shape[0]
        world = []
        for b in range(model["nb"]):
            pts = points[b].to(F64)
            w = qrot(brP[:, :, b, None, :].expand(B, -1, pts.shape[0], 4), pts.expand(B, brP.shape[1], -1, 3)) + bpP[:, :, b, None, :]
            world.append(w.reshape(B, -1, 3))
        world = torch.cat(world, 1)
        xn, xp, yn, yp = cfg["grid"]
        hf = hfs_normalized.reshape(B, 1 + xn + xp, 1 + yn + yp) * cfg["max_h"]
        sdf = points_hf_sdf(world, hf, (-cfg["dx"] * xn, -cfg["dx"] * yn), (cfg["dx"], cfg["dx"]), -cfg["max_h"] - 5.0, diag)
        if diag is not None:
            diag["min_abs_sdf"] = min(diag.get("min_abs_sdf", math.inf), float(sdf.detach().abs().min()))
            diag["frac_inside"] = float((sdf.detach() < 0).double().mean())
        neg2 = sdf.clamp(max=0.0) ** 2
        w = cfg["weights"]["w_hf"]
        L["HF_COLLISION_LOSS"] = w * (0.5 * neg2.sum(-1))
        bounds["HF_COLLISION_LOSS"] = abs(w) * 0.5 * reorder_bound(neg2.shape[1], neg2.detach().sum(-1))
    if cfg["use_target_loss"]:
        raw = (-target_dir.reshape(-1, 2) * (rpP[:, -1, :2] - rpP[:, cfg["num_prev_states"] - 1, :2])).sum(-1)
        if diag is not None:
            diag.setdefault("target_raw_plus_eps", []).extend((raw.detach() + cfg["target_dir_len_eps"]).tolist())
        L["TARGET_LOSS"] = raw.clamp(min=-cfg["target_dir_len_eps"]) * cfg["weights"]["w_target"]
        bounds["TARGET_LOSS"] = torch.zeros_like(raw.detach())
    return L, bounds


def reduce(losses, ood_mask=None):
    """mdm.py:936-940 (not in place here) and :953-958"""
    total = 0.0
    for k, v in losses.items():
        if ood_mask is not None and k not in UNMASKED:
            v = torch.where(ood_mask, torch.zeros_like(v), v)
        total = total + v.mean()
    return total


# ------------------------------------------------------------------------------------------------------------------- fixture access
def reference_root():
    """where the fixture generators look for the reference tree: $PARC_REFERENCE, else the default that tests/golden/gen_golden.py names
    (read from its source; importing it would already need the tree)"""
    import re
    with open(os.path.join(HERE, "golden", "gen_golden.py")) as f:
        default = re.search(r'^REF = os\.environ\.get\("PARC_REFERENCE", "([^"]+)"\)', f.read(), re.M).group(1)
    return os.environ.get("PARC_REFERENCE", default)


def load_fixture():
    import json
    z = np.load(G33)
    with open(G33_JSON) as f:
        meta = json.load(f)
    return z, meta


def true_windows(case):
    """the case's true motion windows from the clips committed with G32, the root of frame num_prev_states - 1 moved over the origin"""
    z = np.load(G32)
    S, ref = case["S"], case["num_prev_states"] - 1
    out = {k: [] for k in ("ROOT_POS", "ROOT_ROT", "JOINT_ROT", "CONTACTS")}
    for clip, t0 in case["windows"]:
        rp = z["c%d_root_pos" % clip][t0:t0 + S].astype(np.float32).copy()
        rp[:, :2] -= rp[ref, :2]
        out["ROOT_POS"].append(rp)
        out["ROOT_ROT"].append(z["c%d_root_rot" % clip][t0:t0 + S])
        out["JOINT_ROT"].append(z["c%d_joint_rot" % clip][t0:t0 + S])
        out["CONTACTS"].append(z["c%d_contacts" % clip][t0:t0 + S])
    return {k: np.stack(v).astype(np.float32) for k, v in out.items()}


def case_points(z):
    counts = z["point_counts"]
    pts, out, i = torch.tensor(z["points"]), [], 0
    for n in counts:
        out.append(pts[i:i + int(n)])
        i += int(n)
    return out


def case_eval(model, case, z, with_grad=True, diag=None, x=None):
    """float64 losses, bounds and the two reduced gradients (without / with the ood mask) of case `case` of the fixture"""
    n = case["name"]
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=F64)
    true = {k: t64(v) for k, v in true_windows(case).items()}
    if "JOINT_POS" in case["components"]:
        true["JOINT_POS"] = forward_kinematics(model, true["ROOT_POS"], true["ROOT_ROT"], true["JOINT_ROT"])[0][..., 1:, :]
    mean, std = t64(z[n + "_mean"]), t64(z[n + "_std"])
    xx = (t64(z[n + "_x"]) if x is None else x).clone().requires_grad_(with_grad)
    args = (model, case, true, xx, mean, std, t64(z[n + "_hfs"]), t64(z[n + "_target_dir"]), case_points(z), case["loss_fn"])
    L, bounds = motion_loss(*args, diag=diag)
    out = dict(losses=L, bounds=bounds, true=true, mean=mean, std=std)
    if with_grad:
        out["grad"] = torch.autograd.grad(reduce(L), xx, retain_graph=True)[0]
        out["grad_ood"] = torch.autograd.grad(reduce(L, torch.tensor(z[n + "_ood_mask"])), xx)[0]
    return out


def rel_err(got, want, unit):
    return float((np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / unit).max())


def measure_ebar(model=None, which="cases"):
    """(e-bar of the losses relative to max(1, |value|), e-bar of the gradients relative to the per-sample max) over G33's six cases
    (which="cases") or over its two cases of other rot_types (which="rot_cases")"""
    if model is None:
        from parc_amd.anim import kin_char_model as kcm
        km = kcm.KinCharModel("cpu")
        km.load_char_file(kcm.default_char_file())
        model = model_from_char(km)
    z, meta = load_fixture()
    e_loss, e_grad = 0.0, 0.0
    for case in meta[which]:
        n = case["name"]
        r = case_eval(model, case, z)
        for k, v in r["losses"].items():
            want = v.detach().numpy()
            e_loss = max(e_loss, rel_err(z[n + "_loss_" + k], want, np.maximum(1.0, np.abs(want))))
        for key in ("grad", "grad_ood"):
            want = r[key].numpy()
            unit = np.abs(want).reshape(want.shape[0], -1).max(-1).reshape(-1, 1, 1)
            e_grad = max(e_grad, rel_err(z[n + "_" + key], want, np.where(unit > 0, unit, 1.0)))
    return e_loss, e_grad


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    el, eg = measure_ebar()
    print("e-bar losses   %.3e" % el)
    print("e-bar gradient %.3e" % eg)
    el, eg = measure_ebar(which="rot_cases")
    print("e-bar losses   %.3e (rot_type EXP_MAP / QUAT cases)" % el)
    print("e-bar gradient %.3e (rot_type EXP_MAP / QUAT cases)" % eg)
