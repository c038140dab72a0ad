"""Float64 numpy restatement of the generator's training-batch sampler (reference diffusion/mdm_heightfield_contact_motion_sampler.py
with the functions it calls) -- TEST INFRASTRUCTURE.  Reads fixture G32 (tests/golden/g32_mdm_sampler.npz, written by
tests/golden/gen_mdm_sampler.py from the reference's own sampler) and evaluates every case from the recorded draws.

Used three ways: by the fixture generator for its preconditions (no grid lookup within 1e-3 cells of a rounding tie, no reference heading
within 1e-3 of the atan2 branch, at most 2 % of a sample's cells within 1e-4 cells of a box edge), by measure_ebar() - the largest
|reference fp32 - float64| over the fixture, the unit of the tests' bounds -, and by the tests as the second thing both builds of
parc_mdm_batch_core.h are compared against.
"""
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "g32_mdm_sampler.npz")
MODES = {"NOISE": 0, "MAXPOOL_AND_BOXES": 1, "NONE": 2}
Z_STYLES = {"RELATIVE_TO_ROOT": 0, "RELATIVE_TO_ROOT_FLOOR": 1}
EDGE_EPS = 1e-4         # cells: a cell this close to a box edge may fall on either side in fp32
EDGE_SHARE = 0.02       # at most this share of a sample's cells may be that close
MOTION_KEYS = ("root_pos", "root_rot", "body_pos", "joint_rot", "contacts")


def load(path=FIXTURE):
    z = {k: v for k, v in np.load(path).items()}
    meta = json.loads(str(z["meta"]))
    return z, meta


def clip_tables(z, meta):
    clips = []
    for c in range(meta["clips"]):
        g = lambda k: z["c%d_%s" % (c, k)]          # noqa: E731
        clips.append(dict(root_pos=g("root_pos"), root_rot=g("root_rot"), joint_rot=g("joint_rot"), contacts=g("contacts"), fps=float(g("fps")),
                          loop=int(g("loop")), length=np.float32(g("length")), pos_delta=g("pos_delta"), hf=g("hf"), hf_maxmin=g("hf_maxmin"),
                          min_point=g("min_point"), dxdy=g("dxdy"), cell_start=g("cell_start"), cells=g("cells")))
    return clips


def case_arrays(z, k):
    p = "k%d_" % k
    return {key[len(p):]: v for key, v in z.items() if key.startswith(p)}


# ------------------------------------------------------------------------------------------------------------------- quaternions (xyzw)
def quat_mul(a, b):
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
                     w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def quat_rotate(q, v):
    qv, qw = q[..., :3], q[..., 3:]
    t = 2 * np.cross(qv, v)
    return v + qw * t + np.cross(qv, t)


def calc_heading(q):
    d = quat_rotate(q, np.array([1.0, 0.0, 0.0]))
    return math.atan2(d[1], d[0])


def heading_quat(angle):
    return np.array([0.0, 0.0, math.sin(angle / 2), math.cos(angle / 2)])


def slerp(q0, q1, t):
    c = np.sum(q0 * q1, -1, keepdims=True)
    q1 = np.where(c < 0, -q1, q1)
    c = np.abs(c)
    with np.errstate(invalid="ignore", divide="ignore"):
        ht = np.arccos(np.minimum(c, 1.0))
        s = np.sqrt(np.maximum(1.0 - c * c, 0.0))
        out = np.sin((1 - t) * ht) / s * q0 + np.sin(t * ht) / s * q1
    out = np.where(np.abs(s) < 0.001, 0.5 * q0 + 0.5 * q1, out)
    return np.where(c >= 1, q0, out)


# ------------------------------------------------------------------------------------------------------------------- clip lookup
def lookup(clip, time):
    """root_pos [3], quats [B, 4] (root first), contacts [B] at `time`; the inputs are the fixture's fp32 values, the arithmetic float64"""
    length = float(clip["length"])
    nf = clip["root_pos"].shape[0]
    phase = time / length
    loop_phase = math.floor(phase)
    if clip["loop"] == 1:
        phase = phase - math.floor(phase)
    phase = min(max(phase, 0.0), 1.0)
    fp = phase * (nf - 1)
    i0 = int(fp)
    i1 = min(i0 + 1, nf - 1)
    b = fp - i0
    pos = (1 - b) * clip["root_pos"][i0].astype(np.float64) + b * clip["root_pos"][i1].astype(np.float64)
    if clip["loop"] == 1:
        pos = pos + loop_phase * clip["pos_delta"].astype(np.float64)
    q0 = np.concatenate([clip["root_rot"][i0][None], clip["joint_rot"][i0]]).astype(np.float64)
    q1 = np.concatenate([clip["root_rot"][i1][None], clip["joint_rot"][i1]]).astype(np.float64)
    con = (1 - b) * clip["contacts"][i0].astype(np.float64) + b * clip["contacts"][i1].astype(np.float64)
    return pos, slerp(q0, q1, b), con


def forward_kinematics(model, root_pos, root_rot, joint_rot):
    B = len(model["parent"])
    pos, rot = [root_pos], [root_rot]
    for j in range(1, B):
        p = int(model["parent"][j])
        pos.append(pos[p] + quat_rotate(rot[p], model["local_translation"][j].astype(np.float64)))
        rot.append(quat_mul(rot[p], quat_mul(model["local_rotation"][j].astype(np.float64), joint_rot[j - 1])))
    return np.stack(pos), np.stack(rot)


# ------------------------------------------------------------------------------------------------------------------- heightfields
def _round_half_even(x):
    return np.rint(x)


def _pool(hf, r, axis):
    X = hf.shape[axis]
    out = np.empty_like(hf)
    for i in range(X):
        lo, hi = max(i - r, 0), min(i + r, X - 1)
        sl = [slice(None)] * 2
        sl[axis] = slice(lo, hi + 1)
        dst = [slice(None)] * 2
        dst[axis] = i
        out[tuple(dst)] = hf[tuple(sl)].max(axis=axis)
    return out


def heightfield(cfg, clip, start, ref_pos, ref_rot, draws, s, info=None):
    """one sample: returns (hfs [X, Y], center_h, pre [3, X, Y], cell [X, Y], masked [X, Y], unsafe [X, Y])"""
    X, Y = cfg["dim_x"], cfg["dim_y"]
    S = cfg["seq_len"]
    nf = len(clip["cell_start"]) - 1
    TX, TY = clip["hf"].shape
    f0 = int(np.rint(np.float32(start) / np.float32(cfg["dt"])))         # the index is the reference's fp32 expression
    f0c, f1c = min(max(f0, 0), nf), min(max(f0 + S, 0), nf)
    mask = np.zeros(TX * TY, bool)
    mask[clip["cells"][clip["cell_start"][f0c]:clip["cell_start"][f1c]]] = True
    heading = calc_heading(ref_rot)
    gx, gy = np.meshgrid(cfg["grid_x"].astype(np.float64), cfg["grid_y"].astype(np.float64), indexing="ij")
    px = gx * math.cos(heading) - gy * math.sin(heading) + ref_pos[0]
    py = gx * math.sin(heading) + gy * math.cos(heading) + ref_pos[1]
    fx = (px - float(clip["min_point"][0])) / float(clip["dxdy"][0])
    fy = (py - float(clip["min_point"][1])) / float(clip["dxdy"][1])
    if info is not None:
        tie = np.minimum(np.abs(fx - np.floor(fx) - 0.5), np.abs(fy - np.floor(fy) - 0.5))
        inside = (fx > -0.5 - 1e-3) & (fx < TX - 0.5 + 1e-3) & (fy > -0.5 - 1e-3) & (fy < TY - 0.5 + 1e-3)
        info["tie"] = float(np.min(np.where(inside, tie, 1.0)))
        info["heading"] = heading
        info["outside"] = bool(np.any((fx < -0.5) | (fx > TX - 0.5) | (fy < -0.5) | (fy > TY - 0.5)))
        info["window_past_end"] = f0 + S > nf
    ti = np.clip(_round_half_even(fx), 0, TX - 1).astype(np.int64)
    tj = np.clip(_round_half_even(fy), 0, TY - 1).astype(np.int64)
    cell = ti * TY + tj
    masked = mask[cell]
    hf = clip["hf"].astype(np.float64).reshape(-1)[cell]
    band = clip["hf_maxmin"].astype(np.float64).reshape(-1, 2)[cell]
    max_h, min_h = float(np.float32(cfg["max_h"])), float(np.float32(cfg["min_h"]))
    bmax = np.where(masked, band[..., 0], 2.0 * max_h)
    bmin = np.where(masked, band[..., 1], 2.0 * min_h)
    center = hf[cfg["num_x_neg"], cfg["num_y_neg"]]
    sub = center if cfg["z_style"] == 1 else ref_pos[2]
    hf, bmax, bmin = hf - sub, bmax - sub, bmin - sub
    pre = np.stack([hf, bmax, bmin])
    unsafe = np.zeros((X, Y), bool)
    clamp = lambda x, lo, hi: np.minimum(np.maximum(x, lo), hi)     # noqa: E731  (torch.clamp, also where lo > hi)
    if cfg["mode"] == 0:
        hf = clamp(draws["noise"][s].astype(np.float64), bmax, bmin)
    elif cfg["mode"] == 1:
        if draws["change"][s]:
            hf = np.full_like(hf, float(draws["new_h"][s]))
        for q in range(3):
            kind, r = int(draws["pool_kind"][s, q]), int(draws["pool_r"][s, q])
            if kind < 0:
                continue
            if kind == 0:
                hf = _pool(_pool(hf, r, 1), r, 0)
            else:
                hf = _pool(hf, r, 0 if kind == 1 else 1)
            hf = clamp(hf, bmin, bmax)
        ii, jj = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), indexing="ij")
        for b in range(int(draws["nboxes"][s])):
            cx, cy, lx, ly, ang, h = (float(v) for v in draws["boxes"][s, b])
            ddx, ddy = ii - cx, jj - cy
            tx = ddx * math.cos(ang) - ddy * math.sin(ang)
            ty = ddx * math.sin(ang) + ddy * math.cos(ang)
            inside = (np.abs(tx) < lx / 2) & (np.abs(ty) < ly / 2)
            # near an edge while inside (or on) the other axis' range
            near = ((np.abs(np.abs(tx) - lx / 2) < EDGE_EPS) & (np.abs(ty) < ly / 2 + EDGE_EPS)) | \
                   ((np.abs(np.abs(ty) - ly / 2) < EDGE_EPS) & (np.abs(tx) < lx / 2 + EDGE_EPS))
            unsafe |= near
            hf = np.where(inside, h, hf)
        hf = clamp(hf, bmin, bmax)
    hf = clamp(hf, min_h, max_h)
    return hf, center, pre, cell, masked, unsafe


# ------------------------------------------------------------------------------------------------------------------- a whole case
def case_cfg(meta, z, k):
    c = dict(meta["cases"][k]["cfg"])
    a = case_arrays(z, k)
    c.update(grid_x=a["grid_x"], grid_y=a["grid_y"], motion_times=a["motion_times"], mode=MODES[c["mode"]], z_style=Z_STYLES[c["z_style"]])
    c["dim_x"], c["dim_y"] = len(a["grid_x"]), len(a["grid_y"])
    c["num_x_neg"], c["num_y_neg"] = c["grid"][0], c["grid"][2]
    c["seq_len"] = len(a["motion_times"])
    c["dt"] = np.float32(1.0 / c["fps"])
    c["min_h"] = -c["max_h"]
    return c


def case64(z, meta, k, model, clips):
    """every output of case k in float64, and per-sample diagnostics"""
    cfg = case_cfg(meta, z, k)
    a = case_arrays(z, k)
    n, S, B = len(a["ids"]), cfg["seq_len"], len(model["parent"])
    X, Y = cfg["dim_x"], cfg["dim_y"]
    out = dict(root_pos=np.zeros((n, S, 3)), root_rot=np.zeros((n, S, 4)), body_pos=np.zeros((n, S, B - 1, 3)), joint_rot=np.zeros((n, S, B - 1, 4)),
               contacts=np.zeros((n, S, B)), hfs=np.zeros((n, X, Y)), center_h=np.zeros(n), future_pos=np.zeros((n, 3)), future_rot=np.zeros((n, 4)),
               pre=np.zeros((n, 3, X, Y)), cell=np.zeros((n, X, Y), np.int64), masked=np.zeros((n, X, Y), bool), unsafe=np.zeros((n, X, Y), bool))
    infos = []
    for s in range(n):
        clip = clips[int(a["ids"][s])]
        start = float(a["starts"][s])
        times = [float(np.float32(a["starts"][s]) + np.float32(t)) for t in cfg["motion_times"]]        # the time is the fp32 sum
        ref_pos, ref_q, _ = lookup(clip, times[cfg["ref_idx"]])
        info = {}
        hf, center, pre, cell, masked, unsafe = heightfield(cfg, clip, start, ref_pos, ref_q[0], a, s, info)
        infos.append(info)
        out["hfs"][s], out["center_h"][s], out["pre"][s], out["cell"][s], out["masked"][s], out["unsafe"][s] = hf, center, pre, cell, masked, unsafe
        hinv = heading_quat(-calc_heading(ref_q[0]))
        for f in range(S):
            pos, q, con = lookup(clip, times[f])
            if cfg["z_style"] == 1:
                pos = pos - np.array([0.0, 0.0, center])
            pos = quat_rotate(hinv, pos - ref_pos)
            rr = quat_mul(hinv, q[0])
            bp, _ = forward_kinematics(model, pos, rr, q[1:])
            out["root_pos"][s, f], out["root_rot"][s, f], out["body_pos"][s, f], out["joint_rot"][s, f], out["contacts"][s, f] = pos, rr, bp[1:], q[1:], con
        fpos, fq, _ = lookup(clip, float(a["future_time"][s]))
        fpos = fpos + a["future_noise"][s].astype(np.float64)
        out["future_pos"][s] = quat_rotate(hinv, fpos - ref_pos)
        out["future_rot"][s] = quat_mul(hinv, fq[0])
        info["future_past_end"] = float(a["future_time"][s]) > float(clip["length"])
    return out, infos


def model_tables(z):
    return dict(parent=z["model_parent"], local_translation=z["model_local_translation"], local_rotation=z["model_local_rotation"])


COMPARED = MOTION_KEYS + ("future_pos", "future_rot", "hfs", "center_h")


def measure_ebar(z, meta):
    """the largest |reference fp32 - float64| over the fixture's motion tensors, targets and heights (cells near a box edge excluded)"""
    model, clips = model_tables(z), clip_tables(z, meta)
    worst = 0.0
    for k in range(len(meta["cases"])):
        out, _ = case64(z, meta, k, model, clips)
        a = case_arrays(z, k)
        for key in COMPARED:
            d = np.abs(a[key].astype(np.float64) - out[key])
            if key == "hfs":
                d = np.where(out["unsafe"], 0.0, d)
            worst = max(worst, float(d.max()) if d.size else 0.0)
    return worst


if __name__ == "__main__":
    z_, meta_ = load()
    print("e-bar = %.6e" % measure_ebar(z_, meta_))
