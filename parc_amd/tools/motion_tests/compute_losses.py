"""Penetration, floating-contact and jerk statistics of a set of motion files.

Mirror of the reference's ``tools/motion_tests/compute_losses.py``: per file the length, the jerk figures (:158-169), and the contact
and penetration losses of ``compute_motion_loss`` at weights 1 (:171-191); then the mean / std summary under the reference's column
names (:43-73), overall and per group.  A group is the file name without its trailing ``_<digits>`` (:123).  Every file is one call of
the motion scorer (tools/procgen/mdm_path.MotionScorer): the reference runs forward kinematics twice and ~30 distance queries per file.

    python -m parc_amd.tools.motion_tests.compute_losses --motions <dir | dataset yaml> --out <csv>
"""
import argparse
import csv
import math
import os
import re
from collections import OrderedDict

MAX_JERK = 11666.3906           # compute_losses.py:78
FPS = 30.0                      # :150, :158
FILE_COLUMNS = ["file", "group", "motion_length", "mean_jerk", "frames_with_jerk_over_X", "contact_loss", "pen_loss", "final_node_dist"]
STATS = ["final_node_dist", "motion_length", "mean_jerk", "frames_with_jerk_over_X", "contact_loss", "pen_loss"]
# the per-group columns of the reference drop the underscores of three names (:60-71)
_GROUP_LABEL = {"final_node_dist": "final node dist", "motion_length": "motion length", "mean_jerk": "mean jerk",
                "frames_with_jerk_over_X": "frames_with_jerk_over_X", "contact_loss": "contact loss", "pen_loss": "pen loss"}


def group_of(path):
    """file name without extension and without a trailing _<digits> (compute_losses.py:123)"""
    return re.sub(r"_\d+$", "", os.path.splitext(os.path.basename(path))[0])


def motion_paths(motions):
    """--motions: a directory (its .pkl files, sorted) or a dataset yaml (its `motions: - file: ...` rows)"""
    if os.path.isdir(motions):
        return [os.path.join(motions, f) for f in sorted(os.listdir(motions)) if os.path.splitext(f)[1] == ".pkl"]
    import yaml
    with open(motions) as f:
        doc = yaml.safe_load(f)
    return [m["file"] for m in doc["motions"]]


def mean_std(values):
    """mean and the sample standard deviation torch.std gives (NaN for fewer than two values); values that are None are left out"""
    v = [float(x) for x in values if x is not None]
    if not v:
        return float("nan"), float("nan")
    m = sum(v) / len(v)
    if len(v) < 2:
        return m, float("nan")
    return m, math.sqrt(sum((x - m) ** 2 for x in v) / (len(v) - 1))


def summary_header(groups):
    h = ["exp_name"]
    for k in STATS:
        h += [k + " mean", k + " std"]
    for g in groups:
        for k in STATS:
            h += [g + _GROUP_LABEL[k] + " mean", g + _GROUP_LABEL[k] + " std"]
    return h


def summarize(rows, exp_name):
    """(header, row): the reference's summary line over the per-file rows, overall first and then per group in order of appearance"""
    groups = list(OrderedDict((r["group"], None) for r in rows))
    out = [exp_name]
    for k in STATS:
        out += list(mean_std([r.get(k) for r in rows]))
    for g in groups:
        for k in STATS:
            out += list(mean_std([r.get(k) for r in rows if r["group"] == g]))
    return summary_header(groups), out


def compute_metrics(paths, char_model, body_points=None, max_jerk=MAX_JERK, device=None):
    """One dict per file with the FILE_COLUMNS (final_node_dist None when the file carries no path_nodes)."""
    import torch

    from ...util import geom_util, motion_util
    from ...zmotion_editing_tools import motion_edit_lib as medit_lib
    from ..procgen import mdm_path
    device = char_model._device if device is None else device
    if body_points is None:
        body_points = geom_util.get_char_point_samples(char_model)
    rows, pending = [], []
    for path in paths:
        md = medit_lib.load_motion_file(path, device=device)
        frames, contacts, terrain = md.get_frames(), md.get_contacts(), md.get_terrain()
        if frames.dim() == 3 and frames.shape[0] == 1:
            frames = frames.squeeze(0)
        if contacts.dim() == 3 and contacts.shape[0] == 1:
            contacts = contacts.squeeze(0)
        mf = motion_util.motion_frames_from_mlib_format(frames.contiguous(), char_model=char_model, contacts=contacts).unsqueeze(0)
        sc = mdm_path.MotionScorer(char_model, body_points, terrain).score(mf, 1.0, 1.0, dt=1.0 / FPS, max_jerk=max_jerk)
        dist = None
        if "path_nodes" in md._data:
            dist = torch.linalg.norm(frames[-1, 0:2] - md._data["path_nodes"][-1, 0:2].to(frames))
        rows.append({"file": os.path.basename(path), "group": group_of(path), "motion_length": frames.shape[0] / FPS})
        pending.append((sc, dist))
    for r, (sc, dist) in zip(rows, pending):          # the host reads, after every file is queued
        r["mean_jerk"], r["frames_with_jerk_over_X"] = float(sc.mean_jerk[0]), float(sc.frac_over[0])
        r["contact_loss"], r["pen_loss"] = float(sc.contact_loss[0]), float(sc.pen_loss[0])
        r["final_node_dist"] = None if dist is None else float(dist)
    return rows


def write_csv(rows, out, exp_name):
    header, line = summarize(rows, exp_name)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(FILE_COLUMNS)
        for r in rows:
            w.writerow(["" if r.get(k) is None else r[k] for k in FILE_COLUMNS])
        w.writerow([])
        w.writerow(header)
        w.writerow(line)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--motions", required=True, help="a directory of motion .pkl files, or a dataset yaml")
    ap.add_argument("--out", required=True, help="csv to write")
    ap.add_argument("--char_file", default=None, help="MJCF of the character (default: the packaged humanoid)")
    ap.add_argument("--max_jerk", type=float, default=MAX_JERK)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from ...anim.kin_char_model import KinCharModel
    from ...assets import humanoid_spec
    km = KinCharModel(args.device)
    km.load_char_file(args.char_file or humanoid_spec.write_mjcf())
    rows = compute_metrics(motion_paths(args.motions), km, max_jerk=args.max_jerk)
    write_csv(rows, args.out, args.motions)
    print("wrote", args.out, "({} files)".format(len(rows)))


if __name__ == "__main__":
    main()
