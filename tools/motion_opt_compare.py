#!/usr/bin/env python
"""What the motion optimiser computes and launches, dumped from the tree this file sits in, and two or more such dumps compared.

  python tools/motion_opt_compare.py --dump DIR
      runs, through the public functions only, on fixture G20 and the motions A, B, C derived from it (tests/tools/moopt_host.three_motions):
      motion_terrain_contact_loss (full and nocon: terms, total, gradient), motion_terrain_contact_loss_batch of (A, B, C), the
      40-iteration descents single and batch, eager and replayed (traces and frames), compute_approx_body_constraints and its batch
      form, and the number of kernel launches of one whole warm call of motion_contact_optimization(num_iters=3, use_graph=False) and
      of the batch call for M = 1 and M = 3 (and of the same calls with num_iters=0: what is launched around the iterations).
      Every array goes to DIR/<name>.npy.
  python tools/motion_opt_compare.py --compare DIR_A DIR_B [DIR_B2 ...] [--bench-a F ...] [--bench-b F ...] [--json OUT] [--note TEXT]
      prints, per array, whether DIR_A equals DIR_B bit for bit, else the largest difference; with several DIR_B (repeated runs of one
      tree) also their own spread, and the verdict: equal where they agree with each other, within twice their spread where they do
      not; launch counts must be equal.  --bench-a / --bench-b: result files of tools/bench_motion_opt_batch.py run in the two trees;
      tree A's median of every series must lie inside tree B's fastest-to-slowest range.

A refactor of the host code is checked by dumping from a checkout of the parent commit (three times) and from the branch (once).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
W_NAMES = ("w_root_pos", "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding", "w_body_constraints", "w_jerk")
SERIES = ("opt_batch_ms", "opt_loop_ms", "bc_batch_ms", "bc_loop_ms")


def dump(out_dir):
    import torch
    import moopt_host as mh
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.util import terrain_util, torch_util
    dev = "cuda:0"
    os.makedirs(out_dir, exist_ok=True)
    T = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=dev)
    save = lambda name, x: np.save(os.path.join(out_dir, name + ".npy"), x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x))
    km = KinCharModel(dev)
    km.load_char_file(humanoid_spec.write_mjcf())
    g = mh.g20()
    counts = [int(n) for n in g["pts_count"]]
    pts = [T(p) for p in np.split(g["pts"], np.cumsum(counts)[:-1])]
    w = dict(zip(W_NAMES, [float(v) for v in g["weights"][:9]]))
    max_jerk = float(g["weights"][9])
    motions = mh.three_motions(g)
    names = "ABC"
    print("motion_optimization from", mo.__file__)

    def constraints(rows):
        if rows is None:
            return None
        out = [[] for _ in range(km.get_num_joints())]
        for r in rows:
            c = mo.BodyConstraint()
            c.start_frame_idx, c.end_frame_idx, c.constraint_point = int(r[1]), int(r[2]), T(r[3:6])
            out[int(r[0])].append(c)
        return out

    src, tgt, con = ([T(m[k]) for m in motions] for k in ("frames", "tgt", "contacts"))
    ter = [terrain_util.SubTerrain.from_arrays(m["hf"], m["min_point"], m["dxdy"], device=dev) for m in motions]
    bc = [constraints(m["rows"]) for m in motions]
    rows_of = lambda lists: np.array([[b, c.start_frame_idx, c.end_frame_idx] + c.constraint_point.tolist() for b, lst in enumerate(lists) for c in lst],
                                     dtype=np.float64).reshape(-1, 6)

    def poses(f):
        rp, rq, jr = f[:, 0:3].contiguous(), torch_util.exp_map_to_quat(f[:, 3:6]), km.dof_to_rot(f[:, 6:].contiguous())
        return rp, rq, jr

    # ------------------------------------------------------------------ the loss at the target frames
    rp, rq, jr = poses(src[0])
    bp, br = km.forward_kinematics(rp, rq, jr)
    source = (rp, rq, jr, bp[1:] - bp[:-1], torch_util.quat_diff_angle(br[1:], br[:-1]))
    for case in ("full", "nocon"):
        wc = w if case == "full" else dict(w, w_contact=0.0, w_sliding=0.0)
        p = [tgt[0][:, 0:3].clone().requires_grad_(True), tgt[0][:, 3:6].clone().requires_grad_(True), tgt[0][:, 6:].clone().requires_grad_(True)]
        loss, ld = mo.motion_terrain_contact_loss(*p, *source, con[0], ter[0], pts, km, body_constraints=bc[0] if case == "full" else None,
                                                  max_jerk=max_jerk, **wc)
        loss.backward()
        save("loss_" + case + "_terms", np.array([ld[k] for k in sorted(ld, key=lambda k: k.value)], dtype=np.float64))
        save("loss_" + case + "_total", loss)
        save("loss_" + case + "_grad", torch.cat([x.grad for x in p], dim=-1))
    totals, terms, grads = mo.motion_terrain_contact_loss_batch(tgt, src_frames=src, contacts=con, terrains=ter, body_points=pts, char_model=km,
                                                                body_constraints=bc, max_jerk=max_jerk, **w)
    save("loss_batch_totals", totals)
    save("loss_batch_terms", terms)
    for m in range(3):
        save("loss_batch_grad_" + names[m], grads[m])

    # ------------------------------------------------------------------ the 40-iteration descents
    def single(num_iters, use_graph, trace=None):
        return mo.motion_contact_optimization(src_frames=src[0], contacts=con[0], body_points=pts, terrain=ter[0], char_model=km, num_iters=num_iters,
                                              step_size=0.001, body_constraints=bc[0], max_jerk=max_jerk, exp_name="a", use_wandb=False, log_file=None,
                                              use_graph=use_graph, verbose=False, loss_trace=trace, **w)

    def batch(ids, num_iters, use_graph, trace=None):
        return mo.motion_contact_optimization_batch(src_frames=[src[i] for i in ids], contacts=[con[i] for i in ids], body_points=pts,
                                                    terrains=[ter[i] for i in ids], char_model=km, num_iters=num_iters, step_size=0.001,
                                                    body_constraints=[bc[i] for i in ids], max_jerk=max_jerk, exp_names=[names[i] for i in ids],
                                                    use_wandb=False, log_files=[None] * len(ids), use_graph=use_graph, verbose=False, loss_trace=trace,
                                                    **w)

    for use_graph in (False, True):
        tag = "replayed" if use_graph else "eager"
        trace = []
        save("descent_single_" + tag + "_frames", single(40, use_graph, trace))
        save("descent_single_" + tag + "_trace", trace[0])
        trace = []
        outs = batch([0, 1, 2], 40, use_graph, trace)
        save("descent_batch_" + tag + "_trace", trace[0])
        for m in range(3):
            save("descent_batch_" + tag + "_frames_" + names[m], outs[m])

    # ------------------------------------------------------------------ constraints from the contact labels
    save("constraints_single", rows_of(mo.compute_approx_body_constraints(rp, rq, jr, con[0], km, ter[0])))
    two = [poses(src[i]) for i in (0, 1)]
    got = mo.compute_approx_body_constraints_batch([x[0] for x in two], [x[1] for x in two], [x[2] for x in two], [con[0], con[1]], km,
                                                   [ter[0], ter[1]])
    for k in range(2):
        save("constraints_batch_" + names[k], rows_of(got[k]))

    # ------------------------------------------------------------------ kernel launches of whole warm calls
    def kernel_count(fn):
        from torch.profiler import ProfilerActivity, profile
        fn()                                                    # warm
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name])

    for n in (3, 0):
        save("launches_single_%diters" % n, np.array(kernel_count(lambda: single(n, False))))
        save("launches_batch_m1_%diters" % n, np.array(kernel_count(lambda: batch([0], n, False))))
        save("launches_batch_m3_%diters" % n, np.array(kernel_count(lambda: batch([0, 1, 2], n, False))))
    print("dumped", len(os.listdir(out_dir)), "arrays to", out_dir)


def compare(dir_a, dirs_b, bench_a, bench_b, json_out, note=None):
    doc, ok = {"arrays": {}, "launches": {}}, True
    if note:
        doc["note"] = note
    names = sorted(f[:-4] for f in os.listdir(dirs_b[0]) if f.endswith(".npy"))
    missing = [n for d in [dir_a] + dirs_b for n in names if not os.path.exists(os.path.join(d, n + ".npy"))]
    assert not missing and names == sorted(f[:-4] for f in os.listdir(dir_a) if f.endswith(".npy")), ("the dumps hold different arrays", missing)
    same = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
    diff = lambda x, y: float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.shape == y.shape and x.size else (0.0 if x.shape == y.shape else float("inf"))
    for n in names:
        a, bs = np.load(os.path.join(dir_a, n + ".npy")), [np.load(os.path.join(d, n + ".npy")) for d in dirs_b]
        if n.startswith("launches_"):
            good = all(int(b) == int(a) for b in bs)
            doc["launches"][n] = {"a": int(a), "b": [int(b) for b in bs], "verdict": "equal" if good else "DIFFERENT"}
            print("{:38s} a {:5d}  b {}  {}".format(n, int(a), [int(b) for b in bs], doc["launches"][n]["verdict"]))
        else:
            stable = all(same(bs[0], b) for b in bs[1:])
            spread = max([diff(x, y) for i, x in enumerate(bs) for y in bs[i + 1:]] + [0.0])
            d = max(diff(a, b) for b in bs)
            if stable:
                good = same(a, bs[0])
                verdict = "bit-identical" if good else "DIFFERENT (b agrees with itself bit for bit)"
            else:
                good = d <= 2.0 * spread
                verdict = "within twice b's own spread" if good else "DIFFERENT (beyond twice b's own spread)"
            doc["arrays"][n] = {"b_runs_bit_identical": stable, "b_spread": spread, "max_abs_diff_a_b": d, "verdict": verdict}
            print("{:38s} b spread {:.3e}  |a - b| {:.3e}  {}".format(n, spread, d, verdict))
        ok = ok and good
    if bench_a or bench_b:
        doc["speed"] = {}
        load = lambda files: [json.load(open(f)) for f in files]
        res_a, res_b = load(bench_a), load(bench_b)
        for M in sorted({r["M"] for d in res_b for r in d["results"]}):
            for key in SERIES:
                va = [v for d in res_a for r in d["results"] if r["M"] == M for v in r[key]]
                vb = [v for d in res_b for r in d["results"] if r["M"] == M for v in r[key]]
                med = statistics.median(va)
                where = "inside b's range" if min(vb) <= med <= max(vb) else "BELOW b's fastest" if med < min(vb) else "ABOVE b's slowest"
                doc["speed"]["M%d_%s" % (M, key)] = {"a_ms": va, "b_ms": vb, "a_median_ms": med, "b_median_ms": statistics.median(vb),
                                                      "b_range_ms": [min(vb), max(vb)], "verdict": where}
                print("M={:<3d}{:13s} a median {:10.3f} ms  b range {:10.3f} .. {:10.3f} ms  {}".format(M, key, med, min(vb), max(vb), where))
                ok = ok and where.startswith("inside")
    doc["verdict"] = "pass" if ok else "FAIL"
    if json_out:
        with open(json_out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("verdict:", doc["verdict"])
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--compare", nargs="+", metavar="DIR", help="DIR_A DIR_B [DIR_B2 ...]")
    ap.add_argument("--bench-a", nargs="*", default=[])
    ap.add_argument("--bench-b", nargs="*", default=[])
    ap.add_argument("--json", default=None)
    ap.add_argument("--note", default=None, help="free text kept in the JSON")
    args = ap.parse_args()
    if args.dump:
        dump(args.dump)
        return 0
    assert args.compare and len(args.compare) >= 2, "--compare DIR_A DIR_B [DIR_B2 ...]"
    return compare(args.compare[0], args.compare[1:], args.bench_a, args.bench_b, args.json, args.note)


if __name__ == "__main__":
    sys.exit(main())
