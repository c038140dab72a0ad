#!/usr/bin/env python
"""Time the batched motion optimiser against the loop over the single-motion path.

For M = 1, 8, 32 clips of synthetic.make_dataset(num_clips=M, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45)), with body
constraints from the contact labels and 300 iterations each:
  * motion_contact_optimization_batch on all M clips (one descent, replayed graph)      -- "batch"
  * a loop of the unchanged motion_contact_optimization over the same clips             -- "loop" (the yardstick)
  * compute_approx_body_constraints_batch against a loop of compute_approx_body_constraints, the same way.
Host clock with a synchronise at both ends, a warm-up call first, 5 repeats per configuration with the two configurations
interleaved.  Every repeat is printed and written to profiles/motion_opt_batch.json.  Without a device the JSON says "not measured".

Each M runs in a child process of its own under a time limit (usage: python tools/bench_motion_opt_batch.py [--m 1 8 32] [--iters 300]);
a child that fails or runs out of time ends the run - nothing more is started on the device after it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "motion_opt_batch.json")
W = dict(w_root_pos=1.0, w_root_rot=10.0, w_joint_rot=1.0, w_smoothness=10.0, w_penetration=1000.0, w_contact=1000.0, w_sliding=10.0,
         w_body_constraints=1000.0, w_jerk=1000.0)


def measure(M, iters, repeats):
    """one configuration pair in this process -> dict"""
    import torch
    from parc_amd import synthetic
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.util import geom_util, terrain_util, torch_util
    dev = "cuda:0"
    km = KinCharModel(dev)
    km.load_char_file(humanoid_spec.write_mjcf())
    body_points = geom_util.get_char_point_samples(km)
    clips = synthetic.make_dataset(num_clips=M, seed=5, frames_range=(150, 300), tile_cells_range=(30, 45))
    frames = [torch.tensor(c["frames"], dtype=torch.float32, device=dev) for c in clips]
    contacts = [torch.tensor(c["contacts"], dtype=torch.float32, device=dev) for c in clips]
    terrains = [terrain_util.SubTerrain.from_arrays(c["hf"], c["min_point"], c["dxdy"], device=dev) for c in clips]
    rp = [f[:, 0:3].contiguous() for f in frames]
    rq = [torch_util.exp_map_to_quat(f[:, 3:6]) for f in frames]
    jr = [km.dof_to_rot(f[:, 6:].contiguous()) for f in frames]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def bc_batch():
        return mo.compute_approx_body_constraints_batch(rp, rq, jr, contacts, km, terrains)

    def bc_loop():
        return [mo.compute_approx_body_constraints(rp[m], rq[m], jr[m], contacts[m], km, terrains[m]) for m in range(M)]

    _, bcs = timed(bc_batch)          # warm-up calls; the constraints of the descents below
    timed(bc_loop)

    def opt_batch():
        return mo.motion_contact_optimization_batch(src_frames=frames, contacts=contacts, body_points=body_points, terrains=terrains, char_model=km,
                                                    num_iters=iters, step_size=0.001, body_constraints=bcs, max_jerk=1000.0, exp_names=[None] * M,
                                                    use_wandb=False, log_files=[None] * M, use_graph=True, verbose=False, **W)

    def opt_loop():
        return [mo.motion_contact_optimization(src_frames=frames[m], contacts=contacts[m], body_points=body_points, terrain=terrains[m], char_model=km,
                                               num_iters=iters, step_size=0.001, body_constraints=bcs[m], max_jerk=1000.0, exp_name=None,
                                               use_wandb=False, log_file=None, use_graph=True, verbose=False, **W) for m in range(M)]

    timed(opt_batch)
    timed(opt_loop)
    res = {"M": M, "iters": iters, "frames": [int(f.shape[0]) for f in frames], "opt_batch_ms": [], "opt_loop_ms": [], "bc_batch_ms": [], "bc_loop_ms": []}
    for r in range(repeats):          # the two configurations interleaved
        for key, fn in (("opt_batch_ms", opt_batch), ("opt_loop_ms", opt_loop), ("bc_batch_ms", bc_batch), ("bc_loop_ms", bc_loop)):
            ms, _ = timed(fn)
            res[key].append(round(ms, 3))
            print("M={} repeat {} {:13s} {:10.3f} ms".format(M, r, key, ms), flush=True)
    for kind in ("opt", "bc"):
        b, lo = res[kind + "_batch_ms"], res[kind + "_loop_ms"]
        res[kind + "_batch_median_ms"], res[kind + "_loop_median_ms"], res[kind + "_loop_min_ms"] = statistics.median(b), statistics.median(lo), min(lo)
    res["opt_batch_ms_per_iter"] = res["opt_batch_median_ms"] / iters
    res["opt_batch_ms_per_motion_iter"] = res["opt_batch_median_ms"] / iters / M
    res["opt_loop_ms_per_motion_iter"] = res["opt_loop_median_ms"] / iters / M
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child", type=int, default=None, help="internal: measure this M in this process and print the JSON result")
    ap.add_argument("--limit", type=int, default=420, help="time limit of one child, seconds")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.child is not None:
        print("RESULT " + json.dumps(measure(args.child, args.iters, args.repeats)), flush=True)
        return 0
    import torch
    if not torch.cuda.is_available():
        doc = {"status": "not measured", "reason": "no device"}
    else:
        doc = {"status": "measured", "device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "results": []}
        for M in args.m:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(M), "--iters", str(args.iters),
                   "--repeats", str(args.repeats)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(p.stdout)
            line = [ln for ln in p.stdout.split("\n") if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stderr[-4000:])
                doc["status"] = "incomplete"
                doc["failed"] = {"M": M, "returncode": p.returncode}
                break           # nothing more is started on the device after a failure
            doc["results"].append(json.loads(line[0][len("RESULT "):]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "results"}))
    return 0 if doc["status"] != "incomplete" else 1


if __name__ == "__main__":
    sys.exit(main())
