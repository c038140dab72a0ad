#!/usr/bin/env python3
"""Optimizer step time at the model's size (run on the GPU box): the flat AdamW step (parc_adamw_step: norm pass + update pass over flat
buffers) beside what `optimizer.type: Adam` ran before it - torch.linalg.vector_norm + parc_scale_by_clipped_norm + the fused
multi-tensor torch.optim.AdamW.step() over separately allocated parameters whose gradients are views of the flat gradient - and the flat
SGD step (parc_sgd_momentum_step) as a yardstick, each with the clip active (max_norm below the gradient's norm) and inactive (above).

Device events around windows of `--reps` steps issued back to back; the variants take turns in `--rounds` rounds in one process, and every
window is printed.  Algorithmic bytes: AdamW 28 B per element (p, g, m, v read; p, m, v written) + 4 B for the norm pass, SGD 20 + 4 B;
the fraction of peak is those bytes over the median time over 8 TB/s (HBM-bound: ~12 flops per 28 bytes).

    python tools/bench_optimizer.py [--n 10638877] [--rounds 7] [--reps 300] [--out profiles/adamw_step.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import _hip  # noqa: E402

HBM_PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=10638877)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "adamw_step.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("bench_optimizer.py measures on the GPU: no device found (nothing is written: not measured)")
dev = "cuda:0"
n = args.n
L = _hip.lib()
LR, WD = 1e-3, 0.01


def mlp_split(n):
    """16 tensors shaped like the actor's and the critic's four layers (weight, bias), the first weight of each net taking what is left."""
    fixed = [2048, 2048 * 1024, 1024, 1024 * 512, 512, 512 * 32, 32]
    half = [n // 2, n - n // 2]
    sizes = []
    for h in half:
        if h <= sum(fixed):
            return [h for h in half if h]
        sizes += [h - sum(fixed)] + fixed
    return sizes


torch.manual_seed(0)
p0 = torch.randn(n, device=dev) * 0.05
grad = torch.randn(n, device=dev) * 1e-2
gnorm = float(torch.linalg.vector_norm(grad))
MAX_NORM = {"clip_active": 0.5 * gnorm, "clip_inactive": 2.0 * gnorm}
ws = torch.empty(int(L.parc_sgd_workspace_floats()), device=dev)
norm_out = torch.zeros(1, device=dev)


class FlatAdamW:
    name, bytes_per_elem = "flat_adamw", 28 + 4

    def __init__(self):
        self.p, self.m, self.v, self.g, self.t = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), grad.clone(), 0

    def step(self, max_norm):
        self.t += 1
        _hip.check(L.parc_adamw_step(_hip.stream(), n, _hip.ptr(self.p), _hip.ptr(self.g), _hip.ptr(self.m), _hip.ptr(self.v), self.t, max_norm, LR,
                                     0.9, 0.999, 1e-8, WD, _hip.ptr(ws), _hip.ptr(norm_out)), "parc_adamw_step")

    def params(self):
        return self.p


class FlatSGD:
    name, bytes_per_elem = "flat_sgd", 20 + 4

    def __init__(self):
        self.p, self.m, self.g = p0.clone(), torch.zeros_like(p0), grad.clone()

    def step(self, max_norm):
        _hip.check(L.parc_sgd_momentum_step(_hip.stream(), n, _hip.ptr(self.p), _hip.ptr(self.g), _hip.ptr(self.m), max_norm, LR, 0.9, WD, _hip.ptr(ws),
                                            _hip.ptr(norm_out)), "parc_sgd_momentum_step")

    def params(self):
        return self.p


class TorchAdamW:
    """MPOptimizer._finish_step of `type: Adam` without the flat path, launch for launch."""
    name, bytes_per_elem = "torch_adamw", None

    def __init__(self):
        self.g = grad.clone()
        self.plist, off = [], 0
        for s in mlp_split(n):
            q = torch.nn.Parameter(p0[off:off + s].clone())
            q.grad = self.g[off:off + s]
            self.plist.append(q)
            off += s
        assert off == n
        self.opt = torch.optim.AdamW(self.plist, LR, weight_decay=WD, fused=True)

    def step(self, max_norm):
        norm = torch.linalg.vector_norm(self.g)
        _hip.check(L.parc_scale_by_clipped_norm(_hip.stream(), n, _hip.ptr(self.g), _hip.ptr(norm.reshape(1)), float(max_norm)), "parc_scale_by_clipped_norm")
        self.opt.step()

    def params(self):
        return torch.cat([q.detach().reshape(-1) for q in self.plist])


def window(fn, reps):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


# the two AdamW paths compute the same thing at this size: one clipped step from the same state
a, b = FlatAdamW(), TorchAdamW()
a.step(MAX_NORM["clip_active"])
b.step(MAX_NORM["clip_active"])
agree = float((a.params() - b.params()).abs().max())
print("first clipped step, max |flat - torch| over {} parameters: {:.3e}".format(n, agree), flush=True)
assert agree <= 1e-6, agree

variants = {(cls.name, clip): cls() for clip in MAX_NORM for cls in (FlatAdamW, TorchAdamW, FlatSGD)}
for (name, clip), obj in variants.items():       # warm-up: code objects, the fused optimizer's state, every shape the windows use
    for _ in range(20):
        obj.step(MAX_NORM[clip])
times = {k: [] for k in variants}
for r in range(args.rounds):
    for (name, clip), obj in variants.items():
        t = window(lambda: obj.step(MAX_NORM[clip]), args.reps)
        times[name, clip].append(t)
        print("round {} {:>12} {:>13}: {:8.2f} us per step".format(r, name, clip, t), flush=True)
for obj in variants.values():
    assert torch.isfinite(obj.params()).all()

out = {"n": n, "tensors_in_torch_path": len(mlp_split(n)), "reps_per_window": args.reps, "rounds": args.rounds, "hbm_peak_bytes_per_s": HBM_PEAK,
       "first_step_max_abs_diff_flat_vs_torch": agree, "us_per_step": {}}
for (name, clip), v in times.items():
    med = float(np.median(v))
    row = {"median": round(med, 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2), "windows": [round(x, 2) for x in v]}
    bpe = variants[name, clip].bytes_per_elem
    if bpe is not None:
        row["algorithmic_bytes"] = bpe * n
        row["fraction_of_hbm_peak"] = round(bpe * n / (med * 1e-6) / HBM_PEAK, 4)
    out["us_per_step"].setdefault(clip, {})[name] = row
for clip, rows in out["us_per_step"].items():
    f, t = rows["flat_adamw"], rows["torch_adamw"]
    rows["torch_over_flat"] = round(t["median"] / f["median"], 3)
    rows["flat_no_slower_beyond_spread"] = bool(f["median"] <= t["median"] + max(f["max"] - f["min"], t["max"] - t["min"]))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
