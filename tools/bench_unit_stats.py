#!/usr/bin/env python3
"""Microseconds per unit-statistics update (run on the GPU box): parc_netstats_update alone (two launches for all layers and the mean
net) at rows 4096 and 8192 with widths 2048 / 1024 / 512 and A = 28, against the torch op chain that computes the same values (S_l
precomputed for both).  HIP events around a window of WINDOW updates, after a warm-up round, REPEATS times per configuration, the
configurations interleaved; every repeat is printed.  The figures go under the key "update_time" of profiles/unit_stats.json (--out
FILE writes there instead; the other keys of the file are kept).  Without a device the entry says "not measured".

Algorithmic bytes per update: 4 * rows * (sum of the widths + 3 A) - every activation read once, the mean read, mean_net_acts read and
written - plus the vectors: 4 * 5 * sum of the widths (S, activations and utility read, the latter two written)."""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "unit_stats.json")
WIDTHS, A, ROWS, WINDOW, REPEATS = [2048, 1024, 512], 28, [4096, 8192], 200, 5
PEAK_BYTES_PER_S = 8e12
shape = {"widths": WIDTHS, "A": A, "rows": ROWS, "window": WINDOW, "repeats": REPEATS}


def write(entry):
    doc = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    doc["update_time"] = entry
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if not torch.cuda.is_available():
    write({"tool": "tools/bench_unit_stats.py", "status": "not measured", "reason": "no device", **shape})
    raise SystemExit("bench_unit_stats.py measures on the GPU: no device found ({} says: not measured)".format(OUT))

from parc_amd import _hip, _hip_netstats as ns

dev = "cuda:0"
torch.manual_seed(0)
L = _hip.lib()
ETA, GAIN = 0.99, 1.0 - 0.99


def setup(rows):
    f32 = dict(dtype=torch.float32, device=dev)
    H = [torch.relu(torch.randn(rows, d, **f32)) for d in WIDTHS]
    mean = torch.randn(rows, A, **f32)
    S = [torch.rand(d, **f32) * 10.0 for d in WIDTHS]
    state = lambda: ([torch.zeros(d, **f32) for d in WIDTHS], [torch.zeros(d, **f32) for d in WIDTHS], torch.zeros(rows, A, **f32))   # noqa: E731
    fa, fu, fm = state()
    ca, cu, cm = state()
    table = ns.table([(h.data_ptr(), d, s.data_ptr(), a.data_ptr(), u.data_ptr()) for h, d, s, a, u in zip(H, WIDTHS, S, fa, fu)])
    ws = torch.empty(int(L.parc_netstats_workspace_floats(rows, table)), **f32)
    stream = _hip.stream()

    def fused():
        _hip.check(L.parc_netstats_update(stream, rows, table, A, _hip.ptr(mean), _hip.ptr(fm), ETA, GAIN, _hip.ptr(ws)), "parc_netstats_update")

    def chain():
        cm.mul_(ETA).add_(mean.abs(), alpha=GAIN)
        for l in range(len(WIDTHS)):
            m = H[l].mean(dim=0).abs_().mul_(GAIN)
            cu[l].mul_(ETA).addcmul_(m, S[l])
            ca[l].mul_(ETA).add_(m)
    return fused, chain, (fa, fu, fm), (ca, cu, cm), (H, mean, S, ws)


res = {"tool": "tools/bench_unit_stats.py", "status": "measured", "device": torch.cuda.get_device_name(0), **shape, "per_rows": {}}
for rows in ROWS:
    fused, chain, f_state, c_state, keep = setup(rows)
    fused(), chain()
    torch.cuda.synchronize()
    agree = max(float(((a - b).abs() / b.abs().clamp_min(1e-30)).max()) for x, y in ((f_state[0], c_state[0]), (f_state[1], c_state[1]), ([f_state[2]], [c_state[2]]))
                for a, b in zip(x, y))
    configs = {"fused": fused, "chain": chain}
    times = {k: [] for k in configs}
    for rep in range(REPEATS + 1):          # round 0 is the warm-up
        for k, fn in configs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(WINDOW):
                fn()
            e.record()
            torch.cuda.synchronize()
            if rep > 0:
                times[k].append(round(s.elapsed_time(e) * 1e3 / WINDOW, 2))
    nbytes = 4 * rows * (sum(WIDTHS) + 3 * A) + 4 * 5 * sum(WIDTHS)
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    entry = {"us_per_update": times, "median": med, "min": {k: min(v) for k, v in times.items()}, "algorithmic_bytes": nbytes,
             "fraction_of_8TBps_peak": {k: round(nbytes / (med[k] * 1e-6) / PEAK_BYTES_PER_S, 4) for k in med},
             "max_relative_difference_after_one_update": agree}
    entry["fused_median_below_fastest_chain_repeat"] = med["fused"] < entry["min"]["chain"]
    res["per_rows"][str(rows)] = entry
    for k, v in times.items():
        print(json.dumps({"rows": rows, "config": k, "us_per_update": v, "median": med[k], "min": entry["min"][k]}))
    print(json.dumps({"rows": rows, **{k: entry[k] for k in ("algorithmic_bytes", "fraction_of_8TBps_peak", "max_relative_difference_after_one_update",
                                                           "fused_median_below_fastest_chain_repeat")}}))
write(res)
