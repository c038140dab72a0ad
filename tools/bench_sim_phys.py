#!/usr/bin/env python3
"""Simulator step time with and without the per-env physics table (run on the GPU box): for every control mode the kernel without a table
(sim_step_bpl_kernel / sim_step_bpl_ctl_kernel<MODE>) beside sim_step_bpl_phys_kernel<MODE> with the neutral table, N envs of
boxes_64clips, by the method of tools/bench_sim_modes.py: device events around R launches, the two interleaved in rounds in one process.
The R launches are issued as ONE captured hipGraph on both sides, which is how the rollout issues them - and inside a capture
parc_sim_step_phys skips the check of the rows (include/parc_sim.h), so the figure is the kernel's.  `eager_us` times the same R launches
issued eagerly, where every call with a table first waits for the verdict of the row check.  Prints one JSON object.

    python tools/bench_sim_phys.py [--envs 4096] [--rounds 5] [--reps 20] [--plain]     (--plain: one short round, for profiler runs)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import _hip, _hip_sim, workloads  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--plain", action="store_true")
args = ap.parse_args()
if args.plain:
    args.rounds, args.reps = 1, 5
dev = "cuda:0"
N = args.envs
env, _, _ = workloads.build_env("boxes_64clips", N, dev, seed=0)
env.reset()
c = env._core
D = env._cfg.dof_size
L = _hip.lib()
torch.manual_seed(0)
MODES = list(_hip_sim.CONTROL_MODES)
act = {m: torch.zeros((N, D), device=dev) for m in MODES}
eff = torch.tensor([env._sim_model.struct.effort[d] for d in range(D)], device=dev)
act["torque"] = (torch.rand((N, D), device=dev) * 2 - 1) * 0.1 * eff
act["vel"] = (torch.rand((N, D), device=dev) * 2 - 1) * 0.5
lo = {m: env._action_bound_low for m in MODES}
hi = {m: env._action_bound_high for m in MODES}
lo["vel"], hi["vel"] = torch.full((D,), -2 * np.pi, device=dev), torch.full((D,), 2 * np.pi, device=dev)
lo["torque"], hi["torque"] = -eff, eff
torque_out = torch.zeros((N, D), device=dev)
n_sub = env._sim_steps * env._substeps
tensors = (c.root_state, c.dof_state, c.rigid_body_state, c.contact_forces)
snap = [t.clone() for t in tensors]
env.set_physics_params(None)                  # allocates the neutral table
table = env._phys_table


def launch(mode, phys):
    args_ = (_hip.stream(), env._sim_model.device_ptr(dev), c._terrain_struct, N, _hip.ptr(c.root_state), _hip.ptr(c.dof_state),
             _hip.ptr(c.rigid_body_state), _hip.ptr(c.contact_forces), _hip.ptr(c.env_offsets), _hip.ptr(act[mode]), _hip.ptr(lo[mode]),
             _hip.ptr(hi[mode]), n_sub, env._sim_h)
    tq = _hip.ptr(torque_out) if mode in ("torque", "pd_exp", "pd_1d") else None
    if phys:
        rc = L.parc_sim_step_phys(*args_, env._substeps, _hip.ptr(table), _hip_sim.CONTROL_MODES[mode], tq, None, None, 0.0)
    elif mode == "pd":
        rc = L.parc_sim_step(*args_)
    else:
        rc = L.parc_sim_step_ctl(*args_, env._substeps, _hip_sim.CONTROL_MODES[mode], tq, None, None, 0.0)
    _hip.check(rc, mode)


def restore():
    for t, s in zip(tensors, snap):
        t.copy_(s)


def timed(fn):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / args.reps


graphs = {}
for mode in MODES:
    for phys in (False, True):
        restore()
        for _ in range(3):
            launch(mode, phys)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.reps):
                launch(mode, phys)
        graphs[mode, phys] = g
times = {(m, p): [] for m in MODES for p in (False, True)}
eager = {(m, p): [] for m in MODES for p in (False, True)}
for r in range(args.rounds):
    for mode in MODES:
        for phys in (False, True):
            restore()
            times[mode, phys].append(timed(graphs[mode, phys].replay))
            assert torch.isfinite(c.dof_state).all(), mode
            restore()
            eager[mode, phys].append(timed(lambda: [launch(mode, phys) for _ in range(args.reps)]))


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "samples": [round(x, 2) for x in v]}


out = {"envs": N, "substeps_per_launch": n_sub, "substeps_per_hold": env._substeps, "reps_per_sample": args.reps, "us_per_launch": {}}
for m in MODES:
    a, b = stat(times[m, False]), stat(times[m, True])
    out["us_per_launch"][m] = {"without_table": a, "with_table": b, "ratio": round(b["median"] / a["median"], 4),
                               "eager_us": {"without_table": float(np.median(eager[m, False])), "with_table_and_row_check": float(np.median(eager[m, True]))}}
print(json.dumps(out))
