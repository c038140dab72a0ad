#!/usr/bin/env python3
"""Simulator step time per control mode (run on the GPU box): sim_step_bpl_kernel (pd, parc_sim_step) and sim_step_bpl_ctl_kernel (vel /
torque / pd_exp / pd_1d, parc_sim_step_ctl) at N envs of boxes_64clips, device events around R launches, pd and the other modes
interleaved in rounds in the same process (so that clock and thermal drift fall on all of them alike).  Prints one JSON object.
(pd_1d runs the humanoid only to time the kernel: the env refuses that mode on a character with spherical joints.)

    python tools/bench_sim_modes.py [--envs 4096] [--rounds 5] [--reps 20] [--plain]     (--plain: one short round, for profiler runs)"""
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
act = {m: torch.zeros((N, D), device=dev) for m in _hip_sim.CONTROL_MODES}
eff = torch.tensor([env._sim_model.struct.effort[d] for d in range(D)], device=dev)
act["torque"] = (torch.rand((N, D), device=dev) * 2 - 1) * 0.1 * eff
act["vel"] = (torch.rand((N, D), device=dev) * 2 - 1) * 0.5
lo = {m: env._action_bound_low for m in _hip_sim.CONTROL_MODES}
hi = {m: env._action_bound_high for m in _hip_sim.CONTROL_MODES}
lo["vel"], hi["vel"] = torch.full((D,), -2 * np.pi, device=dev), torch.full((D,), 2 * np.pi, device=dev)
lo["torque"], hi["torque"] = -eff, eff
torque_out = torch.zeros((N, D), device=dev)
n_sub = env._sim_steps * env._substeps
snap = [t.clone() for t in (c.root_state, c.dof_state, c.rigid_body_state, c.contact_forces)]


def launch(mode):
    args_ = (_hip.stream(), env._sim_model.device_ptr(dev), c._terrain_struct, N, _hip.ptr(c.root_state), _hip.ptr(c.dof_state),
             _hip.ptr(c.rigid_body_state), _hip.ptr(c.contact_forces), _hip.ptr(c.env_offsets), _hip.ptr(act[mode]), _hip.ptr(lo[mode]),
             _hip.ptr(hi[mode]), n_sub, env._sim_h)
    if mode == "pd":
        rc = L.parc_sim_step(*args_)
    else:
        rc = L.parc_sim_step_ctl(*args_, env._substeps, _hip_sim.CONTROL_MODES[mode], _hip.ptr(torque_out) if mode in ("torque", "pd_exp", "pd_1d") else None,
                                 None, None, 0.0)
    _hip.check(rc, mode)


def restore():
    for t, s in zip((c.root_state, c.dof_state, c.rigid_body_state, c.contact_forces), snap):
        t.copy_(s)


times = {m: [] for m in _hip_sim.CONTROL_MODES}
for r in range(args.rounds):
    for mode in ("pd", "vel", "pd", "torque", "pd", "pd_exp", "pd", "pd_1d"):
        restore()
        for _ in range(3):
            launch(mode)
        restore()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(args.reps):
            launch(mode)
        e.record()
        torch.cuda.synchronize()
        times[mode].append(s.elapsed_time(e) * 1e3 / args.reps)
        assert torch.isfinite(c.dof_state).all(), mode
print(json.dumps({"envs": N, "substeps_per_launch": n_sub, "substeps_per_hold": env._substeps, "reps_per_sample": args.reps,
                  "us_per_launch": {m: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v)), "samples": [round(x, 2) for x in v]}
                                    for m, v in times.items()}}))
