#!/usr/bin/env python3
"""Microseconds per parc_render launch: 1, 4 and 16 views at 640 x 360, shadows on and off (run on the GPU box).  The C entry point is
called directly with prebuilt arguments, as tools/bench_sim.py does; HIP events around a batch of BATCH launches, after a warm-up
batch, REPEATS times per configuration, the configurations interleaved; one JSON line per configuration with every repeat."""
import ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from parc_amd import _hip, render, workloads
from parc_amd.envs import base_env

dev = "cuda:0"
W, H, BATCH, REPEATS = 640, 360, 500, 5
env, clips, tiled = workloads.build_env("boxes_64clips", 16, dev, seed=0)
env.set_mode(base_env.EnvMode.TEST)
env.reset()
for _ in range(5):
    env.step(env._ref_dof_pos.clone())
L, p, c = _hip.lib(), _hip.ptr, env._core
configs = [(views, shadows) for views in (1, 4, 16) for shadows in (True, False)]
calls = {}
for views, shadows in configs:
    r = render.Renderer(env, W, H, list(range(views)), shadows=shadows)
    r.render()              # places the views and fills the reference body poses that the timed launches read
    args = (_hip.stream(), r._terrain_struct(), ctypes.byref(r._scene), views, p(r._views), W, H, p(c.root_state), p(c.rigid_body_state),
            p(r._ref_body_pos), p(r._ref_body_rot), p(c.contact_forces), p(c.env_offsets), env.get_num_envs(), p(r._rgba), None, None)
    calls[(views, shadows)] = (r, args)
times = {k: [] for k in configs}
for rep in range(REPEATS + 1):          # round 0 is the warm-up
    for k in configs:
        args = calls[k][1]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(BATCH):
            L.parc_render(*args)
        e.record()
        torch.cuda.synchronize()
        if rep > 0:
            times[k].append(round(s.elapsed_time(e) * 1e3 / BATCH, 2))
for (views, shadows), t in times.items():
    print(json.dumps({"views": views, "width": W, "height": H, "shadows": shadows, "batch": BATCH, "us_per_parc_render_launch": t,
                      "median": sorted(t)[len(t) // 2], "min": min(t), "max": max(t)}))
