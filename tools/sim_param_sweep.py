#!/usr/bin/env python3
"""How sensitive is a tracker to the simulator's hand-picked contact constants?  (run on the GPU box)

Assigns a grid of ONE physics parameter across the envs of one launch (set_physics_params: env i gets value i % bins of the grid,
log-spaced unless --linear), runs test-mode episodes (the policy's mode action, no exploration) and writes mean return, mean episode
length and fail rate per bin to a JSON.  A return that is flat across a band says the policy does not hinge on the default value; it
says nothing about which value is right.

    python tools/sim_param_sweep.py --param contact_kn --lo 1e4 --hi 1.6e5 [--model_file m.pt | --untrained] [--workload boxes_64clips]
                                    [--envs 4096] [--bins 9] [--episodes 4] [--linear] [--out sweep.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from parc_amd import _hip_sim, workloads  # noqa: E402
from parc_amd.envs.base_env import DoneFlags  # noqa: E402
from parc_amd.learning.dm_ppo_agent import AgentMode  # noqa: E402


def sweep(env, agent, param, grid, episodes):
    N, dev = env.get_num_envs(), env._device
    bins = len(grid)
    bin_of = torch.arange(N, device=dev) % bins
    env.set_physics_params(None, **{param: torch.tensor(grid, dtype=torch.float32)[bin_of.cpu()]})
    agent.eval()
    agent.set_mode(AgentMode.TEST)
    obs, info = env.reset()
    ret = torch.zeros(N, device=dev)
    length = torch.zeros(N, device=dev)
    acc = torch.zeros((bins, 4), dtype=torch.float64, device=dev)       # episodes, return, length, fails
    eps = torch.zeros(N, dtype=torch.long, device=dev)
    with torch.no_grad():
        while int(eps.min().item()) < episodes:
            action, _ = agent._decide_action(obs, info)
            obs, r, done, info = env.step(action)
            ret += r
            length += 1
            fin = done != DoneFlags.NULL.value
            if fin.any():
                count = fin & (eps < episodes)                           # every env contributes the same number of episodes
                rows = torch.stack([count.double(), ret.double() * count, length.double() * count,
                                    ((done == DoneFlags.FAIL.value) & count).double()], dim=1)
                acc.index_add_(0, bin_of, rows)
                eps += fin
                ret[fin], length[fin] = 0.0, 0.0
                obs, info = env.reset(torch.nonzero(fin).flatten())
    a = acc.cpu().numpy()
    return [{"value": float(grid[b]), "episodes": int(a[b, 0]), "mean_return": a[b, 1] / a[b, 0], "mean_ep_len": a[b, 2] / a[b, 0],
             "fail_rate": a[b, 3] / a[b, 0]} for b in range(bins)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--param", required=True)
    ap.add_argument("--lo", type=float, required=True)
    ap.add_argument("--hi", type=float, required=True)
    ap.add_argument("--linear", action="store_true")
    ap.add_argument("--bins", type=int, default=9)
    ap.add_argument("--workload", default="boxes_64clips")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--model_file", default="")
    ap.add_argument("--untrained", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert bool(args.model_file) != args.untrained, "give --model_file or --untrained"
    assert args.param in _hip_sim.PHYS_FIELDS, "--param: one of {}".format(", ".join(_hip_sim.PHYS_FIELDS))
    dev = "cuda:0"
    torch.manual_seed(args.seed)
    env, _, _ = workloads.build_env(args.workload, args.envs, dev, seed=args.seed)
    agent = workloads.build_agent(env, dev)
    if args.model_file:
        agent.load(args.model_file)
    grid = np.linspace(args.lo, args.hi, args.bins) if args.linear else np.geomspace(args.lo, args.hi, args.bins)
    res = {"workload": args.workload, "envs": args.envs, "episodes_per_env": args.episodes, "policy": args.model_file or "untrained",
           "param": args.param, "spacing": "linear" if args.linear else "log", "default": float(getattr(env._sim_model.struct, args.param)) if hasattr(env._sim_model.struct, args.param) else 1.0,      # (the scales: 1)
           
           "bins": sweep(env, agent, args.param, grid, args.episodes)}
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
