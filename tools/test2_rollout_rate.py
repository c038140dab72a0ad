#!/usr/bin/env python3
"""Steps per second of a test2 rollout (unit statistics on) beside a test rollout, 4096 envs of boxes_64clips (run on the GPU box):
python3 tools/test2_rollout_rate.py [--envs=4096] [--episodes=4096] [--out FILE].  The two modes alternate REPEATS times after one
warm-up round each; a step is one env.step of all envs, the clock a host clock around _rollout_test with a device synchronise at both
ends (the whole call, with test_model2's rank figures, is given beside it).  The figures go under the key "rollout" of profiles/unit_stats.json (the other keys are kept)."""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch

OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(REPO, "profiles", "unit_stats.json")
opt = lambda name, default: int(([a.split("=")[1] for a in sys.argv if a.startswith("--%s=" % name)] or [default])[0])   # noqa: E731
ENVS, EPISODES, REPEATS = opt("envs", 4096), opt("episodes", 4096), 3
if not torch.cuda.is_available():
    raise SystemExit("test2_rollout_rate.py measures on the GPU: no device found")
from parc_amd import workloads
from parc_amd.util import mp_util

dev = "cuda:0"
mp_util.init(0, 1, dev)
torch.manual_seed(0)
env, _, _ = workloads.build_env("boxes_64clips", ENVS, dev, seed=0)
agent = workloads.build_agent(env, dev, mp_scale_rollout=False)
steps, spent = [0], [0.0]
env_step, rollout_test = env.step, agent._rollout_test


def counted(action):
    steps[0] += 1
    return env_step(action)


def timed_rollout(num_episodes):
    """the rollout alone: test_model2's rank figures (a float64 SVD on the host, once) are not part of a step"""
    torch.cuda.synchronize()
    t0 = time.time()
    out = rollout_test(num_episodes)
    torch.cuda.synchronize()
    spent[0] = time.time() - t0
    return out


env.step, agent._rollout_test = counted, timed_rollout


def run(fn):
    steps[0] = 0
    t0 = time.time()
    fn(EPISODES)
    return {"steps": steps[0], "rollout_seconds": round(spent[0], 4), "steps_per_s": round(steps[0] / spent[0], 1), "whole_call_seconds": round(time.time() - t0, 4)}


modes = {"test": agent.test_model, "test2": lambda n: agent.test_model2(n)}
runs = {k: [] for k in modes}
for rep in range(REPEATS + 1):          # round 0 is the warm-up
    for k, fn in modes.items():
        r = run(fn)
        if rep > 0:
            runs[k].append(r)
            print(json.dumps({"mode": k, **r}))
res = {"tool": "tools/test2_rollout_rate.py", "status": "measured", "device": torch.cuda.get_device_name(0), "workload": "boxes_64clips", "envs": ENVS,
       "episodes": EPISODES, "runs": runs, "median_steps_per_s": {k: sorted(r["steps_per_s"] for r in v)[len(v) // 2] for k, v in runs.items()}}
print(json.dumps(res["median_steps_per_s"]))
doc = {}
if os.path.exists(OUT):
    with open(OUT) as f:
        doc = json.load(f)
doc["rollout"] = res
with open(OUT, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
