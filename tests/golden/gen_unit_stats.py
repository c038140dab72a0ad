#!/usr/bin/env python3
"""Generate tests/golden/g29_unit_stats.npz from the REFERENCE's own DMPPOAgent.test_model2 (learning/dm_ppo_agent.py:607-773; CPU, torch).

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference
on the path.  test_model2 is called unbound on a small stand-in object: `_model._actor_layers` is a Sequential of three Linear / ReLU
pairs (12 -> 20 -> 12 -> 8), `_model._action_dist._mean_net` a Linear(8, 4), eval / set_mode do nothing, `_env.reset` returns nothing
of use, and `_rollout_test` feeds K = 400 batches of N = 5 observations through the two modules - the reference's forward hooks fire
and keep its running values - and copies `_activations`, `_utility` and `_mean_net_acts` after every batch, together with the hidden
activations and the mean the modules produced (the inputs of the device update).  What the reference prints is captured; the rank lines
are parsed from it and the rest is dropped.

The running values start at 0 and move by 1 % per step, so after 400 steps they stand at 98 % of a stationary activity.  Every
weight row has a scale of its own (log-spaced over three decades), which leaves dormant (< 0.01) and live units in every layer; unit 3
of every layer, and action 1, have zero weights and a negative bias (zero bias for the mean net): they never fire.  No final value may
lie within a relative 1e-4 of the threshold.

usage:  python tests/golden/gen_unit_stats.py            # rewrites tests/golden/g29_unit_stats.npz
        python tests/golden/gen_unit_stats.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import contextlib
import io
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

N, OBS, WIDTHS, A, K = 5, 12, (20, 12, 8), 4, 400
DEAD = 3
THRESHOLD, MARGIN = 0.01, 1e-4


def build_modules(gen):
    layers, in_size = [], OBS
    for li, d in enumerate(WIDTHS + (A,)):
        lin = torch.nn.Linear(in_size, d)
        scale = torch.logspace(-2.6, 0.4, d)[torch.randperm(d, generator=gen)]
        with torch.no_grad():
            lin.weight.copy_(torch.randn(d, in_size, generator=gen) * scale[:, None] / np.sqrt(in_size) * (2.0 + li))
            lin.bias.copy_(0.3 * scale * torch.rand(d, generator=gen))
            dead = 1 if d == A else DEAD
            lin.weight[dead] = 0.0
            lin.bias[dead] = 0.0 if d == A else -1.0
        layers.append(lin)
        in_size = d
    seq = []
    for lin in layers[:-1]:
        seq += [lin, torch.nn.ReLU()]
    return torch.nn.Sequential(*seq), layers[-1]


class _Obj:
    pass


def main():
    gg._import_learning()
    import learning.dm_ppo_agent as ref_agent
    out = tempfile.mkdtemp(prefix="parc_g29_check_") if "--check" in sys.argv else HERE
    gen = torch.Generator().manual_seed(29)
    actor, mean_net = build_modules(gen)
    obs = torch.randn(K, N, OBS, generator=gen)

    agent = _Obj()
    agent._model = _Obj()
    agent._model._actor_layers = actor
    agent._model._action_dist = _Obj()
    agent._model._action_dist._mean_net = mean_net
    agent._device = "cpu"
    agent._env = _Obj()
    agent._env.reset = lambda: (None, None)
    agent.eval = lambda: None
    agent.set_mode = lambda mode: None
    snaps = dict(activations=[], utility=[], mean_net_acts=[], hidden=[], mean=[])

    def rollout(num_eps):
        with torch.no_grad():
            for k in range(K):
                x, hidden = obs[k], []
                for m in actor:
                    x = m(x)
                    if isinstance(m, torch.nn.ReLU):
                        hidden.append(x.clone())
                mean = mean_net(x)
                snaps["hidden"].append(torch.cat(hidden, dim=1))
                snaps["mean"].append(mean.clone())
                snaps["activations"].append(torch.cat(agent._activations).clone())
                snaps["utility"].append(torch.cat(agent._utility).clone())
                snaps["mean_net_acts"].append(agent._mean_net_acts.clone())
        return {"mean_return": 0.0, "mean_ep_len": 0.0, "num_eps": num_eps}
    agent._rollout_test = rollout

    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = ref_agent.DMPPOAgent.test_model2(agent, 7)
    assert res["num_eps"] == 7 and len(snaps["mean"]) == K
    text = text.getvalue()
    ints = lambda pat: [int(v) for v in re.findall(pat, text)]          # noqa: E731
    floats = lambda pat: [float(v) for v in re.findall(pat, text)]      # noqa: E731
    L = len(WIDTHS)
    max_rank = ints(r"Max possible rank of layer \d+ : (\d+)") + ints(r"Max possible rank of mean_net: (\d+)")
    stab_rank = ints(r"Stable rank of layer \d+ : (\d+)") + ints(r"Stable rank of mean_net: (\d+)")
    avg_mag = floats(r"Average weight magnitude of layer \d+ : (\S+)") + floats(r"Average weight magnitude of mean_net: (\S+)")
    assert len(max_rank) == len(stab_rank) == len(avg_mag) == L + 1, (max_rank, stab_rank, avg_mag)

    arrs = {k: torch.stack(v) for k, v in snaps.items()}
    assert arrs["mean_net_acts"].shape == (K, N, A), arrs["mean_net_acts"].shape      # zeros[A] broadcast against |mean| [N, A]
    finals = list(torch.split(arrs["activations"][-1], list(WIDTHS))) + [arrs["mean_net_acts"][-1].flatten()]
    for v in finals:
        v, d = v.double().numpy(), v.numel()
        dormant = int((v < THRESHOLD).sum())
        print("width", d, "dormant", dormant, "never fired", int((v == 0.0).sum()))
        assert 0 < dormant < d and (v == 0.0).any(), (d, dormant)
        assert (np.abs(v / THRESHOLD - 1.0) > MARGIN).all(), "a final value sits on the threshold"
    lins = [m for m in actor if isinstance(m, torch.nn.Linear)] + [mean_net]
    for i, lin in enumerate(lins):
        arrs["weight%d" % i], arrs["bias%d" % i] = lin.weight.detach(), lin.bias.detach()
    arrs.update(widths=np.array(WIDTHS, np.int32), max_rank=np.array(max_rank, np.int32), stable_rank=np.array(stab_rank, np.int32),
                avg_weight_mag=np.array(avg_mag, np.float64))
    print("ranks", max_rank, stab_rank, avg_mag)
    dst = os.path.join(out, "g29_unit_stats.npz")
    np.savez_compressed(dst, **{k: gg.npy(v) for k, v in arrs.items()})
    print("wrote", dst, os.path.getsize(dst), "bytes")
    if "--check" in sys.argv:
        a, b = np.load(dst), np.load(os.path.join(HERE, "g29_unit_stats.npz"))
        bad = 0
        for k in sorted(set(a.files) | set(b.files)):
            same = k in a.files and k in b.files and a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
            if not same:
                bad += 1
                print("DIFFERS", k)
        print("check: {} arrays differ from the committed fixture".format(bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
