"""Actor unit statistics of DMPPOAgent.test_model2 (learning/dm_ppo_agent.py:607-773 of the reference): rank figures of the actor's
weight matrices, and the running activity / utility of every hidden unit and of the mean head during a test rollout.

The reference keeps the running values with forward hooks on the ReLU modules and prints them at every step.  Here the hidden
activations come from DMPPOModel.eval_actor_tapped (FusedMLP runs Linear + ReLU as one GEMM, so such hooks would never fire) and one
device call per step (parc_netstats_update: two launches, no host read) updates every layer; the host reads the figures when a report is
asked for.
"""
import numpy as np
import torch

from . import dm_ppo_model

ETA = 0.99              # dm_ppo_agent.py:692
THRESHOLD = 0.01        # dm_ppo_agent.py:714


def stable_rank(singular_values):
    """First 0-based k at which cumsum(S)[k] / sum(S) > 0.99 for S sorted largest first, 0 if that never happens
    (dm_ppo_agent.py:640-649)."""
    S = np.asarray(singular_values, np.float64)
    over = np.nonzero(np.cumsum(S) / np.sum(S) > 0.99)[0]
    return int(over[0]) if over.size else 0


def rank_figures(weight):
    """{"max_rank", "stable_rank", "avg_weight_mag"} of one weight matrix, in float64 on the host."""
    W = weight.detach().to(device="cpu", dtype=torch.float64)
    S = torch.linalg.svdvals(W).numpy()
    return {"max_rank": int(S.shape[0]), "stable_rank": stable_rank(S), "avg_weight_mag": float(W.abs().mean())}


def hidden_linears(model):
    return [m for m in model._actor_layers if isinstance(m, torch.nn.Linear)]


def model_rank_figures(model):
    return {"layers": [rank_figures(lin.weight) for lin in hidden_linears(model)], "mean_net": rank_figures(model._action_dist._mean_net.weight)}


def rank_lines(ranks):
    """the reference's wording (dm_ppo_agent.py:650-671)"""
    out = []
    for l, r in enumerate(ranks["layers"]):
        out += ["Max possible rank of layer {} : {}".format(l, r["max_rank"]), "Stable rank of layer {} : {}".format(l, r["stable_rank"]),
                "Average weight magnitude of layer {} : {}".format(l, r["avg_weight_mag"])]
    r = ranks["mean_net"]
    return out + ["Max possible rank of mean_net: {}".format(r["max_rank"]), "Stable rank of mean_net: {}".format(r["stable_rank"]),
                  "Average weight magnitude of mean_net: {}".format(r["avg_weight_mag"])]


def report_lines(report):
    """the reference's wording (dm_ppo_agent.py:711-736)"""
    out = []
    for l, y in enumerate(report["layers"]):
        out += ["layer {}".format(l), "Percentage dormant units: {} %".format(y["percent_dormant"]),
                "Number of dormant units: {} / {}".format(y["num_dormant"], y["num_units"])]
        for name, key in (("Activation", "activation"), ("Utility", "utility")):
            out += ["{} {}: {}".format(name, s, y[key][s]) for s in ("mean", "std", "max", "min")]
    m = report["mean_net"]
    out += ["Mean Net Percentage dormant units: {} %".format(m["percent_dormant"]),
            "Mean Net Number of dormant units: {} / {}".format(m["num_dormant"], m["num_rows"])]
    return out + ["Mean Net Activation {}: {}".format(s, m["activation"][s]) for s in ("mean", "std", "max", "min")]


def check_model(model):
    """test_model2 needs the network the device update covers; anything else is refused (there is no slower path)."""
    from .. import _hip_netstats
    mods = list(model._actor_layers)
    plain = len(mods) >= 2 and len(mods) % 2 == 0 and all(isinstance(m, torch.nn.Linear) for m in mods[0::2]) \
        and all(isinstance(m, torch.nn.ReLU) for m in mods[1::2])
    if not plain:
        raise ValueError("unit statistics need an actor of Linear + ReLU pairs; got {}".format([type(m).__name__ for m in mods]))
    widths = [m.out_features for m in mods[0::2]]
    if len(widths) > _hip_netstats.MAX_LAYERS:
        raise ValueError("unit statistics cover at most {} hidden layers; the actor has {}".format(_hip_netstats.MAX_LAYERS, len(widths)))
    if any(w % 4 for w in widths):
        raise ValueError("unit statistics need hidden widths that are multiples of 4 (parc_netstats_update); the actor has {}".format(widths))
    if model._action_dist._std_type == dm_ppo_model.StdType.VARIABLE:
        raise ValueError("unit statistics do not cover a state-dependent log-std (actor_std_type: VARIABLE)")


def _moments(v):
    return torch.stack([v.mean(), v.std(), v.max(), v.min()])


class UnitStats:
    """Device state of one statistics run: per hidden layer activations [d_l], utility [d_l] and the summed outgoing weights S_l [d_l];
    mean_net_acts [N, A] (the reference starts it as zeros[A] and its first update broadcasts it against |mean| [N, A]: one running value
    per env and action); the workspace of the update and the dormant counts."""

    def __init__(self, model, num_rows, device, tap=None):
        from .. import _hip, _hip_netstats
        check_model(model)
        if not str(device).startswith("cuda"):
            raise RuntimeError("unit statistics run on the GPU (parc_netstats_update); device is {}".format(device))
        self._ns, self._hip = _hip_netstats, _hip
        L = _hip.lib()
        lins = hidden_linears(model)
        mnet = model._action_dist._mean_net
        f32 = dict(dtype=torch.float32, device=device)
        self.num_rows, self.num_actions = int(num_rows), int(mnet.out_features)
        self.widths = [lin.out_features for lin in lins]
        self.activations = [torch.zeros(d, **f32) for d in self.widths]
        self.utility = [torch.zeros(d, **f32) for d in self.widths]
        self.mean_net_acts = torch.zeros(self.num_rows, self.num_actions, **f32)
        self.out_abs_sum = []
        for l in range(len(lins)):        # the weights do not change during the rollout: S_l once
            W = (lins[l + 1] if l + 1 < len(lins) else mnet).weight.detach().contiguous()
            S = torch.empty(self.widths[l], **f32)
            _hip.check(L.parc_netstats_abs_colsum(_hip.stream(), W.shape[0], W.shape[1], _hip.ptr(W), _hip.ptr(S)), "parc_netstats_abs_colsum")
            self.out_abs_sum.append(S)
        need = int(L.parc_netstats_workspace_floats(self.num_rows, self._table([0] * len(lins))))
        if need < 0:
            raise RuntimeError("parc_netstats_workspace_floats refused rows {} widths {}".format(self.num_rows, self.widths))
        self._workspace = torch.empty(need, **f32)
        self._counts = torch.zeros(len(lins) + 1, dtype=torch.int32, device=device)
        self.steps = 0
        self.tap = tap          # tests: a list that receives (hidden activations, mean) of every step

    def _table(self, act_ptrs):
        return self._ns.table([(a, d, s.data_ptr(), x.data_ptr(), u.data_ptr())
                               for a, d, s, x, u in zip(act_ptrs, self.widths, self.out_abs_sum, self.activations, self.utility)])

    def update(self, acts, mean):
        """acts: the post-ReLU outputs [N, d_l] of this step; mean [N, A].  Two launches, nothing read back."""
        assert len(acts) == len(self.widths) and mean.shape == self.mean_net_acts.shape and all(a.is_contiguous() for a in acts) \
            and mean.is_contiguous(), "unit statistics follow the full batch of environments"
        h = self._hip
        h.check(h.lib().parc_netstats_update(h.stream(), self.num_rows, self._table([a.data_ptr() for a in acts]), self.num_actions, h.ptr(mean),
                                             h.ptr(self.mean_net_acts), ETA, 1.0 - ETA, h.ptr(self._workspace)), "parc_netstats_update")
        self.steps += 1
        if self.tap is not None:
            self.tap.append(([a.clone() for a in acts], mean.clone()))

    def report(self):
        """The figures the reference prints per step, as nested dicts of Python numbers (one count launch and one host read).

        The mean net has two dormant figures.  The reference counts the entries of mean_net_acts [N, A] below the threshold and divides
        by shape[0] = N, so its `percent_dormant` runs up to 100 * A; that quantity is kept under the reference's name, and
        `fraction_dormant` = count / (N * A) is the well-defined share beside it."""
        h = self._hip
        n_mean = self.mean_net_acts.numel()
        h.check(h.lib().parc_netstats_dormant_count(h.stream(), self._table([0] * len(self.widths)), n_mean, h.ptr(self.mean_net_acts), THRESHOLD,
                                                    h.ptr(self._counts)), "parc_netstats_dormant_count")
        rows = [_moments(v) for pair in zip(self.activations, self.utility) for v in pair] + [_moments(self.mean_net_acts)]
        vals = torch.stack(rows).to(torch.float64)
        vals = torch.cat([vals.flatten(), self._counts.to(torch.float64)]).tolist()          # the one host read
        counts = [int(c) for c in vals[4 * len(rows):]]
        names = ("mean", "std", "max", "min")
        layers = []
        for l, d in enumerate(self.widths):
            layers.append({"num_dormant": counts[l], "num_units": d, "percent_dormant": counts[l] / d * 100.0,
                           "activation": dict(zip(names, vals[8 * l:8 * l + 4])), "utility": dict(zip(names, vals[8 * l + 4:8 * l + 8]))})
        k = 8 * len(self.widths)
        mean_net = {"num_dormant": counts[-1], "num_rows": self.num_rows, "num_entries": n_mean,
                    "percent_dormant": counts[-1] / self.num_rows * 100.0, "fraction_dormant": counts[-1] / n_mean,
                    "activation": dict(zip(names, vals[k:k + 4]))}
        return {"layers": layers, "mean_net": mean_net, "steps": self.steps}
