#!/usr/bin/env python3
"""Generate tests/golden/g30_nonfinite.npz: what the REFERENCE's own code (CPU, torch) makes of NaN and Inf at the places where the
learner kernels restate it.

Runs ONLY in the build container (needs the reference tree).  Importing gen_golden registers the stub modules and puts the reference
on the path.  Three reference functions are called:

* PPOAgent._compute_critic_loss and _compute_actor_loss (learning/ppo_agent.py:259-330), unbound on the stub agent of gen_golden's G14
  stage, with autograd gradients w.r.t. mean, logstd and the critic's prediction.  _compute_loss itself is not called: its NaN trap
  (ppo_agent.py:242-252) ends the process; loss = actor_loss + critic_w critic_loss is formed here as it does (no case reaches the
  "LARGE CRITIC LOSS" branch: a NaN compares false).  B = 70, A = 28; the poison sits in rows 3 and 66.
* the advantage normalisation of DMPPOAgent._build_train_data (learning/dm_ppo_agent.py:343-411), unbound on a stub whose critic
  returns the observation itself and whose discount is 0, so that the TD(lambda) return IS the reward row: `ret` = what the method
  stored as tar_val, `vals` = the observations.  One time row of n = 300 (with more rows a NaN return would reach the row
  before it through 0 x NaN).
* Normalizer.normalize (learning/normalizer.py:83-86) on a [5, 8] block with clip 5.

usage:  python tests/golden/gen_nonfinite.py            # rewrites tests/golden/g30_nonfinite.npz
        python tests/golden/gen_nonfinite.py --check    # regenerate into a scratch dir and compare with the committed fixture
"""
import os
import sys
import tempfile
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as gg  # noqa: E402  (stubs + reference path + chdir to the reference root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, A = 70, 28
ROWS = (3, 66)                 # one in each 64-sample block of the 32-lane loss kernel
COLS = (5, A - 1)              # the poisoned element of a [B, A] row: an inner lane and the last one
PPO_CASES = ["finite", "nan_action_selected", "nan_action_unselected", "nan_mean_selected", "nan_mean_unselected", "inf_ratio_unselected",
             "nan_tar_val"]
PPO_PARAMS = np.array([0.2, 10.0, 0.0, 0.0, 0.5, 20.0, 0.0], np.float64)      # clip, bound_w, entropy_w, reg_w, critic_w, gate, l1 (as G14)
INFO_NAMES = ["loss", "critic_loss", "actor_loss", "clip_frac", "imp_ratio", "action_bound_loss"]
ADV_T, ADV_N, ADV_CLIP = 1, 300, 4.0
ADV_CASES = ["finite", "nan_selected", "nan_unselected", "inf_selected", "one_selected", "none_selected"]
NAN, INF = float("nan"), float("inf")


def ppo_cases(out):
    base_agent, dgd, _, _, ppo_agent, _ = gg._import_learning()
    g = torch.Generator().manual_seed(30)
    mean0 = torch.randn(B, A, generator=g) * 0.7             # some |mean| > 1: the action-bound term is active
    logstd0 = torch.randn(A, generator=g) * 0.2 - 1.5
    pred0 = torch.randn(B, generator=g)
    norm_a0 = mean0 + torch.exp(logstd0) * torch.randn(B, A, generator=g)
    adv0 = torch.randn(B, generator=g)
    adv0[ROWS[0]], adv0[ROWS[1]] = -0.7, -1.3                # negative: an overflowed ratio gives l0 = -inf there
    tar0 = torch.randn(B, generator=g)
    logp0 = dgd.DistributionGaussianDiag(mean0, logstd0.expand(B, A)).log_prob(norm_a0) + 0.3 * torch.randn(B, generator=g)
    mask0 = (torch.rand(B, generator=g) < 0.75).float()
    a_low, a_high = -np.ones(A, np.float32) * 2.0, np.ones(A, np.float32) * 3.0
    out.update(ppo_mean=mean0, ppo_logstd=logstd0, ppo_pred=pred0, ppo_norm_action=norm_a0, ppo_adv=adv0, ppo_tar_val=tar0, ppo_a_logp=logp0,
               ppo_case_names=np.array(PPO_CASES), ppo_info_names=np.array(INFO_NAMES), ppo_params=PPO_PARAMS,
               ppo_rows=np.array(ROWS, np.int64), ppo_cols=np.array(COLS, np.int64))
    clip, bw, ew, rw, cw = [float(v) for v in PPO_PARAMS[:5]]
    for name in PPO_CASES:
        mean_in, norm_a, logp, tar, mask = mean0.clone(), norm_a0.clone(), logp0.clone(), tar0.clone(), mask0.clone()
        for r in ROWS:
            mask[r] = 0.0 if name.endswith("_unselected") else 1.0
        for r, c in zip(ROWS, COLS):
            if name.startswith("nan_action"):
                norm_a[r, c] = NAN
            if name.startswith("nan_mean"):
                mean_in[r, c] = NAN
            if name == "inf_ratio_unselected":
                logp[r] = -INF
            if name == "nan_tar_val":
                tar[r] = NAN
        mean, logstd, pred = mean_in.clone().requires_grad_(True), logstd0.clone().requires_grad_(True), pred0.clone().requires_grad_(True)
        ag = gg._Stub()
        ag._ppo_clip_ratio, ag._critic_loss_weight, ag._critic_loss_type = clip, cw, "L2"
        ag._action_bound_weight, ag._action_entropy_weight, ag._action_reg_weight = bw, ew, rw
        ag._env = gg._Stub()
        ag._env.get_action_space = lambda: gg._Box(a_low, a_high)
        model = gg._Stub()
        # "observations" are row numbers, so that the rows the reference selects by mask reach the right means
        model.eval_actor = lambda o: dgd.DistributionGaussianDiag(mean[o[:, 0].long()], torch.broadcast_to(logstd, (o.shape[0], A)))
        model.eval_critic = lambda o: pred[o[:, 0].long()].unsqueeze(-1)
        ag._model = model
        ag._compute_action_bound_loss = base_agent.BaseAgent._compute_action_bound_loss.__get__(ag)
        obs = torch.arange(B, dtype=torch.float32).unsqueeze(-1)
        info = {**ppo_agent.PPOAgent._compute_critic_loss(ag, {"norm_obs": obs, "tar_val": tar}),
                **ppo_agent.PPOAgent._compute_actor_loss(ag, {"norm_obs": obs, "norm_action": norm_a, "a_logp": logp, "adv": adv0,
                                                               "rand_action_mask": mask})}
        assert not (float(info["critic_loss"].detach()) > 20.0)
        info["loss"] = info["actor_loss"] + cw * info["critic_loss"]
        grads = torch.autograd.grad(info["loss"], [mean, logstd, pred])
        p = "ppo_" + name + "_"
        out[p + "info"] = np.array([float(info[k]) for k in INFO_NAMES], np.float64)
        out[p + "mask"] = mask
        for k, v, v0 in (("mean", mean_in, mean0), ("norm_action", norm_a, norm_a0), ("a_logp", logp, logp0), ("tar_val", tar, tar0)):
            if not torch.equal(v, v0):                        # an input the case leaves alone is the shared one (ppo_<name>)
                out[p + k] = v
        out[p + "grad_mean"], out[p + "grad_logstd"], out[p + "grad_pred"] = grads
        print(name, dict(zip(INFO_NAMES, out[p + "info"])), "selected", int(mask.sum()))


def adv_cases(out):
    import envs.base_env as base_env
    import learning.dm_ppo_agent as ref_agent
    g = torch.Generator().manual_seed(31)
    ret0 = torch.randn(ADV_T, ADV_N, generator=g) * 3.0 + 1.0
    ret0[0, 5], ret0[0, 6] = 40.0, -40.0                     # both sides of the clamp are reached
    vals0 = torch.randn(ADV_T, ADV_N, generator=g)
    mask0 = (torch.rand(ADV_T, ADV_N, generator=g) < 0.8).float()
    sel, uns = (0, 37), (0, ADV_N - 1)                        # (row, env) of the poisoned element; the unselected one is the last sample
    mask0[sel], mask0[uns] = 1.0, 0.0
    out.update(adv_case_names=np.array(ADV_CASES), adv_vals=vals0, adv_clip=np.float64(ADV_CLIP))
    for name in ADV_CASES:
        ret, mask = ret0.clone(), mask0.clone()
        if name == "nan_selected":
            ret[sel] = NAN
        if name == "nan_unselected":
            ret[uns] = NAN
        if name == "inf_selected":
            ret[sel] = INF
        if name in ("one_selected", "none_selected"):
            mask.zero_()
        if name == "one_selected":
            mask[sel] = 1.0
        data = {"obs": vals0.unsqueeze(-1), "next_obs": torch.zeros(ADV_T, ADV_N, 1), "reward": ret, "rand_action_mask": mask,
                "done": torch.full((ADV_T, ADV_N), base_env.DoneFlags.NULL.value, dtype=torch.int)}
        ag = gg._Stub()
        ag.eval = lambda: None
        ag._exp_buffer = gg._Stub()
        ag._exp_buffer.get_data = lambda k: data[k]
        ag._exp_buffer.set_data = lambda k, v: data.__setitem__(k, v)
        ident = gg._Stub()
        ident.normalize = lambda x: x
        ag._obs_norm = ident
        ag._model = gg._Stub()
        ag._model.eval_critic = lambda o: o                   # the critic's value of an "observation" is the observation
        ag._compute_val_bound = lambda: (-1e30, 1e30)
        ag._compute_succ_val = ag._compute_fail_val = lambda: 0.0
        ag._discount, ag._td_lambda, ag._norm_adv_clip, ag._device = 0.0, 0.95, ADV_CLIP, "cpu"
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                   # std_mean of fewer than two elements warns about the degrees of freedom
            info = ref_agent.DMPPOAgent._build_train_data(ag)
        same = (data["tar_val"] == ret) | (torch.isnan(data["tar_val"]) & torch.isnan(ret))
        assert same.all(), "discount 0: the return is the reward row"
        p = "adv_" + name + "_"
        out[p + "ret"], out[p + "mask"], out[p + "norm_adv"] = data["tar_val"], mask, data["adv"]
        out[p + "adv_mean"], out[p + "adv_std"] = info["adv_mean"], info["adv_std"]
        print(name, "mean", float(info["adv_mean"]), "std", float(info["adv_std"]), "NaN advantages", int(torch.isnan(data["adv"]).sum()))


def normalizer_case(out):
    _, _, _, normalizer, _, _ = gg._import_learning()
    g = torch.Generator().manual_seed(32)
    rows, dim, clip = 5, 8, 5.0
    mean = torch.randn(dim, generator=g)
    std = torch.rand(dim, generator=g) + 0.5
    x = torch.randn(rows, dim, generator=g) * 4.0            # some |x - mean| / std > clip
    x[0, 0], x[1, 5], x[2, 7] = NAN, INF, -INF
    mean[3] = NAN
    std[6] = 0.0
    x[4, 6] = mean[6]                                         # 0 / 0 in this row, +-inf -> +-clip in the others
    nz = normalizer.Normalizer((dim,), "cpu", init_mean=mean, init_std=std, clip=clip)
    out.update(nz_x=x, nz_mean=mean, nz_std=std, nz_clip=np.float64(clip), nz_normalized=nz.normalize(x))


def main():
    check = "--check" in sys.argv
    dst_dir = tempfile.mkdtemp(prefix="parc_g30_check_") if check else HERE
    out = {}
    ppo_cases(out)
    adv_cases(out)
    normalizer_case(out)
    dst = os.path.join(dst_dir, "g30_nonfinite.npz")
    np.savez_compressed(dst, **{k: gg.npy(v) for k, v in out.items()})
    print("wrote", dst, os.path.getsize(dst), "bytes")
    if check:
        a, b = np.load(dst), np.load(os.path.join(HERE, "g30_nonfinite.npz"))
        bad = 0
        for k in sorted(set(a.files) | set(b.files)):
            same = k in a.files and k in b.files and a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")
            if not same:
                bad += 1
                print("DIFFERS", k)
        print("check: {} arrays differ from the committed fixture".format(bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
