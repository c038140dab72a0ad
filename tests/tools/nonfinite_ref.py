"""CPU torch, fp32 statements of the learner operations that have no class of their own in the reference - it calls torch for them -
and the comparison rule of the non-finite tests (tests/test_nonfinite_ref_cpu.py pins them, tests/test_nonfinite_gpu.py uses them):

* clip_grad_norm_ followed by torch.optim.SGD(momentum=0.9)        (MPOptimizer.step, learning/mp_optimizer.py:20-40 of the reference)
* clip_grad_norm_ followed by torch.optim.AdamW(foreach=False)      (optimizer type "Adam", learning/mp_optimizer.py:51-62)
* aten.threshold_backward followed by a column sum                  (what autograd runs behind relu(x W^T + b))
* PPOAgent._compute_loss (learning/ppo_agent.py:212-330) as one torch expression that SELECTS the random-action rows with a boolean
  index, as the reference does: an unselected row is never evaluated, whatever it holds.

Nothing here treats NaN or Inf specially: what comes out is what torch does with them."""
import numpy as np
import torch

LOG_2PI = float(np.log(2.0 * np.pi))


def assert_same(got, want, rtol=0.0, atol=0.0, what=""):
    """The comparison rule: NaN at the same positions, +-Inf at the same positions with the same sign, finite entries within
    atol + rtol |want| (both 0: bit-equal values, with -0 == +0 as torch.equal has it)."""
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, np.float64)
    want = np.asarray(want.detach().cpu() if isinstance(want, torch.Tensor) else want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert np.array_equal(nan_g, nan_w), "{}: NaN at {} here, at {} in the reference".format(
        what, np.argwhere(nan_g)[:8].tolist(), np.argwhere(nan_w)[:8].tolist())
    inf_g, inf_w = np.isinf(got), np.isinf(want)
    assert np.array_equal(inf_g, inf_w) and np.array_equal(got[inf_g], want[inf_w]), "{}: Inf {} at {} here, {} at {} in the reference".format(
        what, got[inf_g][:8].tolist(), np.argwhere(inf_g)[:8].tolist(), want[inf_w][:8].tolist(), np.argwhere(inf_w)[:8].tolist())
    fin = ~(nan_w | inf_w)
    err = np.abs(got[fin] - want[fin])
    bad = err > atol + rtol * np.abs(want[fin])
    assert not bad.any(), "{}: {} of {} finite entries differ, max |d| {:.3e} (atol {}, rtol {}); first at {}".format(
        what, int(bad.sum()), int(fin.sum()), float(err.max()), atol, rtol, np.argwhere(fin)[bad.nonzero()[0][:4]].tolist())


def _params(p0):
    return torch.nn.Parameter(torch.as_tensor(p0, dtype=torch.float32).detach().cpu().clone())


def sgd_steps(p0, grads, max_norm, lr, momentum=0.9, weight_decay=0.0):
    """One flat parameter, one step per gradient.  -> per step (params, momentum buffer, gradient as clip_grad_norm_ left it, norm);
    max_norm <= 0: no clip, norm None."""
    p = _params(p0)
    opt = torch.optim.SGD([p], lr, momentum=momentum, weight_decay=weight_decay)
    out = []
    for g in grads:
        p.grad = torch.as_tensor(g, dtype=torch.float32).detach().cpu().clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm > 0 else None
        opt.step()
        out.append((p.detach().clone(), opt.state[p]["momentum_buffer"].clone(), p.grad.clone(), norm))
    return out


def adamw_steps(p0, grads, max_norm, lr, betas, eps, weight_decay, dtype=torch.float32):
    """As sgd_steps for torch.optim.AdamW(foreach=False).  -> per step (params, exp_avg, exp_avg_sq, clipped gradient, norm).
    dtype float64: the yardstick of the 4 E_ref rule of tests/test_adamw_gpu.py, on the same fp32 inputs."""
    p = torch.nn.Parameter(torch.as_tensor(p0, dtype=torch.float32).detach().cpu().to(dtype).clone())
    opt = torch.optim.AdamW([p], lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.as_tensor(g, dtype=torch.float32).detach().cpu().to(dtype).clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm) if max_norm > 0 else None
        opt.step()
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), p.grad.clone(), norm))
    return out


def relu_bwd_bias(gy, y):
    """-> (gy masked by threshold_backward(gy, y, 0), its column sums)"""
    g = torch.ops.aten.threshold_backward(torch.as_tensor(gy, dtype=torch.float32).cpu(), torch.as_tensor(y, dtype=torch.float32).cpu(), 0.0)
    return g, g.sum(dim=0)


def ppo_loss(mean, logstd, pred, norm_a, old_logp, adv, mask, tar_val, clip, bound_w, critic_w, large_critic_loss=20.0):
    """L2 critic, entropy and regulariser weights 0 (the configuration of fixture G30).  mean [B, A], logstd [A], pred [B].
    -> (info dict of floats incl. "cnt", (grad mean, grad logstd, grad pred))"""
    t = lambda v: torch.as_tensor(v, dtype=torch.float32).detach().cpu().clone()      # noqa: E731
    mean, logstd, pred = t(mean).requires_grad_(True), t(logstd).requires_grad_(True), t(pred).requires_grad_(True)
    norm_a, old_logp, adv, mask, tar_val = t(norm_a), t(old_logp), t(adv), t(mask), t(tar_val)
    A = mean.shape[1]
    critic_loss = torch.mean(torch.square(tar_val - pred))
    sel = mask == 1.0
    mu, na = mean[sel], norm_a[sel]
    logp = -0.5 * torch.sum(torch.square((na - mu) / torch.exp(logstd)), dim=-1) + (-0.5 * A * LOG_2PI - torch.sum(logstd))
    ratio = torch.exp(logp - old_logp[sel])
    l0, l1 = adv[sel] * ratio, adv[sel] * torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    actor_loss = -torch.mean(torch.minimum(l0, l1))
    viol = torch.sum(torch.square(torch.clamp_max(mu + 1.0, 0.0)), dim=-1) + torch.sum(torch.square(torch.clamp_min(mu - 1.0, 0.0)), dim=-1)
    abl = torch.mean(viol)
    actor_loss = actor_loss + bound_w * abl
    term = actor_loss.detach() if critic_loss.item() > large_critic_loss else actor_loss
    loss = term + critic_w * critic_loss
    grads = torch.autograd.grad(loss, [mean, logstd, pred], allow_unused=True)
    grads = tuple(torch.zeros_like(p) if g is None else g for g, p in zip(grads, (mean, logstd, pred)))
    info = {"loss": loss.item(), "critic_loss": critic_loss.item(), "actor_loss": actor_loss.item(),
            "clip_frac": torch.mean((torch.abs(ratio - 1.0) > clip).float()).item(), "imp_ratio": torch.mean(ratio).item(),
            "action_bound_loss": abl.item(), "cnt": float(sel.sum())}
    return info, grads


def g30_ppo_case(z, name):
    """Inputs, terms and gradients of one loss case of fixture G30 (an input the case leaves alone is stored once, as ppo_<input>)."""
    p = "ppo_" + name + "_"
    c = {k: z[p + k] if p + k in z.files else z["ppo_" + k] for k in ("mean", "norm_action", "a_logp", "tar_val")}
    c.update(logstd=z["ppo_logstd"], pred=z["ppo_pred"], adv=z["ppo_adv"], mask=z[p + "mask"], info=dict(zip([str(k) for k in z["ppo_info_names"]], z[p + "info"])),
             grad_mean=z[p + "grad_mean"], grad_logstd=z[p + "grad_logstd"], grad_pred=z[p + "grad_pred"])
    return c
