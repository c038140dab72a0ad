"""clip_grad_norm_ + AdamW (amsgrad off, maximize off) in float64 on the CPU, written out from the update rule - the yardstick of
tests/test_adamw_gpu.py and tests/test_adamw_cpu.py (which pins it against torch.optim.AdamW in float64):

    coef = min(max_norm / (norm + 1e-6), 1)        (max_norm None or <= 0: no clip)
    g'   = coef g
    p   <- p (1 - lr wd)
    m   <- beta1 m + (1 - beta1) g'
    v   <- beta2 v + (1 - beta2) g'^2
    p   <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)            t = 1, 2, ...
"""
import math

import torch


class AdamWRef:
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.p = [torch.as_tensor(p).detach().to("cpu", torch.float64).clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps, self.wd, self.t = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay), 0

    def step(self, grads, max_norm=None):
        """One step on `grads` (one tensor per parameter, any float dtype: widened to float64, left untouched).  Returns the gradient norm."""
        g = [torch.as_tensor(x).detach().to("cpu", torch.float64) for x in grads]
        norm = math.sqrt(sum(float((x * x).sum()) for x in g))
        coef = 1.0
        if max_norm is not None and max_norm > 0:
            coef = min(float(max_norm) / (norm + 1e-6), 1.0)
        self.t += 1
        b1, b2 = self.betas
        step_size = self.lr / (1.0 - b1 ** self.t)
        bc2_sqrt = math.sqrt(1.0 - b2 ** self.t)
        for p, m, v, x in zip(self.p, self.m, self.v, g):
            x = coef * x
            p.mul_(1.0 - self.lr * self.wd)
            m.mul_(b1).add_(x, alpha=1.0 - b1)
            v.mul_(b2).add_(x * x, alpha=1.0 - b2)
            p.sub_(step_size * m / (v.sqrt() / bc2_sqrt + self.eps))
        return norm


def check_against_torch(steps=5, seed=0):
    """max |AdamWRef - torch.optim.AdamW(float64)| over parameters and both moments after `steps` clipped steps on two tensors."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(7, 5), (11,)]
    p0 = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    tp = [torch.nn.Parameter(p.clone()) for p in p0]
    opt = torch.optim.AdamW(tp, 1e-3, weight_decay=0.01, foreach=False)
    ref = AdamWRef(p0, 1e-3, weight_decay=0.01)
    for _ in range(steps):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 3, (1,), generator=gen)) for s in shapes]
        for p, x in zip(tp, grads):
            p.grad = x.clone()
        torch.nn.utils.clip_grad_norm_(tp, 0.5)
        opt.step()
        ref.step(grads, 0.5)
    err = 0.0
    for i, p in enumerate(tp):
        st = opt.state[p]
        err = max(err, float((p.detach() - ref.p[i]).abs().max()), float((st["exp_avg"] - ref.m[i]).abs().max()),
                  float((st["exp_avg_sq"] - ref.v[i]).abs().max()))
    return err
