"""The flat AdamW step of `optimizer.type: Adam`: parc_adamw_step (clip by global norm + torch.optim.AdamW over flat buffers, two passes)
and MPOptimizer's flat path around it.

The tolerance rule of this file: the yardstick is a float64 AdamW on the CPU (tests/tools/adamw_ref.py, pinned against torch's float64
AdamW).  torch's own fp32 AdamW on the same gradients has the error E_ref = max |torch fp32 - float64|; the kernel's error
E_kernel = max |kernel - float64| must not exceed 4 E_ref (the factor covers fma contraction and another sqrt / divide sequence),
for the parameters and for each moment buffer against its own E_ref."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import adamw_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
K_STEPS = 5
# 2 097 152 + 7: more float4s than one round of the update kernel's grid has threads, and not a multiple of 4: grid-stride loop + tail
SIZES = [1, 3, 255, 2284, 2097152 + 7]


def _adamw(L, n, p, g, m, v, step, max_norm, wd, ws, norm, lr=LR, b1=BETAS[0], b2=BETAS[1], eps=EPS, stream=None):
    from parc_amd import _hip
    ptr = lambda t: t if (t is None or isinstance(t, ctypes.c_void_p)) else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return L.parc_adamw_step(stream if stream is not None else _hip.stream(), n, ptr(p), ptr(g), ptr(m), ptr(v), step, max_norm, lr, b1, b2, eps, wd,
                             ptr(ws), ptr(norm))


def _recorded_gradients(n, seed):
    """K fp32 gradients with magnitudes from 1e-6 to 1e2; the first n // 3 elements are exact zeros in every step (there m = v = 0, the
    update is 0 and only the decay acts)."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = []
    for _ in range(K_STEPS):
        g = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 8.0 - 6.0)
        g[:n // 3] = 0.0
        grads.append(g)
    return p0, grads


def _max_norm_for(clip, grads):
    norms = [float(g.double().norm()) for g in grads]
    if clip == "off":
        return -1.0                                          # no clip and no norm pass
    if clip == "inactive":
        return float(np.float32(2.0 * max(norms)))           # the norm pass runs, coef = 1
    return float(np.float32(0.5 * min(norms)))               # coef < 1 in every step


def _ratio_check(what, got, ref32, ref64):
    e_ref = float((ref32.double() - ref64).abs().max())
    e_ker = float((got.double().cpu() - ref64).abs().max())
    ratio = e_ker / e_ref if e_ref > 0 else (0.0 if e_ker == 0 else float("inf"))
    print("  {:>10}: E_kernel {:.3e}  E_ref {:.3e}  ratio {:.3f}".format(what, e_ker, e_ref, ratio))
    assert e_ker <= 4.0 * e_ref, (what, e_ker, e_ref)
    return ratio


def test_float64_yardstick_is_torch_adamw():
    assert adamw_ref.check_against_torch(steps=K_STEPS) <= 1e-12


@pytest.mark.parametrize("clip", ["off", "inactive", "active"])
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_float64(n, wd, clip):
    """(a) CPU torch.optim.AdamW(foreach=False) fp32, (b) parc_adamw_step, (c) float64, on the same recorded fp32 gradients, K = 5 steps."""
    from parc_amd import _hip
    L = _hip.lib()
    p0, grads = _recorded_gradients(n, seed=n % 1000)
    max_norm = _max_norm_for(clip, grads)
    # (a)
    pa = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pa], LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    # (c)
    ref = adamw_ref.AdamWRef([p0], LR, BETAS, EPS, wd)
    # (b)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ws = torch.empty(int(L.parc_sgd_workspace_floats()), device=DEV)
    norm_out = torch.full((1,), -7.0, device=DEV)
    for k, g in enumerate(grads):
        pa.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([pa], max_norm, foreach=False)
        opt.step()
        norm64 = ref.step([g], max_norm)
        gd = g.to(DEV)
        assert _adamw(L, n, p, gd, m, v, k + 1, max_norm, wd, ws, norm_out) == 0
        assert torch.equal(gd.cpu(), g)                                       # grad is left as it was, bit for bit
        if max_norm > 0:
            assert abs(norm_out.item() - norm64) <= 1e-5 * norm64, (k, norm_out.item(), norm64)
            assert (norm64 > max_norm) == (clip == "active")
        else:
            assert norm_out.item() == -7.0
    st = opt.state[pa]
    print("n = {} wd = {} clip = {} (max_norm {:.6g})".format(n, wd, clip, max_norm))
    _ratio_check("params", p, pa.detach(), ref.p[0])
    _ratio_check("exp_avg", m, st["exp_avg"], ref.m[0])
    _ratio_check("exp_avg_sq", v, st["exp_avg_sq"], ref.v[0])
    z = n // 3                                                                # the block of zero gradients: only the decay acted
    if z:
        assert float(m[:z].abs().max()) == 0.0 and float(v[:z].abs().max()) == 0.0
        assert torch.equal(p[:z].cpu(), pa.detach()[:z])                      # K roundings of p (1 - lr wd), the same factor in both
        assert torch.equal(p[:z].cpu(), p0[:z]) == (wd == 0.0)


def test_misaligned_buffers_take_the_scalar_path_with_the_same_arithmetic():
    """params / exp_avg / exp_avg_sq 4 bytes off a 16-byte boundary (grad aligned): the element-wise path; bit for bit the vector path."""
    from parc_amd import _hip
    L = _hip.lib()
    n = 2284
    p0, grads = _recorded_gradients(n, seed=5)
    ws = torch.empty(int(L.parc_sgd_workspace_floats()), device=DEV)
    norm_out = torch.zeros(1, device=DEV)
    out = []
    for off in (0, 1):
        store = [torch.zeros(n + 8, device=DEV) for _ in range(3)]
        p, m, v = [s[off:off + n] for s in store]
        assert all((t.data_ptr() % 16 == 0) == (off == 0) for t in (p, m, v))
        p.copy_(p0)
        for k, g in enumerate(grads):
            assert _adamw(L, n, p, g.to(DEV), m, v, k + 1, 0.5, 0.01, ws, norm_out) == 0
        assert all(float(s[:off].abs().max() if off else 0.0) == 0.0 and float(s[off + n:].abs().max()) == 0.0 for s in store)   # nothing beyond
        out.append([t.clone() for t in (p, m, v)])
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_bad_arguments_are_refused_and_nothing_is_written():
    from parc_amd import _hip
    L = _hip.lib()
    n = 64
    bufs = {k: torch.full((n + 4,), 3.0, device=DEV) for k in ("p", "g", "m", "v")}
    ws = torch.full((int(L.parc_sgd_workspace_floats()),), 3.0, device=DEV)
    norm_out = torch.full((1,), 3.0, device=DEV)
    p, g, m, v = [bufs[k][:n] for k in ("p", "g", "m", "v")]
    null = ctypes.c_void_p(0)
    good = dict(n=n, p=p, g=g, m=m, v=v, step=1, max_norm=0.5, wd=0.01, ws=ws, norm=norm_out)
    bad = [dict(p=null), dict(g=null), dict(m=null), dict(v=null), dict(ws=null), dict(n=-1), dict(step=0), dict(step=-3), dict(g=bufs["g"][1:n + 1]),
           dict(b1=1.0), dict(b1=-0.1), dict(b1=float("nan")), dict(b2=1.0), dict(b2=-0.1), dict(eps=0.0), dict(eps=-1e-8)]
    for change in bad:
        assert _adamw(L, **dict(good, **change)) == -1, change
    assert _adamw(L, **dict(good, n=0)) == 0
    torch.cuda.synchronize()
    for t in list(bufs.values()) + [ws, norm_out]:
        assert float((t - 3.0).abs().max()) == 0.0
    assert _adamw(L, **dict(good, norm=null)) == 0              # norm_out may be NULL, as in the SGD entry
    torch.cuda.synchronize()
    assert float((g - 3.0).abs().max()) == 0.0 and float((p - 3.0).abs().max()) > 0.0 and float((bufs["p"][n:] - 3.0).abs().max()) == 0.0


# ---- MPOptimizer ----------------------------------------------------------------------------------------------------------------------

CFG = {"type": "Adam", "learning_rate": 1e-3, "weight_decay": 0.01}


def _mlp(dtype=torch.float32, device=None):
    return torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.ReLU(), torch.nn.Linear(53, 5)).to(device=device or DEV, dtype=dtype)


_REFERENCE = {}


def _reference_run(max_norm):
    """Three steps of clip_grad_norm_ + torch.optim.AdamW on the device (fp32) and of the float64 run on the CPU, on the same inputs:
    computed once per max_norm and shared.  Returns (initial state_dict, inputs, fp32 parameters, float64 parameters, fp32 grad norms)."""
    if max_norm not in _REFERENCE:
        torch.manual_seed(1)
        ref = _mlp()
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        xs = [torch.randn(64, 37, device=DEV) for _ in range(3)]
        opt_ref = torch.optim.AdamW(ref.parameters(), CFG["learning_rate"], weight_decay=CFG["weight_decay"])
        m64 = _mlp(torch.float64, "cpu")
        m64.load_state_dict({k: v.double().cpu() for k, v in sd.items()})
        ref64 = adamw_ref.AdamWRef(list(m64.parameters()), CFG["learning_rate"], BETAS, EPS, CFG["weight_decay"])
        norms = []
        for x in xs:
            opt_ref.zero_grad()
            ref(x).square().sum().backward()
            norms.append(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm).item())
            opt_ref.step()
            g64 = torch.autograd.grad(m64(x.double().cpu()).square().sum(), list(m64.parameters()))
            ref64.step(g64, max_norm)
            with torch.no_grad():
                for q, new in zip(m64.parameters(), ref64.p):
                    q.copy_(new)
        _REFERENCE[max_norm] = (sd, xs, torch.cat([q.detach().reshape(-1) for q in ref.parameters()]).cpu(), torch.cat([q.reshape(-1) for q in ref64.p]), norms)
    return _REFERENCE[max_norm]


def _train_three_steps(cfg, max_norm):
    from parc_amd.learning import mp_optimizer
    sd, xs, p32, p64, norms = _reference_run(max_norm)
    mine = _mlp()
    mine.load_state_dict(sd)
    opt = mp_optimizer.MPOptimizer(cfg, list(mine.parameters()))
    for k, x in enumerate(xs):
        opt.step(mine(x).square().sum(), model=mine, max_norm=max_norm)
        if getattr(opt, "_flat_adam", False):
            assert abs(opt._grad_norm.item() - norms[k]) <= 1e-5 * norms[k]
    assert (norms[-1] > max_norm) == (max_norm == 0.5)
    print("max_norm", max_norm, "flat_adam", cfg.get("flat_adam", True))
    _ratio_check("params", torch.cat([q.detach().reshape(-1) for q in mine.parameters()]), p32, p64)
    return mine, opt


@pytest.mark.parametrize("max_norm", [1000.0, 0.5])
def test_flat_adam_step_equals_torch_adamw_with_clipping(max_norm):
    mine, opt = _train_three_steps(dict(CFG), max_norm)
    assert opt._flat_adam and not opt._flat_sgd and opt._optimizer is None
    off = 0
    for q in mine.parameters():                                   # every parameter is its slice of the flat buffer
        assert q.data_ptr() == opt._flat_param.data_ptr() + 4 * off
        off += q.numel()
    assert off == opt._flat_param.numel() == opt._flat_exp_avg.numel() == opt._flat_exp_avg_sq.numel()
    assert float(opt._flat_exp_avg.abs().max()) > 0 and float(opt._flat_exp_avg_sq.min()) >= 0 and opt._adam_steps == 3
    sd = mine.state_dict()                                        # parameters are views of the flat buffer: state_dict round trip
    mine.load_state_dict({k: v.clone() + 1.0 for k, v in sd.items()})
    assert torch.allclose(opt._flat_param, torch.cat([q.reshape(-1) for q in mine.parameters()]))
    opt._check_aliasing()


@pytest.mark.parametrize("max_norm", [1000.0, 0.5])
def test_flat_adam_false_keeps_the_torch_path(max_norm):
    """`flat_adam: False` is the path from before the flat step: a torch AdamW over separately allocated parameters."""
    mine, opt = _train_three_steps(dict(CFG, flat_adam=False), max_norm)
    assert isinstance(opt._optimizer, torch.optim.AdamW) and not hasattr(opt, "_flat_param") and not getattr(opt, "_flat_adam", False)
    assert opt._optimizer.param_groups[0]["weight_decay"] == 0.01


def test_step_explicit_equals_step_bit_for_bit():
    from parc_amd.learning import mp_optimizer
    torch.manual_seed(3)
    a, b = _mlp(), _mlp()
    b.load_state_dict(a.state_dict())
    oa = mp_optimizer.MPOptimizer(dict(CFG), list(a.parameters()))
    ob = mp_optimizer.MPOptimizer(dict(CFG), list(b.parameters()))
    for _ in range(3):
        x = torch.randn(32, 37, device=DEV)
        oa.step(a(x).square().sum(), model=a, max_norm=0.5)
        params = list(b.parameters())
        grads = torch.autograd.grad(b(x).square().sum(), params)

        def write(grad_of, done):
            for q, gq in reversed(list(zip(params, grads))):
                grad_of(q).copy_(gq)
                done(q)
        ob.step_explicit(write, model=b, max_norm=0.5)
        assert torch.equal(oa._flat_grad, ob._flat_grad)
    assert torch.equal(oa._flat_param, ob._flat_param) and torch.equal(oa._flat_exp_avg_sq, ob._flat_exp_avg_sq)
    assert oa._adam_steps == ob._adam_steps == 3 and oa._grad_norm.item() == ob._grad_norm.item()


def test_reset_state_restarts_moments_and_bias_correction():
    from parc_amd.learning import mp_optimizer
    torch.manual_seed(4)
    a = _mlp()
    oa = mp_optimizer.MPOptimizer(dict(CFG), list(a.parameters()))
    xs = [torch.randn(32, 37, device=DEV) for _ in range(3)]
    for x in xs[:2]:
        oa.step(a(x).square().sum(), model=a, max_norm=0.5)
    oa.reset_state()
    assert oa._adam_steps == 0 and float(oa._flat_exp_avg.abs().max()) == 0.0 and float(oa._flat_exp_avg_sq.abs().max()) == 0.0
    b = _mlp()
    b.load_state_dict(a.state_dict())
    ob = mp_optimizer.MPOptimizer(dict(CFG), list(b.parameters()))
    oa.step(a(xs[2]).square().sum(), model=a, max_norm=0.5)
    ob.step(b(xs[2]).square().sum(), model=b, max_norm=0.5)
    assert torch.equal(oa._flat_param, ob._flat_param) and torch.equal(oa._flat_exp_avg, ob._flat_exp_avg)
    assert torch.equal(oa._flat_exp_avg_sq, ob._flat_exp_avg_sq) and oa.get_steps() == 3 and ob.get_steps() == 1


def test_flat_adam_notices_a_rebound_parameter():
    from parc_amd.learning import mp_optimizer
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2)).to(DEV)
    opt = mp_optimizer.MPOptimizer({"type": "Adam", "learning_rate": 0.1}, list(m.parameters()))
    assert opt._flat_adam and opt._optimizer is None
    opt.CHECK_ALIAS_STEPS = 1
    x = torch.randn(5, 8, device=DEV)
    w0 = m[0].weight.detach().clone()
    opt.step(torch.mean(torch.square(m(x))))
    assert not torch.equal(w0, m[0].weight)                   # the view moved with the flat buffer
    opt._check_aliasing()
    m[0].weight.data = m[0].weight.data.clone()
    with pytest.raises(RuntimeError, match="no longer aliases the optimizer's flat parameter buffer"):
        opt.step(torch.mean(torch.square(m(x))))
    m2 = torch.nn.Linear(4, 4).to(DEV)
    opt2 = mp_optimizer.MPOptimizer({"type": "Adam", "learning_rate": 0.1}, list(m2.parameters()))
    m2.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="no longer aliases the flat gradient buffer"):
        opt2._check_aliasing()


def test_end_epoch_exchanges_exactly_the_three_flat_buffers():
    """Single process: end_epoch() is a no-op; the buffers the "epoch" cadence would all-reduce in place are the flat parameters and the
    two flat moments themselves (no packed copy)."""
    from parc_amd.learning import mp_optimizer
    torch.manual_seed(0)
    m = _mlp()
    opt = mp_optimizer.MPOptimizer(dict(CFG, grad_allreduce="epoch"), list(m.parameters()))
    opt.step(m(torch.randn(8, 37, device=DEV)).square().sum(), model=m, max_norm=0.5)
    before = [t.clone() for t in (opt._flat_param, opt._flat_exp_avg, opt._flat_exp_avg_sq)]
    opt.end_epoch()
    bufs = opt._epoch_exchange_buffers()
    assert len(bufs) == 3 and bufs[0] is opt._flat_param and bufs[1] is opt._flat_exp_avg and bufs[2] is opt._flat_exp_avg_sq
    assert all(torch.equal(a, b) for a, b in zip(before, bufs))
    flat, scatter = opt._flat_view_of_params()
    assert flat is opt._flat_param and scatter is None
    sgd = mp_optimizer.MPOptimizer({"type": "SGD", "learning_rate": 0.1}, list(_mlp().parameters()))
    sb = sgd._epoch_exchange_buffers()
    assert len(sb) == 2 and sb[0] is sgd._flat_param and sb[1] is sgd._flat_mom
