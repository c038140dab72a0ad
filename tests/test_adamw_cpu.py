"""`optimizer.type: Adam` without a GPU: MPOptimizer keeps torch.optim.AdamW for CPU parameters (the flat AdamW step is a device path
only), and the float64 AdamW that tests/test_adamw_gpu.py measures the kernel against is torch's update rule."""
import os
import sys

import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import adamw_ref  # noqa: E402


def test_cpu_parameters_keep_the_torch_adamw():
    from parc_amd.learning import mp_optimizer
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(6, 9), torch.nn.ReLU(), torch.nn.Linear(9, 2))
    before = [p.data_ptr() for p in m.parameters()]
    opt = mp_optimizer.MPOptimizer({"type": "Adam", "learning_rate": 1e-3, "weight_decay": 0.01}, list(m.parameters()))
    assert opt._flat_adam is False and opt._flat_sgd is False
    assert isinstance(opt._optimizer, torch.optim.AdamW) and not hasattr(opt, "_flat_param")
    assert [p.data_ptr() for p in m.parameters()] == before          # the parameters stay where they were allocated
    group = opt._optimizer.param_groups[0]
    assert group["betas"] == (0.9, 0.999) and group["eps"] == 1e-8 and group["weight_decay"] == 0.01 and group["lr"] == 1e-3
    w0 = m[0].weight.detach().clone()
    opt.step(m(torch.randn(4, 6)).square().sum(), model=m, max_norm=0.5)
    assert not torch.equal(w0, m[0].weight) and opt.get_steps() == 1
    opt.reset_state()
    assert len(opt._optimizer.state) == 0


def test_float64_helper_is_torch_adamw():
    """AdamWRef (the six lines of the update rule, with the clip) against clip_grad_norm_ + torch.optim.AdamW in float64: 5 steps,
    parameters and both moments to 1e-12."""
    err = adamw_ref.check_against_torch(steps=5)
    print("max |AdamWRef - torch float64| =", err)
    assert err <= 1e-12
