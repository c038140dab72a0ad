"""The generator's training loss on the device: parc_mdm_loss_forward / _backward through MDMMotionLoss, against fixture G33 and the
float64 restatement with the bounds of tests/test_mdm_loss.py (2 e-bar, plus the re-ordering bound for the summed terms), and against
the torch path on the same device tensors."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import mdm_loss_host as mh      # noqa: E402
import mdm_loss_ref as mlr      # noqa: E402
from test_mdm_loss import EBAR_GRAD_RECORDED, EBAR_LOSS_RECORDED, case_names, case_of, check_grad, check_losses      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = mh.T
SHIPPED = dict(grid=[10, 20, 15, 15], dx=0.2, S=16, num_prev_states=2)


@pytest.fixture(scope="module")
def km():
    from parc_amd.anim import kin_char_model as kcm
    m = kcm.KinCharModel(DEV)
    m.load_char_file(kcm.default_char_file())
    return m


@pytest.fixture(scope="module")
def km_cpu():
    from parc_amd.anim import kin_char_model as kcm
    m = kcm.KinCharModel("cpu")
    m.load_char_file(kcm.default_char_file())
    return m


@pytest.fixture(scope="module")
def g33():
    return mlr.load_fixture()


@pytest.fixture(scope="module")
def ref64(km_cpu, g33):
    z, meta = g33
    model = mlr.model_from_char(km_cpu)
    return {c["name"]: mlr.case_eval(model, c, z) for c in meta["cases"]}


def dev_inputs(km, c, z):
    n = c["name"]
    return (mh.true_data(km, c, DEV), torch.tensor(z[n + "_hfs"], device=DEV), torch.tensor(z[n + "_target_dir"], device=DEV))


def synthetic_batch(km_cpu, g33, B, seed):
    """B samples on the shipped grid: windows of the committed clips, prediction = standardised truth + noise, seeded terrain"""
    z, meta = g33
    rng = np.random.default_rng(seed)
    c = dict(case_of(meta, "shipped"))
    starts = {0: 40 - 16, 1: 25 - 16, 3: 20 - 16}
    clips = rng.choice([0, 1, 3], size=B)
    c["windows"] = [[int(k), int(rng.integers(0, starts[int(k)] + 1))] for k in clips]
    L = mh.make_loss(km_cpu, c, z)
    true = mh.true_data(km_cpu, c)
    g = rng.standard_normal((B, 16, 91))
    x = L.assemble_mdm_features(true) + torch.tensor(np.sign(g) * (0.03 + 0.08 * np.abs(g)), dtype=torch.float32)
    hfs = torch.tensor((0.45 + np.round(rng.uniform(-0.5, 0.5, size=(B, 1, 31, 31)), 1)) / 3.0, dtype=torch.float32)
    ang = rng.uniform(0, 2 * np.pi, size=B)
    td = torch.tensor(np.stack([np.cos(ang), np.sin(ang)], -1).reshape(B, 1, 2), dtype=torch.float32)
    return c, {k: v.to(DEV) for k, v in true.items()}, x.to(DEV), hfs.to(DEV), td.to(DEV)


def run(L, true, x, hfs, td, loss_fn, mask=None):
    xr = x.clone().requires_grad_(True)
    losses = L(true, xr, hfs, td, loss_fn)
    vals = {k.name: v.detach().clone() for k, v in losses.items()}
    L.reduce(losses, mask).backward()
    torch.cuda.synchronize()
    return vals, xr.grad


@pytest.mark.parametrize("name", case_names())
def test_device_matches_fixture_and_restatement(name, km, g33, ref64):
    z, meta = g33
    c, r = case_of(meta, name), ref64[name]
    L = mh.make_loss(km, c, z, DEV)
    assert L._path == "device", L._path_reason
    true, hfs, td = dev_inputs(km, c, z)
    x = torch.tensor(z[name + "_x"], device=DEV)
    for key, mask in (("grad", None), ("grad_ood", torch.tensor(z[name + "_ood_mask"], device=DEV))):
        vals, g = run(L, true, x, hfs, td, c["loss_fn"], mask)
        assert L.last_path == "device"
        if mask is None:
            check_losses({k: v.cpu().numpy() for k, v in vals.items()}, r, z, name, EBAR_LOSS_RECORDED, "device")
        assert torch.isfinite(g).all()
        check_grad(g.cpu().numpy(), r, z, name, key, EBAR_GRAD_RECORDED, "device")


@pytest.mark.parametrize("loss_fn", ["squared_l2", "pseudo_huber"])
def test_device_agrees_with_torch_path_at_64(loss_fn, km, km_cpu, g33):
    """B = 64, S = 16, 31 x 31: both paths on the same device tensors; each is an fp32 evaluation within e-bar of the truth, so they
    agree within 2 e-bar plus the re-ordering bound of the summed terms (taken from the terms' own fp32 magnitude: log2(n) 2^-24 |term|
    bounds it for sums of non-negative summands, n <= 16 * 43 points or 16 * 15 * 3 elements -> 10)"""
    c, true, x, hfs, td = synthetic_batch(km_cpu, g33, 64, 11)
    z, _ = g33
    Ld, Lt = mh.make_loss(km, c, z, DEV), mh.make_loss(km, c, z, DEV, path="torch")
    mask = torch.arange(64, device=DEV) % 5 == 0
    vd, gd = run(Ld, true, x, hfs, td, loss_fn, mask)
    vt, gt = run(Lt, true, x, hfs, td, loss_fn, mask)
    assert Ld.last_path == "device" and Lt.last_path == "torch" and list(vd) == list(vt)
    for k in vd:
        a, b = vd[k].double().cpu().numpy(), vt[k].double().cpu().numpy()
        tol = 2 * EBAR_LOSS_RECORDED * np.maximum(1.0, np.abs(b)) + 10 * 2.0 ** -24 * np.abs(b)
        print(k, np.abs(a - b).max(), tol.min())
        assert (np.abs(a - b) <= tol).all(), (k, np.abs(a - b).max())
    unit = gt.abs().reshape(64, -1).max(-1)[0].reshape(-1, 1, 1).clamp(min=1e-30)
    err = float(((gd - gt).abs() / unit).max())
    print("grad", err)
    assert err <= 2 * EBAR_GRAD_RECORDED, err


@pytest.mark.parametrize("B", [1, 67])
def test_batch_sizes_and_repeatability(B, km, km_cpu, g33):
    c, true, x, hfs, td = synthetic_batch(km_cpu, g33, B, 100 + B)
    z, _ = g33
    L = mh.make_loss(km, c, z, DEV)
    v1, g1 = run(L, true, x, hfs, td, "squared_l2")
    v2, g2 = run(L, true, x, hfs, td, "squared_l2")
    assert all(torch.equal(v1[k], v2[k]) for k in v1) and torch.equal(g1, g2)
    assert all(v.shape == (B,) and torch.isfinite(v).all() for v in v1.values()) and torch.isfinite(g1).all()
    # every sample of the batch equals the same sample evaluated alone (a workgroup reads its own sample only)
    b = B - 1
    one = {k: v[b:b + 1] for k, v in true.items()}
    v3, g3 = run(L, one, x[b:b + 1], hfs[b:b + 1], td[b:b + 1], "squared_l2")
    assert all(torch.equal(v1[k][b:b + 1], v3[k]) for k in v1)
    # the gradient is linear in the cotangent (1 / B in the batch, 1 alone) up to the rounding of the products it enters
    np.testing.assert_allclose(g3.cpu().numpy() / B, g1[b:b + 1].cpu().numpy(), rtol=0, atol=8 * 2.0 ** -24 * float(g3.abs().max()) / B)


def test_nan_stays_in_its_sample(km, km_cpu, g33):
    c, true, x, hfs, td = synthetic_batch(km_cpu, g33, 6, 5)
    z, _ = g33
    L = mh.make_loss(km, c, z, DEV)
    v1, g1 = run(L, true, x, hfs, td, "pseudo_huber")
    xd = x.clone()
    xd[2, 3, 1] = float("nan")
    xd[2, 7, 50] = float("inf")
    v2, g2 = run(L, true, xd, hfs, td, "pseudo_huber")
    keep = torch.tensor([0, 1, 3, 4, 5], device=DEV)
    assert all(torch.equal(v1[k][keep], v2[k][keep]) for k in v1) and torch.equal(g1[keep], g2[keep])
    assert not torch.isfinite(v2["SIMPLE_ROOT_POS_LOSS"][2]) and not torch.isfinite(v2["HF_COLLISION_LOSS"][2])


def test_ood_cotangent_zeroes_the_masked_terms(km, km_cpu, g33):
    """the trainer's `losses[k][mask] *= 0.0` on selections of the one [14, B] output: the cotangent that reaches the backward launch is
    0 exactly at (term, sample) pairs of mdm.py:936-940 and 1 / B elsewhere"""
    c, true, x, hfs, td = synthetic_batch(km_cpu, g33, 8, 9)
    z, _ = g33
    L = mh.make_loss(km, c, z, DEV)
    seen = {}
    mask = torch.tensor([True, False, False, True, False, False, False, True], device=DEV)
    xr = x.clone().requires_grad_(True)
    losses = L(true, xr, hfs, td, "squared_l2")
    out = next(iter(losses.values()))._base          # the one [14, B] function output every value is a selection of
    assert out.shape == (14, 8) and all(v._base is out for v in losses.values())
    out.register_hook(lambda g: seen.__setitem__("g", g.detach().clone()))
    L.reduce(losses, mask).backward()
    torch.cuda.synchronize()
    g = seen["g"].cpu()
    assert g.shape == (14, 8)
    for t, name in enumerate(mlr.TERM_ORDER):
        want = torch.full((8,), 1.0 / 8)
        if name not in mlr.UNMASKED:
            want[mask.cpu()] = 0.0
        assert torch.equal(g[t], want), name
        if name not in mlr.UNMASKED:
            assert (losses[L.LossType[name]][mask] == 0).all()
    # the masked samples' gradient comes from the terrain and target terms alone
    assert torch.isfinite(xr.grad).all() and (xr.grad[mask][..., L._feature_slices[T.CONTACTS]] == 0).all()


def test_adamw_step_through_the_device_loss(km, km_cpu, g33):
    """a tiny nn.Linear "denoiser" takes one AdamW step through the device loss and one through the torch path; the parameters whose
    gradient stands well above the propagated error land within what 2 e-bar of predicted_x_0.grad can move Adam's first step by"""
    c, true, x, hfs, td = synthetic_batch(km_cpu, g33, 8, 21)
    z, _ = g33
    lr = 1e-3
    out = []
    for path in (None, "torch"):
        torch.manual_seed(3)
        net = torch.nn.Linear(91, 91).to(DEV)
        with torch.no_grad():
            net.weight.copy_(torch.eye(91, device=DEV) + 0.01 * net.weight)
            net.bias.mul_(0.01)
        opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=0.01)
        L = mh.make_loss(km, c, z, DEV, path=path)
        losses = L(true, net(x), hfs, td, "squared_l2")
        L.reduce(losses).backward()
        grads = [p.grad.detach().clone() for p in net.parameters()]
        opt.step()
        torch.cuda.synchronize()
        out.append(([p.detach().clone() for p in net.parameters()], grads, L.last_path))
    assert out[0][2] == "device" and out[1][2] == "torch"
    # what 2 e-bar of x.grad (relative to each sample's max) can move a parameter's gradient by: W[i, j] sums x.grad[r, i] * in[r, j] over
    # the B * S rows r, the bias sums x.grad[r, i]
    xr = x.clone().requires_grad_(True)
    torch.manual_seed(3)
    net = torch.nn.Linear(91, 91).to(DEV)
    with torch.no_grad():
        net.weight.copy_(torch.eye(91, device=DEV) + 0.01 * net.weight)
        net.bias.mul_(0.01)
    y = net(xr).detach().requires_grad_(True)
    Lt = mh.make_loss(km, c, z, DEV, path="torch")
    Lt.reduce(Lt(true, y, hfs, td, "squared_l2")).backward()
    unit = y.grad.abs().reshape(8, -1).max(-1)[0].reshape(8, 1).expand(8, 16).reshape(-1)          # per row
    err_w = 2 * EBAR_GRAD_RECORDED * (unit.unsqueeze(-1) * x.reshape(-1, 91).abs()).sum(0).unsqueeze(0).expand(91, 91)
    err_b = (2 * EBAR_GRAD_RECORDED * unit.sum()).expand(91)
    n_tight = n_all = 0
    for pd, pt, gt_, err in zip(out[0][0], out[1][0], out[1][1], (err_w, err_b)):
        # Adam's first step is lr * g / (|g| + eps): a gradient off by err moves it by lr * err / (|g| - err).  Only parameters whose
        # gradient stands well above that error are a test of anything (for the rest any step, a sign flip included, is within what the
        # error allows): the assertion is made on those with err / (|g| - err) <= 0.01, a step pinned to 1 % of lr
        ratio = err / (gt_.abs() - err).clamp(min=1e-30)
        tight = (gt_.abs() > err) & (ratio <= 0.01)
        n_tight, n_all = n_tight + int(tight.sum()), n_all + tight.numel()
        bound = lr * ratio + 2.0 ** -22 * (1 + pt.abs())
        assert ((pd - pt).abs()[tight] <= bound[tight]).all(), float(((pd - pt).abs()[tight] / bound[tight]).max())
        assert ((pd - pt).abs() <= 2 * lr + 2.0 ** -22 * (1 + pt.abs())).all()          # no step can differ by more than a sign flip
    print("adamw: %d of %d parameters under the tight bound" % (n_tight, n_all))
    assert n_tight > 0
