"""NaN and Inf through the learner kernels: they must surface where the reference's torch code surfaces them, and nowhere else.

The reference stops a run when a loss becomes NaN (learning/ppo_agent.py:242-252; here DMPPOAgent._nan_trap).  A kernel that swallows a
NaN (C fminf / fmaxf return the operand that is not NaN) lets a run go on that the reference ends; a kernel that makes one out of a
row the reference never evaluates (0 x NaN from a mask product) ends a run that the reference continues.  Expectations: fixture G30
(tests/golden/gen_nonfinite.py, the reference's own loss, advantage normalisation and normaliser) and the torch statements of
tests/tools/nonfinite_ref.py (pinned by tests/test_nonfinite_ref_cpu.py).

The comparison rule, everywhere (nonfinite_ref.assert_same): NaN at the same positions, +-Inf at the same positions with the same
sign, finite entries within the tolerance the existing test of that kernel uses (named at each call)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import nonfinite_ref as nf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
EINVAL = -1
PPO_CASES = ["finite", "nan_action_selected", "nan_action_unselected", "nan_mean_selected", "nan_mean_unselected", "inf_ratio_unselected",
             "nan_tar_val"]
ADV_CASES = ["finite", "nan_selected", "nan_unselected", "inf_selected", "one_selected", "none_selected"]


def T(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def z():
    return golden("g30_nonfinite")


# ------------------------------------------------------------------------------------------------ normalisation: bit-identical
def test_normalize_clamp_in_place_and_out_of_place(z):
    """parc_normalize_clamp on the G30 block: NaN observation, +-inf observation, NaN mean, 0 / 0 and x / 0 under a zero std."""
    from parc_amd import _hip
    x, mean, std, clip = T(z["nz_x"]), T(z["nz_mean"]), T(z["nz_std"]), float(z["nz_clip"])
    rows, dim = x.shape
    out = torch.full_like(x, 77.0)
    p = _hip.ptr
    _hip.check(_hip.lib().parc_normalize_clamp(_hip.stream(), rows, dim, p(x), p(mean), p(std), clip, p(out)), "parc_normalize_clamp")
    nf.assert_same(out, z["nz_normalized"], what="out of place")
    nf.assert_same(x, z["nz_x"], what="the input of the out-of-place call")
    _hip.check(_hip.lib().parc_normalize_clamp(_hip.stream(), rows, dim, p(x), p(mean), p(std), clip, p(x)), "parc_normalize_clamp")
    nf.assert_same(x, z["nz_normalized"], what="in place")


def _padded_block(z):
    """65 rows: 60 finite filler rows, then the G30 rows in reverse order, so that the row with the NaN is row 64 - alone in the second
    64-row chunk of parc_obs_ingest."""
    x5 = torch.tensor(z["nz_x"])
    x = torch.randn(65, 8, generator=torch.Generator().manual_seed(33)) * 4.0
    x[60:65] = x5.flip(0)
    mean, std, clip = torch.tensor(z["nz_mean"]), torch.tensor(z["nz_std"]), float(z["nz_clip"])
    want = torch.clamp((x - mean) / std, -clip, clip)              # Normalizer.normalize, learning/normalizer.py:83-86
    nf.assert_same(want[60:65].flip(0), z["nz_normalized"], what="the G30 rows of the padded block")
    assert torch.isnan(x[64, 0]) and int((~torch.isfinite(x)).sum()) == 3
    return x, mean, std, clip, want


@pytest.mark.parametrize("optional", [False, True])
def test_obs_ingest_padded_to_65_rows(z, optional):
    """parc_obs_ingest with and without its raw copy and its moment sums.  The copy is the input, bit for bit (NaN payload aside); the
    sums are non-finite in exactly the poisoned columns - NaN under the NaN, +-inf / +inf under the infinities, as torch's column sums -
    and every other column is bit-equal to the run with the poison replaced by 0."""
    from parc_amd import _hip
    x_c, mean, std, clip, want = _padded_block(z)
    L, p = _hip.lib(), _hip.ptr
    x, mean, std = x_c.to(DEV), mean.to(DEV), std.to(DEV)
    if not optional:
        out = torch.full_like(x, 77.0)
        _hip.check(L.parc_obs_ingest(_hip.stream(), 65, 8, p(x), p(mean), p(std), clip, p(out), None, None, None, None), "parc_obs_ingest")
        nf.assert_same(out, want, what="norm_out")
        return
    ws = torch.empty(int(L.parc_moments_workspace_floats(65, 8)), device=DEV)
    row = torch.tensor([1], dtype=torch.int64, device=DEV)
    results = []
    for poisoned in (True, False):
        xi = x if poisoned else torch.where(torch.isfinite(x), x, torch.zeros_like(x))
        out, buf, acc = torch.full_like(x, 77.0), torch.full((2, 65, 8), -1.0, device=DEV), torch.zeros(2, 8, device=DEV)
        _hip.check(L.parc_obs_ingest(_hip.stream(), 65, 8, p(xi), p(mean), p(std), clip, p(out), p(buf), p(row), p(acc), p(ws)), "parc_obs_ingest")
        results.append((out.cpu(), buf.cpu(), acc.cpu()))
    (out, buf, acc), (out0, _, acc0) = results
    nf.assert_same(out, want, what="norm_out")
    nf.assert_same(buf[1], x_c, what="raw copy")
    assert (buf[0] == -1.0).all()
    nf.assert_same(acc, torch.stack([x_c.sum(0), (x_c * x_c).sum(0)]), atol=np.inf, what="moment sums (positions)")
    bad_cols = [0, 5, 7]
    assert np.argwhere(~np.isfinite(acc.numpy()).all(axis=0)).flatten().tolist() == bad_cols and torch.isnan(acc[:, 0]).all()
    keep = [c for c in range(8) if c not in bad_cols]
    assert torch.equal(acc[:, keep], acc0[:, keep]) and torch.isfinite(acc0).all()
    clean_rows = torch.isfinite(x_c).all(dim=1)
    nf.assert_same(out[clean_rows], out0[clean_rows], what="norm_out of the rows without poison")


def test_normalizer_kernel_path_equals_its_fallback_path(z):
    """Normalizer.normalize: the kernel path and the torch.clamp path (a tensor the kernel cannot take: an unaligned view) on non-finite data."""
    from parc_amd.learning.normalizer import Normalizer
    nz = Normalizer((8,), DEV, clip=float(z["nz_clip"]))
    nz._mean[:] = T(z["nz_mean"])
    nz._std[:] = T(z["nz_std"])
    x = T(z["nz_x"])
    pad = torch.zeros(x.numel() + 1, device=DEV)
    pad[1:] = x.flatten()
    assert x.data_ptr() % 16 == 0 and pad[1:].data_ptr() % 16 != 0
    a, b = nz.normalize(x), nz.normalize(pad[1:].view_as(x))
    nf.assert_same(a, b, what="kernel path against fallback path")
    nf.assert_same(a, z["nz_normalized"], what="kernel path")
    nf.assert_same(b, z["nz_normalized"], what="fallback path")


# ------------------------------------------------------------------------------------------------ advantage normalisation
@pytest.mark.parametrize("case", ADV_CASES)
def test_adv_normalize_against_reference(z, case):
    """parc_adv_normalize (mean_std_out included) on the G30 cases of DMPPOAgent._build_train_data (learning/dm_ppo_agent.py:393-400).
    Finite entries: 1e-4, the tolerance of test_g9_td_lambda_and_advantage."""
    from parc_amd.learning import rl_util
    ret, vals, mask = T(z["adv_%s_ret" % case]), T(z["adv_vals"]), T(z["adv_%s_mask" % case])
    adv, ms = rl_util.normalize_advantage(ret, vals, mask, float(z["adv_clip"]))
    torch.cuda.synchronize()
    print(case, "mean / std", ms.tolist(), "reference", float(z["adv_%s_adv_mean" % case]), float(z["adv_%s_adv_std" % case]))
    nf.assert_same(ms, np.array([z["adv_%s_adv_mean" % case], z["adv_%s_adv_std" % case]]), atol=1e-4, what="mean_std_out")
    nf.assert_same(adv, z["adv_%s_norm_adv" % case], atol=1e-4, what="norm_adv")


# ------------------------------------------------------------------------------------------------ fused loss
def _widen(c, A):
    """The G30 batch with A - 28 extra finite action columns (A = 33: the one-thread-per-sample kernel); the stored log-probability moves
    by the extra columns' share, so the ratios stay where they were."""
    extra = A - 28
    if extra == 0:
        return c
    g = torch.Generator().manual_seed(34)
    B = c["mean"].shape[0]
    mean_x, logstd_x = torch.randn(B, extra, generator=g) * 0.7, torch.randn(extra, generator=g) * 0.2 - 1.5
    noise = torch.randn(B, extra, generator=g)
    logp_x = -0.5 * (noise * noise).sum(-1) + (-0.5 * extra * nf.LOG_2PI - logstd_x.sum())
    d = dict(c)
    d["mean"] = np.concatenate([c["mean"], mean_x.numpy()], axis=1)
    d["norm_action"] = np.concatenate([c["norm_action"], (mean_x + torch.exp(logstd_x) * noise).numpy()], axis=1)
    d["logstd"] = np.concatenate([c["logstd"], logstd_x.numpy()])
    d["a_logp"] = c["a_logp"] + logp_x.numpy()
    return d


def _run_loss(c, params, packed):
    from parc_amd.learning import rl_util
    clip, bw, ew, rw, cw, gate, l1 = params
    cfg = rl_util.ppo_cfg(clip, bw, ew, rw, cw, gate, bool(l1))
    mean, logstd, pred = T(c["mean"]), T(c["logstd"]), T(c["pred"])
    B, A = mean.shape
    if packed:
        W = 32 if A <= 28 else 40
        rec = torch.full((B, W), 123.0, device=DEV)
        rec[:, 0:A], rec[:, A], rec[:, A + 1], rec[:, A + 2], rec[:, A + 3] = T(c["norm_action"]), T(c["a_logp"]), T(c["adv"]), T(c["mask"]), T(c["tar_val"])
        res = rl_util.ppo_loss_and_grads_packed(mean, logstd, pred, rec, cfg)
    else:
        res = rl_util.ppo_loss_and_grads(mean, logstd, pred, T(c["norm_action"]), T(c["a_logp"]), T(c["adv"]), T(c["mask"]), T(c["tar_val"]), cfg)
    torch.cuda.synchronize()
    return [t.cpu() for t in res]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("A", [28, 33])
@pytest.mark.parametrize("case", PPO_CASES)
def test_ppo_loss_against_reference(z, case, A, packed):
    """parc_ppo_loss / parc_ppo_loss_packed: out[0..5], out[8] and the three gradients.  A = 28 (32 lanes per sample; rows 3 and 66 sit in
    different 64-sample blocks) against the reference's own terms and autograd gradients; A = 33 (one thread per sample) against
    nonfinite_ref.ppo_loss, which test_nonfinite_ref_cpu.py holds against the same fixture.  Tolerances of
    test_g14_fused_ppo_loss_against_reference: 2e-5 max(1, |r|) for the terms, 3e-5 scale for the gradients.

    The reference's gradient of a poisoned SELECTED row is NaN in every element of the row, and its whole log-std gradient is NaN -
    which is also the mathematics (d loss / d logp of that row is NaN) - so the rule is applied to them as to everything else.
    Unselected rows are exactly 0 in g_mean.  Every row without poison is bit-identical to the same launch with the poison taken out
    (same mask, hence the same selected count and gate)."""
    params = [float(v) for v in z["ppo_params"]]
    c = _widen(nf.g30_ppo_case(z, case), A)
    if A == 28:
        ref_info, ref_grads = dict(c["info"], cnt=float(c["mask"].sum())), (c["grad_mean"], c["grad_logstd"], c["grad_pred"])
    else:
        ref_info, ref_grads = nf.ppo_loss(c["mean"], c["logstd"], c["pred"], c["norm_action"], c["a_logp"], c["adv"], c["mask"], c["tar_val"],
                                          params[0], params[1], params[4], params[5])
        ref_grads = [g.numpy() for g in ref_grads]
    out, g_mean, g_logstd, g_pred = _run_loss(c, params, packed)
    slots = {"loss": 0, "critic_loss": 1, "actor_loss": 2, "clip_frac": 3, "imp_ratio": 4, "action_bound_loss": 5, "cnt": 8}
    print(case, A, "packed" if packed else "separate", {k: (out[i].item(), float(ref_info[k])) for k, i in slots.items()})
    for k, i in slots.items():
        r = float(ref_info[k])
        nf.assert_same(out[i], np.float64(r), atol=(0.0 if k == "cnt" else 2e-5 * max(1.0, abs(r))) if np.isfinite(r) else 0.0, what=k)
    for got, ref, name in zip((g_mean, g_logstd, g_pred), ref_grads, ("g_mean", "g_logstd", "g_pred")):
        fin = ref[np.isfinite(ref)]
        scale = max(float(np.abs(fin).max()) if fin.size else 0.0, 1e-6)
        nf.assert_same(got, ref, atol=3e-5 * scale + 1e-9, what=name)
    unselected = torch.tensor(c["mask"]) != 1.0
    assert (g_mean[unselected] == 0.0).all(), "an unselected row has a gradient"
    # the same launch without the poison
    rows = z["ppo_rows"].tolist()
    clean = _widen(dict(nf.g30_ppo_case(z, "finite"), mask=c["mask"]), A)
    out0, g_mean0, g_logstd0, g_pred0 = _run_loss(clean, params, packed)
    others = [i for i in range(g_mean.shape[0]) if i not in rows]
    assert torch.isfinite(out0[:9]).all() and out0[8] == out[8] and out0[9] == out[9], "selected count and gate are the same"
    assert torch.equal(g_mean[others], g_mean0[others]) and torch.equal(g_pred[others], g_pred0[others])
    if case.endswith("_unselected") or case == "finite":
        assert torch.equal(out[:9], out0[:9]) and torch.equal(g_logstd, g_logstd0) and torch.equal(g_pred, g_pred0)


# ------------------------------------------------------------------------------------------------ clip + optimizer step
OPT_CASES = [(NAN, 1), (NAN, 6), (INF, 1)]          # n = 7: one float4 and a tail of 3; index 1 is in the float4, index 6 in the tail


def _opt_inputs(poison, where):
    gen = torch.Generator().manual_seed(7)
    p0, g0, g1 = torch.randn(7, generator=gen), torch.randn(7, generator=gen), torch.randn(7, generator=gen)
    g1[where] = poison
    return p0, g0, g1


@pytest.mark.parametrize("max_norm", [1.0, -1.0])
@pytest.mark.parametrize("poison,where", OPT_CASES)
def test_sgd_momentum_step_with_a_nonfinite_gradient(poison, where, max_norm):
    """parc_sgd_momentum_step against clip_grad_norm_ + torch.optim.SGD(momentum=0.9): a healthy step, then one whose gradient holds a NaN or
    +inf.  rtol 1e-5, atol 1e-7 (test_flat_sgd_step_equals_torch_sgd_with_clipping).  The kernel leaves grad as it was (parc_hip.h)."""
    from parc_amd import _hip
    p0, g0, g1 = _opt_inputs(poison, where)
    ref = nf.sgd_steps(p0, [g0, g1], max_norm, 5e-3)
    L, ptr = _hip.lib(), _hip.ptr
    p, m, g = p0.to(DEV), torch.zeros(7, device=DEV), torch.empty(7, device=DEV)
    ws, norm = torch.empty(int(L.parc_sgd_workspace_floats()), device=DEV), torch.full((1,), -1.0, device=DEV)
    for step, gi in enumerate((g0, g1)):
        g.copy_(gi)
        _hip.check(L.parc_sgd_momentum_step(_hip.stream(), 7, ptr(p), ptr(g), ptr(m), max_norm, 5e-3, 0.9, 0.0, ptr(ws), ptr(norm)), "parc_sgd_momentum_step")
        torch.cuda.synchronize()
        p_ref, m_ref, _, n_ref = ref[step]
        print(step, "params", p.tolist(), "reference", p_ref.tolist(), "norm", norm.item(), n_ref)
        nf.assert_same(p, p_ref, rtol=1e-5, atol=1e-7, what="params, step %d" % step)
        nf.assert_same(m, m_ref, rtol=1e-5, atol=1e-7, what="momentum, step %d" % step)
        nf.assert_same(g, gi, what="grad, step %d" % step)
        if max_norm > 0:
            nf.assert_same(norm, n_ref.reshape(1), rtol=1e-5, what="norm_out, step %d" % step)
        else:
            assert norm.item() == -1.0
    others = [i for i in range(7) if i != where]
    if max_norm > 0 and poison != poison:
        assert torch.isnan(norm).all() and torch.isnan(p).all() and torch.isnan(m).all()
    else:
        assert torch.isfinite(p[others]).all() and torch.isfinite(m[others]).all() and not torch.isfinite(p[where]) and not torch.isfinite(m[where])


@pytest.mark.parametrize("max_norm", [1.0, -1.0])
@pytest.mark.parametrize("poison,where", OPT_CASES)
def test_adamw_step_with_a_nonfinite_gradient(poison, where, max_norm):
    """parc_adamw_step against clip_grad_norm_ + torch.optim.AdamW(foreach=False), the same two steps.  Finite entries: the rule of
    tests/test_adamw_gpu.py - the kernel's distance from float64 AdamW is at most 4 x that of torch's own fp32 AdamW."""
    from parc_amd import _hip
    lr, betas, eps, wd = 1e-3, (0.9, 0.999), 1e-8, 0.01
    p0, g0, g1 = _opt_inputs(poison, where)
    ref32 = nf.adamw_steps(p0, [g0, g1], max_norm, lr, betas, eps, wd)
    ref64 = nf.adamw_steps(p0, [g0, g1], max_norm, lr, betas, eps, wd, dtype=torch.float64)
    L, ptr = _hip.lib(), _hip.ptr
    p, m, v, g = p0.to(DEV), torch.zeros(7, device=DEV), torch.zeros(7, device=DEV), torch.empty(7, device=DEV)
    ws, norm = torch.empty(int(L.parc_sgd_workspace_floats()), device=DEV), torch.full((1,), -1.0, device=DEV)
    for step, gi in enumerate((g0, g1)):
        g.copy_(gi)
        _hip.check(L.parc_adamw_step(_hip.stream(), 7, ptr(p), ptr(g), ptr(m), ptr(v), step + 1, max_norm, lr, betas[0], betas[1], eps, wd, ptr(ws),
                                     ptr(norm)), "parc_adamw_step")
        torch.cuda.synchronize()
        for got, r32, r64, name in zip((p, m, v), ref32[step][:3], ref64[step][:3], ("params", "exp_avg", "exp_avg_sq")):
            print(step, name, got.tolist(), "reference", r32.tolist())
            nf.assert_same(got, r32, atol=np.inf, what="%s, step %d (positions)" % (name, step))
            fin = torch.isfinite(r32)
            e_ref = float((r32.double() - r64)[fin].abs().max()) if fin.any() else 0.0
            e_ker = float((got.cpu().double() - r64)[fin].abs().max()) if fin.any() else 0.0
            assert e_ker <= 4.0 * e_ref, (name, step, e_ker, e_ref)
        nf.assert_same(g, gi, what="grad, step %d" % step)
        if max_norm > 0:
            nf.assert_same(norm, ref32[step][4].reshape(1), rtol=1e-5, what="norm_out, step %d" % step)
    others = [i for i in range(7) if i != where]
    if max_norm > 0 and poison != poison:
        assert torch.isnan(norm).all() and torch.isnan(p).all() and torch.isnan(m).all() and torch.isnan(v).all()
    else:
        for t in (p, m, v):
            assert torch.isfinite(t[others]).all() and not torch.isfinite(t[where])


@pytest.mark.parametrize("poison,where", OPT_CASES)
def test_scale_by_clipped_norm_with_a_nonfinite_norm(poison, where):
    """parc_scale_by_clipped_norm: the gradient as clip_grad_norm_ leaves it, given the norm torch computed.  A max_norm <= 0 is refused."""
    from parc_amd import _hip
    _, _, g1 = _opt_inputs(poison, where)
    par = torch.nn.Parameter(torch.zeros(7))
    par.grad = g1.clone()
    n_ref = torch.nn.utils.clip_grad_norm_([par], 1.0)
    x, norm = g1.to(DEV), n_ref.reshape(1).to(DEV)
    L = _hip.lib()
    _hip.check(L.parc_scale_by_clipped_norm(_hip.stream(), 7, _hip.ptr(x), _hip.ptr(norm), 1.0), "parc_scale_by_clipped_norm")
    torch.cuda.synchronize()
    print("scaled", x.tolist(), "reference", par.grad.tolist())
    nf.assert_same(x, par.grad, rtol=1e-5, atol=1e-7, what="clipped gradient")
    assert torch.isnan(x).all() if poison != poison else (torch.isnan(x[where]) and float(x.nan_to_num(0.0).abs().max()) == 0.0)
    assert L.parc_scale_by_clipped_norm(_hip.stream(), 7, _hip.ptr(x), _hip.ptr(norm), -1.0) == EINVAL


# ------------------------------------------------------------------------------------------------ ReLU backward
def test_relu_bwd_bias_grad_with_a_nan_activation():
    """parc_relu_bwd_bias_grad, rows = 3, dim = 4: aten.threshold_backward is y <= 0 ? 0 : g, which passes g at a NaN activation."""
    from parc_amd import _hip
    g = torch.Generator().manual_seed(3)
    gy = torch.randn(3, 4, generator=g)
    y = torch.tensor([[0.5, 0.0, 1.5, 2.0], [0.0, 0.7, NAN, 0.0], [1.0, 0.0, 0.3, 0.0]])
    g_ref, db_ref = nf.relu_bwd_bias(gy, y)
    assert g_ref[1, 2] == gy[1, 2] and (g_ref == 0).sum() == 5
    L = _hip.lib()
    gy_d, y_d, db = gy.to(DEV), y.to(DEV), torch.full((4,), 3.0, device=DEV)
    ws = torch.empty(int(L.parc_relu_bwd_workspace_floats(3, 4)), device=DEV)
    _hip.check(L.parc_relu_bwd_bias_grad(_hip.stream(), 3, 4, _hip.ptr(gy_d), _hip.ptr(y_d), _hip.ptr(db), _hip.ptr(ws)), "parc_relu_bwd_bias_grad")
    torch.cuda.synchronize()
    print("gy", gy_d.tolist(), "reference", g_ref.tolist())
    nf.assert_same(gy_d, g_ref, what="masked gradient")
    nf.assert_same(db, db_ref, atol=1e-5 * max(1.0, float(db_ref.abs().max())) * 3 ** 0.5, what="bias gradient")      # as test_relu_bwd_bias_grad_kernel


# ------------------------------------------------------------------------------------------------ the agent
@pytest.mark.parametrize("poisoned", ["selected", "unselected"])
@pytest.mark.parametrize("explicit", [True, False])
def test_nan_trap_fires_for_selected_rows_only(explicit, poisoned, tmp_path, monkeypatch):
    """The 64-env agent of test_nan_trap_stops_at_the_epoch_and_dumps_the_offending_minibatch, half of its rows unselected.  A NaN in the
    stored action of every SELECTED row: the reference's actor loss is NaN in the first minibatch and the run stops there.  The same
    NaN in every UNSELECTED row: the reference never looks at those rows, the iteration runs to its end."""
    from parc_amd import workloads
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(0)
    env, _, _ = workloads.build_env("flat_1clip", 64, DEV, seed=0)
    agent = workloads.build_agent(env, DEV, steps_per_iter=4, update_epochs=3, batch_size=2, explicit_backward=explicit)
    agent._curr_obs, agent._curr_info = env.reset()
    agent._init_train()
    orig = agent._build_train_data

    def poison():
        info = orig()
        eb = agent._exp_buffer
        mask = eb.get_data("rand_action_mask")
        mask[:, ::2] = 0.0                                     # every other env took no random action
        hit = (mask == 1.0) if poisoned == "selected" else (mask != 1.0)
        eb.get_data("action")[..., 0][hit] = NAN
        if eb.has_buffer("loss_rec"):                          # the packed copy the update reads: [norm action 28 | a_logp | adv | MASK | tar_val]
            rec = eb.get_data("loss_rec")
            rec[..., 30] = mask
            rec[..., 0][hit] = NAN
        assert 0 < int(hit.sum()) < hit.numel()
        return info
    agent._build_train_data = poison
    params = lambda: torch.cat([q.detach().reshape(-1) for q in agent._model.parameters()])      # noqa: E731
    if poisoned == "selected":
        with pytest.raises(FloatingPointError, match="minibatch 0 of update epoch 0"):
            agent._train_iter()
        return
    before = params().clone()
    info = agent._train_iter()
    after = params()
    print({k: float(v) for k, v in info.items() if k in ("loss", "critic_loss", "actor_loss")})
    assert torch.isfinite(after).all() and not torch.equal(before, after)
    assert all(np.isfinite(float(info[k])) for k in ("loss", "critic_loss", "actor_loss"))
