"""Fixture G30 (tests/golden/gen_nonfinite.py: the reference's loss, advantage normalisation and normaliser on NaN / Inf) and the torch
statements of tests/tools/nonfinite_ref.py, checked without a GPU: the fixture holds what its case names promise, the torch
primitives the reference's non-finite behaviour rests on still behave as they did when the fixture was written, and the restated loss
reproduces the reference's terms and gradients, NaN for NaN."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from conftest import REPO, golden

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import nonfinite_ref as nf  # noqa: E402

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def z():
    return golden("g30_nonfinite")


def test_g30_loss_cases_hold_what_their_names_promise(z):
    names = [str(c) for c in z["ppo_case_names"]]
    assert names == ["finite", "nan_action_selected", "nan_action_unselected", "nan_mean_selected", "nan_mean_unselected", "inf_ratio_unselected",
                     "nan_tar_val"]
    rows, cols = z["ppo_rows"].tolist(), z["ppo_cols"].tolist()
    B, A = z["ppo_mean"].shape
    assert (B, A) == (70, 28) and rows == [3, 66] and rows[0] // 64 != rows[1] // 64 and cols[1] == A - 1
    for k in ("mean", "logstd", "pred", "norm_action", "adv", "tar_val", "a_logp"):
        assert np.isfinite(z["ppo_" + k]).all(), k
    assert (z["ppo_adv"][rows] < 0).all()
    others = np.delete(np.arange(B), rows)
    for name in names:
        c = nf.g30_ppo_case(z, name)
        mask, info = c["mask"], c["info"]
        assert set(np.unique(mask)) == {0.0, 1.0} and 0.2 < 1.0 - mask[others].mean() < 0.3          # about a quarter unselected
        assert (mask[rows] == (0.0 if name.endswith("_unselected") else 1.0)).all()
        poisoned = {"nan_action": "norm_action", "nan_mean": "mean", "inf_ratio": "a_logp", "nan_tar": "tar_val"}.get(name[:name.index("_", 4)] if name != "finite" else "")
        for k in ("mean", "norm_action", "a_logp", "tar_val"):
            bad = ~np.isfinite(c[k])
            if k != poisoned:
                assert not bad.any(), (name, k)
            elif k in ("mean", "norm_action"):
                assert np.argwhere(bad).tolist() == [[rows[0], cols[0]], [rows[1], cols[1]]] and np.isnan(c[k][bad]).all()
            else:
                assert np.argwhere(bad).flatten().tolist() == rows
                assert (c[k][rows] == -INF).all() if k == "a_logp" else np.isnan(c[k][rows]).all()
        gm, gl, gp = c["grad_mean"], c["grad_logstd"], c["grad_pred"]
        if name.endswith("_selected"):         # the reference's actor loss is NaN: its trap stops the run
            assert np.isnan(info["actor_loss"]) and np.isnan(info["loss"]) and np.isnan(info["imp_ratio"]) and np.isfinite(info["critic_loss"])
            assert np.isfinite(info["clip_frac"])           # |NaN - 1| > clip is false: the row counts as unclipped
            assert np.isnan(info["action_bound_loss"]) == (name == "nan_mean_selected")
            assert np.isnan(gm[rows]).all() and np.isfinite(gm[others]).all() and np.isnan(gl).all() and np.isfinite(gp).all()
        elif name.endswith("_unselected"):      # the row is never evaluated: finite loss, zero gradient
            assert all(np.isfinite(v) for v in info.values())
            assert (gm[rows] == 0.0).all() and np.isfinite(gm).all() and np.isfinite(gl).all() and np.isfinite(gp).all()
        elif name == "nan_tar_val":
            assert np.isnan(info["critic_loss"]) and np.isnan(info["loss"]) and np.isfinite(info["actor_loss"])
            assert np.isfinite(gm).all() and np.isfinite(gl).all() and np.argwhere(np.isnan(gp)).flatten().tolist() == rows
        else:
            assert all(np.isfinite(v) for v in info.values()) and np.isfinite(gm).all() and np.isfinite(gl).all() and np.isfinite(gp).all()
    # the three unselected cases are the same batch as far as the reference looks at it
    a = nf.g30_ppo_case(z, "nan_action_unselected")
    for name in ("nan_mean_unselected", "inf_ratio_unselected"):
        b = nf.g30_ppo_case(z, name)
        assert a["info"] == b["info"] and all(np.array_equal(a[k], b[k]) for k in ("grad_mean", "grad_logstd", "grad_pred"))


def test_g30_advantage_cases_hold_what_their_names_promise(z):
    names = [str(c) for c in z["adv_case_names"]]
    assert names == ["finite", "nan_selected", "nan_unselected", "inf_selected", "one_selected", "none_selected"]
    n = z["adv_vals"].size
    assert n == 300 and np.isfinite(z["adv_vals"]).all()
    for name in names:
        ret, mask, na = z["adv_%s_ret" % name], z["adv_%s_mask" % name], z["adv_%s_norm_adv" % name]
        mean, std = float(z["adv_%s_adv_mean" % name]), float(z["adv_%s_adv_std" % name])
        bad = np.argwhere(~np.isfinite(ret.reshape(-1))).flatten().tolist()
        if name in ("nan_selected", "nan_unselected", "inf_selected"):
            assert len(bad) == 1 and mask.reshape(-1)[bad[0]] == (0.0 if name == "nan_unselected" else 1.0)
            assert np.isinf(ret.reshape(-1)[bad[0]]) == (name == "inf_selected")
        else:
            assert not bad
        assert int(mask.sum()) == {"one_selected": 1, "none_selected": 0}.get(name, int(z["adv_finite_mask"].sum()))
        if name == "finite":
            assert np.isfinite(na).all() and np.isfinite(mean) and std > 0 and (na == float(z["adv_clip"])).any() and (na == -float(z["adv_clip"])).any()
        elif name == "nan_unselected":             # the NaN stays in its element
            assert np.argwhere(np.isnan(na.reshape(-1))).flatten().tolist() == bad == [n - 1]
            assert mean == float(z["adv_finite_adv_mean"]) and std == float(z["adv_finite_adv_std"])
        else:
            assert np.isnan(na).all() and np.isnan(std)
            assert np.isnan(mean) == (name != "one_selected")


def test_g30_normaliser_case_holds_what_it_promises(z):
    x, mean, std, want = z["nz_x"], z["nz_mean"], z["nz_std"], z["nz_normalized"]
    clip = float(z["nz_clip"])
    assert x.shape == (5, 8) and np.isnan(x[0, 0]) and x[1, 5] == INF and x[2, 7] == -INF and int((~np.isfinite(x)).sum()) == 3
    assert np.argwhere(np.isnan(mean)).flatten().tolist() == [3] and std[6] == 0.0 and (np.delete(std, 6) > 0).all()
    on_mean = x[:, 6] == mean[6]
    assert on_mean.tolist() == [False, False, False, False, True]
    nan_want = np.zeros((5, 8), bool)
    nan_want[0, 0] = nan_want[:, 3] = nan_want[4, 6] = True
    assert np.array_equal(np.isnan(want), nan_want)
    assert want[1, 5] == clip and want[2, 7] == -clip and (np.abs(want[:4, 6]) == clip).all() and not np.isinf(want).any()
    inner = np.abs(want) < clip
    assert inner.sum() >= 10 and (np.abs(want) == clip).sum() >= 8           # both sides of the clamp are used
    got = torch.clamp((torch.tensor(x) - torch.tensor(mean)) / torch.tensor(std), -clip, clip)
    nf.assert_same(got, want, what="Normalizer.normalize restated")


def test_torch_primitives_treat_nan_as_the_fixture_assumes():
    v = torch.tensor([NAN, -7.0, 0.5, 7.0, INF, -INF])
    assert torch.isnan(torch.clamp(v, -4.0, 4.0)[0]) and torch.clamp(v, -4.0, 4.0)[1:].tolist() == [-4.0, 0.5, 4.0, 4.0, -4.0]
    assert torch.isnan(torch.clamp_min(v, 1e-5)[0]) and torch.isnan(torch.clamp_max(v, 0.0)[0])
    assert torch.isnan(torch.minimum(torch.tensor([NAN, 1.0]), torch.tensor([1.0, NAN]))).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s0, m0 = torch.std_mean(torch.zeros(0))
        s1, m1 = torch.std_mean(torch.tensor([2.5]))
    assert torch.isnan(s0) and torch.isnan(m0) and torch.isnan(s1) and m1.item() == 2.5
    s, m = torch.std_mean(torch.tensor([1.0, INF, 2.0]))    # a running mean: the element after the infinite one adds inf - inf
    assert torch.isnan(s) and torch.isnan(m)
    p = torch.nn.Parameter(torch.zeros(7))
    p.grad = torch.arange(7.0)
    p.grad[6] = NAN
    norm = torch.nn.utils.clip_grad_norm_([p], 1.0)
    assert torch.isnan(norm) and torch.isnan(p.grad).all()
    p.grad = torch.arange(7.0)
    p.grad[1] = INF
    norm = torch.nn.utils.clip_grad_norm_([p], 1.0)         # coef = 1 / inf = 0: the infinite element becomes 0 x inf, the others 0
    assert norm.item() == INF and torch.isnan(p.grad).tolist() == [False, True] + [False] * 5 and float(p.grad[2:].abs().max()) == 0.0
    g, db = nf.relu_bwd_bias(torch.ones(3, 4), torch.tensor([[1.0, 0.0, -1.0, NAN]] * 3))
    assert g[0].tolist() == [1.0, 0.0, 0.0, 1.0] and db.tolist() == [3.0, 0.0, 0.0, 3.0]        # y <= 0 ? 0 : g passes g at a NaN activation


@pytest.mark.parametrize("poison,where", [(NAN, 1), (NAN, 6), (INF, 1)])
def test_clipped_optimizer_statements(poison, where):
    gen = torch.Generator().manual_seed(7)
    p0, g0, g1 = torch.randn(7, generator=gen), torch.randn(7, generator=gen), torch.randn(7, generator=gen)
    g1[where] = poison
    others = [i for i in range(7) if i != where]
    for max_norm in (1.0, -1.0):
        (p_a, m_a, _, n_a), (p, m, g, n) = nf.sgd_steps(p0, [g0, g1], max_norm, 5e-3)
        (q_a, e_a, v_a, _, _), (q, e, v, h, n2) = nf.adamw_steps(p0, [g0, g1], max_norm, 1e-3, (0.9, 0.999), 1e-8, 0.01)
        assert all(torch.isfinite(t).all() for t in (p_a, m_a, q_a, e_a, v_a))
        if max_norm > 0 and poison != poison:
            assert torch.isnan(n) and torch.isnan(n2)
            assert all(torch.isnan(t).all() for t in (p, m, g, q, e, v, h))
        else:
            for t in (p, m, q, e, v):
                assert not torch.isfinite(t[where]) and torch.isfinite(t[others]).all()
            assert max_norm < 0 or (n.item() == INF and float(g[others].abs().max()) == 0.0 and torch.isnan(g[where]))


@pytest.mark.parametrize("case", ["finite", "nan_action_selected", "nan_action_unselected", "nan_mean_selected", "nan_mean_unselected",
                                  "inf_ratio_unselected", "nan_tar_val"])
def test_restated_loss_reproduces_the_reference_on_g30(z, case):
    """nonfinite_ref.ppo_loss - the expectation of the GPU tests at action widths the fixture does not hold - against the reference's
    own terms and autograd gradients: G14's tolerances on finite entries, NaN where the reference has NaN."""
    c = nf.g30_ppo_case(z, case)
    clip, bw, _, _, cw, gate, _ = [float(v) for v in z["ppo_params"]]
    info, grads = nf.ppo_loss(c["mean"], c["logstd"], c["pred"], c["norm_action"], c["a_logp"], c["adv"], c["mask"], c["tar_val"], clip, bw, cw, gate)
    for k, r in c["info"].items():
        nf.assert_same(np.float64(info[k]), np.float64(r), atol=2e-5 * max(1.0, abs(r)) if np.isfinite(r) else 0.0, what=case + " " + k)
    assert info["cnt"] == float(c["mask"].sum())
    for g, name in zip(grads, ("grad_mean", "grad_logstd", "grad_pred")):
        fin = c[name][np.isfinite(c[name])]
        nf.assert_same(g, c[name], atol=3e-5 * max(float(np.abs(fin).max()) if fin.size else 0.0, 1e-6) + 1e-9, what=case + " " + name)
