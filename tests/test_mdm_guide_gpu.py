"""The generator's guidance step on the device: parc_mdm_guide_step through parc_amd.diffusion.mdm_guidance.MDMGuidance, against fixture
G35, the float64 restatement and the torch path on the same device tensors.  Bounds as in tests/test_mdm_guide.py: 2 e-bar (+ the
re-ordering bound of the restatement for the terms)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import mdm_guide_host as gh     # noqa: E402
import mdm_guide_ref as mgr     # noqa: E402
import mdm_loss_ref as mlr      # noqa: E402
import test_mdm_guide as tg     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
bits = lambda t: t.detach().cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def km():
    from parc_amd.anim import kin_char_model as kcm
    m = kcm.KinCharModel(DEV)
    m.load_char_file(kcm.default_char_file())
    return m


@pytest.fixture(scope="module")
def g35():
    return mgr.load_fixture()


@pytest.fixture(scope="module")
def ref64(g35):
    z, meta = g35
    model = mgr.default_model()
    return {c["name"]: mgr.case_eval(model, c, z) for c in meta["cases"]}


@pytest.fixture(scope="module")
def ebar(ref64):
    e = mgr.measure_ebar(evals=ref64)
    assert all(abs(a - b) <= 1e-9 for a, b in zip(e, (tg.EBAR_TERMS_RECORDED, tg.EBAR_XOUT_RECORDED, tg.EBAR_STEP_RECORDED))), e
    return e


def raw_step(G, x, gp, conds, x_out):
    """parc_mdm_guide_step out of place, with the arguments apply_guidance builds"""
    from parc_amd import _hip, _hip_mdm_guide as H
    reason, (c, target, hfs, points, start) = G._device_call(x, gp, conds, G._enabled(gp, conds))
    assert reason is None
    B, S, _ = x.shape
    F = G._features
    gx, gy = G._grid_points() if hfs is not None else (None, None)
    terms = torch.empty((H.TERMS, B), dtype=torch.float32, device=x.device)
    p = _hip.ptr
    _hip.check(_hip.lib().parc_mdm_guide_step(_hip.stream(), G._char_model.c_struct(), c, int(B), p(x), p(F._mdm_features_mean[:S].contiguous()),
                                              p(F._mdm_features_std[:S].contiguous()), p(hfs), p(target), p(gx), p(gy), p(points), p(start),
                                              p(x_out), p(terms)), "parc_mdm_guide_step")
    return terms


@pytest.mark.parametrize("name", tg.CASES)
def test_device_path_matches_fixture_and_restatement(name, km, g35, ref64, ebar):
    z, meta = g35
    case = tg.case_of(meta, name)
    G = gh.make_guide(km, case, z, device=DEV)
    assert G._path == "device"
    conds, gp = gh.guidance_inputs(case, z, device=DEV)
    x0 = torch.tensor(z[name + "_x"], device=DEV)
    x = x0.clone()
    terms = G.guidance_step(x, gp, conds)          # in place, as apply_guidance calls it
    assert G.last_path == "device"
    tg.check_result(terms.cpu().numpy(), x.cpu().numpy(), x0.cpu().numpy(), ref64[name], z, name, ebar, "device")
    x_out = torch.full_like(x0, float("nan"))
    terms2 = raw_step(G, x0, gp, conds, x_out)
    assert np.array_equal(bits(x_out), bits(x)) and np.array_equal(bits(terms2), bits(terms))
    cols = tg.unread_columns(G)
    assert np.array_equal(bits(x)[..., cols], bits(x0)[..., cols])


def test_device_against_torch_path_at_batch_64(km, g35, ref64, ebar):
    z, meta = g35
    case = tg.case_of(meta, "shipped")
    points = gh.body_points(case, z, DEV)
    conds, gp = gh.guidance_inputs(case, z, device=DEV, points=points, B=64)
    x0 = torch.tensor(gh.batch_x(case, z, 64), device=DEV)
    Gd, Gt = gh.make_guide(km, case, z, device=DEV), gh.make_guide(km, case, z, device=DEV, path="torch")
    xd, xt = x0.clone(), x0.clone()
    td, tt = Gd.guidance_step(xd, gp, conds), Gt.guidance_step(xt, gp, conds)
    assert (Gd.last_path, Gt.last_path) == ("device", "torch")
    et, ex, es = ebar
    r = ref64["shipped"]
    nb = len(r["terms"][0])
    rep = lambda a: np.concatenate([a] * (64 // nb + 1), axis=-1 if a.ndim == 2 else 0)
    bound, unit = rep(r["bounds"])[:, :64], rep(mgr.step_unit(r["step"]))[:64]
    td, tt, xd, xt, x0 = (t.cpu().numpy().astype(np.float64) for t in (td, tt, xd, xt, x0))
    assert (np.abs(td - tt) <= 2 * et * np.maximum(1.0, np.abs(tt)) + bound).all()
    assert mgr.rel_terms(xd, xt).max() <= 2 * ex and (np.abs((x0 - xd) - (x0 - xt)) / unit).max() <= 2 * es


@pytest.mark.parametrize("B", [1, 67])
def test_two_runs_give_the_same_bits_and_a_sample_does_not_see_its_batch(B, km, g35):
    z, meta = g35
    case = tg.case_of(meta, "all_7x9")
    G = gh.make_guide(km, case, z, device=DEV)
    points = gh.body_points(case, z, DEV)
    conds, gp = gh.guidance_inputs(case, z, device=DEV, points=points, B=B)
    x0 = torch.tensor(gh.batch_x(case, z, B), device=DEV)
    x1, x2 = x0.clone(), x0.clone()
    t1, t2 = G.guidance_step(x1, gp, conds), G.guidance_step(x2, gp, conds)
    assert G.last_path == "device" and np.array_equal(bits(x1), bits(x2)) and np.array_equal(bits(t1), bits(t2))
    # the last sample alone
    alone = types.SimpleNamespace(**{k: getattr(gp, k) for k in dir(gp) if not k.startswith("_")})
    alone.target_xy = gp.target_xy[B - 1:]
    xa = x0[B - 1:].clone()
    ta = G.guidance_step(xa, alone, {gh.K.GUIDANCE_PARAMS: alone, gh.K.OBS_KEY: conds[gh.K.OBS_KEY][B - 1:]})
    assert np.array_equal(bits(xa)[0], bits(x1)[B - 1]) and np.array_equal(bits(ta)[:, 0], bits(t1)[:, B - 1])


def test_nan_stays_in_its_sample_and_nothing_enabled_launches_nothing(km, g35):
    from parc_amd.diffusion import diffusion_util as du
    z, meta = g35
    case = tg.case_of(meta, "all_7x9")
    G = gh.make_guide(km, case, z, device=DEV)
    conds, gp = gh.guidance_inputs(case, z, device=DEV)
    x0 = torch.tensor(z["all_7x9_x"], device=DEV)
    x = x0.clone()
    t = G.guidance_step(x, gp, conds)
    xn = x0.clone()
    xn[1, 2, G._features._feature_slices[G.MDMFrameType.ROOT_POS].start] = float("nan")
    xb = xn.clone()
    tb = G.guidance_step(xb, gp, conds)
    assert not torch.isfinite(xb[1]).all() and not torch.isfinite(tb[:, 1]).all()
    for b in (0, 2):
        assert np.array_equal(bits(xb)[b], bits(x)[b]) and np.array_equal(bits(tb)[:, b], bits(t)[:, b])
    # no term enabled: nothing is launched, x_t keeps its bits (a NaN included)
    G.last_path = None
    assert G.apply_guidance(xn, {gh.K.GUIDANCE_PARAMS: du.MDMCustomGuidance()}) is None and G.last_path is None


def test_hand_over_onto_an_object_with_the_reference_names(km, g35, ref64, ebar):
    """apply_guidance assigned onto a bare object carrying the reference's attribute names, called with conds keyed by a foreign
    MDMKeyType: it updates the tensor in place"""
    import enum
    from parc_amd.diffusion import diffusion_util as du
    z, meta = g35
    case = tg.case_of(meta, "no_pos_con")
    Foreign = enum.Enum("MDMKeyType", {m.name: m.value for m in du.MDMKeyType})
    ns = types.SimpleNamespace(MDMKeyType=Foreign, MDMFrameType=du.MDMFrameType, LossType=du.LossType)
    G = gh.make_guide(km, case, z, device=DEV, types=ns)
    mdm = types.SimpleNamespace(_kin_char_model=km, _sequence_fps=case["fps"], _mdm_features_mean=G._features._mdm_features_mean,
                                _mdm_features_std=G._features._mdm_features_std, _device=DEV)
    mdm.apply_guidance = G.apply_guidance
    conds, gp = gh.guidance_inputs(case, z, device=DEV, key_type=Foreign)
    x0 = torch.tensor(z["no_pos_con_x"], device=DEV)
    x = x0.clone()
    assert mdm.apply_guidance(x, conds) is None and G.last_path == "device"
    r = ref64["no_pos_con"]
    assert mgr.rel_terms(x.cpu().numpy(), r["x_out"]).max() <= 2 * ebar[1] and not torch.equal(x, x0)
