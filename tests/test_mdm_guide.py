"""The generator's guidance step without a GPU: the torch path of parc_amd.diffusion.mdm_guidance and the host build of the kernel's
shared header parc_mdm_guide_core.h (tests/tools/mdm_guide_host.cpp), against fixture G35 (the reference's own MDM.apply_guidance, run
by tests/golden/gen_mdm_guide.py) and against the float64 restatement tests/mdm_guide_ref.py.

Bounds.  e-bar is the largest |reference fp32 - float64 restatement| over the fixture, measured separately for the terms (relative to
max(1, |value|)), for x_out (relative to max(1, |value|)) and for the step x - x_out (relative to the per-sample max of the float64
step); measured by `python tests/mdm_guide_ref.py`, recorded in DESIGN.md.  Every build is held within 2 e-bar of the restatement and
within 2 e-bar of G35: it is one more fp32 evaluation of the same chain.  A term is a sum, so the textbook bound on what re-ordering
its fp32 summation can change (the restatement computes it per term) is added for the terms.  The step is compared as it is stored:
x - x_out of fp32 numbers whose difference is exact in float64.
"""
import ctypes
import os
import subprocess
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

EBAR_TERMS_RECORDED = 9.0892e-07       # python tests/mdm_guide_ref.py
EBAR_XOUT_RECORDED = 1.0285e-05
EBAR_STEP_RECORDED = 3.6451e-06
FEATURE_TOL = 16 * 2.0 ** -23   # a sample point is a handful of fp32 operations on O(1) values: 16 ulp of 1 (as tests/test_mdm_loss.py)
CASES = ["all_7x9", "shipped", "hf_only", "target_only", "dt_only", "short", "no_pos_con"]


@pytest.fixture(scope="module")
def km():
    from parc_amd.anim import kin_char_model as kcm
    m = kcm.KinCharModel("cpu")
    m.load_char_file(kcm.default_char_file())
    return m


@pytest.fixture(scope="module")
def g35():
    return mgr.load_fixture()


@pytest.fixture(scope="module")
def ref64(km, g35):
    """the float64 restatement of every case (terms, bounds, gradient, x_out, step, the preconditions' figures), computed once"""
    z, meta = g35
    model = mlr.model_from_char(km)
    out = {}
    for case in meta["cases"]:
        diag = {}
        out[case["name"]] = mgr.case_eval(model, case, z, diag=diag)
        diag.pop("world", None)
        out[case["name"]]["diag"] = diag
    return out


@pytest.fixture(scope="module")
def ebar(ref64):
    e = mgr.measure_ebar(evals=ref64)
    rec = (EBAR_TERMS_RECORDED, EBAR_XOUT_RECORDED, EBAR_STEP_RECORDED)
    assert all(abs(a - b) <= 1e-9 for a, b in zip(e, rec)), e          # the recorded figures are the fixture's
    return e


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return gh.build_host(str(tmp_path_factory.mktemp("mdm_guide_host")))


def case_of(meta, name):
    return [c for c in meta["cases"] if c["name"] == name][0]


def check_result(terms, x_out, x, r, z, n, ebar, what):
    """terms [5, B], x_out [B, S, D] of input x: within 2 e-bar (+ the re-ordering bound for the terms) of the restatement and of G35"""
    et, ex, es = ebar
    t, xo, x = np.asarray(terms, np.float64), np.asarray(x_out, np.float64), np.asarray(x, np.float64)
    unit = mgr.step_unit(r["step"])
    for name, rt, rx in (("float64", r["terms"], r["x_out"]), ("G35", z[n + "_terms"].astype(np.float64), z[n + "_x_out"].astype(np.float64))):
        err, tol = np.abs(t - rt), 2 * et * np.maximum(1.0, np.abs(rt)) + r["bounds"]
        print("%s %s terms vs %s: worst err / tol %.3f" % (what, n, name, (err / tol).max()))
        assert (err <= tol).all(), (what, n, name, "terms", err.max())
        e_x = mgr.rel_terms(xo, rx).max()
        e_s = (np.abs((x - xo) - (x - rx)) / unit).max()
        print("%s %s x_out vs %s: err %.3e of %.3e; step err %.3e of %.3e" % (what, n, name, e_x, 2 * ex, e_s, 2 * es))
        assert e_x <= 2 * ex and e_s <= 2 * es, (what, n, name, e_x, e_s)


def unread_columns(G):
    """feature columns the guidance loss never reads: JOINT_POS and CONTACTS"""
    F, T = G._features, G.MDMFrameType
    cols = []
    for name in ("JOINT_POS", "CONTACTS"):
        if name in F._component_names:
            s = F._feature_slices[T[name]]
            cols += list(range(s.start, s.stop))
    return cols


# ------------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_is_intact(g35):
    z, meta = g35
    assert [c["name"] for c in meta["cases"]] == CASES
    shapes = {"all_7x9": (3, 5), "shipped": (2, 16), "hf_only": (1, 5), "target_only": (2, 3), "dt_only": (2, 4), "short": (1, 2), "no_pos_con": (2, 5)}
    for c in meta["cases"]:
        n = c["name"]
        B, S, D = z[n + "_x"].shape
        assert (B, S) == shapes[n] == (len(c["windows"]), c["S"]) and z[n + "_x_out"].shape == (B, S, D) and z[n + "_terms"].shape == (5, B)
        assert z[n + "_mean"].shape == z[n + "_std"].shape == (S, D)
        assert ("hf" in c["terms"]) == (n + "_hfs" in z.files) and ("target" in c["terms"]) == (n + "_target_xy" in z.files)
    assert z["points_dense"].shape == (304, 3) and os.path.getsize(mgr.G35) < 1 << 20
    sh = case_of(meta, "shipped")
    assert (sh["grid"], sh["dx"], sh["points"], sh["terms"], sh["w"][:2], sh["guidance_str"]) == ([10, 20, 15, 15], 0.2, "dense", ["target", "hf"], [1.0, 10.0], 0.1)


def test_generator_check_regenerates_the_fixture():
    """gen_mdm_guide.py --check: the reference's own apply_guidance gives the committed fixture again, 0 differences.  Where the
    reference tree does not exist the test is skipped and says so - decided here, before the generator runs."""
    root = mlr.reference_root()
    if not os.path.isdir(root):
        pytest.skip("the reference tree ({}) is not on this machine: the fixture generator cannot run".format(root))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "gen_mdm_guide.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0 and "0 differences" in res.stdout, (res.returncode, res.stdout[-2000:] + res.stderr[-2000:])


def test_preconditions_hold(g35, ref64):
    z, meta = g35
    for c in meta["cases"]:
        assert mgr.preconditions(ref64[c["name"]]["diag"], c) == [], c["name"]


def test_point_sets_match_fixture(km, g35):
    from parc_amd.util import geom_util
    z, _ = g35
    for name, pts in (("minimal", geom_util.get_minimal_char_point_samples(km)), ("dense", geom_util.get_char_point_samples(km))):
        assert [int(p.shape[0]) for p in pts] == [int(c) for c in z["counts_" + name]], name
        np.testing.assert_allclose(torch.cat(pts).numpy(), z["points_" + name], atol=FEATURE_TOL, rtol=0)


@pytest.mark.parametrize("name", ["all_7x9", "hf_only", "dt_only"])
def test_restatement_gradient_agrees_with_central_differences(name, km, g35, ref64):
    z, meta = g35
    case, model, r = case_of(meta, name), mlr.model_from_char(km), ref64[name]
    rng = np.random.default_rng(35)
    x0 = torch.tensor(z[name + "_x"], dtype=torch.float64)
    for _ in range(3):
        d = rng.standard_normal(x0.shape)
        d /= np.linalg.norm(d)
        h = 1e-6
        lp = mgr.case_eval(model, case, z, x=x0 + h * torch.tensor(d))["loss"]
        lm = mgr.case_eval(model, case, z, x=x0 - h * torch.tensor(d))["loss"]
        # central differences: truncation h^2 f''' and rounding eps |f| / h, both far below 1e-6 of the gradient's norm here
        assert abs((lp - lm) / (2 * h) - float((r["grad"] * d).sum())) <= 1e-6 * np.linalg.norm(r["grad"]), name


# ------------------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("name", CASES)
def test_torch_path_matches_fixture_and_restatement(name, km, g35, ref64, ebar):
    z, meta = g35
    case = case_of(meta, name)
    G = gh.make_guide(km, case, z)
    assert G._path == "torch" and "not a HIP device" in G._path_reason
    conds, gp = gh.guidance_inputs(case, z)
    x0 = torch.tensor(z[name + "_x"])
    x = x0.clone()
    terms = G.guidance_step(x, gp, conds)
    assert G.last_path == "torch"
    check_result(terms.numpy(), x.numpy(), x0.numpy(), ref64[name], z, name, ebar, "torch path")
    cols = unread_columns(G)
    assert np.array_equal(x.numpy()[..., cols].view(np.uint32), x0.numpy()[..., cols].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("name", CASES)
def test_host_build_matches_fixture_and_restatement(name, km, g35, ref64, ebar, hostlib):
    z, meta = g35
    case = case_of(meta, name)
    a = gh.Args(km, case, z)
    terms, x_out = gh.run_host(hostlib, a)
    check_result(terms, x_out, a.x, ref64[name], z, name, ebar, "host build")
    terms_ip, x_ip = gh.run_host(hostlib, a, in_place=True)
    assert np.array_equal(x_ip.view(np.uint32), x_out.view(np.uint32)) and np.array_equal(terms_ip.view(np.uint32), terms.view(np.uint32))
    cols = unread_columns(gh.make_guide(km, case, z))
    assert np.array_equal(x_out[..., cols].view(np.uint32), a.x[..., cols].view(np.uint32))
    b = a.B - 1          # a sample of a batch equals the same sample alone
    t1, x1 = gh.run_host(hostlib, a.only(b))
    assert np.array_equal(x1[0].view(np.uint32), x_out[b].view(np.uint32)) and np.array_equal(t1[:, 0].view(np.uint32), terms[:, b].view(np.uint32))


def test_host_nan_stays_in_its_sample_and_true_features_give_no_nan(km, g35, hostlib):
    z, meta = g35
    case = case_of(meta, "all_7x9")
    a = gh.Args(km, case, z)
    terms, x_out = gh.run_host(hostlib, a)
    for bad in (np.nan, np.inf):
        x = a.x.copy()
        x[1, 2, a.cfg.off_root_pos] = bad          # a column the chain reads (an exponential map drops a NaN, as the reference's does)
        tb, xb = gh.run_host(hostlib, gh.Args(km, case, z, x=x))
        assert not np.isfinite(xb[1]).all() and not np.isfinite(tb[:, 1]).all()
        for b in (0, 2):
            assert np.array_equal(xb[b].view(np.uint32), x_out[b].view(np.uint32)) and np.array_equal(tb[:, b].view(np.uint32), terms[:, b].view(np.uint32))
    # x = the standardised truth: hinge angles and exponential maps straight from quaternions, the fixed hand joints
    tt, xt = gh.run_host(hostlib, gh.Args(km, case, z, x=z["all_7x9_x_true"]))
    assert np.isfinite(tt).all() and np.isfinite(xt).all()


def test_sanitized_program_runs_the_cases(tmp_path, km, g35, hostlib):
    """the same header under ASan + UBSan in a stand-alone program (its own main), run as a child process, over every case, out of place
    and in place; its results equal the plain host build's bit for bit"""
    z, meta = g35
    exe = gh.build_program(str(tmp_path))
    for case in meta["cases"]:
        a = gh.Args(km, case, z)
        terms, x_out = gh.run_host(hostlib, a)
        for in_place in (False, True):
            cf, of = str(tmp_path / (case["name"] + ".case")), str(tmp_path / (case["name"] + ".out"))
            gh.dump(cf, a, in_place)
            res = subprocess.run([exe, cf, of], capture_output=True, text=True)
            assert res.returncode == 0 and "mdm guide ok" in res.stdout, (case["name"], res.returncode, res.stderr[-3000:])
            t2, x2 = gh.read_program_output(of, a)
            assert np.array_equal(t2.view(np.uint32), terms.view(np.uint32)) and np.array_equal(x2.view(np.uint32), x_out.view(np.uint32)), case["name"]


# ------------------------------------------------------------------------------------------------------------------- the library
def test_exports_sizes_and_abi(hostlib, km, g35):
    from parc_amd import _hip, _hip_mdm_guide as H
    assert {"parc_mdm_guide_step", "parc_mdm_guide_lds_bytes", "parc_mdm_guide_abi"} <= set(_hip.EXPORTED)
    assert "parc_mdm_guide.hip" in _hip.SOURCES and "parc_mdm_guide.hip" in _hip.DIAG_SOURCES
    assert "-ffp-contract=off" in _hip.OPT_LEVEL["parc_mdm_guide.hip"].split()
    L = _hip.lib()
    for name in ("parc_mdm_guide_step", "parc_mdm_guide_lds_bytes", "parc_mdm_guide_abi"):
        assert hasattr(L, name), name
    assert L.parc_mdm_guide_abi() == 1
    sizes = (ctypes.c_int * 2)()
    assert gh.host_lib(hostlib).mdm_guide_struct_sizes(sizes) == 2
    assert (sizes[0], sizes[1]) == (ctypes.sizeof(H.MdmGuideCfgS), ctypes.sizeof(_hip.CharModelS))
    # the LDS of a workgroup, from the host build of the core: the formula of include/parc_mdm_guide.h for every case of the fixture, and
    # the figure that header gives for the shipped configuration (S 16, 15 bodies, 31 x 31 grid, 304 points, D 91)
    z, meta = g35
    for case in meta["cases"]:
        a = gh.Args(km, case, z)
        c = a.cfg
        assert gh.host_lib(hostlib).mdm_guide_lds_bytes_host(a.model, c) == \
            H.lds_formula(c.seq_len, km.get_num_joints(), c.feat_dim, c.dim_x * c.dim_y, c.num_points), case["name"]
    c = gh.Args(km, case_of(meta, "shipped"), z).cfg
    assert (c.seq_len, km.get_num_joints(), c.dim_x, c.dim_y, c.num_points, c.feat_dim) == (16, 15, 31, 31, 304, 91)
    assert gh.host_lib(hostlib).mdm_guide_lds_bytes_host(km.c_struct(), c) == 59780


def test_argument_refusals_need_no_gpu(km, g35):
    """every refusal of include/parc_mdm_guide.h in its order, from the library itself: all of them come before any HIP call"""
    import copy
    from parc_amd import _hip, _hip_mdm_guide as H
    z, meta = g35
    L = _hip.lib()
    a = gh.Args(km, case_of(meta, "shipped"), z)
    one = ctypes.c_void_p(8)          # a non-NULL pointer that is never followed: nothing is launched in this test

    def call(cfg=None, model=None, B=2, ptrs=None):
        p = [one] * 11 if ptrs is None else ptrs
        return L.parc_mdm_guide_step(None, model if model is not None else a.model, cfg if cfg is not None else a.cfg, B, *p)

    def cfg_with(**kw):
        c = copy.copy(a.cfg)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    # the shipped configuration fits, and its size is the documented formula
    need = L.parc_mdm_guide_lds_bytes(a.model, a.cfg)
    assert need == H.lds_formula(16, 15, a.D, 31 * 31, 304) and need <= H.MAX_LDS == 65536, need
    # 1. EINVAL: counts, layout, unknown bits, the terrain term without points, bodies not parents-first
    for c in (cfg_with(seq_len=0), cfg_with(dim_x=0), cfg_with(dim_y=0), cfg_with(num_points=-1), cfg_with(feat_dim=a.D + 1),
              cfg_with(off_contacts=a.cfg.off_contacts - 1), cfg_with(enabled=1 << 5), cfg_with(enabled=3, num_points=0)):
        assert call(cfg=c) == H.EINVAL
    assert call(B=-1) == H.EINVAL
    m = copy.copy(a.model)
    m.parent[3] = 5
    assert call(model=m) == H.EINVAL
    # ... also where the window would not fit, where nothing is enabled and where pointers are NULL: EINVAL comes first
    assert call(cfg=cfg_with(seq_len=64, dim_x=0), B=0, ptrs=[None] * 11) == H.EINVAL
    # 2. EUNSUPPORTED before "nothing to do" and before the pointers
    big = cfg_with(seq_len=64)
    assert L.parc_mdm_guide_lds_bytes(a.model, big) > H.MAX_LDS
    assert call(cfg=big) == call(cfg=big, B=0) == call(cfg=cfg_with(seq_len=64, enabled=0), ptrs=[None] * 11) == H.EUNSUPPORTED
    # 3. OK with nothing launched: B == 0, or no term enabled - before the pointers are looked at
    assert call(B=0, ptrs=[None] * 11) == 0 and call(cfg=cfg_with(enabled=0), ptrs=[None] * 11) == 0
    # 4. EINVAL for a NULL required pointer: x, mean, std, hfs, target_xy, grid_x, grid_y, points, point_start, x_out, terms
    for i in range(11):
        p = [one] * 11
        p[i] = None
        assert call(ptrs=p) == H.EINVAL, i
    # a term that is off does not need its arrays
    p = [one] * 11
    p[4] = None
    assert call(cfg=cfg_with(enabled=2), ptrs=p, B=0) == 0
    assert L.parc_mdm_guide_step(None, a.model, cfg_with(enabled=0), 2, *p) == 0


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_interface(km, g35, capsys):
    from parc_amd.diffusion import diffusion_util as du, mdm_guidance as mg
    z, meta = g35
    case = case_of(meta, "all_7x9")
    # the reference's names and values
    assert (du.MDMKeyType.OBS_KEY.value, du.MDMKeyType.GUIDANCE_PARAMS.value, du.MDMKeyType.IN_PAINT_PARAMS.value) == (0, 9, 16)
    gp0 = du.MDMCustomGuidance()
    assert (gp0.guidance_str, gp0.w_target_loss, gp0.w_hf_loss, gp0.verbose, gp0.strong_hf_guidance, gp0.max_speed, gp0.max_jerk) == \
        (0.1, 1.0, 10.0, True, False, 16.1498, 14062.6680) and gp0.target_xy is None and gp0.body_points is None and not gp0.guide_speed
    # a types= namespace replaces the enums: a foreign MDMKeyType keys conds
    import enum
    Foreign = enum.Enum("MDMKeyType", {m.name: m.value for m in du.MDMKeyType})
    ns = types.SimpleNamespace(MDMKeyType=Foreign, MDMFrameType=du.MDMFrameType, LossType=du.LossType)
    G = gh.make_guide(km, case, z, types=ns)
    conds, gp = gh.guidance_inputs(case, z, key_type=Foreign)
    x0 = torch.tensor(z["all_7x9_x"])
    x = x0.clone()
    gp.verbose = True
    assert G.apply_guidance(x, conds) is None and not torch.equal(x, x0)
    out = capsys.readouterr().out
    for label in ("target_loss:", "scaled target loss:", "hf_loss:", "scaled hf_loss:", "speed_loss:", "scaled speed_loss:", "acc_loss:",
                  "scaled acc_loss:", "jerk_loss:", "scaled jerk_loss:"):
        assert label in out, label
    assert abs(float(out.split("hf_loss:")[1].split()[0]) - float(z["all_7x9_terms"][1].sum())) <= 1e-4 * float(z["all_7x9_terms"][1].sum())
    # with our own keys the foreign-keyed instance sees no OBS_KEY: has_hf_guidance keeps the reference's rule
    assert not (G._enabled(gp, {du.MDMKeyType.OBS_KEY: 0}) & 2) and (G._enabled(gp, conds) & 2)
    # nothing enabled: x_t untouched, nothing printed
    x = x0.clone()
    assert G.apply_guidance(x, {Foreign.GUIDANCE_PARAMS: du.MDMCustomGuidance()}) is None and torch.equal(x, x0) and capsys.readouterr().out == ""
    strong = du.MDMCustomGuidance()
    strong.strong_hf_guidance = True
    with pytest.raises(NotImplementedError, match="strong_hf_guidance"):
        G.apply_guidance(x, {Foreign.GUIDANCE_PARAMS: strong})
    # unsupported configurations select the torch path and name the reason
    F = mg.MDMGuidance(gh.gen_cfg(case, rot_type="EXP_MAP"), km, torch.zeros(5, 6 + 3 * 14 * 2 + 15), torch.ones(5, 6 + 3 * 14 * 2 + 15))
    assert F._path == "torch" and "EXP_MAP" in F._path_reason
    assert G._path == "torch" and "cpu" in G._path_reason
    with pytest.raises(ValueError):
        gh.make_guide(km, case, z, path="device")
    # guidance_params_from_settings switches the terms gen_util switches
    S = types.SimpleNamespace(use_cfg=False, cfg_scale=0.65, guide_speed=False, guide_acc=True, guide_jerk=False, w_speed=0.1, w_acc=0.2, w_jerk=0.3,
                              max_jerk=1000.0, strong_hf_guidance=False, target_guidance=False, hf_collision_guidance=False, guidance_str=0.25)
    p, attach = mg.guidance_params_from_settings(S, "t", km)
    assert not attach and p.target_xy is None and p.body_points is None and p.guidance_str == 0.1 and p.obs_cfg_scale is None
    assert (p.guide_speed, p.guide_acc, p.guide_jerk, p.w_speed, p.w_acc, p.w_jerk, p.max_jerk, p.max_speed) == (False, True, False, 0.1, 0.2, 0.3, 1000.0, 16.1498)
    S.target_guidance, S.use_cfg = True, True
    p, attach = mg.guidance_params_from_settings(S, "t", km)
    assert attach and p.target_xy == "t" and p.body_points is None and p.guidance_str == 0.25 and p.obs_cfg_scale == 0.65
    S.target_guidance, S.hf_collision_guidance = False, True
    p, attach = mg.guidance_params_from_settings(S, "t", km)
    assert attach and p.target_xy is None and sum(int(b.shape[0]) for b in p.body_points) == 304 and p.guidance_str == 0.25
    # the packing of a body-point list happens once per distinct list
    a1, a2 = G.pack_points(p.body_points), G.pack_points(p.body_points)
    assert a1[0] is a2[0] and a1[2] == 304 and a1[1].tolist()[-1] == 304
