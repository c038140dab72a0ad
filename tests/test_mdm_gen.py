"""The generator call without a GPU: the torch path of parc_amd.diffusion.gen_util and the host build of the kernels' shared header
parc_mdm_gen_core.h (tests/tools/mdm_gen_host.cpp), against fixture G36 (the reference's own gen_mdm_motion, run by
tests/golden/gen_mdm_gen.py) and against the float64 restatement tests/mdm_gen_ref.py.

Bounds.
  Heights.  A cell of hf_z / obs is near a boundary when, in the restatement, either grid coordinate lies within 2e-4 cells of a rounding
  boundary (six fp32 roundings at |index| < 128, ulp 7.6e-6, plus the sin / cos error over a 30-cell arm).  Every other cell is bit-equal
  to the fixture: one subtraction and one division after an exact selection.  A near-boundary cell equals the value from one of the at
  most four adjacent terrain cells.  At most 0.5 % of a case's cells are near a boundary (the generator asserts it; a test repeats it).
  contacts and the canonical root z are single roundings of the same operands: bit-equal to the fixture.
  Every other output, per group (canonical frames and body positions; prev_state; target and target_dir; decoded world root_pos,
  root_rot, joint_rot; frames): e-bar is the largest |reference fp32 fixture - float64 restatement| over G36, measured by
  `python tests/mdm_gen_ref.py` and recorded below; every path is held within 2 e-bar of the restatement and of G36 - operation order
  and libm differ from torch's by a few ulp, and that is all the margin is for.
RELATIVE_TO_ROOT_FLOOR is held against the restatement alone (the reference's branch raises for B != 2), within the same bounds.
"""
import ctypes
import copy
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
import mdm_gen_host as gh       # noqa: E402
import mdm_gen_ref as mgn       # noqa: E402
import mdm_loss_ref as mlr      # noqa: E402

# python tests/mdm_gen_ref.py
EBAR_CANON_RECORDED = 2.771427e-07
EBAR_PREV_STATE_RECORDED = 4.567621e-07
EBAR_TARGET_RECORDED = 1.867771e-07
EBAR_ROOT_POS_RECORDED = 5.320385e-07
EBAR_ROOT_ROT_RECORDED = 1.412500e-07
EBAR_JOINT_ROT_RECORDED = 7.740386e-08
EBAR_FRAMES_RECORDED = 5.320385e-07
EBAR_RECORDED = dict(canon=EBAR_CANON_RECORDED, prev_state=EBAR_PREV_STATE_RECORDED, target=EBAR_TARGET_RECORDED, root_pos=EBAR_ROOT_POS_RECORDED,
                     root_rot=EBAR_ROOT_ROT_RECORDED, joint_rot=EBAR_JOINT_ROT_RECORDED, frames=EBAR_FRAMES_RECORDED)
CASES = ["shipped", "edge_7x9", "pair", "no_pos_con", "zero_target", "components"]


@pytest.fixture(scope="module")
def km():
    from parc_amd.anim import kin_char_model as kcm
    m = kcm.KinCharModel("cpu")
    m.load_char_file(kcm.default_char_file())
    return m


@pytest.fixture(scope="module")
def g36():
    return mgn.load_fixture()


@pytest.fixture(scope="module")
def ref64(km, g36):
    """the float64 restatement of every case (and the preconditions' figures), computed once"""
    z, meta = g36
    model = mlr.model_from_char(km)
    out = {}
    for case in meta["cases"]:
        diag = {}
        out[case["name"]] = mgn.case_eval(model, case, z, diag=diag)
        out[case["name"]]["diag"] = diag
    return out


@pytest.fixture(scope="module")
def ebar(ref64):
    e = mgn.measure_ebar(evals=ref64)
    assert set(e) == set(EBAR_RECORDED) and all(abs(e[g] - EBAR_RECORDED[g]) <= 1e-9 for g in e), e          # the recorded figures are the fixture's
    return e


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return gh.build_host(str(tmp_path_factory.mktemp("mdm_gen_host")))


def case_of(meta, name):
    return [c for c in meta["cases"] if c["name"] == name][0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def f64(a):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------- the checks
def check_heights(what, case, z, r, hf_z, obs, z_ref, fixture=True):
    """hf_z [B, X, Y] and obs [B, X, Y] (either may be None) of a path: bit-equal to the expected value away from the rounding boundaries,
    one of the adjacent cells' values near them.  The expected values are the fixture's (obs of a feature-mode case, hf_z of the
    component-mode case) or, with fixture=False, the restatement's selection evaluated in fp32."""
    n, enc = case["name"], r["enc"]
    ter = mgn.fixture_terrain(z)
    near = mgn.near_boundary(enc["coords"]).numpy()
    assert near.mean() <= mgn.MAX_NEAR, (n, near.mean())
    zr = np.asarray(z_ref, np.float32).reshape(-1, 1, 1)
    h32 = mgn.lookup(ter, enc["coords"]).numpy().astype(np.float32)
    adj32 = mgn.adjacent_values(ter, enc["coords"]).numpy().astype(np.float32)          # [B, X, Y, 4]
    mh = np.float32(case["max_h"])
    norm = lambda h: np.clip(h, -mh, mh) / mh
    for name, got, fix_key, fn in (("hf_z", hf_z, "_hf_z", lambda h: h), ("obs", obs, "_obs", norm)):
        if got is None:
            continue
        got = np.asarray(got, np.float32).reshape(near.shape)
        want = z[n + fix_key].reshape(near.shape) if fixture and n + fix_key in z.files else fn(h32 - zr)
        ok = bits(got) == bits(want)
        print("%s %s %s: %d cells, %d near a boundary, %d differ" % (what, n, name, near.size, near.sum(), (~ok).sum()))
        assert ok[~near].all(), (what, n, name, "a cell away from every boundary differs")
        cand = fn(adj32 - zr[..., None])
        assert (bits(got)[..., None] == bits(cand)).any(-1)[near].all(), (what, n, name, "a near-boundary cell is none of the adjacent cells")


def check_group(what, n, group, got, ref, fix, ebar):
    """within 2 e-bar of the restatement and (where the fixture records it) of G36"""
    tol = 2 * ebar[group]
    for name, want in (("float64", ref), ("G36", fix)):
        if want is None:
            continue
        err = float(np.abs(f64(got) - f64(want).reshape(f64(got).shape)).max())
        print("%s %s %s vs %s: err %.3e of %.3e" % (what, n, group, name, err, tol))
        assert err <= tol, (what, n, group, name, err, tol)


def check_encode(what, case, z, r, ebar, o, fixture=True):
    """o: dict with canonical root_pos / root_rot / body_pos [B, T, ...], target, target_dir [B, 2], prev_state (or None), z_ref [B]"""
    n, enc, P = case["name"], r["enc"], case["num_prev_states"]
    fx = lambda key: z[n + key] if fixture and n + key in z.files else None
    check_group(what, n, "canon", f64(o["root_pos"])[:, :P], enc["root_pos"][:, :P], fx("_canon_root_pos"), ebar)
    check_group(what, n, "canon", f64(o["root_rot"])[:, :P], enc["root_rot"][:, :P], fx("_canon_root_rot"), ebar)
    check_group(what, n, "canon", f64(o["body_pos"])[:, :P], enc["body_pos"][:, :P], fx("_canon_body_pos"), ebar)
    check_group(what, n, "canon", o["root_pos"], enc["root_pos"], None, ebar)
    check_group(what, n, "canon", o["body_pos"], enc["body_pos"], None, ebar)
    check_group(what, n, "target", o["target"], enc["target"], fx("_target"), ebar)
    check_group(what, n, "target", o["target_dir"], enc["target_dir"], fx("_target_dir"), ebar)
    if o.get("prev_state") is not None:
        check_group(what, n, "prev_state", o["prev_state"], enc["prev_state"], fx("_prev_state"), ebar)
    if fixture and n + "_canon_root_pos" in z.files:          # a single rounding: z - z_ref
        assert np.array_equal(bits(f64(o["root_pos"])[:, :P, 2]), bits(z[n + "_canon_root_pos"][..., 2])), (what, n, "canonical root z")
    if case["z_style"] == "RELATIVE_TO_ROOT" and fixture:
        assert np.array_equal(bits(o["z_ref"]), bits(z[n + "_prev_root_pos"][:, P - 1, 2])), (what, n, "z_ref")


def check_decode(what, case, z, r, ebar, o, fixture=True):
    """o: dict root_pos, root_rot, joint_rot, contacts (or None), frames"""
    n, dec = case["name"], r["dec"]
    for g in ("root_pos", "root_rot", "joint_rot", "frames"):
        check_group(what, n, g, o[g], dec[g], z[n + "_out_" + g] if fixture else None, ebar)
    if "CONTACTS" in case["components"]:
        if fixture:          # x * std + mean of the same operands
            assert np.array_equal(bits(f64(o["contacts"])), bits(z[n + "_out_contacts"])), (what, n, "contacts")
        else:
            assert float(np.abs(f64(o["contacts"]) - f64(dec["contacts"])).max()) <= 2 * ebar["prev_state"]
    else:
        assert o["contacts"] is None


def ctx_dict(ctx, conds_prev_state=None):
    return dict(root_pos=ctx.root_pos, root_rot=ctx.root_rot, body_pos=ctx.body_pos, target=ctx.target[:, 0], target_dir=ctx.target_dir[:, 0],
                prev_state=conds_prev_state, z_ref=ctx.z_ref.detach().cpu().numpy())


def frames_dict(mf):
    return dict(root_pos=mf.root_pos, root_rot=mf.root_rot, joint_rot=mf.joint_rot, contacts=mf.contacts, frames=mf.frames)


# ------------------------------------------------------------------------------------------------------------------- the fixture
def test_fixture_is_intact(g36):
    z, meta = g36
    assert [c["name"] for c in meta["cases"]] == CASES
    shapes = {"shipped": (3, 2, 2, 16), "edge_7x9": (2, 3, 2, 5), "pair": (1, 1, 1, 2), "no_pos_con": (2, 2, 2, 3), "zero_target": (2, 2, 2, 3),
              "components": (2, 2, 2, 4)}
    for c in meta["cases"]:
        n = c["name"]
        B, T = z[n + "_prev_root_pos"].shape[:2]
        S, D = z[n + "_mean"].shape
        xn, xp, yn, yp = c["grid"]
        X, Y = 1 + xn + xp, 1 + yn + yp
        assert (B, T, c["num_prev_states"], S) == shapes[n] == (len(c["windows"]), c["T"], c["num_prev_states"], c["S"])
        assert z[n + "_x"].shape == (B, S, D) and z[n + "_out_root_pos"].shape == (B, S, 3) and z[n + "_out_frames"].shape == (B, S, 34)
        assert z[n + "_target_dir"].shape == (B, 1, 2) and z[n + "_flags"].shape == (4, B)
        if c["mode"] == "feature":
            assert z[n + "_obs"].shape == (B, 1, X, Y) and z[n + "_prev_state"].shape == (B, c["num_prev_states"], D)
        else:
            assert z[n + "_hf_z"].shape == (B, X, Y) and z[n + "_canon_body_pos"].shape == (B, c["num_prev_states"], 14, 3)
        assert ("CONTACTS" in c["components"]) == (n + "_out_contacts" in z.files) and c["target_guidance"] == (n + "_target" in z.files)
    sh = case_of(meta, "shipped")
    assert (sh["grid"], sh["dx"], sh["use_prev_state"], z["shipped_mean"].shape[1]) == ([10, 20, 15, 15], 0.2, [True, False, True], 91)
    assert z["shipped_flags"][1].tolist() == [True, False, True] and z["shipped_flags"][[0, 2, 3]].all()
    assert float(np.abs(z["shipped_obs"]).max()) == 1.0          # the tower or the pit: the normalised heights clamp
    assert np.array_equal(z["zero_target_target_world"][0], z["zero_target_prev_root_pos"][0, 1, :2])
    assert np.array_equal(z["zero_target_target_dir"][0], np.zeros((1, 2), np.float32)) and np.array_equal(z["zero_target_target"][0], np.zeros((1, 2), np.float32))
    assert os.path.getsize(mgn.G36) < 1 << 20


def test_generator_check_regenerates_the_fixture():
    """gen_mdm_gen.py --check: the reference's own gen_mdm_motion gives the committed fixture again, 0 differences.  Where the
    reference tree does not exist the test is skipped and says so - decided here, before the generator runs."""
    root = mlr.reference_root()
    if not os.path.isdir(root):
        pytest.skip("the reference tree ({}) is not on this machine: the fixture generator cannot run".format(root))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "gen_mdm_gen.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0 and "0 differences" in res.stdout, (res.returncode, res.stdout[-2000:] + res.stderr[-2000:])


def test_preconditions_hold(g36, ref64):
    z, meta = g36
    for c in meta["cases"]:
        d = ref64[c["name"]]["diag"]
        assert mgn.preconditions(d, c) == [], c["name"]
    d = ref64["edge_7x9"]["diag"]
    assert d["max_abs_heading"] > 3.0
    # part of edge_7x9's grid lies outside the terrain on both sides: indices below 0 and above dim - 1
    co = ref64["edge_7x9"]["enc"]["coords"]
    assert float(co.min()) < -0.5 and float(co[..., 0].max()) > z["terrain_hf"].shape[0] - 0.5
    # within 1 m of a corner
    mn, dxy, dims = z["terrain_min_point"], z["terrain_dxdy"], np.array(z["terrain_hf"].shape)
    p = z["edge_7x9_prev_root_pos"][:, 1, :2]
    assert np.abs(p[0] - (mn + (dims - 1) * dxy)).max() < 1.0 and np.abs(p[1] - mn).max() < 1.0


# ------------------------------------------------------------------------------------------------------------------- the torch path
@pytest.mark.parametrize("name", CASES)
def test_torch_path_matches_fixture_and_restatement(name, km, g36, ref64, ebar):
    from parc_amd.diffusion import diffusion_util as du, gen_util
    z, meta = g36
    case, r = case_of(meta, name), ref64[name]
    K, T = du.MDMKeyType, du.MDMFrameType
    feat = case["mode"] == "feature"
    io = gh.make_io(km, case, z)
    assert io._path == "torch" and "not a HIP device" in io._path_reason
    tw, prev, s = gh.call_inputs(case, z)
    m = gh.stand_in(case, z, components=not feat)
    if not feat:
        m.components_out = io._features.extract_motion_features(torch.tensor(z[name + "_x"]))
    out = gen_util.gen_mdm_motion(tw, prev, gh.fixture_terrain(z), m, km, s, io=io)
    assert io.last_path == "torch" and len(m.calls) == 1 and m.calls[0][0] == ("ddim" if feat else "components")
    conds = m.calls[0][1]
    # the keys and shapes the reference's sampling loop receives
    B, P, D = len(case["windows"]), case["num_prev_states"], z[name + "_mean"].shape[1]
    X, Y = z[name + ("_obs" if feat else "_hf_z")].shape[-2:]
    assert set(conds) == {K.OBS_KEY, K.OBS_FLAG_KEY, K.PREV_STATE_KEY, K.PREV_STATE_NOISE_IND_KEY, K.TARGET_KEY, K.TARGET_FLAG_KEY, K.PREV_STATE_FLAG_KEY,
                          K.GUIDANCE_PARAMS}
    assert conds[K.TARGET_KEY].shape == (B, 1, 2) and conds[K.OBS_KEY].shape == ((B, 1, X, Y) if feat else (B, X, Y))
    flags = np.stack([conds[k].numpy() for k in (K.OBS_FLAG_KEY, K.PREV_STATE_NOISE_IND_KEY, K.TARGET_FLAG_KEY, K.PREV_STATE_FLAG_KEY)])
    assert flags.dtype == bool and np.array_equal(flags, z[name + "_flags"])
    gp = conds[K.GUIDANCE_PARAMS]
    assert gp.obs_cfg_scale == 0.65 and (gp.target_xy is not None) == case["target_guidance"] and gp.body_points is None
    # encode, through a second call that hands the context out
    conds2, ctx = io.encode(tw, prev, gh.fixture_terrain(z), s, components=not feat)
    if feat:
        assert conds[K.PREV_STATE_KEY].shape == (B, P, D) and torch.equal(conds2[K.PREV_STATE_KEY], conds[K.PREV_STATE_KEY])
        check_heights("torch path", case, z, r, ctx.hf_z.numpy(), conds[K.OBS_KEY].numpy(), ctx.z_ref.numpy())
        check_encode("torch path", case, z, r, ebar, ctx_dict(ctx, conds[K.PREV_STATE_KEY]))
        check_decode("torch path", case, z, r, ebar, frames_dict(out))
        if case["target_guidance"]:
            assert torch.equal(gp.target_xy, ctx.target)
    else:
        ps = conds[K.PREV_STATE_KEY]
        assert set(ps) == {T.ROOT_POS, T.ROOT_ROT, T.JOINT_POS, T.JOINT_ROT, T.CONTACTS} and ps[T.JOINT_POS].shape == (B, P, 14, 3)
        assert np.array_equal(bits(ps[T.JOINT_ROT].numpy()), bits(z[name + "_prev_joint_rot"][:, :P]))
        check_heights("torch path", case, z, r, conds[K.OBS_KEY].numpy(), None, ctx.z_ref.numpy())
        check_encode("torch path", case, z, r, ebar, ctx_dict(ctx))
        for g in ("root_pos", "root_rot", "joint_rot"):
            check_group("torch path", name, g, getattr(out, g), r["dec"][g], z[name + "_out_" + g], ebar)
        assert np.array_equal(bits(out.contacts.numpy()), bits(z[name + "_out_contacts"])) and out.body_pos is None and out.body_rot is None


def test_dispatch_and_settings(km, g36):
    """the dispatch of mdm.py:1381-1390, eval() on the denoiser, a bool use_prev_state, and the guidance parameters of gen_util.py:173-199"""
    from parc_amd.diffusion import diffusion_util as du, gen_util
    z, meta = g36
    case = case_of(meta, "edge_7x9")
    K = du.MDMKeyType
    tw, prev, s = gh.call_inputs(case, z)
    ter = gh.fixture_terrain(z)
    m = gh.stand_in(case, z)
    m._denoise_model = types.SimpleNamespace(evals=0)
    m._denoise_model.eval = lambda: setattr(m._denoise_model, "evals", m._denoise_model.evals + 1)
    s.use_ddim, s.ddim_stride = True, 7
    a = gen_util.gen_mdm_motion(tw, prev, ter, m, km, s)
    s.use_ddim = False
    b = gen_util.gen_mdm_motion(tw, prev, ter, m, km, s)
    assert [(c[0], c[2]) for c in m.calls] == [("ddim", 7), ("reverse", 1000)] and m._denoise_model.evals == 2
    assert torch.equal(a.root_pos, b.root_pos) and torch.equal(a.frames, b.frames)
    # use_prev_state False: the sample's own first rows are decoded
    s.use_prev_state = False
    c = gen_util.gen_mdm_motion(tw, prev, ter, m, km, s)
    assert not m.calls[-1][1][K.PREV_STATE_NOISE_IND_KEY].any() and not torch.equal(c.root_pos[:, :2], a.root_pos[:, :2])
    assert torch.equal(c.root_pos[:, 2:], a.root_pos[:, 2:])
    # no guidance parameters without cfg and guidance; body points with hf_collision_guidance
    s.use_cfg = False
    gen_util.gen_mdm_motion(tw, prev, ter, m, km, s)
    assert K.GUIDANCE_PARAMS not in m.calls[-1][1]
    s.hf_collision_guidance, s.guidance_str = True, 0.25
    gen_util.gen_mdm_motion(tw, prev, ter, m, km, s)
    gp = m.calls[-1][1][K.GUIDANCE_PARAMS]
    assert gp.guidance_str == 0.25 and sum(int(p.shape[0]) for p in gp.body_points) == 304 and gp.obs_cfg_scale is None
    with pytest.raises(TypeError):
        gen_util.gen_mdm_motion(tw, prev, ter, types.SimpleNamespace(**{k: v for k, v in vars(m).items() if k not in ("ddim_inference", "reverse_diffusion")}),
                                km, s)


def test_settings_defaults_and_unsupported(km, g36):
    from parc_amd.diffusion import gen_util
    z, meta = g36
    case = case_of(meta, "pair")
    s = gen_util.MDMGenSettings()
    assert (s.use_prev_state, s.use_cfg, s.cfg_scale, s.guide_speed, s.guide_acc, s.guide_jerk, s.w_speed, s.w_acc, s.w_jerk, s.max_jerk, s.strong_hf_guidance,
            s.target_guidance, s.hf_collision_guidance, s.prev_state_ind_key, s.target_condition_key, s.feature_vector_key, s.use_ddim, s.ddim_stride,
            s.guidance_str, s.input_root_pos, s.starting_diffusion_timestep) == \
        (True, True, 0.65, False, False, False, 0.1, 0.1, 0.1, 1000.0, False, False, False, True, True, True, True, 10, 0.1, False, 0)
    tw, prev, s = gh.call_inputs(case, z)
    ter = gh.fixture_terrain(z)
    io = gh.make_io(km, case, z)
    s.input_root_pos = True
    with pytest.raises(NotImplementedError, match="input_root_pos"):
        io.encode(tw, prev, ter, s)
    s.input_root_pos = False
    with pytest.raises(NotImplementedError, match="_use_feature_vector"):
        gh.make_io(km, case, z, use_feature_vector=True).encode(tw, prev, ter, s)
    # unsupported configurations select the torch path and name the reason
    D = 6 + 3 * 14 * 2 + 15
    F = gen_util.MDMGenIO(gh.gen_cfg(case, rot_type="EXP_MAP"), km, torch.zeros(2, D), torch.ones(2, D))
    assert F._path == "torch" and "EXP_MAP" in F._path_reason
    assert io._path == "torch" and "cpu" in io._path_reason
    with pytest.raises(ValueError):
        gh.make_io(km, case, z, path="device")
    with pytest.raises(ValueError, match="num_prev_states"):
        gh.make_io(km, case_of(meta, "shipped"), z).encode(tw, prev, ter, s)          # P = 2 with one previous frame


# ------------------------------------------------------------------------------------------------------------------- the host build
@pytest.mark.parametrize("name", CASES)
def test_host_build_matches_fixture_and_restatement(name, km, g36, ref64, ebar, hostlib):
    z, meta = g36
    case, r = case_of(meta, name), ref64[name]
    feat = case["mode"] == "feature"
    a = gh.Args(km, case, z, features=feat)
    enc = gh.run_encode(hostlib, a)
    assert all(np.isfinite(v).all() for v in enc.values())          # every element was written
    o = dict(enc, z_ref=enc["frame"][:, 6])
    check_heights("host build", case, z, r, enc["hf_z"], enc.get("obs"), enc["frame"][:, 6])
    check_encode("host build", case, z, r, ebar, o)
    # the frame record: canon_xy and z_ref are copies of the inputs, the quaternion and the heading are the restatement's
    P = a.P
    assert np.array_equal(bits(enc["frame"][:, 0:2]), bits(a.root_pos[:, P - 1, 0:2]))
    assert np.abs(enc["frame"][:, 2:6] - r["enc"]["heading_quat"].numpy()).max() <= 2 * ebar["root_rot"]
    assert np.abs(enc["frame"][:, 7] - r["enc"]["heading"].numpy()).max() <= 4 * 2.0 ** -22          # an angle below 4: a few ulp of atan2f
    b = a.B - 1          # a sample of a batch equals the same sample alone
    enc1 = gh.run_encode(hostlib, a.only(b))
    for k in enc:
        assert np.array_equal(bits(enc1[k][0]), bits(enc[k][b])), k
    if feat:
        dec = gh.run_decode(hostlib, a, enc)
        assert all(np.isfinite(v).all() for v in dec.values())
        check_decode("host build", case, z, r, ebar, dict(dec, contacts=dec.get("contacts")))
        dec_nf = gh.run_decode(hostlib, a, enc, frames=False)          # frames is optional: the other outputs do not depend on it
        assert set(dec_nf) == set(dec) - {"frames"} and all(np.array_equal(bits(dec_nf[k]), bits(dec[k])) for k in dec_nf)
        dec1 = gh.run_decode(hostlib, a.only(b), enc1)
        for k in dec:
            assert np.array_equal(bits(dec1[k][0]), bits(dec[k][b])), k


@pytest.mark.parametrize("name", ["shipped", "edge_7x9"])
def test_root_floor_style_matches_restatement(name, km, g36, ebar, hostlib):
    """RELATIVE_TO_ROOT_FLOOR, per sample: torch path and host build against the float64 restatement alone"""
    from parc_amd.diffusion import gen_util
    z, meta = g36
    case = dict(case_of(meta, name), z_style="RELATIVE_TO_ROOT_FLOOR")
    model = mlr.model_from_char(km)
    r = mgn.case_eval(model, case, z)
    zr = r["enc"]["z_ref"].numpy()
    assert np.ptp(zr) > 0.0 and np.abs(zr - z[name + "_prev_root_pos"][:, 1, 2]).min() > 0.1          # not the root's height, and one per sample
    a = gh.Args(km, case, z, z_style="RELATIVE_TO_ROOT_FLOOR")
    assert a.cfg_enc.z_style == 1
    enc = gh.run_encode(hostlib, a)
    assert np.array_equal(bits(enc["frame"][:, 6]), bits(zr))          # a terrain cell's height, selected exactly
    check_heights("host build, floor", case, z, r, enc["hf_z"], enc["obs"], enc["frame"][:, 6], fixture=False)
    check_encode("host build, floor", case, z, r, ebar, dict(enc, z_ref=enc["frame"][:, 6]), fixture=False)
    check_decode("host build, floor", case, z, r, ebar, dict(gh.run_decode(hostlib, a, enc)), fixture=False)
    io = gh.make_io(km, case, z, z_style="RELATIVE_TO_ROOT_FLOOR")
    tw, prev, s = gh.call_inputs(case, z)
    m = gh.stand_in(case, z)
    out = gen_util.gen_mdm_motion(tw, prev, gh.fixture_terrain(z), m, km, s, io=io)
    conds, ctx = io.encode(tw, prev, gh.fixture_terrain(z), s)
    K = io.MDMKeyType
    assert np.array_equal(bits(ctx.z_ref.numpy()), bits(zr))
    check_heights("torch path, floor", case, z, r, ctx.hf_z.numpy(), conds[K.OBS_KEY].numpy(), ctx.z_ref.numpy(), fixture=False)
    check_encode("torch path, floor", case, z, r, ebar, ctx_dict(ctx, conds[K.PREV_STATE_KEY]), fixture=False)
    check_decode("torch path, floor", case, z, r, ebar, frames_dict(out), fixture=False)


def test_host_nan_stays_in_its_sample(km, g36, hostlib):
    z, meta = g36
    case = case_of(meta, "shipped")
    a = gh.Args(km, case, z)
    enc = gh.run_encode(hostlib, a)
    dec = gh.run_decode(hostlib, a, enc)
    for bad in (np.nan, np.inf):
        b = copy.copy(a)
        b.root_pos, b.x = a.root_pos.copy(), a.x.copy()
        b.root_pos[1, 1, 0] = bad          # the reference frame's x: canon_xy, every grid coordinate and the target
        b.x[1, 5, a.cfg_dec.off_root_pos] = bad
        enc_b = gh.run_encode(hostlib, b)          # every terrain index is clamped before its load: no fault, whatever the coordinate
        dec_b = gh.run_decode(hostlib, b, enc_b)
        assert not np.isfinite(enc_b["root_pos"][1]).all() and not np.isfinite(enc_b["target"][1]).all() and not np.isfinite(dec_b["root_pos"][1]).all()
        for s in (0, 2):
            for k in enc:
                assert np.array_equal(bits(enc_b[k][s]), bits(enc[k][s])), (k, s)
            for k in dec:
                assert np.array_equal(bits(dec_b[k][s]), bits(dec[k][s])), (k, s)


def test_sanitized_program_runs_the_cases(tmp_path, km, g36, hostlib):
    """the same header under ASan + UBSan in a stand-alone program (its own main), run as a child process, over every case and both
    z styles; its results equal the plain host build's bit for bit"""
    z, meta = g36
    exe = gh.build_program(str(tmp_path))
    for case in meta["cases"]:
        for z_style in ("RELATIVE_TO_ROOT", "RELATIVE_TO_ROOT_FLOOR"):
            feat = case["mode"] == "feature"
            a = gh.Args(km, case, z, z_style=z_style, features=feat)
            enc = gh.run_encode(hostlib, a)
            dec = gh.run_decode(hostlib, a, enc) if feat else None
            cf, of = str(tmp_path / (case["name"] + ".case")), str(tmp_path / (case["name"] + ".out"))
            gh.dump(cf, a)
            res = subprocess.run([exe, cf, of], capture_output=True, text=True)
            assert res.returncode == 0 and "mdm gen ok" in res.stdout, (case["name"], res.returncode, res.stderr[-3000:])
            enc2, dec2 = gh.read_program_output(of, a)
            for k in enc:
                assert np.array_equal(bits(enc2[k]), bits(enc[k])), (case["name"], k)
            for k in (dec or {}):
                assert np.array_equal(bits(dec2[k]), bits(dec[k])), (case["name"], k)


# ------------------------------------------------------------------------------------------------------------------- the library
def test_exports_sizes_and_abi(hostlib):
    from parc_amd import _hip, _hip_mdm_gen as H
    names = ("parc_mdm_gen_encode", "parc_mdm_gen_decode", "parc_mdm_gen_abi")
    assert set(names) <= set(_hip.EXPORTED)
    assert "parc_mdm_gen.hip" in _hip.SOURCES and "parc_mdm_gen.hip" in _hip.DIAG_SOURCES
    assert "-ffp-contract=off" in _hip.OPT_LEVEL["parc_mdm_gen.hip"].split()
    L = _hip.lib()
    for name in names:
        assert hasattr(L, name), name
    assert L.parc_mdm_gen_abi() == 1
    sizes = (ctypes.c_int * 3)()
    assert gh.host_lib(hostlib).mdm_gen_struct_sizes(sizes) == 3
    assert tuple(sizes) == (ctypes.sizeof(H.MdmGenCfgS), ctypes.sizeof(_hip.CharModelS), ctypes.sizeof(_hip.TerrainS))
    # the LDS of an encode workgroup: 4 * T * (11 * num_bodies - 4) bytes; 101 previous frames of the humanoid fit, 102 do not
    from parc_amd.anim import kin_char_model as kcm
    model = kcm.KinCharModel("cpu")
    model.load_char_file(kcm.default_char_file())
    c = H.MdmGenCfgS()
    for T in (2, 101, 102):
        c.num_frames = T
        assert gh.host_lib(hostlib).mdm_gen_lds_bytes_host(model.c_struct(), c) == 4 * T * (11 * 15 - 4)
    assert 4 * 101 * 161 <= H.MAX_LDS < 4 * 102 * 161


def test_argument_refusals_need_no_gpu(km, g36):
    """every refusal of include/parc_mdm_gen.h in its order, from the library itself: all of them come before any HIP call"""
    from parc_amd import _hip, _hip_mdm_gen as H
    z, meta = g36
    L = _hip.lib()
    a = gh.Args(km, case_of(meta, "shipped"), z)
    one = ctypes.c_void_p(8)          # a non-NULL pointer that is never followed: nothing is launched in this test
    ter = _hip.TerrainS(one, 4, 4, 0.0, 0.0, 1.0, 1.0)
    NE, ND = 18, 11

    def enc(cfg=None, model=None, B=2, ptrs=None, terrain=ter):
        return L.parc_mdm_gen_encode(None, model if model is not None else a.model, cfg if cfg is not None else a.cfg_enc, terrain, B,
                                     *([one] * NE if ptrs is None else ptrs))

    def dec(cfg=None, model=None, B=2, ptrs=None):
        return L.parc_mdm_gen_decode(None, model if model is not None else a.model, cfg if cfg is not None else a.cfg_dec, B,
                                     *([one] * ND if ptrs is None else ptrs))

    def with_(c, **kw):
        c = copy.copy(c)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    ce, cd = a.cfg_enc, a.cfg_dec
    # 1. EINVAL: counts and configurations that name no layout
    for c in (with_(ce, num_prev_states=0), with_(ce, num_prev_states=3), with_(ce, dim_x=0), with_(ce, dim_y=0), with_(ce, feat_dim=a.D + 1),
              with_(ce, off_contacts=ce.off_contacts - 1), with_(ce, z_style=2), with_(ce, rot_type=3), with_(ce, rot_type=H.ROT_QUAT)):
        assert enc(cfg=c) == H.EINVAL          # (the last: D = 91 is no tiling with quaternions)
    for c in (with_(cd, seq_len=1), with_(cd, num_prev_states=0), with_(cd, feat_dim=a.D - 1), with_(cd, dim_x=0)):
        assert dec(cfg=c) == H.EINVAL
    assert enc(B=-1) == dec(B=-1) == H.EINVAL
    m = copy.copy(a.model)
    m.parent[3] = 5
    assert enc(model=m) == dec(model=m) == H.EINVAL
    # ... also where B == 0 and where pointers are NULL: EINVAL comes first
    assert enc(cfg=with_(ce, dim_x=0), B=0, ptrs=[None] * NE) == dec(cfg=with_(cd, seq_len=1), B=0, ptrs=[None] * ND) == H.EINVAL
    # 2. EUNSUPPORTED: a rot_type-dependent layout that tiles [0, D) but is not DEFAULT; previous frames beyond a workgroup's LDS
    J = a.J
    quat = with_(ce, rot_type=H.ROT_QUAT, feat_dim=3 + 4 + 3 * J + 4 * J + a.nb, off_root_pos=0, off_root_rot=3, off_joint_pos=7, off_joint_rot=7 + 3 * J,
                 off_contacts=7 + 7 * J)
    expm = with_(ce, rot_type=H.ROT_EXP_MAP, feat_dim=6 + 6 * J + a.nb, off_joint_rot=6 + 3 * J, off_contacts=6 + 6 * J)
    for c in (quat, expm):
        assert enc(cfg=c) == enc(cfg=c, B=0, ptrs=[None] * NE) == H.EUNSUPPORTED
        assert dec(cfg=with_(c, seq_len=16)) == dec(cfg=with_(c, seq_len=16), B=0, ptrs=[None] * ND) == H.EUNSUPPORTED
    assert enc(cfg=with_(ce, num_frames=102)) == enc(cfg=with_(ce, num_frames=102), B=0, ptrs=[None] * NE) == H.EUNSUPPORTED          # 4 T (11 * 15 - 4) bytes
    # 3. OK with nothing launched for B == 0, before the pointers are looked at
    assert enc(B=0, ptrs=[None] * NE, terrain=_hip.TerrainS(None, 0, 0, 0.0, 0.0, 0.0, 0.0)) == 0 and dec(B=0, ptrs=[None] * ND) == 0
    # 4. EINVAL for a NULL required pointer.  encode: root_pos, root_rot, joint_rot, contacts, target_world, grid_x, grid_y, mean, std, frame,
    #    out_root_pos, out_root_rot, out_body_pos, hf_z, target, target_dir, prev_state, obs (the last two optional)
    #    (only refusals are asked for with these pointers: an accepted call would launch.  The host build's tests run the accepted
    #    forms: without prev_state and obs, without frames)
    for i in range(16):
        p = [one] * NE
        p[i] = None
        assert enc(ptrs=p) == H.EINVAL, i
    assert enc(terrain=_hip.TerrainS(None, 4, 4, 0.0, 0.0, 1.0, 1.0)) == enc(terrain=_hip.TerrainS(one, 0, 4, 0.0, 0.0, 1.0, 1.0)) == H.EINVAL
    #    decode: x, prev_state, no_noise, mean, std, frame, root_pos, root_rot, joint_rot, contacts, frames (the last optional)
    for i in range(10):
        p = [one] * ND
        p[i] = None
        assert dec(ptrs=p) == H.EINVAL, i          # prev_state without no_noise (or the reverse) is refused too
    nocon = gh.Args(km, case_of(meta, "no_pos_con"), z)
    assert dec(cfg=nocon.cfg_dec) == H.EINVAL          # contacts given for a layout without


# ------------------------------------------------------------------------------------------------------------------- the env's callable
def test_generator_callable_and_plan_rows(km, g36):
    """MDMGenerator around a stand-in with ddim_inference: the attributes MotionGenDeepMimicEnv reads, the env's settings carried over,
    the plan of gen_mdm_motion, and `frames` = the rows the env's three conversions give (here in torch ops), which the env takes as
    they are."""
    from parc_amd.diffusion import diffusion_util as du, gen_util
    from parc_amd.envs.ig_parkour import mgdm_env
    from parc_amd.util import torch_util
    z, meta = g36
    case = case_of(meta, "shipped")
    tw, prev, s = gh.call_inputs(case, z)
    ter = gh.fixture_terrain(z)
    m = gh.stand_in(case, z)
    gen = gen_util.MDMGenerator(m)
    assert (gen._num_prev_states, gen._sequence_fps, gen._dx, gen._dy, gen._num_x_neg, gen._num_x_pos, gen._num_y_neg, gen._num_y_pos, gen._target_type.name) == \
        (2, 30, 0.2, 0.2, 10, 20, 15, 15, "XY_DIR")
    es = mgdm_env.MDMGenSettings()          # what replan() sets
    es.ddim_stride, es.use_cfg, es.cfg_scale = 100, True, 0.3
    es.use_prev_state = torch.tensor([True, False, True])
    es.prev_state_ind_key = torch.tensor([True, False, True])
    plan = gen(tw, prev, ter, km, es)
    kind, conds, stride = m.calls[-1]
    K = du.MDMKeyType
    assert (kind, stride) == ("ddim", 100) and conds[K.GUIDANCE_PARAMS].obs_cfg_scale == 0.3 and conds[K.GUIDANCE_PARAMS].target_xy is None
    assert conds[K.PREV_STATE_FLAG_KEY] is es.prev_state_ind_key and conds[K.PREV_STATE_NOISE_IND_KEY] is es.use_prev_state
    s.target_guidance = False
    want = gen_util.gen_mdm_motion(tw, prev, ter, m, km, s, io=gh.make_io(km, case, z, path="torch"))
    for k in ("root_pos", "root_rot", "joint_rot", "contacts", "frames"):
        assert torch.equal(getattr(plan, k), getattr(want, k)), k
    rows = torch.cat([plan.root_pos, torch_util.quat_to_exp_map(plan.root_rot), gen._io._features._rot_to_dof(plan.joint_rot)], dim=-1)
    assert plan.frames.shape == (3, 16, 34) and torch.equal(plan.frames, rows)

    class Gen:
        _num_prev_states, _sequence_fps = 2, 30
        _dx = _dy = 0.4
        _num_x_neg, _num_x_pos, _num_y_neg, _num_y_pos = 2, 5, 3, 3
    import json
    from conftest import golden
    cfg = json.loads(bytes(golden("g21_mgdm")["config_json"]).decode())
    env = mgdm_env.MotionGenDeepMimicEnv(cfg, 3, "cpu", False, km, generator=Gen())
    assert env._plan_rows(plan) is plan.frames
