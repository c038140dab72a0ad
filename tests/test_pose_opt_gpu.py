"""The four differentiable primitives of stage 2's motion optimiser (parc_amd/csrc/parc_pose_opt.hip and the shared bodies of
parc_moopt_core.h) through their Python surfaces, against float64: the float64 record on the designed inputs of fixture
G34 (tests/golden/gen_pose_opt.py) and, at other batch sizes, tests/tools/pose_opt_ref.py (pinned by tests/test_pose_opt_ref_cpu.py).

Bounds: e-bar is |torch fp32 - float64| on the CPU over G34 (pose_opt_ref.MEASURED_*: the reference's own code, and for the
frame-to-frame terms a restatement of its expressions); the kernels get 4 e-bar, the torch fp32 path on the device 2 e-bar.  The pose
chain's values: the kernels 4 e-bar of each output, the torch path 2 e-bar of the primitive (why: pose_opt_ref).  Values are compared absolutely, gradients relative to the frame's (pair's) largest float64 entry of that input
tensor, the angle's gradient per decade of |v|.  Where the float64 gradient of a whole frame is zero the kernel's must be exactly zero.

One documented difference: for an exactly zero root exponential map autograd (the reference's too) returns NaN in g_root_exp (0 / 0
through torch.where); the kernel returns 0.
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from test_hip_parity import DEV, T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import moopt_host as mh  # noqa: E402
import pose_opt_ref as por  # noqa: E402

pytestmark = pytest.mark.gpu
K, KT = por.DEVICE_FACTOR, por.TORCH_FACTOR
SEEDS = {"hum": 3410, "syn": 3420}
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0], np.float32)


@pytest.fixture(scope="module")
def z():
    return golden("g34_pose_opt")


@pytest.fixture(scope="module")
def chars():
    """name -> (model on the device, its float64 copy on the host)"""
    out = {}
    for name in por.CHARS:
        km = por.load_char(name, DEV)
        out[name] = (km, por.f64_model(km))
    return out


def _np(x):
    return x.detach().cpu().numpy()


def _check_value(got, ref64, ebar, factor, what):
    err = por.value_error(got, ref64)
    print("{:44s} err {:.3e}  bound {:.3e} ({:g} e-bar)".format(what, err, factor * ebar, factor))
    assert got.shape == ref64.shape and err <= factor * ebar, (what, err, factor * ebar)


def _check_grad(got, ref64, ebar, factor, what):
    rel, dead = por.grad_error(got, ref64)
    print("{:44s} rel {:.3e}  bound {:.3e} ({:g} e-bar)  all-zero rows {}".format(what, rel, factor * ebar, factor, int(dead.sum())))
    assert got.shape == ref64.shape and rel <= factor * ebar, (what, rel, factor * ebar)
    assert (np.asarray(got).reshape(len(ref64), -1)[dead] == 0.0).all(), what + ": a frame whose float64 gradient is zero"


# ------------------------------------------------------------------------------------------------------------------ pose chain
def _pose_chain_device(km, rp, re, dof, cots):
    x = [T(a).requires_grad_(True) for a in (rp, re, dof)]
    out = km.pose_chain(*x)
    g = torch.autograd.grad(out, x, [T(cots[k]) for k in por.OUTS])
    return dict(zip(por.OUTS, (_np(o) for o in out))), dict(zip(por.INS, (_np(v) for v in g)))


@pytest.mark.parametrize("c", por.CHARS)
def test_pose_chain_kernels_on_g34(z, chars, c):
    km, _ = chars[c]
    rp, re, dof = (z["{}_{}".format(c, k)] for k in por.INS)
    cots = {k: z["{}_cot_{}".format(c, k)] for k in por.OUTS}
    for run in por.RUNS:
        outs, grads = _pose_chain_device(km, rp, re, dof, por.run_cotangents(cots, run))
        if run == "all":
            for k in por.OUTS:
                _check_value(outs[k], z["{}_f64_{}".format(c, k)], por.MEASURED_POSE_VALUE_BY_OUTPUT[k], K, "{} {}".format(c, k))
            # the sign rule: the root quaternion is the float64 one and not its negative, on every frame
            assert ((outs["root_quat"].astype(np.float64) * z[c + "_f64_root_quat"]).sum(axis=1) > 0.99).all()
            first = (outs, grads)
        for k in por.INS:
            ref = z["{}_f64_{}_g_{}".format(c, run, k)]
            if k == "root_exp":
                ref = por.expected_root_exp_grad(ref, re)
            _check_grad(grads[k], ref, por.MEASURED_POSE_GRAD[k], K, "{} run {} g_{}".format(c, run, k))
    outs, grads = first
    # branch selection is exact.  Frame 0 (5e-6, below the threshold): identity and a zero gradient, on the root and on the spherical
    # joint that carries the angle; frames 1, 10, 11 (2e-5, 2 pi -+ 2e-5, above it): neither.
    sph = por.spherical_joints(km)
    j0, d0 = sph[0], km.get_joint_dof_idx(sph[0])
    assert np.array_equal(outs["root_quat"][0], IDENTITY) and (grads["root_exp"][0] == 0.0).all()
    assert np.array_equal(outs["joint_rot"][0, j0 - 1], IDENTITY) and (grads["dof"][0, d0:d0 + 3] == 0.0).all()
    for f in (1, 10, 11):
        j, d = sph[f % len(sph)], km.get_joint_dof_idx(sph[f % len(sph)])
        assert np.abs(outs["root_quat"][f, :3]).max() > 5e-6 and np.abs(grads["root_exp"][f]).max() > 1e-3, f
        assert np.abs(outs["joint_rot"][f, j - 1, :3]).max() > 5e-6 and np.abs(grads["dof"][f, d:d + 3]).max() > 1e-3, f
    # the zero map: gradient exactly 0 (the reference: NaN), and the other frames of the launch do not notice the frame
    zf = por.ZERO_FRAME
    assert (re[zf] == 0.0).all() and (grads["root_exp"][zf] == 0.0).all() and np.array_equal(outs["root_quat"][zf], IDENTITY)
    assert np.isnan(z[c + "_f64_all_g_root_exp"][zf]).all() and np.isnan(z[c + "_f32_all_g_root_exp"][zf]).all()
    re2 = re.copy()
    re2[zf] = [0.3, -0.2, 0.5]
    outs2, grads2 = _pose_chain_device(km, rp, re2, dof, cots)
    others = np.arange(re.shape[0]) != zf
    assert all(np.array_equal(outs[k][others], outs2[k][others]) for k in por.OUTS)
    assert all(np.array_equal(grads[k][others], grads2[k][others]) for k in por.INS)
    assert np.abs(grads2["root_exp"][zf]).max() > 1e-3


@pytest.mark.parametrize("c", por.CHARS)
def test_pose_chain_torch_path_on_device(z, chars, c):
    km, _ = chars[c]
    rp, re, dof = (z["{}_{}".format(c, k)] for k in por.INS)
    cots = {k: z["{}_cot_{}".format(c, k)] for k in por.OUTS}
    outs, grads = por.pose_chain(km, rp, re, dof, cots=cots, dtype=torch.float32, device=DEV)
    for k in por.OUTS:
        _check_value(outs[k], z["{}_f64_{}".format(c, k)], por.MEASURED_POSE_VALUE, KT, "torch {} {}".format(c, k))
    for k in por.INS:
        ref, got = z["{}_f64_all_g_{}".format(c, k)], grads[k]
        if k == "root_exp":                             # the torch path keeps the reference's NaN at the zero map
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            ref, got = np.delete(ref, por.ZERO_FRAME, axis=0), np.delete(got, por.ZERO_FRAME, axis=0)
        _check_grad(got, ref, por.MEASURED_POSE_GRAD[k], KT, "torch {} g_{}".format(c, k))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("c", por.CHARS)
def test_pose_chain_shape_sweep(chars, c, n):
    """workgroups of 64 frames: one frame, one short of a workgroup, one full, one over, two and one over"""
    km, km64 = chars[c]
    rp, re, dof = por.pose_chain_inputs(km, n, SEEDS[c] + 7)
    assert por.pose_conditions(km, re, dof) == []
    cots = por.pose_chain_cotangents(km, n, SEEDS[c] + 8)
    want_o, want_g = por.pose_chain(km64, rp, re, dof, cots=cots)
    outs, grads = _pose_chain_device(km, rp, re, dof, cots)
    for k in por.OUTS:
        _check_value(outs[k], want_o[k], por.MEASURED_POSE_VALUE_BY_OUTPUT[k], K, "{} n={} {}".format(c, n, k))
    for k in por.INS:
        ref = por.expected_root_exp_grad(want_g[k], re) if k == "root_exp" else want_g[k]
        _check_grad(grads[k], ref, por.MEASURED_POSE_GRAD[k], K, "{} n={} g_{}".format(c, n, k))


def _kernel_count(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name])


def test_empty_batches_and_the_body_limit(chars):
    from parc_amd import _hip
    km, _ = chars["syn"]
    L, st, cs = _hip.lib(), _hip.stream(), km.c_struct()
    assert cs.num_bodies == 16 == _hip.MAX_BODIES                  # the 16-body tree passes model_ok (every test above launches with it)
    B, D = 16, km.get_dof_size()
    # empty batches: the shapes come out and nothing is launched
    x = [torch.zeros((0, k), device=DEV, requires_grad=True) for k in (3, 3, D)]
    out = km.pose_chain(*x)
    assert [tuple(o.shape) for o in out] == [(0, 4), (0, B - 1, 4), (0, B, 3), (0, B, 4)]
    g = torch.autograd.grad(out, x, [torch.zeros_like(o) for o in out])
    assert [tuple(v.shape) for v in g] == [(0, 3), (0, 3), (0, D)]
    q = torch.zeros((0, 4), device=DEV, requires_grad=True)
    assert tuple(torch_util_fused(q, q).shape) == (0,)
    buf = torch.full((64,), -7.0, device=DEV)
    ibuf = torch.zeros((64,), dtype=torch.int32, device=DEV)
    p, ip = _hip.ptr(buf), _hip.ptr(ibuf)

    def empty_calls():
        rcs = [L.parc_pose_chain_forward(st, cs, 0, p, p, p, p, p, p, p), L.parc_pose_chain_backward(st, cs, 0, p, p, p, p, p, p, p, p, p),
               L.parc_quat_diff_angle(st, 0, p, p, p), L.parc_quat_diff_angle_grad(st, 0, p, p, p, p, p),
               L.parc_body_points_world(st, 0, 15, 37, p, p, p, ip, p), L.parc_body_points_world_grad(st, 0, 15, 37, p, p, ip, p, p, p),
               L.parc_temporal_terms(st, 0, 15, p, p, p, p, p, 0.03, 0.0009, 7.0, p), L.parc_temporal_terms_grad(st, 0, 15, p, p, p, p, p, 0.03, 0.0009, 7.0, p, p, p)]
        assert rcs == [0] * 8, rcs

    assert _kernel_count(empty_calls) == 0
    # a 17th body: the loader refuses the tree, and the entry points refuse the struct before anything is written
    import tempfile
    from parc_amd.anim.kin_char_model import KinCharModel
    with tempfile.TemporaryDirectory() as d, pytest.raises(AssertionError):
        KinCharModel(DEV).load_char_file(por.write_synthetic(os.path.join(d, "tree17.xml"), extra_leaf=True))
    s17 = type(cs).from_buffer_copy(cs)
    s17.num_bodies = 17
    n = 2
    ins = [torch.zeros((n, k), device=DEV) for k in (3, 3, D)]
    outs = [torch.full((n * 17 * 4,), -7.0, device=DEV) for _ in range(4)]
    rc = L.parc_pose_chain_forward(st, s17, n, *[_hip.ptr(t) for t in ins + outs])
    assert rc == -1                                                 # PARC_EINVAL
    gin = [torch.zeros((n * 17 * 4,), device=DEV) for _ in range(4)]
    gout = [torch.full((n * 64,), -7.0, device=DEV) for _ in range(3)]
    rc = L.parc_pose_chain_backward(st, s17, n, _hip.ptr(ins[1]), _hip.ptr(ins[2]), *[_hip.ptr(t) for t in gin + gout])
    assert rc == -1
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs + gout) and bool((buf == -7.0).all())


def torch_util_fused(q0, q1):
    from parc_amd.util import torch_util
    return torch_util.quat_diff_angle_fused(q0, q1)


# ------------------------------------------------------------------------------------------------------------------ angle
def _angle_device(q0, q1, cot):
    a, b = T(q0).requires_grad_(True), T(q1).requires_grad_(True)
    ang = torch_util_fused(a, b)
    ga, gb = torch.autograd.grad(ang, (a, b), T(cot))
    return _np(ang), _np(ga), _np(gb)


def _check_angle(ang, g0, g1, q0, q1, cot, ref, factor, what, g0_pairs=None):
    """ref = float64 (angle, g_q0, g_q1) with q0 expanded to the pairs"""
    s, _ = por.pair_difference(q0, q1)
    below = s < por.THRESHOLD
    _check_value(ang, ref[0], por.MEASURED_ANGLE_VALUE, factor, what + " angle")
    # branch selection is exact: zero value and zero gradient below the threshold, neither above it
    assert (ang[below] == 0.0).all() and (ang[~below] > 0.0).all() and (g1[below] == 0.0).all() and (np.abs(g1[~below]).max(axis=1) > 0).all()
    bound = factor * np.array(por.MEASURED_ANGLE_GRAD_DECADE)
    e1 = por.angle_grad_by_decade(g1, ref[2], s)
    print("{:44s} per decade {}  bounds {}".format(what + " g_q1", " ".join("%.3e" % v for v in e1), " ".join("%.3e" % v for v in bound)))
    assert (e1 <= bound).all(), (what, e1, bound)
    if g0.shape == g1.shape:
        assert (g0[below] == 0.0).all()
        e0 = por.angle_grad_by_decade(g0, ref[1], s)
        print("{:44s} per decade {}".format(what + " g_q0", " ".join("%.3e" % v for v in e0)))
        assert (e0 <= bound).all(), (what, e0, bound)
    else:
        # the broadcast operand: the same path with q0 expanded gives every pair's own g_q0, held per decade like g_q1; the broadcast
        # kernel launch's g_q0 is the fp32 sum of those n rows, in some order: within (n - 1) 2^-24 sum |row| of their float64 sum
        assert g0.shape == (1, 4) and g0_pairs.shape == g1.shape and (g0_pairs[below] == 0.0).all()
        e0 = por.angle_grad_by_decade(g0_pairs, ref[1], s)
        print("{:44s} per decade {}".format(what + " g_q0 (per pair)", " ".join("%.3e" % v for v in e0)))
        assert (e0 <= bound).all(), (what, e0, bound)
        if factor == K:
            rows = g0_pairs.astype(np.float64)
            err = np.abs(g0[0].astype(np.float64) - rows.sum(axis=0))
            allow = (len(rows) - 1) * 2.0 ** -24 * np.abs(rows).sum(axis=0)
            print("{:44s} err {:.3e}  bound {:.3e} (fp32 sum of {} rows)".format(what + " g_q0 (summed)", err.max(), allow.min(), len(rows)))
            assert (err <= allow).all(), (what, err, allow)
        else:
            # autograd reduces inside the graph, op by op, not the finished rows: only the pairs' bounds added up hold for its sum
            allow = sum(bound[d] * np.abs(ref[1][i]).max() for i, d in enumerate(por.decade_of(s)) if d >= 0)
            err = np.abs(g0.astype(np.float64) - ref[1].sum(axis=0, keepdims=True)).max()
            print("{:44s} err {:.3e}  bound {:.3e} (sum of the pairs')".format(what + " g_q0 (summed)", err, allow))
            assert err <= allow, (what, err, allow)


def test_quat_diff_angle_kernels_on_g34(z):
    for tag in ("ang", "angb"):
        q0, q1, cot = z[tag + "_q0"], z[tag + "_q1"], z[tag + "_cot"]
        if tag == "ang":
            ref = (z["ang_f64_angle"], z["ang_f64_g_q0"], z["ang_f64_g_q1"])
        else:                                           # the pairs' own shares of the summed gradient of the broadcast q0
            ref = (z["angb_f64_angle"], por.quat_diff_angle(np.broadcast_to(q0, q1.shape).copy(), q1, cot)[1][0], z["angb_f64_g_q1"])
            assert por.value_error(ref[1].sum(axis=0, keepdims=True), z["angb_f64_g_q0"]) <= 1e-9
        wide = np.broadcast_to(q0, q1.shape).copy()
        pairs_k = _angle_device(wide, q1, cot)[1] if tag == "angb" else None
        _check_angle(*_angle_device(q0, q1, cot), q0, q1, cot, ref, K, "kernel " + tag, g0_pairs=pairs_k)
        ang, (g0, g1) = por.quat_diff_angle(q0, q1, cot, dtype=torch.float32, device=DEV)
        pairs_t = por.quat_diff_angle(wide, q1, cot, dtype=torch.float32, device=DEV)[1][0] if tag == "angb" else None
        _check_angle(ang, g0, g1, q0, q1, cot, ref, KT, "torch " + tag, g0_pairs=pairs_t)
    # d.w < 0 exactly where the generator put it, and the exact half turns give pi
    s, w = por.pair_difference(z["ang_q0"], z["ang_q1"])
    ang, _, _ = _angle_device(z["ang_q0"], z["ang_q1"], z["ang_cot"])
    half = z["ang_group"] == 2
    assert (w[half] == 0.0).all() and np.abs(ang[half] - np.float32(np.pi)).max() <= 2.4e-7 and (w < 0).sum() > 60


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_quat_diff_angle_shape_sweep(n):
    """workgroups of 256 pairs"""
    q0, q1, cot = por.angle_sweep_inputs(n, seed=n)
    want = por.quat_diff_angle(q0, q1, cot)
    _check_angle(*_angle_device(q0, q1, cot), q0, q1, cot, (want[0],) + want[1], K, "n=%d" % n)


# ------------------------------------------------------------------------------------------------------------------ body points
def test_body_points_kernels_on_g34(z):
    from parc_amd.util import terrain_util
    counts = z["pts_counts"]
    _, start = por.point_tables(counts)
    bp = terrain_util.BodyPoints([T(z["pts_local"][start[b]:start[b + 1]]) for b in range(len(counts))], DEV)
    assert bp.num_points == 37 and bp.start[3] == bp.start[2]
    pos, rot = T(z["pts_pos"]).requires_grad_(True), T(z["pts_rot"]).requires_grad_(True)
    w = bp.world(pos, rot)
    gp, gr = torch.autograd.grad(w, (pos, rot), T(z["pts_cot"]))
    nb = len(counts)
    _check_value(_np(w), z["pts_f64_world"], por.MEASURED_POINTS_VALUE, K, "points world")
    for got, k in ((gp, "body_pos"), (gr, "body_rot")):
        ref = z["pts_f64_g_" + k]
        _check_grad(_np(got).reshape(8, -1), ref.reshape(8, -1), por.MEASURED_POINTS_GRAD[k], K, "points g_" + k)
        assert (_np(got)[..., 2, :] == 0.0).all() and got.shape == (2, 4, nb, ref.shape[-1])        # the body that owns no point
    w32, (gp32, gr32) = por.body_points_world(z["pts_pos"], z["pts_rot"], z["pts_local"], counts, z["pts_cot"], dtype=torch.float32, device=DEV)
    _check_value(w32, z["pts_f64_world"], por.MEASURED_POINTS_VALUE, KT, "torch points world")
    _check_grad(gp32.reshape(8, -1), z["pts_f64_g_body_pos"].reshape(8, -1), por.MEASURED_POINTS_GRAD["body_pos"], KT, "torch points g_body_pos")
    _check_grad(gr32.reshape(8, -1), z["pts_f64_g_body_rot"].reshape(8, -1), por.MEASURED_POINTS_GRAD["body_rot"], KT, "torch points g_body_rot")


# ------------------------------------------------------------------------------------------------------------------ temporal terms
def _tt_single(case):
    from parc_amd.tools.motion_opt import motion_optimization as mo
    pos, r = T(case.pos).requires_grad_(True), T(case.r[:max(case.N - 1, 0)]).requires_grad_(True)
    got = mo._TemporalTerms.apply(pos, r, T(case.sv), T(case.keep), T(case.pc), case.lim)
    gp, gr = torch.autograd.grad(got, (pos, r), T(case.w[:, 0]))
    g_r = np.zeros((case.N, case.B), np.float32)
    g_r[:case.N - 1] = _np(gr)
    return _np(got).reshape(3, 1), _np(gp), g_r


def _tt_seg(case):
    from parc_amd.tools.motion_opt import motion_optimization as mo
    pos, r = T(case.pos).requires_grad_(True), T(case.r).requires_grad_(True)
    got = mo._TemporalTermsSeg.apply(pos, r, T(case.sv), T(case.keep), T(case.pc), case.lim, torch.tensor(case.ss, device=DEV),
                                     torch.tensor(case.sf, device=DEV))
    gp, gr = torch.autograd.grad(got, (pos, r), T(case.w))
    return _np(got), _np(gp), _np(gr)


@pytest.mark.parametrize("name", mh.DESIGNED_TT)
def test_temporal_terms_kernels_on_g34(z, name):
    case = mh.designed_tt(name)
    ref = tuple(z["tt_{}_f64_{}".format(name, k)] for k in ("sums", "g_pos", "g_r"))
    paths = [("seg", _tt_seg(case), K), ("torch", por.temporal_terms_torch(case, dtype=torch.float32, device=DEV), KT)]
    if case.M == 1:
        paths.insert(0, ("single", _tt_single(case), K))
    for what, (sums, g_pos, g_r), factor in paths:
        _check_value(sums, ref[0], por.MEASURED_TT_VALUE, factor, "{} {} sums".format(name, what))
        _check_grad(g_pos, ref[1], por.MEASURED_TT_GRAD["g_pos"], factor, "{} {} g_pos".format(name, what))
        _check_grad(g_r, ref[2], por.MEASURED_TT_GRAD["g_r"], factor, "{} {} g_r".format(name, what))
        for m, T_ in enumerate(case.lengths):                       # a term that does not exist yet is exactly zero
            assert T_ >= 2 or (sums[0, m] == 0.0 and sums[1, m] == 0.0)
            assert T_ >= 4 or sums[2, m] == 0.0
    if name == "kink":
        # on the kink the clamp passes the gradient (torch: x >= min): the frames placed there carry their share of the jerk gradient
        only_jerk = mh.designed_tt("kink")
        only_jerk.w[:2] = 0.0
        _, gp_k, _ = _tt_seg(only_jerk)
        _, gp_ref, _ = only_jerk.float64()
        assert np.abs(gp_ref[0, 0]).max() > 0.1 and np.abs(gp_ref[7, 1]).max() > 0.1
        _check_grad(gp_k, gp_ref, por.MEASURED_TT_GRAD["g_pos"], K, "kink, jerk term alone, g_pos")
    if name == "zero":
        only_jerk = mh.designed_tt("zero")
        only_jerk.w[:2] = 0.0
        sums_z, gp_z, _ = _tt_seg(only_jerk)
        assert (gp_z[:, 0] == 0.0).all() and np.abs(gp_z[:, 1:]).max() > 0.1       # |j| = 0 at limit 0: no gradient and no NaN
