"""Stage 2's motion optimiser against fixture G20, which the REFERENCE's tools/motion_opt/motion_optimization.py
produced on CPU (tests/golden/gen_golden.py stage motion-opt): body constraints from contact labels (:34-181), the nine loss terms +
total + autograd gradient (:183-395) and a 40-iteration Adam descent (:404-500)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from test_hip_parity import DEV, T, close, km  # noqa: F401  (km is a fixture)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import moopt_host as mh      # noqa: E402

pytestmark = pytest.mark.gpu

W_NAMES = ("w_root_pos", "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding", "w_body_constraints", "w_jerk")


def _problem(g):
    from parc_amd.util import terrain_util
    counts = g["pts_count"].tolist()
    pts, s = [], 0
    for n in counts:
        pts.append(T(g["pts"][s:s + n]))
        s += n
    ter = terrain_util.SubTerrain.from_arrays(g["hf"], g["min_point"], g["dxdy"], device=DEV)
    w = dict(zip(W_NAMES, [float(v) for v in g["weights"][:9]]))
    return pts, ter, w, float(g["weights"][9])


def _source_terms(km, src):
    from parc_amd.util import torch_util
    rp, rq = src[:, 0:3].contiguous(), torch_util.exp_map_to_quat(src[:, 3:6])
    jr = km.dof_to_rot(src[:, 6:].contiguous())
    bp, br = km.forward_kinematics(rp, rq, jr)
    return rp, rq, jr, bp[1:] - bp[:-1], torch_util.quat_diff_angle(br[1:], br[:-1])


def test_g20_body_constraints_from_contact_labels(km):
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.util import torch_util
    g = golden("g20_motion_opt")
    pts, ter, w, max_jerk = _problem(g)
    src, con = T(g["src_frames"]), T(g["contacts"])
    bc = mo.compute_approx_body_constraints(src[:, 0:3].contiguous(), torch_util.exp_map_to_quat(src[:, 3:6]), km.dof_to_rot(src[:, 6:].contiguous()),
                                            con, km, ter)
    rows = np.array([[b, c.start_frame_idx, c.end_frame_idx] + c.constraint_point.tolist() for b, lst in enumerate(bc) for c in lst])
    ref = g["body_constraints"]
    assert rows.shape == ref.shape and len(ref) >= 4
    assert np.array_equal(rows[:, 0:3], ref[:, 0:3])                 # bodies and frame ranges: exact (incl. the dropped one-frame run)
    # the points are the end of a 1000-step descent onto the column surfaces
    assert np.abs(rows[:, 3:6] - ref[:, 3:6]).max() < 2e-4, np.abs(rows[:, 3:6] - ref[:, 3:6]).max()
    assert {int(r[0]) for r in ref} >= {km.get_body_id("left_foot"), km.get_body_id("left_hand")}


@pytest.mark.parametrize("case", ["full", "nocon"])
def test_g20_loss_terms_and_gradient(km, case):
    from parc_amd.tools.motion_opt import motion_optimization as mo
    g = golden("g20_motion_opt")
    pts, ter, w, max_jerk = _problem(g)
    src, con, tgt = T(g["src_frames"]), T(g["contacts"]), T(g["tgt_frames"])
    bc = mh.constraints_from_rows(g["body_constraints"], km.get_num_joints(), DEV) if case == "full" else None
    if case == "nocon":
        w = dict(w, w_contact=0.0, w_sliding=0.0)
    a, b, c = (tgt[:, 0:3].clone().requires_grad_(True), tgt[:, 3:6].clone().requires_grad_(True), tgt[:, 6:].clone().requires_grad_(True))
    loss, ld = mo.motion_terrain_contact_loss(a, b, c, *_source_terms(km, src), con, ter, pts, km, body_constraints=bc, max_jerk=max_jerk, **w)
    loss.backward()
    ref_terms = dict(zip([mo.LossType(int(i)) for i in g[case + "_term_ids"]], g[case + "_terms"]))
    for k, r in ref_terms.items():
        assert abs(ld[k] - r) <= 2e-4 * max(abs(r), 1e-2), (k, ld[k], r)
    if case == "full":
        assert all(ref_terms[k] > 0 for k in ref_terms), ref_terms       # every term is exercised
    ref_loss = float(g[case + "_loss"])
    assert abs(loss.item() - ref_loss) <= 2e-4 * abs(ref_loss), (loss.item(), ref_loss)
    got = torch.cat([a.grad, b.grad, c.grad], dim=-1).cpu().numpy()
    ref = g[case + "_grad"]
    # penalty terms are sums of |.| and clamps: a sample point within rounding of a kink (or of two columns) may take the other branch,
    # which moves single entries by one point's weight; the bulk must agree
    scale = np.abs(ref).max()
    err = np.abs(got - ref)
    assert np.median(err) < 1e-4 * scale, (np.median(err), scale)
    assert (err > 2e-3 * scale).mean() < 0.01, ((err > 2e-3 * scale).mean(), err.max(), scale)
    cos = float((got * ref).sum() / np.sqrt((got ** 2).sum() * (ref ** 2).sum()))
    assert cos > 0.9995, cos


def test_g20_descent_follows_the_reference(km):
    """40 Adam iterations: the loss of every iteration against the reference's run, eagerly and as a replayed hipGraph.  Adam's first
    steps move every entry by the step size whatever the size of its gradient, so entries whose gradient is rounding noise end up
    anywhere within +-40 steps: the loss curve is the meaningful comparison, the frames are compared in the bulk."""
    from parc_amd.tools.motion_opt import motion_optimization as mo
    g = golden("g20_motion_opt")
    pts, ter, w, max_jerk = _problem(g)
    bc = mh.constraints_from_rows(g["body_constraints"], km.get_num_joints(), DEV)
    ref = g["opt_loss_trace"]
    assert ref[-1] < 0.5 * ref[0]                                    # the descent does reduce the loss
    moved = np.abs(g["opt_frames"] - g["src_frames"]).max()
    assert moved > 0.01
    traces = {}
    for use_graph in (False, True):
        trace = []
        out = mo.motion_contact_optimization(src_frames=T(g["src_frames"]), contacts=T(g["contacts"]), body_points=pts, terrain=ter, char_model=km,
                                             num_iters=40, step_size=0.001, body_constraints=bc, max_jerk=max_jerk, exp_name="g20", use_wandb=False,
                                             log_file=None, use_graph=use_graph, verbose=False, loss_trace=trace, **w)
        got = trace[0].cpu().numpy()
        assert got.shape == ref.shape == (40,)
        rel = np.abs(got - ref) / ref
        assert rel[0] < 2e-4 and rel.max() < 2e-2, (use_graph, rel[0], rel.max())
        d = np.abs(out.cpu().numpy() - g["opt_frames"])
        assert np.median(d) < 0.05 * moved and np.quantile(d, 0.9) < 0.25 * moved, (use_graph, moved, np.median(d), np.quantile(d, 0.9))
        traces[use_graph] = got
    # the replayed graph is the same computation as the eager launches
    assert np.abs(traces[True] - traces[False]).max() <= 2e-3 * ref[0], np.abs(traces[True] - traces[False]).max()


def test_pose_chain_kernels_equal_the_torch_chain(km):
    """parc_pose_chain_forward / _backward against exp_map_to_quat + dof_to_rot_torch + forward_kinematics_torch and their autograd:
    values, and the vector-Jacobian product for random cotangents on all four outputs (incl. wrapped angles > pi and a near-zero map)."""
    from parc_amd.util import torch_util
    torch.manual_seed(4)
    n, D = 96, km.get_dof_size()
    rp = torch.randn((n, 3), device=DEV)
    re = 0.8 * torch.randn((n, 3), device=DEV)
    dof = 0.7 * torch.randn((n, D), device=DEV)
    re[0] = torch.tensor([0.0, 0.0, 4.0])            # angle beyond pi: wrapped
    re[1] = torch.tensor([2e-6, 0.0, 1e-6])          # below the small-angle threshold: identity, zero gradient
    dof[2, 0:3] = torch.tensor([3.5, 0.2, -0.1])
    ins = [x.clone().requires_grad_(True) for x in (rp, re, dof)]
    ref_in = [x.clone().requires_grad_(True) for x in (rp, re, dof)]
    out = km.pose_chain(*ins)
    rq = torch_util.exp_map_to_quat(ref_in[1])
    jr = km.dof_to_rot_torch(ref_in[2])
    bp, br = km.forward_kinematics_torch(ref_in[0], rq, jr)
    ref = (rq, jr, bp, br)
    for a, b, name in zip(out, ref, ("root_quat", "joint_rot", "body_pos", "body_rot")):
        assert a.shape == b.shape
        close(a, b.detach().cpu().numpy(), atol=3e-6, rtol=0)
    cot = [torch.randn_like(o) for o in out]
    torch.autograd.backward(out, cot)
    torch.autograd.backward(ref, cot)
    for a, b, name in zip(ins, ref_in, ("root_pos", "root_exp", "dof")):
        ga, gb = a.grad, b.grad
        scale = float(gb.abs().max())
        err = float((ga - gb).abs().max())
        assert err <= 2e-5 * scale, (name, err, scale)
    assert float(ins[1].grad[1].abs().max()) == 0.0


def test_pose_chain_and_sdf_edge_cases(km, oracle):
    """Ragged and degenerate inputs of the two kernels the optimiser leans on: empty / single / non-multiple-of-64 batches of the pose
    chain, and the windowed terrain query for points far outside the field, on its border, at a NaN coordinate and on a one-cell field."""
    from parc_amd.util import terrain_util
    D = km.get_dof_size()
    for n in (0, 1, 65):
        rp = torch.randn((n, 3), device=DEV, requires_grad=True)
        re = (0.5 * torch.randn((n, 3), device=DEV)).requires_grad_(True)
        dof = (0.5 * torch.randn((n, D), device=DEV)).requires_grad_(True)
        rq, jr, bp, br = km.pose_chain(rp, re, dof)
        assert rq.shape == (n, 4) and jr.shape == (n, 14, 4) and bp.shape == (n, 15, 3) and br.shape == (n, 15, 4)
        (bp.sum() + br.sum() + rq.sum() + jr.sum()).backward()
        assert rp.grad.shape == (n, 3) and torch.isfinite(dof.grad).all()
        if n:
            close(bp[:, 0], rp.detach().cpu().numpy(), atol=0, rtol=0)
            assert float((rp.grad - 15.0).abs().max()) < 1e-4            # every body position carries the root translation once
    rng = np.random.default_rng(9)
    X, Y = 23, 17
    hf = rng.uniform(-1, 1, size=(1, X, Y)).astype(np.float32)
    mbc = np.array([[0.3, -0.2]], np.float32)
    dxdy = np.array([0.4, 0.25], np.float32)
    far = rng.uniform(-400, 400, size=(1, 300, 3)).astype(np.float32)         # hundreds of cells away: the window covers the whole field
    near = np.concatenate([rng.uniform(-1, 10, size=(1, 300, 1)), rng.uniform(-1, 5, size=(1, 300, 1)), rng.uniform(-3, 3, size=(1, 300, 1))], axis=-1)
    edge = np.array([[[0.3, -0.2, 0.0], [0.3 + 0.4 * (X - 1), -0.2 + 0.25 * (Y - 1), 5.0], [0.3 - 0.2, -0.2 - 0.125, -20.0], [0.5, 0.05, 1e6]]], np.float32)
    for pts in (far, near.astype(np.float32), edge):
        for kw in ({}, dict(inverted=False), dict(inverted=False, radius=0.1)):
            got = terrain_util.points_hf_sdf(T(pts), T(hf), T(mbc), T(dxdy), **kw)
            want = oracle.points_hf_sdf(pts, hf, mbc, dxdy, **kw)
            close(got, want, atol=1e-6, rtol=2e-7)
    bad = near.astype(np.float32).copy()
    bad[0, 0, 0] = np.nan
    out = terrain_util.points_hf_sdf(T(bad), T(hf), T(mbc), T(dxdy))
    assert torch.isnan(out[0, 0]) and torch.isfinite(out[0, 1:]).all()
    one = terrain_util.points_hf_sdf(T(near.astype(np.float32)), T(hf[:, :1, :1]), T(mbc), T(dxdy))
    close(one, oracle.points_hf_sdf(near.astype(np.float32), hf[:, :1, :1], mbc, dxdy), atol=1e-6, rtol=2e-7)


def test_body_points_world_kernels_equal_the_torch_formula(km):
    """parc_body_points_world / _grad against pos[owner] + quat_rotate(rot[owner], local) and its autograd, incl. a body without points
    and a leading batch dimension."""
    from parc_amd.util import geom_util, terrain_util, torch_util
    torch.manual_seed(7)
    pts = geom_util.get_char_point_samples(km)
    pts[2] = pts[2][:0]                                       # a body that owns no point
    bp = terrain_util.BodyPoints(pts, DEV)
    assert bp.num_points == sum(int(p.shape[0]) for p in pts) and bp.start[3] == bp.start[2]
    B = km.get_num_joints()
    pos = torch.randn((2, 37, B, 3), device=DEV)
    rot = torch.randn((2, 37, B, 4), device=DEV)
    rot = rot / rot.norm(dim=-1, keepdim=True) * (1.0 + 0.01 * torch.randn((2, 37, B, 1), device=DEV))       # not exactly unit, like slerped frames
    a = [pos.clone().requires_grad_(True), rot.clone().requires_grad_(True)]
    b = [pos.clone().requires_grad_(True), rot.clone().requires_grad_(True)]
    w = bp.world(a[0], a[1])
    ref = torch_util.quat_rotate(b[1][..., bp.owner, :], bp.local.expand(2, 37, bp.num_points, 3)) + b[0][..., bp.owner, :]
    assert w.shape == ref.shape == (2, 37, bp.num_points, 3)
    close(w, ref.detach().cpu().numpy(), atol=2e-6, rtol=0)
    cot = torch.randn_like(ref)
    w.backward(cot)
    ref.backward(cot)
    for x, y in zip(a, b):
        assert float((x.grad - y.grad).abs().max()) <= 2e-5 * float(y.grad.abs().max())
    assert float(a[0].grad[..., 2, :].abs().max()) == 0.0 and float(a[1].grad[..., 2, :].abs().max()) == 0.0


def test_quat_diff_angle_kernels_equal_torch():
    """parc_quat_diff_angle / _grad against torch_util.quat_diff_angle and its autograd: random pairs, identical pairs (the zero branch),
    antipodal representatives (w < 0) and a broadcast operand."""
    from parc_amd.util import torch_util
    torch.manual_seed(11)
    a = torch.randn((7, 33, 4), device=DEV)
    b = torch.randn((7, 33, 4), device=DEV)
    a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
    b[0, :5] = a[0, :5]
    b[1, :5] = -a[1, :5] * 1.0
    b[2] = torch_util.quat_mul(torch_util.exp_map_to_quat(1e-3 * torch.randn((33, 3), device=DEV)), a[2])       # small angles
    for q0, q1 in ((a, b), (a[:, :1], b)):
        x = [q0.clone().requires_grad_(True), q1.clone().requires_grad_(True)]
        y = [q0.clone().requires_grad_(True), q1.clone().requires_grad_(True)]
        got, ref = torch_util.quat_diff_angle_fused(*x), torch_util.quat_diff_angle(*y)
        assert got.shape == ref.shape
        close(got, ref.detach().cpu().numpy(), atol=3e-6, rtol=1e-5)
        cot = torch.randn_like(ref)
        got.backward(cot)
        ref.backward(cot)
        for u, v in zip(x, y):
            assert u.grad.shape == v.grad.shape
            assert float((u.grad - v.grad).abs().max()) <= 3e-4 * max(float(v.grad.abs().max()), 1.0), float((u.grad - v.grad).abs().max())


def test_temporal_terms_kernels_equal_torch():
    """parc_temporal_terms / _grad against the torch expressions of the smoothness, sliding and jerk terms and their autograd (values
    and the vector-Jacobian product for random cotangents), incl. masked pairs and a jerk limit that clips part of the frames."""
    from parc_amd.tools.motion_opt import motion_optimization as mo
    torch.manual_seed(5)
    for T_, B in ((37, 15), (4, 3), (5, 1)):
        pos = torch.randn((T_, B, 3), device=DEV)
        r = torch.rand((T_ - 1, B), device=DEV)
        s_bv = 0.3 * torch.randn((T_ - 1, B, 3), device=DEV)
        keep = (torch.rand((T_ - 1, B), device=DEV) > 0.3).float()
        pc = torch.rand((T_ - 1, B), device=DEV)
        lim = 1.5
        a = [pos.clone().requires_grad_(True), r.clone().requires_grad_(True)]
        b = [pos.clone().requires_grad_(True), r.clone().requires_grad_(True)]
        got = mo._TemporalTerms.apply(a[0], a[1], s_bv, keep, pc, lim)
        v = b[0][1:] - b[0][:-1]
        e2 = torch.square(v - s_bv)
        c, c2 = 0.03, 0.0009
        smooth = e2.sum() + b[1].sum()
        slide = ((torch.sqrt((e2 * keep.unsqueeze(-1)).sum(-1) + c2) - c) * pc).sum() + ((torch.sqrt(b[1] * keep + c2) - c) * pc).sum()
        acc = v[1:] - v[:-1]
        jl = torch.clamp(torch.linalg.vector_norm(acc[1:] - acc[:-1], dim=-1) - lim, min=0.0).sum()
        ref = torch.stack([smooth, slide, jl])
        close(got, ref.detach().cpu().numpy(), atol=1e-4, rtol=2e-5)
        assert float(jl.detach()) > 0 or T_ < 37
        cot = torch.tensor([1.3, -0.7, 2.1], device=DEV)
        got.backward(cot)
        ref.backward(cot)
        for x, y in zip(a, b):
            assert float((x.grad - y.grad).abs().max()) <= 3e-5 * max(float(y.grad.abs().max()), 1.0), float((x.grad - y.grad).abs().max())
