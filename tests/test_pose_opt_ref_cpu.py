"""tests/tools/pose_opt_ref.py pinned without a GPU: it is the yardstick of tests/test_pose_opt_gpu.py, so it has to equal the
float64 record in fixture G34 (the reference's own; for the frame-to-frame terms a torch restatement, which the numpy one here must equal), its gradients have to be the derivatives of its values (central differences), the
designed inputs have to be the fixture's and to meet their conditions, and the e-bars in the module have to be the fixture's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import moopt_host as mh  # noqa: E402
import pose_opt_ref as por  # noqa: E402

H = 1e-6            # step of the central differences
FD_TOL = 1e-7       # relative to the frame's (pair's) largest gradient entry
FAR = 0.999e-3      # "at least 1e-3 from a branch point"; the designed frames at pi +- 1e-3 are 1e-3 away up to their fp32 rounding


@pytest.fixture(scope="module")
def z():
    return golden("g34_pose_opt")


@pytest.fixture(scope="module")
def chars():
    out = {}
    for name in por.CHARS:
        km = por.load_char(name)
        out[name] = (km, por.f64_model(km))
    return out


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == np.float64 and b.dtype == np.float64, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    ok = ~np.isnan(b)
    err = np.abs(a[ok] - b[ok]).max() if ok.any() else 0.0
    tol = 1e-12 * max(1.0, np.abs(b[ok]).max() if ok.any() else 0.0)
    assert err <= tol, (what, err, tol)


def test_synthetic_character_is_what_the_issue_asks_for(chars):
    km, _ = chars["syn"]
    kmt = por.kin_char_model.JointType
    B = km.get_num_joints()
    assert B == 16 == por.kin_char_model._hip.MAX_BODIES
    par = km._parent_indices.tolist()
    kinds = [km._joints[b].joint_type for b in range(B)]
    fixed_with_child = [b for b in range(1, B) if kinds[b] == kmt.FIXED and b in par and kinds[par[b]] != kmt.ROOT]
    assert fixed_with_child and all(kinds[par.index(b)] != kmt.FIXED for b in fixed_with_child)         # a moving child below it
    assert max(par.count(b) for b in range(1, B)) >= 3                                                   # a branching body
    axes = np.stack([km.get_joint(j).axis.numpy() for j in por.hinge_joints(km)])
    assert (np.abs(np.linalg.norm(axes, axis=1) - 1.0) > 0.01).all() and ((axes != 0).sum(axis=1) >= 2).all()      # oblique, not unit
    assert len(por.spherical_joints(km)) >= 4
    lr = km._local_rotation.numpy()[1:]
    assert (np.abs(lr[:, :3]).max(axis=1) > 0).sum() >= 10                                               # non-identity local rotations
    assert kinds[B - 1] == kmt.HINGE and km.get_joint(B - 1).dof_idx == km.get_dof_size() - 1           # the dof vector ends on a hinge
    hum, _ = chars["hum"]
    assert hum.get_num_joints() == 15 and all(abs(float(hum.get_joint(j).axis.norm()) - 1.0) < 1e-6 for j in por.hinge_joints(hum))


def test_designed_inputs_are_the_fixtures_and_meet_their_conditions(z, chars):
    for c, seed in (("hum", 3410), ("syn", 3420)):
        km, _ = chars[c]
        rp, re, dof = por.pose_chain_inputs(km, 64, seed)
        for k, a in zip(por.INS, (rp, re, dof)):
            assert a.dtype == np.float32 and np.array_equal(a, z["{}_{}".format(c, k)]), (c, k)
        cots = por.pose_chain_cotangents(km, 64, seed + 1)
        assert all(np.array_equal(cots[k], z["{}_cot_{}".format(c, k)]) for k in por.OUTS)
        assert por.pose_conditions(km, re, dof) == []
        # every angle of the list on the root, on one spherical joint and on every hinge; the zero map
        raw = np.linalg.norm(por.exp_maps_of(km, re, dof), axis=-1)
        for f, ang in enumerate(por.ANGLES):
            assert abs(raw[f, 0] - ang) < 1e-6 and abs(raw[f, 1 + f % (raw.shape[1] - 1)] - ang) < 1e-6
            assert all(abs(dof[f, km.get_joint_dof_idx(j)] - ang) < 1e-6 for j in por.hinge_joints(km))
        assert (re[por.ZERO_FRAME] == 0.0).all() and (np.abs(re).max(axis=1) == 0.0).sum() == 1
        w = por.wrapped(raw[:len(por.ANGLES), 0])
        assert (w < por.THRESHOLD).sum() == 1 and ((w > por.THRESHOLD) & (w < 3e-5)).sum() == 3          # 5e-6 | 2e-5 and 2 pi -+ 2e-5
        # a prefix of the designed list, and random frames behind it
        assert np.array_equal(por.pose_chain_inputs(km, 5, seed)[1], re[:5])
        assert np.array_equal(por.pose_chain_inputs(km, 129, seed)[1][:por.N_DESIGNED], re[:por.N_DESIGNED])
    a = por.angle_pair_inputs()
    for k, name in (("q0", "ang_q0"), ("q1", "ang_q1"), ("cot", "ang_cot"), ("bq0", "angb_q0"), ("bq1", "angb_q1"), ("bcot", "angb_cot"), ("group", "ang_group")):
        assert np.array_equal(a[k], z[name]), k
    assert a["q0"].shape[0] + a["bq1"].shape[0] == 320 and a["bq0"].shape == (1, 4)
    assert por.angle_conditions(a["q0"], a["q1"]) == [] and por.angle_conditions(a["bq0"], a["bq1"]) == []
    s, w = por.pair_difference(a["q0"], a["q1"])
    g = a["group"]
    assert (w[g == 2] == 0.0).all() and (s[g == 2] == 1.0).all() and (w[g == 1] < 0).all() and (w[g == 0] > 0).all()
    n3 = np.linalg.norm(a["q0"][g == 3].astype(np.float64), axis=1)
    assert np.abs(n3 - 1.0).max() <= 0.0101 and np.abs(n3 - 1.0).max() > 0.005
    dec = por.decade_of(np.concatenate([s, por.pair_difference(a["bq0"], a["bq1"])[0]]))
    assert all((dec == k).sum() >= 16 for k in range(-1, 4))                   # both sides of the threshold and every decade are populated
    p = por.body_points_inputs()
    assert all(np.array_equal(p[k], z["pts_" + k]) for k in p)
    assert p["counts"][2] == 0 and p["pos"].shape[:2] == (2, 4) and 8 * p["local"].shape[0] > 256 and np.abs(np.linalg.norm(p["rot"], axis=-1) - 1).max() > 0.005
    for name in mh.DESIGNED_TT:
        case = mh.designed_tt(name)
        for k, a_ in (("pos", case.pos), ("r", case.r), ("sv", case.sv), ("keep", case.keep), ("pc", case.pc), ("w", case.w)):
            assert np.array_equal(a_, z["tt_{}_{}".format(name, k)]), (name, k)
        assert list(z["tt_{}_lengths".format(name)]) == case.lengths and float(z["tt_{}_lim".format(name)]) == case.lim
        gaps = case.jerk_gaps()
        assert ((gaps == 0.0) | (gaps >= 1e-4)).all(), (name, gaps.min())
    kink, zero = mh.designed_tt("kink"), mh.designed_tt("zero")
    assert (kink.jerk_gaps() == 0.0).sum() >= 2 and kink.lim == 2.5 and zero.lim == 0.0 and (zero.jerk_gaps() == 0.0).sum() == 4
    assert not mh.designed_tt("keep0").keep.any() and not mh.designed_tt("pc0").pc.any()
    assert mh.designed_tt("n270").N * 15 == 270 and mh.designed_tt("seams").lengths[:4] == [1, 2, 3, 4]


def test_module_equals_the_references_float64_record(z, chars):
    for c in por.CHARS:
        _, km64 = chars[c]
        ins = [z["{}_{}".format(c, k)] for k in por.INS]
        cots = {k: z["{}_cot_{}".format(c, k)] for k in por.OUTS}
        for run in por.RUNS:
            outs, grads = por.pose_chain(km64, *ins, cots=por.run_cotangents(cots, run))
            for k in por.OUTS:
                _same(outs[k], z["{}_f64_{}".format(c, k)], (c, k))
            for k in por.INS:
                _same(grads[k], z["{}_f64_{}_g_{}".format(c, run, k)], (c, run, k))
        # the reference's NaN sits in g_root_exp of the zero-map frame and nowhere else, in both precisions
        for prec in ("f32", "f64"):
            g = z["{}_{}_all_g_root_exp".format(c, prec)]
            assert np.isnan(g[por.ZERO_FRAME]).all() and np.isfinite(np.delete(g, por.ZERO_FRAME, axis=0)).all()
            assert np.isfinite(z["{}_{}_all_g_dof".format(c, prec)]).all() and np.isfinite(z["{}_{}_all_g_root_pos".format(c, prec)]).all()
        want = por.expected_root_exp_grad(z[c + "_f64_all_g_root_exp"], z[c + "_root_exp"])
        assert (want[por.ZERO_FRAME] == 0.0).all() and np.isfinite(want).all()
    for tag in ("ang", "angb"):
        ang, (g0, g1) = por.quat_diff_angle(z[tag + "_q0"], z[tag + "_q1"], z[tag + "_cot"])
        _same(ang, z[tag + "_f64_angle"], tag)
        # The gradient holds v / |v| of the difference rotation.  v is a sum of four products in either port of the quaternion product
        # (the reference's has another order of operations): each carries up to 4 * 1.1e-16 of rounding, the two differ by up to
        # 9e-16, and |v| divides that.  1e-12 therefore holds where |v| >= 1e-3; below, the two float64 evaluations may differ by
        # 1e-15 / |v| - the same 1 / |v| that sets the fp32 e-bar per decade.
        s, _ = por.pair_difference(z[tag + "_q0"], z[tag + "_q1"])
        live = s > por.THRESHOLD
        for g, name in ((g0, "_f64_g_q0"), (g1, "_f64_g_q1")):
            ref = z[tag + name]
            assert g.shape == ref.shape and g.dtype == np.float64
            if ref.shape[0] != s.shape[0]:              # the broadcast operand: one summed row
                _same(g / len(s), ref / len(s), tag + name)
                continue
            assert (g[~live] == 0.0).all() and (ref[~live] == 0.0).all()
            err = np.abs(g - ref).max(axis=1)[live]
            tol = 1e-12 * np.maximum(1.0, 1e-3 / s[live]) * np.maximum(1.0, np.abs(ref).max(axis=1)[live])
            assert (err <= tol).all(), (tag + name, float((err / tol).max()))
    w, (gp, gr) = por.body_points_world(z["pts_pos"], z["pts_rot"], z["pts_local"], z["pts_counts"], z["pts_cot"])
    _same(w, z["pts_f64_world"], "world")
    _same(gp, z["pts_f64_g_body_pos"], "g_body_pos")
    _same(gr, z["pts_f64_g_body_rot"], "g_body_rot")
    for name in mh.DESIGNED_TT:
        sums, g_pos, g_r = por.temporal_terms(mh.designed_tt(name))
        _same(sums, z["tt_{}_f64_sums".format(name)], name)
        _same(g_pos, z["tt_{}_f64_g_pos".format(name)], name)
        _same(g_r, z["tt_{}_f64_g_r".format(name)], name)


def _fd_check(grad, fd, rows, what):
    """grad, fd [n, k]; rows: the frames that count"""
    scale = np.abs(grad).max(axis=1)
    err = np.abs(grad - fd).max(axis=1)
    rel = err[rows] / scale[rows]
    print("{}: {} rows, central differences off by at most {:.2e} of the row's largest entry".format(what, int(rows.sum()), rel.max()))
    assert rows.sum() > 0 and rel.max() <= FD_TOL, (what, rel.max(), int(np.argmax(np.where(rows, err / np.maximum(scale, 1e-300), 0))))


def test_pose_chain_gradients_are_central_differences(z, chars):
    for c in por.CHARS:
        km, km64 = chars[c]
        ins = [z["{}_{}".format(c, k)].astype(np.float64) for k in por.INS]
        cots = {k: z["{}_cot_{}".format(c, k)] for k in por.OUTS}
        _, grads = por.pose_chain(km64, *ins, cots=cots)
        far = por.pose_branch_distance(km, ins[1], ins[2]) >= FAR
        assert far.sum() >= 50 and not far[por.ZERO_FRAME] and far[[3, 4, 5, 6, 7, 8, 12, 13]].all()
        for i, k in enumerate(por.INS):
            fd = np.zeros_like(grads[k])
            for col in range(ins[i].shape[1]):
                lo, hi = [a.copy() for a in ins], [a.copy() for a in ins]
                lo[i][:, col] -= H
                hi[i][:, col] += H
                fd[:, col] = (por.pose_chain_frame_sums(km64, *hi, cots) - por.pose_chain_frame_sums(km64, *lo, cots)) / (2 * H)
            _fd_check(grads[k], fd, far, c + " " + k)


def test_angle_and_point_gradients_are_central_differences(z):
    q0, q1, cot = z["ang_q0"].astype(np.float64), z["ang_q1"].astype(np.float64), z["ang_cot"].astype(np.float64)
    _, (g0, g1) = por.quat_diff_angle(q0, q1, cot)
    s, w = por.pair_difference(q0, q1)
    far = (s >= 1e-3) & (np.abs(w) >= 1e-3)            # |v| = 1e-5 and w = 0 (the flip of quat_pos) are the branch points
    assert far.sum() >= 80
    for i, g in enumerate((g0, g1)):
        fd = np.zeros_like(g)
        for col in range(4):
            lo, hi = [q0.copy(), q1.copy()], [q0.copy(), q1.copy()]
            lo[i][:, col] -= H
            hi[i][:, col] += H
            fd[:, col] = cot * (por.quat_diff_angle(*hi)[0] - por.quat_diff_angle(*lo)[0]) / (2 * H)
        _fd_check(g, fd, far, "angle q%d" % i)
    pos, rot, cot = z["pts_pos"].astype(np.float64), z["pts_rot"].astype(np.float64), z["pts_cot"].astype(np.float64)
    local, counts = z["pts_local"], z["pts_counts"]
    _, (gp, gr) = por.body_points_world(pos, rot, local, counts, cot)
    owner, _ = por.point_tables(counts)
    for i, g in enumerate((gp, gr)):
        fd = np.zeros_like(g)
        for b in range(len(counts)):                   # a body's entries touch its own points only: one body and column at a time
            for col in range(g.shape[-1]):
                lo, hi = [pos.copy(), rot.copy()], [pos.copy(), rot.copy()]
                lo[i][..., b, col] -= H
                hi[i][..., b, col] += H
                d = (por.body_points_world(hi[0], hi[1], local, counts)[0] - por.body_points_world(lo[0], lo[1], local, counts)[0]) / (2 * H)
                fd[..., b, col] = (d * cot).sum(axis=(-1, -2))
        own = np.array([c > 0 for c in counts])
        _fd_check(g.reshape(-1, g.shape[-1]), fd.reshape(-1, g.shape[-1]), np.tile(own, 8), "points input %d" % i)
        assert (g[..., 2, :] == 0.0).all()                          # the body without points


@pytest.mark.parametrize("name", ["t4b1", "t5b15", "kink", "zero", "keep0", "small_seams"])
def test_temporal_gradients_are_central_differences(name):
    # the differences are taken of the whole weighted sum, whose rounding (1e-16 of its size over 2 H) has to stay below the bound:
    # the seams are therefore walked on a packing of two bodies rather than on the designed one of fifteen
    case = mh.TtCase((1, 2, 3, 4, 6), 2, seed=77) if name == "small_seams" else mh.designed_tt(name)
    _, g_pos, g_r = case.float64()
    w = case.w.astype(np.float64)

    def total():
        return float((case.float64()[0] * w).sum())

    # a position enters the third differences of its own and the three frames before: those must be 1e-3 off the kink and off j = 0
    near = np.zeros((case.N, case.B), bool)
    for m, T in enumerate(case.lengths):
        s = int(case.ss[m])
        if T >= 4:
            p = case.pos[s:s + T].astype(np.float64)
            jn = np.linalg.norm(p[3:] - 3.0 * p[2:-1] + 3.0 * p[1:-2] - p[:-3], axis=-1)
            bad = (np.abs(jn - case.lim) < 1e-3) | (jn < 1e-3)
            for off in range(4):
                near[s + off:s + off + T - 3] |= bad
    pos0, r0 = case.pos, case.r
    fd_p, fd_r = np.zeros_like(g_pos), np.zeros_like(g_r)
    for idx in np.ndindex(*case.pos.shape):
        vals = []
        for sgn in (1.0, -1.0):
            case.pos = pos0.astype(np.float64)
            case.pos[idx] += sgn * H
            vals.append(total())
        fd_p[idx] = (vals[0] - vals[1]) / (2 * H)
    case.pos = pos0
    for idx in np.ndindex(*case.r.shape):
        vals = []
        for sgn in (1.0, -1.0):
            case.r = r0.astype(np.float64)
            case.r[idx] += sgn * H
            vals.append(total())
        fd_r[idx] = (vals[0] - vals[1]) / (2 * H)
    case.r = r0
    live = ~near.all(axis=1)
    gp, fp = np.where(near[..., None], 0.0, g_pos), np.where(near[..., None], 0.0, fd_p)
    _fd_check(gp.reshape(case.N, -1), fp.reshape(case.N, -1), live & (np.abs(gp).reshape(case.N, -1).max(axis=1) > 0), name + " g_pos")
    rows = np.abs(g_r).max(axis=1) > 0
    if rows.any():
        _fd_check(g_r, fd_r, rows, name + " g_r")
    assert (fd_r[~rows] == 0.0).all()
    if name in ("kink", "zero"):
        assert near.any() and not near.all()


def test_host_build_of_the_temporal_bodies_on_the_designed_cases(z, tmp_path_factory):
    """the bodies the device kernels share with the host (parc_moopt_core.h, plain fp32) on the designed cases, kink and |j| = 0 included,
    against the reference's float64 record: 2 e-bar, the host build's factor"""
    lib = mh.build_host(str(tmp_path_factory.mktemp("moopt_host_g34")))
    for name in mh.DESIGNED_TT:
        case = mh.designed_tt(name)
        got = case.host(lib)
        err = por.value_error(case.sums(got["partial"]), z["tt_{}_f64_sums".format(name)])
        assert err <= 2 * por.MEASURED_TT_VALUE, (name, err)
        for k in ("g_pos", "g_r"):
            rel, dead = por.grad_error(got[k], z["tt_{}_f64_{}".format(name, k)])
            print("{:8s} {:6s} host rel {:.3e} bound {:.3e}".format(name, k, rel, 2 * por.MEASURED_TT_GRAD[k]))
            assert rel <= 2 * por.MEASURED_TT_GRAD[k], (name, k, rel)
            assert (got[k].reshape(case.N, -1)[dead] == 0.0).all(), (name, k)


def test_measured_e_bars_are_the_fixtures(z):
    m = por.measure(z)
    pairs = [(m["pose_value"][k], por.MEASURED_POSE_VALUE_BY_OUTPUT[k], "pose value " + k) for k in por.OUTS]
    pairs += [(max(m["pose_value"].values()), por.MEASURED_POSE_VALUE, "pose value")]
    pairs += [(m["pose_grad"][k], por.MEASURED_POSE_GRAD[k], "pose gradient " + k) for k in por.INS]
    pairs += [(m["angle_value"], por.MEASURED_ANGLE_VALUE, "angle value"), (m["points_value"], por.MEASURED_POINTS_VALUE, "points value"),
              (m["tt_value"], por.MEASURED_TT_VALUE, "temporal value")]
    pairs += [(m["angle_grad"][k], por.MEASURED_ANGLE_GRAD_DECADE[k], "angle gradient decade %d" % k) for k in range(4)]
    pairs += [(m["points_grad"][k], por.MEASURED_POINTS_GRAD[k], "points gradient " + k) for k in por.MEASURED_POINTS_GRAD]
    pairs += [(m["tt_grad"][k], por.MEASURED_TT_GRAD[k], "temporal gradient " + k) for k in por.MEASURED_TT_GRAD]
    for got, const, what in pairs:
        print("{:32s} measured {:.4e} constant {:.4e}".format(what, got, const))
        assert got > 0 and got <= const <= 1.011 * got, (what, got, const)          # the constant is the figure rounded up to 3 digits
    # the angle gradient's conditioning goes as 1 / |v|: each decade's e-bar is several times the next one's
    d = por.MEASURED_ANGLE_GRAD_DECADE
    assert d[0] > 3 * d[1] > 9 * d[2] > 27 * d[3]


def test_generator_check_regenerates_the_fixture():
    """gen_pose_opt.py --check: the reference's own functions give the committed fixture again, 0 differing arrays.  The generator needs
    the reference's Python; where that tree does not exist the test is skipped and says so - decided here, before the generator runs,
    so that any failure of the generator is a failure of the test."""
    import mdm_loss_ref as mlr
    root = mlr.reference_root()
    if not os.path.isdir(root):
        pytest.skip("the reference tree ({}) is not on this machine: the fixture generator cannot run".format(root))
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "gen_pose_opt.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0 and "0 differing arrays" in res.stdout, (res.returncode, res.stdout[-2000:] + res.stderr[-2000:])
