"""The motion scorer (include/parc_score.h) on the CPU: the host build of parc_score_core.h (tests/tools/score_host.cpp) against the float64
restatement of tests/motion_score_ref.py and against fixture G28 (the reference's own compute_motion_loss), the argument rules through
the real library, and the CPU-only parts of the Python surface.

Tolerances (motion_score_ref): a sum of n contributing terms may differ from float64 by HOST_FACTOR * e_bar * n, and from the fixture's
fp32 value by one e_bar * n more (the fixture's own error); n = 0 means exactly 0.  tests/test_motion_score_gpu.py runs the same cases
through parc_motion_score on the device."""
import ctypes
import subprocess

import numpy as np
import pytest

import motion_score_ref as ref
from motion_score_ref import sh


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return sh.build_host(str(tmp_path_factory.mktemp("score_host")))


@pytest.fixture(scope="module")
def km():
    return ref.humanoid()


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


def check_losses(out, r, factor, what, fixture_losses=None):
    """losses [B,3] against float64 (and the fixture's fp32 values) at the measured bounds; print every figure first"""
    for c in range(out["losses"].shape[0]):
        tol = ref.tolerance(factor, r, c)
        for k, term in enumerate(("total", "contact", "pen")):
            got, want = float(out["losses"][c, k]), float(r[term][c])
            print("{} cand {} {:8s} got {:.9g} f64 {:.12g} err {:.3e} bound {:.3e}".format(what, c, term, got, want, abs(got - want), tol[k]))
            if tol[k] == 0.0:
                assert got == 0.0 and want == 0.0, (what, c, term, got)
            assert abs(got - want) <= tol[k], (what, c, term, got, want, tol[k])
            if fixture_losses is not None:
                extra = ref.tolerance(factor + 1.0, r, c)[k]
                assert abs(got - float(fixture_losses[c, k])) <= extra, (what, c, term, got, float(fixture_losses[c, k]), extra)


@pytest.mark.parametrize("j", [0, 1, 2])
def test_host_core_against_float64_and_fixture(hostlib, km, fx, j):
    n = int(fx["lengths"][j])
    case = sh.fixture_case(km, fx, num_frames=np.full(6, n, np.int32))
    out = case.score_host(hostlib)
    assert out["rc"] == 0
    r = case.float64(ref)
    check_losses(out, r, ref.HOST_FACTOR, "host len %d" % n, fx["losses"][:, j])
    assert np.isclose(fx["losses"][1, 0, 2], 1.44e-3, rtol=5e-3) and fx["losses"][2, 0, 2] == 0.0       # lowered 4 cm / raised 10 cm
    assert (out["frame_terms"][:, n:] == -7.0).all()              # frames beyond num_frames: not touched
    assert np.isfinite(out["frame_terms"][:, :n]).all()


def test_host_num_frames_rows_and_jerk(hostlib, km, fx):
    """num_frames = [F, 3, 0]: the row with 0 frames gives losses 0 and jerk NaN, the row with 3 jerk NaN; thresholds no magnitude is near"""
    r0 = sh.fixture_case(km, fx, cands=[3]).float64(ref)
    thr = ref.jerk_threshold(r0["jerk_mag"][0])
    assert (np.abs(r0["jerk_mag"][0] / thr - 1.0) > 1e-4).all()
    case = sh.fixture_case(km, fx, cands=[3, 3, 3], num_frames=[6, 3, 0], max_jerk=thr)
    out, r = case.score_host(hostlib), case.float64(ref)
    check_losses(out, r, ref.HOST_FACTOR, "host num_frames")
    assert (out["losses"][2] == 0.0).all() and np.isnan(out["jerk"][1:]).all()
    assert 0.0 < r["frac_over"][0] < r["jerk_mag"][0].shape[1]
    assert out["jerk"][0, 1] == np.float32(r["frac_over"][0])                   # the count is exact
    err = abs(float(out["jerk"][0, 0]) - r["mean_jerk"][0])
    print("mean_jerk host {:.7g} f64 {:.10g} err {:.3e} bound {:.3e}".format(out["jerk"][0, 0], r["mean_jerk"][0], err, 2 * ref.MEASURED_E_MEAN_JERK))
    assert err <= ref.HOST_FACTOR * ref.MEASURED_E_MEAN_JERK


def test_host_non_finite_pose_stays_in_its_candidate(hostlib, km, fx):
    clean = sh.fixture_case(km, fx, cands=[0, 1, 3]).score_host(hostlib)
    for bad in (np.nan, np.inf):
        case = sh.fixture_case(km, fx, cands=[0, 1, 3])
        case.root_pos[1, 4, 2] = bad
        out = case.score_host(hostlib)
        assert np.isnan(out["losses"][1]).all() and np.isnan(out["jerk"][1]).all()
        for c in (0, 2):
            assert np.array_equal(out["losses"][c], clean["losses"][c]) and np.array_equal(out["jerk"][c], clean["jerk"][c])
    # ... and in a frame that does not count it is never looked at
    case = sh.fixture_case(km, fx, cands=[0, 1, 3], num_frames=[6, 4, 6])
    ok = case.score_host(hostlib)
    case.root_pos[1, 4, 2] = np.nan
    out = case.score_host(hostlib)
    assert np.array_equal(out["losses"], ok["losses"]) and np.array_equal(out["jerk"], ok["jerk"], equal_nan=True)


def _einval_cases(call):
    """every PARC_EINVAL rule of include/parc_score.h; call(**overrides) -> rc"""
    for kw in (dict(B=-1), dict(F=-1), dict(n_points=0), dict(n_points=-3), dict(num_bodies=17), dict(num_bodies=0), dict(root_pos=None),
               dict(root_rot=None), dict(joint_rot=None), dict(contacts=None), dict(local=None), dict(start=None), dict(frame_terms=None),
               dict(losses=None), dict(body_pos_ws=None), dict(hf=None), dict(x_points=None), dict(dx=0.0), dict(dy=-0.4), dict(dim_x=0),
               dict(dim_y=-5)):
        assert call(**kw) == -1, kw
    assert call(B=0) == 0 and call(F=0) == 0
    assert call(B=65536) == -2


def test_argument_errors_through_the_library(km):
    """parc_motion_score answers before any HIP call: no GPU is needed to be refused (or to be told there is nothing to do)"""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_score
    L = _hip.lib()
    assert L.parc_score_abi() == 1 and L.parc_abi_version() == 1
    dummy = 0x1000          # never dereferenced: every call below is refused, or has nothing to launch

    def call(**kw):
        assert kw, "only refused or empty calls go to the library here"
        ptr = {k: (None if k in kw and kw[k] is None else ctypes.c_void_p(dummy)) for k in
               ("root_pos", "root_rot", "joint_rot", "contacts", "local", "start", "frame_terms", "losses", "body_pos_ws", "hf", "x_points")}
        model = _hip.CharModelS.from_buffer_copy(bytes(km.c_struct()))
        model.num_bodies = kw.get("num_bodies", model.num_bodies)
        ter = _hip_score.ScoreTerrainS(ptr["hf"], kw.get("dim_x", 6), kw.get("dim_y", 5), 0.0, 0.0, kw.get("dx", 0.4), kw.get("dy", 0.4), ptr["x_points"],
                                       ctypes.c_void_p(dummy))
        return L.parc_motion_score(None, model, kw.get("B", 2), kw.get("F", 6), None, ptr["root_pos"], ptr["root_rot"], ptr["joint_rot"], ptr["contacts"],
                                   kw.get("n_points", 308), ptr["local"], ptr["start"], ter, -10.0, 1.0, 1.0, 1.0 / 30.0, 1000.0, ptr["body_pos_ws"],
                                   ptr["frame_terms"], ptr["losses"], ctypes.c_void_p(dummy))
    _einval_cases(call)


def test_argument_errors_of_the_host_build(hostlib, km, fx):
    case = sh.fixture_case(km, fx, cands=[0])
    assert case.score_host(hostlib)["rc"] == 0
    bad = sh.fixture_case(km, fx, cands=[0])
    bad.dxdy = [0.0, 0.4]
    assert bad.score_host(hostlib)["rc"] == -1
    bad = sh.fixture_case(km, fx, cands=[0])
    bad.P = 0
    assert bad.score_host(hostlib)["rc"] == -1


def test_sanitized_program_scores_the_cases(tmp_path, hostlib, km, fx):
    """parc_score_core.h under AddressSanitizer and UBSan in a stand-alone program (its own main): the fixture with ragged lengths, a
    NaN pose, and one point per body on a 1 x 1 field; its results equal the plain build's bit for bit."""
    exe = sh.build_program(str(tmp_path), sanitize=True)
    ragged = sh.fixture_case(km, fx, num_frames=[6, 3, 0, 6, 1, 4], max_jerk=500.0)
    nan = sh.fixture_case(km, fx, cands=[0, 4], max_jerk=500.0)
    nan.root_rot[0, 2, 1] = np.nan
    one = sh.Case(km, fx["root_pos"][:2], fx["root_rot"][:2], fx["joint_rot"][:2], fx["contacts"][:2], np.zeros((15, 3), np.float32), np.arange(16),
                  np.full((1, 1), 0.25, np.float32), [0.3, -0.2], [0.4, 0.4])
    for name, case in (("ragged", ragged), ("nan", nan), ("one", one)):
        f, o = str(tmp_path / (name + ".case")), str(tmp_path / (name + ".out"))
        case.dump(f)
        res = subprocess.run([exe, f, o], capture_output=True, text=True)
        assert res.returncode == 0 and "score ok" in res.stdout, (name, res.returncode, res.stderr[-2000:])
        got, want = case.read_program_output(o), case.score_host(hostlib)
        for key in ("frame_terms", "losses", "jerk"):
            assert np.array_equal(got[key], want[key], equal_nan=True), (name, key)


# ------------------------------------------------------------------------------------------------ the Python surface, CPU-only paths
def test_settings_and_alias_registration():
    import sys
    import parc_amd
    parc_amd.install_reference_aliases()
    import tools.motion_tests.compute_losses as cl
    import tools.procgen.mdm_path as mp
    assert mp is sys.modules["parc_amd.tools.procgen.mdm_path"] and cl is sys.modules["parc_amd.tools.motion_tests.compute_losses"]
    s = mp.MDMPathSettings
    assert (s.next_node_lookahead, s.rewind_num_frames, s.end_of_path_buffer, s.max_motion_length, s.path_batch_size, s.mdm_batch_size, s.top_k,
            s.w_target, s.w_contact, s.w_pen) == (7, 5, 2, 10.0, 16, 32, 4, 2.0, 0.1, 0.1)
    for fn in (mp.gen_mdm_motion_at_path_start, mp.generate_frames_along_path, mp.generate_frames_until_end_of_path):
        with pytest.raises(NotImplementedError, match="planner callable"):
            fn()
    for name in ("MotionScorer", "compute_motion_loss", "rank_motions"):
        assert callable(getattr(mp, name))


def test_grouping_and_csv_columns(tmp_path):
    import csv
    from parc_amd.tools.motion_tests import compute_losses as cl
    assert cl.group_of("/x/PATH_TERRAIN_3_12.pkl") == "PATH_TERRAIN_3" and cl.group_of("walk.pkl") == "walk" and cl.group_of("a_b_7_08.pkl") == "a_b_7"
    rows = [dict(file="t_0.pkl", group="t", motion_length=1.0, mean_jerk=2.0, frames_with_jerk_over_X=0.0, contact_loss=1.0, pen_loss=0.5, final_node_dist=None),
            dict(file="t_1.pkl", group="t", motion_length=2.0, mean_jerk=4.0, frames_with_jerk_over_X=0.5, contact_loss=3.0, pen_loss=0.5, final_node_dist=None),
            dict(file="u_0.pkl", group="u", motion_length=4.0, mean_jerk=1.0, frames_with_jerk_over_X=1.0, contact_loss=0.0, pen_loss=2.0, final_node_dist=0.25)]
    header, line = cl.summarize(rows, "exp")
    # the reference's overall columns (compute_losses.py:44-56), then its per-group ones with the group name in front (:60-71)
    assert header[:13] == ["exp_name", "final_node_dist mean", "final_node_dist std", "motion_length mean", "motion_length std", "mean_jerk mean",
                           "mean_jerk std", "frames_with_jerk_over_X mean", "frames_with_jerk_over_X std", "contact_loss mean", "contact_loss std",
                           "pen_loss mean", "pen_loss std"]
    assert header[13:25] == ["t" + c for c in ("final node dist mean", "final node dist std", "motion length mean", "motion length std", "mean jerk mean",
                                               "mean jerk std", "frames_with_jerk_over_X mean", "frames_with_jerk_over_X std", "contact loss mean",
                                               "contact loss std", "pen loss mean", "pen loss std")]
    assert len(header) == len(line) == 1 + 12 * 3
    col = dict(zip(header, line))
    assert col["motion_length mean"] == pytest.approx(7.0 / 3.0) and col["motion_length std"] == pytest.approx(np.std([1.0, 2.0, 4.0], ddof=1))
    assert col["tmean jerk mean"] == 3.0 and col["tmean jerk std"] == pytest.approx(np.sqrt(2.0)) and col["ufinal node dist mean"] == 0.25
    assert np.isnan(col["ufinal node dist std"]) and np.isnan(col["tfinal node dist mean"]) and col["final_node_dist mean"] == 0.25
    out = str(tmp_path / "m.csv")
    cl.write_csv(rows, out, "exp")
    with open(out, newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == cl.FILE_COLUMNS and [r[0] for r in got[1:4]] == ["t_0.pkl", "t_1.pkl", "u_0.pkl"] and got[1][-1] == "" and got[3][-1] == "0.25"
    assert got[5] == header and got[6][0] == "exp"
