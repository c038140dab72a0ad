"""The numpy references of tests/tools/bookkeeping_ref.py against the fixtures and against numpy's own routines: they are the
yardstick of tests/test_bookkeeping_gpu.py, so they are pinned first, without a GPU."""
import os
import sys

import numpy as np

from conftest import golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import bookkeeping_ref as bk  # noqa: E402


def test_frame_query_ref_reproduces_the_blend_of_fixture_g3(ref_mlib):
    z = golden("g3_motion")
    cos, blend = ref_mlib.slerp_cosines(z["q_ids"], z["q_times"])
    i0, i1, b, lp = bk.frame_query_ref(z["motion_lengths"], z["clip_loop"], z["motion_num_frames"], z["q_ids"], z["q_times"])
    assert b.dtype == np.float32 and np.array_equal(b, blend)
    nf = z["motion_num_frames"][z["q_ids"]]
    assert np.all((i0 >= 0) & (i0 < nf) & (i1 >= i0) & (i1 <= i0 + 1) & (i1 < nf))
    # the row-copied outputs of the fixture name the frame: the reference's root velocity at the query is row i0 of its table
    rows = z["motion_start_idx"][z["q_ids"]] + i0
    assert np.array_equal(z["frame_root_vel"][rows], z["q_root_vel"])
    assert np.array_equal(z["frame_dof_vel"][rows], z["q_dof_vel"])
    # float64 agrees wherever the frame position is not next to an integer
    j0, dist = bk.frame_query_f64(z["motion_lengths"], z["clip_loop"], z["motion_num_frames"], z["q_ids"], z["q_times"])
    far = dist > 1e-3
    assert far.sum() > 300 and np.array_equal(i0[far], j0[far])
    assert np.array_equal(lp, np.floor(z["q_times"] / z["motion_lengths"][z["q_ids"]]))


def test_select_ref_is_searchsorted_right_on_sorted_tables():
    rng = np.random.default_rng(0)
    for M in (1, 2, 7, 256, 1000):
        w = rng.random(M).astype(np.float32)
        w[rng.random(M) < 0.2] = 0.0
        w[0] = 0.5
        table = np.cumsum(w.astype(np.float64)).astype(np.float32)
        x = np.concatenate([[0.0, table[-1], np.nextafter(table[-1], np.float32(0))], table, np.nextafter(table, np.float32(0)),
                            rng.random(50) * table[-1]]).astype(np.float32)
        want = np.minimum(np.searchsorted(table, x, side="right"), M - 1)
        assert np.array_equal(bk.select_ref(table, x), want)
    # an unsorted table: the definition (first index that exceeds), which a bisection does not give
    assert bk.select_ref(np.array([1.0, 3.0, 2.0, 4.0], np.float32), np.array([2.5], np.float32))[0] == 1


def test_cdf_ref_sums_fp32_products_in_float64():
    w = np.array([0.1, 0.0, 0.3, 0.7], np.float32)
    fr = np.array([0.5, 0.9, 0.001, 1.0], np.float32)
    p = bk.clip_products(w, fr, 0.01)
    assert p.dtype == np.float32 and np.array_equal(p, np.array([np.float32(0.5) * w[0], 0.0, np.float32(0.01) * w[2], w[3]], np.float32))
    assert np.array_equal(bk.cdf_ref(w, fr, 0.01), np.cumsum(p.astype(np.float64)))
    assert np.array_equal(bk.cdf_ref(w, None, 0.01), np.cumsum(w.astype(np.float64)))


def test_hf_ref_reproduces_the_g5_fixtures_away_from_cell_boundaries():
    rays = golden("g4_rays")["ray_xy_points"]
    for name in ("g5_hf_civ", "g5_hf_teaser"):
        z = golden(name)
        out, dist = bk.hf_ref(rays, z["root_pos"], z["heading"], z["hf"], z["min_point"], z["dxdy"], -3.0, 3.0)
        ok = z["boundary_dist"] >= 1e-4
        assert ok.mean() > 0.99
        assert np.array_equal(out[ok], z["ray_hfs"][ok])
        assert np.abs(dist - z["boundary_dist"])[ok].max() < 1e-4          # the fixture's distance is the fp32 evaluation of the same
    # from-state entry: the heading of a yaw rotation is the yaw
    yaw = np.array([0.3, -2.0, 3.0])
    q = np.stack([0 * yaw, 0 * yaw, np.sin(yaw / 2), np.cos(yaw / 2)], -1)
    assert np.allclose(bk.heading_of_quat(q), yaw, atol=1e-12)
