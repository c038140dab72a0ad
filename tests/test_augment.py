"""The dataset augmentation (include/parc_augment.h, tools/motion_opt/augment_motions.py) on the CPU: the host build of
parc_augment_core.h (tests/tools/augment_host.cpp) against fixture G31 (the reference's functions in its script's order) and a float64
restatement (tests/augment_ref.py), the draws against G31, the argument rules through the real library, the same cases in a sanitized
stand-alone program, exports and documentation, and the packing and grouping logic of the Python side.
tests/test_augment_gpu.py runs the same cases on the device.

Bounds.  e-bar is the largest |reference fp32 - float64| over the fixture's frame entries (measured by tests/augment_ref.py, recorded
in DESIGN.md: 1.51e-6).  The host build may differ from float64 and from G31 by 2 e-bar in the turned root rotation (sqrt / atan2 /
sin / cos sequences evaluated by another libm); xy, z, the dofs, the bounds, the dims and the min points are exact, the heights are
bit-identical (boxes: on the cells that are not within 1e-4 grid units of a box edge; at most 2 % of a variant's cells are)."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
import augment_host as ah      # noqa: E402
import augment_ref as ar       # noqa: E402

EBAR_RECORDED = 1.511952e-06       # python tests/augment_ref.py


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return ah.build_host(str(tmp_path_factory.mktemp("augment_host")))


@pytest.fixture(scope="module")
def g31():
    z, meta = ar.load_fixture()
    return z, meta, ah.fixture_clips(z, meta)


@pytest.fixture(scope="module")
def ebar(g31):
    e = ar.measure_ebar(g31[0], g31[1])
    assert abs(e - EBAR_RECORDED) <= 1e-9, e          # the recorded figure is the fixture's
    return e


@pytest.fixture(scope="module")
def host_runs(hostlib, g31):
    """every fixture variant through the host build, grouped as prepare_variants would take them: {k: (HostRun, index in the run)}"""
    z, meta, clips = g31
    runs = {}
    for (pad, sl), ks in ah.setting_groups(meta).items():
        run = ah.HostRun(hostlib, [ah.fixture_spec(z, meta, k) for k in ks], clips, pad, sl)
        for n, k in enumerate(ks):
            runs[k] = (run, n)
    assert sorted(runs) == list(range(len(meta["variants"])))
    return runs


def check_variant(z, meta, k, frames, transformed, contacts, bounds, hf, min_point, tol, what):
    """one variant's outputs against G31 and float64 at `tol` (frames) and exactly (the rest)"""
    v = meta["variants"][k]
    want = z["v%d_frames" % k]
    _, _, ter64 = ar.variant64(z, meta, k)
    assert frames.shape == want.shape
    # pass-through columns (z before localising, the dofs), contacts: bit-identical; xy and the bounds: exact products and sums
    src = z["c%d_frames" % v["clip"]][v["start"]:v["start"] + v["length"]]
    assert np.array_equal(transformed[:, 2].view(np.uint32), src[:, 2].view(np.uint32)), (what, k, "z")
    assert np.array_equal(frames[:, 6:].view(np.uint32), src[:, 6:].view(np.uint32)), (what, k, "dofs")
    assert np.array_equal(contacts.view(np.uint32), z["v%d_contacts" % k].view(np.uint32)), (what, k, "contacts")
    assert np.array_equal(transformed[:, 0:3], z["v%d_transformed" % k][:, 0:3]), (what, k, "transformed xyz")
    assert np.array_equal(bounds, z["v%d_bounds" % k]), (what, k, "bounds")
    assert np.array_equal(frames[:, 0:3], want[:, 0:3]), (what, k, "localised xyz")
    e_ref, e_64 = np.abs(frames.astype(np.float64) - want).max(), np.abs(frames - ter64["frames"]).max()
    print("{} variant {:2d} frames: max |x - G31| {:.3e}  max |x - f64| {:.3e}  bound {:.3e}".format(what, k, e_ref, e_64, tol))
    assert e_ref <= tol and e_64 <= tol, (what, k, e_ref, e_64, tol)
    assert np.array_equal(np.array(hf.shape), z["v%d_dims" % k]), (what, k, "dims")
    assert np.array_equal(min_point, z["v%d_min_point" % k]), (what, k, "min point", min_point, z["v%d_min_point" % k])
    want_hf = z["v%d_hf" % k]
    if v["mode"] == "BOXES_ALONG_PATH":
        unsafe = ter64["unsafe"]
        share = unsafe.mean()
        print("{} variant {:2d} boxes: unsafe share {:.4f}, differing cells {}".format(what, k, share, int((hf != want_hf).sum())))
        assert share <= 0.02, (what, k, share)
        assert np.array_equal(hf[~unsafe].view(np.uint32), want_hf[~unsafe].view(np.uint32)), (what, k, "safe cells")
    else:
        assert np.array_equal(hf.view(np.uint32), want_hf.view(np.uint32)), (what, k, "heights")


def test_host_build_equals_g31_and_float64(host_runs, g31, ebar):
    z, meta, _ = g31
    for k in range(len(meta["variants"])):
        run, n = host_runs[k]
        check_variant(z, meta, k, run.variant_frames(n), run.variant_frames(n, transformed=True), run.variant_contacts(n), run.bounds[n],
                      run.variant_hf(n), run.variant_min_point(n), 2 * ebar, "host")


def test_fixture_covers_the_edge_cases(host_runs, g31):
    """the edge cases G31 is built to hold (tests/golden/gen_augment.py), checked on the fixture and on the host build's output"""
    z, meta, _ = g31
    vs = meta["variants"]
    assert {v["length"] for v in vs} >= {1, 2, 5, 37, 15}
    long_cut = [v for v in vs[:11] if v["length"] == 15][0]
    assert long_cut["start"] == 37 - 15 - 1                         # the last legal start of random.randint(0, T - max - 1)
    assert {0.0, 180.0, -180.0} <= {v["heading"] for v in vs} and {v["pad"] for v in vs} == {0, 3}
    assert {v["mode"] for v in vs} == set(ar.MODES) and {True, False} == {bool(v["slice"]) for v in vs}
    assert {len(v["frame_inds"]) for v in vs[:11] if v["mode"] == "BOXES_ALONG_PATH"} >= {0, 1, 5}
    assert any(float(z["v%d_composed_w_min" % k]) < 0 for k in range(len(vs)))
    assert any(tuple(z["c%d_hf" % v["clip"]].shape) == (1, 1) for v in vs)
    # a zero root exp-map with heading 0 comes out exactly zero
    run, n = host_runs[8]
    assert vs[8]["heading"] == 0.0 and np.all(z["c3_frames"][:, 3:6] == 0)
    out = run.variant_frames(n)[:, 3:6]
    assert np.all(out == 0.0) and not np.signbit(out).any()
    # the order of overlapping boxes decides: stamping variant 2's boxes in reverse order gives other heights
    _, _, fwd = ar.variant64(z, meta, 2)
    boxes = ar.variant_boxes(z, 2)
    v = vs[2]
    fr, _ = ar.transform_frames64(z["c0_frames"], float(z["v2_heading_rad"]), float(np.float32(v["sx"])), float(np.float32(v["sy"])))
    rev = ar.build_terrain64(fr, z["c0_hf"], z["c0_min_point"], z["c0_dxdy"], v["pad"], True, z["v2_dims"], z["v2_grid_min"], v["mode"], 1.0, boxes[::-1])
    assert (fwd["hf"] != rev["hf"]).sum() > 0
    # a box centred outside the grid (it still reaches into it), a path that leaves the source grid
    bc = z["v9_box_centers"]
    assert np.any(bc > z["v9_dims"] - 0.5) or np.any(bc < -0.5)
    assert (z["v9_hf"] != np.pad(z["c0_hf"], 3)).sum() > 4
    lo = z["v4_padded_min"]
    hi = lo + (z["v4_padded_dims"] - 1) * z["c0_dxdy"]
    b = z["v4_bounds"]
    assert b[0] < lo[0] - 1 or b[1] < lo[1] - 1 or b[2] > hi[0] + 1 or b[3] > hi[1] + 1


def test_draw_variants_reproduces_the_draws(g31):
    import torch
    from parc_amd.tools.motion_opt import augment_motions as am
    z, meta, clips = g31
    for run in meta["runs"]:
        random.seed(run["seed"])
        torch.manual_seed(run["seed"])
        specs = am.draw_variants(run["cfg"], clips)
        assert len(specs) == run["count"] == run["cfg"]["num_new_motions"]
        names = {}
        for n, s in enumerate(specs):
            k = run["first"] + n
            v = meta["variants"][k]
            assert (s.file_index, s.start, s.length, s.heading, s.sx, s.sy, s.mode.name) == \
                (v["clip"], v["start"], v["length"], v["heading"], v["sx"], v["sy"], v["mode"]), (k, vars(s), v)
            names[s.file_index] = names.get(s.file_index, 0) + 1
            assert s.name == "clip%d_aug%03d" % (s.file_index, names[s.file_index])
            if v["mode"] == "HEIGHT_SCALE":
                assert s.height_scale == v["height_scale"] and not (run["cfg"]["bad_h_range"][0] < s.height_scale < run["cfg"]["bad_h_range"][1])
            else:
                assert s.frame_inds.tolist() == v["frame_inds"] == z["v%d_frame_inds" % k].tolist()
                assert np.array_equal(s.box_len.numpy().reshape(-1, 2), z["v%d_box_len" % k])
                assert s.box_angle == z["v%d_box_angle" % k].tolist() and s.box_h == z["v%d_box_h" % k].tolist()
    assert any(v.get("tries", 1) > 1 for v in meta["variants"])           # the rejection loop ran
    # the heading terms the frames table carries are the reference's own
    for k, v in enumerate(meta["variants"]):
        assert np.array_equal(np.array(am._heading_terms(v["heading"]), np.float32), z["v%d_heading_terms" % k]), k
    # no variants: no draws at all
    state = (random.getstate(), torch.get_rng_state())
    assert am.draw_variants(dict(meta["runs"][0]["cfg"], num_new_motions=0), clips) == []
    assert random.getstate() == state[0] and torch.equal(torch.get_rng_state(), state[1])


def test_terrain_util_additions_equal_g31(g31):
    """SubTerrain.round_point_to_grid_point and add_boxes_to_hf_at_xy_points (CPU tensor: torch ops) with the reference's draw order"""
    import torch
    from parc_amd.util import terrain_util
    z, meta, clips = g31
    cfg = meta["box_cfg"]
    t = clips[0].terrain
    p = torch.tensor([0.33, -1.27])
    assert torch.equal(t.round_point_to_grid_point(p), torch.round((p - t.min_point) / t.dxdy) * t.dxdy + t.min_point)
    for k in (2, 3, 7, 9):
        v = meta["variants"][k]
        # the heights before the boxes: the same variant with no boxes, by the float64 restatement (heights are gathered, exact in fp32)
        base = ar.build_terrain64(z["v%d_transformed" % k], z["c%d_hf" % v["clip"]], z["c%d_min_point" % v["clip"]], z["c%d_dxdy" % v["clip"]],
                                  v["pad"], v["slice"], z["v%d_dims" % k], z["v%d_grid_min" % k], "NONE")["hf"]
        hf = torch.tensor(base.astype(np.float32))
        random.seed(v["seed"])
        torch.manual_seed(v["seed"])
        terrain_util.add_boxes_to_hf_at_xy_points(torch.tensor(z["v%d_box_centers" % k]), hf, cfg["min_h"], cfg["max_h"], cfg["min_len"], cfg["max_len"],
                                                  cfg["min_angle"], cfg["max_angle"])
        assert np.array_equal(hf.numpy(), z["v%d_hf" % k]), k


def test_not_finite_variant_is_named_and_alone(hostlib, g31):
    """a NaN frame of one variant: its bounds are NaN and TerrainPlan names it; the other variants' frames, bounds and heights are bit-identical"""
    from parc_amd.tools.motion_opt import augment_motions as am
    z, meta, clips = g31
    ks = ah.setting_groups(meta)[(3, True)]
    specs = [ah.fixture_spec(z, meta, k) for k in ks]
    clean = ah.HostRun(hostlib, specs, clips, 3, True)
    bad_clip = am.SeedClip("bad", z["c1_frames"].copy(), z["c1_contacts"], clips[1].terrain, meta["fps"])
    bad_clip.frames[2, 1] = float("nan")
    n_bad = [n for n, k in enumerate(ks) if meta["variants"][k]["clip"] == 1][0]
    clips2 = list(clips) + [bad_clip]
    specs2 = list(specs)
    specs2[n_bad] = ah.fixture_spec(z, meta, ks[n_bad])
    specs2[n_bad].file_index, specs2[n_bad].name = len(clips), "the_bad_one"
    fp = am.FramesPlan(specs2, clips2)
    frames, contacts = np.zeros((fp.n_out, 34), np.float32), np.zeros((fp.n_out, fp.contact_width), np.float32)
    bounds = np.zeros((fp.V, 4), np.float32)
    rc = ah.host_lib(hostlib).augment_frames_host(fp.V, fp.src_frames.shape[0], fp.contact_width, ah._p(fp.src_frames), ah._p(fp.src_contacts),
                                                  ah._p(fp.table), fp.n_out, ah._p(frames), ah._p(contacts), ah._p(bounds))
    assert rc == 0
    assert np.isnan(bounds[n_bad]).all() and np.isfinite(np.delete(bounds, n_bad, axis=0)).all()
    assert np.array_equal(np.delete(bounds, n_bad, axis=0), np.delete(clean.bounds, n_bad, axis=0))
    o, n = fp.out_off[n_bad], fp.lengths[n_bad]
    keep = np.ones(fp.n_out, bool)
    keep[o:o + n] = False
    assert np.array_equal(frames[keep], clean.transformed[keep])
    with pytest.raises(ValueError, match="the_bad_one"):
        am.TerrainPlan(specs2, clips2, bounds, fp, 3, True)
    # a table row that points outside its arrays: NaN for that variant only (source id, window, box frame index)
    run = ah.HostRun(hostlib, specs, clips, 3, True)
    tp, L = run.tp, ah.host_lib(hostlib)
    for field, value in (("src", 99), ("src", -1), ("frame_off", 10 ** 6), ("box_off", 10 ** 6)):
        vt = type(tp.vars).from_buffer_copy(bytes(tp.vars))
        target = 2 if field == "box_off" else 1           # (variant 2 of the group has boxes)
        assert vt[target].mode == 2 or field != "box_off"
        setattr(vt[target], field, value)
        pool, canon = tp.pool.copy(), np.zeros((fp.V, 3), np.float32)
        rc = L.augment_terrains_host(fp.V, tp.n_cells, ah._p(tp.cell_start), ah._p(vt), len(clips), ah._p(tp.src_table), ah._p(tp.src_pool),
                                     tp.src_pool.size, ah._p(tp.out_table), ah._p(pool[tp.out_floats:]), tp.points_floats, ah._p(tp.boxes), tp.n_boxes,
                                     ah._p(clean.transformed), fp.n_out, ah._p(pool), tp.out_floats, ah._p(canon))
        assert rc == 0
        for n in range(fp.V):
            X, Y = tp.shapes[n]
            got = pool[tp.hf_entries[n].off_hf:tp.hf_entries[n].off_hf + X * Y]
            if n == target:
                assert np.isnan(got).all() and np.isnan(canon[n]).all(), (field, value)
            else:
                assert np.array_equal(got.reshape(X, Y), clean.variant_hf(n)) and np.array_equal(canon[n], clean.canon[n]), (field, value, n)


def test_argument_rules_through_the_library():
    """every entry point answers before any HIP call: no GPU is needed to be refused (or to be told there is nothing to do)"""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    L = _hip.lib()
    assert L.parc_augment_abi() == 1 and L.parc_abi_version() == 1
    d = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused, or has nothing to launch

    def frames(V=2, n_src=4, C=3, n_out=4, **null):
        a = {k: (None if k in null else d) for k in ("src_frames", "src_contacts", "vars", "out_frames", "out_contacts", "bounds")}
        return L.parc_augment_frames(None, V, n_src, C, a["src_frames"], a["src_contacts"], a["vars"], n_out, a["out_frames"], a["out_contacts"], a["bounds"])

    assert frames(V=-1) == -1 and frames(n_src=-1) == -1 and frames(C=-1) == -1 and frames(n_out=-1) == -1
    assert frames(V=0) == 0 and frames(V=0, vars=None, bounds=None) == 0
    for n in ("src_frames", "src_contacts", "vars", "out_frames", "out_contacts", "bounds"):
        assert frames(**{n: None}) == -1, n

    t_names = ("cell_start", "vars", "src_table", "src_pool", "out_table", "points", "boxes", "frames", "out_pool", "canon")

    def terrains(V=2, n_cells=8, S=1, sp=4, pts=4, nb=1, rows=4, op=8, **null):
        a = {k: (None if k in null else d) for k in t_names}
        return L.parc_augment_terrains(None, V, n_cells, a["cell_start"], a["vars"], S, a["src_table"], a["src_pool"], sp, a["out_table"], a["points"], pts,
                                       a["boxes"], nb, a["frames"], rows, a["out_pool"], op, a["canon"])

    for kw in ("V", "n_cells", "S", "sp", "pts", "nb", "rows", "op"):
        assert terrains(**{kw: -1}) == -1, kw
    assert terrains(V=0) == 0 and terrains(n_cells=0) == 0
    for n in t_names:
        assert terrains(**{n: None}) == -1, n
    assert terrains(n_cells=0, boxes=None, nb=0) == 0 and terrains(n_cells=0, points=None, pts=0) == 0      # optional when their count is 0

    def localize(V=2, rows=4, **null):
        a = {k: (None if k in null else d) for k in ("vars", "canon", "frames")}
        return L.parc_augment_localize(None, V, a["vars"], a["canon"], a["frames"], rows, None)

    assert localize(V=-1) == -1 and localize(rows=-1) == -1 and localize(V=0) == 0
    for n in ("vars", "canon", "frames"):
        assert localize(**{n: None}) == -1, n


def test_sanitized_program_runs_the_cases(tmp_path, hostlib, g31, host_runs):
    """parc_augment_core.h under AddressSanitizer and UBSan in a stand-alone program (its own main): every fixture variant through all
    three entry points; its results equal the plain build's bit for bit."""
    z, meta, clips = g31
    exe = ah.build_program(str(tmp_path), sanitize=True)
    for (pad, sl), ks in ah.setting_groups(meta).items():
        run = host_runs[ks[0]][0]
        f, o = str(tmp_path / "g{}{}.case".format(pad, int(sl))), str(tmp_path / "g{}{}.out".format(pad, int(sl)))
        ah.dump(f, run.fp, run.tp, len(clips))
        res = subprocess.run([exe, f, o], capture_output=True, text=True)
        assert res.returncode == 0 and "augment ok" in res.stdout, (pad, sl, res.returncode, res.stderr[-2000:])
        got = ah.read_program_output(o, run.fp, run.tp)
        assert np.array_equal(got["frames"], run.frames, equal_nan=True) and np.array_equal(got["contacts"], run.contacts)
        assert np.array_equal(got["bounds"], run.bounds) and np.array_equal(got["pool"], run.pool[:run.tp.out_floats], equal_nan=True)
        assert np.array_equal(got["canon"], run.canon, equal_nan=True)
        assert got["hf_table"].tobytes() == bytes(run.hf_entries)[:run.fp.V * 40]


def test_exports_and_documentation():
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    with open(os.path.join(REPO, "include", "parc_augment.h")) as f:
        names = sorted(set(re.findall(r"\b(parc_[a-z0-9_]+)\s*\(", f.read())))
    assert names == ["parc_augment_abi", "parc_augment_frames", "parc_augment_localize", "parc_augment_terrains"]
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    L = _hip.lib()
    for n in names:
        assert n in _hip.EXPORTED and hasattr(L, n) and n in doc, n
    assert "parc_augment.hip" in _hip.SOURCES and "-ffp-contract=off" in _hip.OPT_LEVEL["parc_augment.hip"]
    assert "augment_motions" in doc and "add_boxes_to_hf_at_xy_points" in doc


# ------------------------------------------------------------------------------------------------------ packing and grouping (pure Python)
def test_packing_and_grouping_logic(g31):
    from parc_amd import _hip_augment, _hip_moopt
    from parc_amd.tools.motion_opt import augment_motions as am
    from parc_amd.util import terrain_util
    z, meta, clips = g31
    assert am.group_ranges(7, 3) == [(0, 3), (3, 6), (6, 7)] and am.group_ranges(0, 3) == [] and am.group_ranges(2, None) == [(0, 1), (1, 2)]
    assert am.group_ranges(3, 8) == [(0, 3)]
    for s, size in ((_hip_augment.AugFramesS, 44), (_hip_augment.AugTerrainS, 36), (_hip_augment.AugVariantS, 36), (_hip_augment.AugBoxS, 28),
                    (_hip_moopt.MooptTerrainS, 40)):
        assert ctypes.sizeof(s) == size, s
    ks = ah.setting_groups(meta)[(3, True)]
    specs = [ah.fixture_spec(z, meta, k) for k in ks]
    fp = am.FramesPlan(specs, clips)
    src_off = np.concatenate([[0], np.cumsum([c.frames.shape[0] for c in clips])])
    assert fp.n_out == sum(s.length for s in specs) and fp.out_off == list(np.concatenate([[0], np.cumsum(fp.lengths)])[:-1])
    assert fp.src_frames.shape == (src_off[-1], 34) and fp.src_contacts.shape == (src_off[-1], 15)
    for n, s in enumerate(specs):
        e = fp.table[n]
        assert (e.src_off, e.src_len, e.start, e.length, e.out_off) == (src_off[s.file_index], clips[s.file_index].frames.shape[0], s.start, s.length,
                                                                        fp.out_off[n])
        assert (e.sx, e.sy) == (np.float32(s.sx), np.float32(s.sy))
    bounds = np.stack([z["v%d_bounds" % k] for k in ks])
    tp = am.TerrainPlan(specs, clips, bounds, fp, 3, True)
    at, pts, boxes = 0, 0, 0
    for n, (k, s) in enumerate(zip(ks, specs)):
        X, Y = (int(v) for v in z["v%d_dims" % k])
        o, h, a = tp.out_table[n], tp.hf_entries[n], tp.vars[n]
        assert tp.shapes[n] == (X, Y) and (o.dim_x, o.dim_y, h.dim_x, h.dim_y) == (X, Y, X, Y)
        assert np.array_equal(np.array([o.min_x, o.min_y], np.float32), z["v%d_grid_min" % k])
        assert (o.off_hf, h.off_hf, h.off_x, h.off_y) == (at, at, at + X * Y, at + X * Y + X) and (o.off_x, o.off_y) == (pts, pts + X)
        grid = terrain_util.HfGrid(clips[s.file_index].terrain.hf.new_empty((X, Y)), clips[s.file_index].terrain.dxdy, "cpu")
        assert np.array_equal(tp.pool[h.off_x:h.off_x + X], grid.xs.numpy()) and np.array_equal(tp.pool[h.off_y:h.off_y + Y], grid.ys.numpy())
        assert (h.half_x, h.half_y, h.base_z) == (grid.half[0], grid.half[1], -10.0)
        xs = tp.pool[tp.out_floats + o.off_x:tp.out_floats + o.off_x + X]
        assert xs[0] == o.min_x and np.allclose(np.diff(xs), o.dx, atol=1e-5)
        assert (a.src, a.pad, a.slice, a.frame_off, a.frame_len, a.box_off, a.box_count) == (s.file_index, 3, 1, fp.out_off[n], s.length, boxes,
                                                                                          len(s.frame_inds))
        assert tp.cell_start[n] == sum(x * y for x, y in tp.shapes[:n])
        at, pts, boxes = at + X * Y + X + Y, pts + X + Y, boxes + len(s.frame_inds)
    assert (tp.out_floats, tp.points_floats, tp.n_boxes, tp.n_cells) == (at, pts, boxes, int(tp.cell_start[-1])) and tp.pool.size == at + pts
    # slice_terrain false keeps the padded source grid
    ks0 = ah.setting_groups(meta)[(3, False)]
    specs0 = [ah.fixture_spec(z, meta, k) for k in ks0]
    tp0 = am.TerrainPlan(specs0, clips, np.stack([z["v%d_bounds" % k] for k in ks0]), am.FramesPlan(specs0, clips), 3, False)
    for n, k in enumerate(ks0):
        c = meta["variants"][k]["clip"]
        assert tp0.shapes[n] == (z["c%d_hf" % c].shape[0] + 6, z["c%d_hf" % c].shape[1] + 6) == tuple(z["v%d_padded_dims" % k])
        assert np.array_equal(np.array(tp0.grid_min[n], np.float32), z["v%d_padded_min" % k]) and tp0.vars[n].slice == 0
    assert tp0.points_floats == 0
    # no variants at all
    e = am.TerrainPlan([], clips, np.zeros((0, 4)), am.FramesPlan([], clips), 0, True)
    assert e.n_cells == 0 and e.pool.size == 0 and list(e.cell_start) == [0]


def test_hf_table_from_pool_is_the_table_of_the_terrains(host_runs, g31):
    """the parc_moopt_terrain_t rows the kernels finish equal what HfTable builds from the finished SubTerrains"""
    import torch
    from parc_amd.util import terrain_util
    z, meta, clips = g31
    run, _ = host_runs[0]
    ks = ah.setting_groups(meta)[(3, True)]
    ters = [terrain_util.SubTerrain.from_arrays(run.variant_hf(n), run.variant_min_point(n), run.tp.dxdy[n], device="cpu") for n in range(len(ks))]
    want = terrain_util.HfTable(ters, base_z=-10.0, device="cpu")
    assert bytes(want.entries) == bytes(run.hf_entries)
    assert np.array_equal(want.pool.numpy(), run.pool[:run.tp.out_floats])
    table = terrain_util.HfTable.from_pool(torch.from_numpy(run.pool[:run.tp.out_floats].copy()),
                                           torch.from_numpy(np.frombuffer(bytes(run.hf_entries), np.uint8).copy()), run.tp.shapes)
    assert len(table) == len(ks) and table.shapes == want.shapes and table.base_z == want.base_z
