"""The dataset augmentation on the device: the three kernels of include/parc_augment.h on every case of fixture G31,
augment_motions.prepare_variants against the host build, a NaN frame that stays alone, 70 000 one-cell variants,
add_boxes_to_hf_at_xy_points on a device tensor, and augment_dataset end to end against per-variant motion_contact_optimization.

Bounds as in tests/test_augment.py, with 4 e-bar for the device's frames (its sqrt / atan2 / sin / cos sequences are not the host's):
xy, z, the dofs, the contacts, bounds, dims and min points exact, heights bit-identical (boxes: on the safe cells, unsafe share <= 2 %)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from test_hip_parity import DEV, T, km  # noqa: F401  (km is a fixture)
from test_motion_opt_gpu import _problem

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
import augment_host as ah      # noqa: E402
import augment_ref as ar       # noqa: E402
from test_augment import check_variant      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return ah.build_host(str(tmp_path_factory.mktemp("augment_host_gpu")))


@pytest.fixture(scope="module")
def g31():
    z, meta = ar.load_fixture()
    return z, meta, ah.fixture_clips(z, meta)


@pytest.fixture(scope="module")
def ebar(g31):
    return ar.measure_ebar(g31[0], g31[1])


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


class DeviceRun:
    """specs through the three device entry points, driven here call by call (HostRun's counterpart); keeps the frames before localising"""

    def __init__(self, specs, clips, pad, slice_terrain, bounds_check=True):
        from parc_amd import _hip
        from parc_amd.tools.motion_opt import augment_motions as am
        L, st = _hip.lib(), _hip.stream()
        fp = self.fp = am.FramesPlan(specs, clips)
        V, C = fp.V, fp.contact_width
        src_frames, src_contacts, ftable = am._upload([fp.src_frames, fp.src_contacts, fp.table], DEV)
        frames = torch.full((fp.n_out, 34), -7.0, dtype=torch.float32, device=DEV)
        contacts = torch.full((fp.n_out, C), -7.0, dtype=torch.float32, device=DEV)
        bounds = torch.full((V, 4), -7.0, dtype=torch.float32, device=DEV)
        _hip.check(L.parc_augment_frames(st, V, fp.src_frames.shape[0], C, _vp(src_frames), _vp(src_contacts), _vp(ftable), fp.n_out, _vp(frames),
                                         _vp(contacts), _vp(bounds)), "parc_augment_frames")
        self.bounds = bounds.cpu().numpy()
        self.transformed = frames.cpu().numpy()
        self.contacts = contacts.cpu().numpy()
        if not bounds_check:
            return
        tp = self.tp = am.TerrainPlan(specs, clips, self.bounds, fp, pad, slice_terrain)
        pool_b, src_pool, src_table, out_table, vars_t, boxes, cell_start, hf_table = am._upload(
            [tp.pool, tp.src_pool, tp.src_table, tp.out_table, tp.vars, tp.boxes, tp.cell_start, tp.hf_entries], DEV)
        pool = pool_b.view(torch.float32)
        canon = torch.full((V, 3), float("nan"), dtype=torch.float32, device=DEV)
        _hip.check(L.parc_augment_terrains(st, V, tp.n_cells, _vp(cell_start), _vp(vars_t), len(clips), _vp(src_table), _vp(src_pool), tp.src_pool.size,
                                           _vp(out_table), _vp(pool[tp.out_floats:]) if tp.points_floats else None, tp.points_floats, _vp(boxes),
                                           tp.n_boxes, _vp(frames), fp.n_out, _vp(pool), tp.out_floats, _vp(canon)), "parc_augment_terrains")
        _hip.check(L.parc_augment_localize(st, V, _vp(vars_t), _vp(canon), _vp(frames), fp.n_out, _vp(hf_table)), "parc_augment_localize")
        torch.cuda.synchronize()
        self.frames, self.pool, self.canon = frames.cpu().numpy(), pool.cpu().numpy(), canon.cpu().numpy()
        self.hf_table = np.frombuffer(hf_table.cpu().numpy().tobytes(), dtype=np.dtype([("i", np.int32, 5), ("f", np.float32, 5)]))

    def variant(self, n):
        o, ln = self.fp.out_off[n], self.fp.lengths[n]
        X, Y = self.tp.shapes[n]
        off = self.tp.hf_entries[n].off_hf
        return dict(frames=self.frames[o:o + ln], transformed=self.transformed[o:o + ln], contacts=self.contacts[o:o + ln], bounds=self.bounds[n],
                    hf=self.pool[off:off + X * Y].reshape(X, Y), min_point=self.hf_table[n]["f"][0:2].copy())


@pytest.fixture(scope="module")
def device_runs(g31):
    z, meta, clips = g31
    runs = {}
    for (pad, sl), ks in ah.setting_groups(meta).items():
        run = DeviceRun([ah.fixture_spec(z, meta, k) for k in ks], clips, pad, sl)
        for n, k in enumerate(ks):
            runs[k] = (run, n)
    return runs


def test_device_kernels_on_every_g31_case(device_runs, g31, ebar):
    z, meta, _ = g31
    for k in range(len(meta["variants"])):
        run, n = device_runs[k]
        v = run.variant(n)
        check_variant(z, meta, k, v["frames"], v["transformed"], v["contacts"], v["bounds"], v["hf"], v["min_point"], 4 * ebar, "device")
    out = device_runs[8][0].variant(device_runs[8][1])["frames"][:, 3:6]          # zero exp-map, heading 0
    assert np.all(out == 0.0) and not np.signbit(out).any()


def test_prepare_variants_equals_the_host_build(hostlib, g31, ebar):
    from parc_amd.tools.motion_opt import augment_motions as am
    z, meta, clips = g31
    for (pad, sl), ks in ah.setting_groups(meta).items():
        specs = [ah.fixture_spec(z, meta, k) for k in ks]
        host = ah.HostRun(hostlib, specs, clips, pad, sl)
        prep = am.prepare_variants(specs, clips, DEV, pad, sl)
        frames, contacts, terrains = prep
        table = prep.hf_table()
        assert len(table) == len(ks) and table.shapes == host.tp.shapes
        dev_table = table.table.cpu().numpy().tobytes()
        assert dev_table == bytes(host.hf_entries)[:len(ks) * 40]                   # offsets, dims, localised origins, half cells, base_z
        for n, k in enumerate(ks):
            f = frames[n].cpu().numpy()
            want = host.variant_frames(n)
            assert np.array_equal(f[:, 0:3], want[:, 0:3]) and np.array_equal(f[:, 6:], want[:, 6:])
            err = np.abs(f - want).max()
            print("variant {:2d}: max |device - host| frames {:.3e} bound {:.3e}".format(k, err, 4 * ebar))
            assert err <= 4 * ebar, (k, err)
            assert np.array_equal(contacts[n].cpu().numpy(), host.variant_contacts(n))
            t = terrains[n]
            hf, want_hf = t.hf.cpu().numpy(), host.variant_hf(n)
            assert hf.shape == want_hf.shape == tuple(t.dims.tolist()) and t.hf.device.type == "cuda"
            assert np.array_equal(t.min_point.cpu().numpy(), host.variant_min_point(n)) and np.array_equal(t.min_point.cpu().numpy(), z["v%d_min_point" % k])
            assert np.array_equal(t.dxdy.cpu().numpy(), z["c%d_dxdy" % meta["variants"][k]["clip"]])
            assert t.hf_mask.shape == hf.shape and t.hf_maxmin.shape == hf.shape + (2,)
            safe = ~ar.variant64(z, meta, k)[2]["unsafe"]
            assert np.array_equal(hf[safe].view(np.uint32), want_hf[safe].view(np.uint32)), k


def test_nan_frame_stays_alone_and_is_named(g31):
    from parc_amd.tools.motion_opt import augment_motions as am
    z, meta, clips = g31
    ks = ah.setting_groups(meta)[(3, True)]
    specs = [ah.fixture_spec(z, meta, k) for k in ks]
    clean = DeviceRun(specs, clips, 3, True)
    bad_clip = am.SeedClip("bad", z["c1_frames"].copy(), z["c1_contacts"], clips[1].terrain, meta["fps"])
    bad_clip.frames[2, 1] = float("nan")
    n_bad = [n for n, k in enumerate(ks) if meta["variants"][k]["clip"] == 1][0]
    clips2, specs2 = list(clips) + [bad_clip], list(specs)
    specs2[n_bad] = ah.fixture_spec(z, meta, ks[n_bad])
    specs2[n_bad].file_index, specs2[n_bad].name = len(clips), "the_bad_one"
    dirty = DeviceRun(specs2, clips2, 3, True, bounds_check=False)
    assert np.isnan(dirty.bounds[n_bad]).all()
    assert np.array_equal(np.delete(dirty.bounds, n_bad, axis=0), np.delete(clean.bounds, n_bad, axis=0))
    keep = np.ones(clean.fp.n_out, bool)
    keep[clean.fp.out_off[n_bad]:clean.fp.out_off[n_bad] + clean.fp.lengths[n_bad]] = False
    assert np.array_equal(dirty.transformed[keep], clean.transformed[keep]) and np.array_equal(dirty.contacts[keep], clean.contacts[keep])
    with pytest.raises(ValueError, match="the_bad_one"):
        am.prepare_variants(specs2, clips2, DEV, 3, True)
    # the terrain kernel with that variant's frames NaN (its table kept): NaN heights for it, every other variant's heights bit-identical
    from parc_amd import _hip
    fp, tp = clean.fp, clean.tp
    pool_b, src_pool, src_table, out_table, vars_t, boxes, cell_start = am._upload(
        [tp.pool, tp.src_pool, tp.src_table, tp.out_table, tp.vars, tp.boxes, tp.cell_start], DEV)
    pool = pool_b.view(torch.float32)
    frames = torch.tensor(dirty.transformed, device=DEV)
    canon = torch.zeros((fp.V, 3), dtype=torch.float32, device=DEV)
    _hip.check(_hip.lib().parc_augment_terrains(_hip.stream(), fp.V, tp.n_cells, _vp(cell_start), _vp(vars_t), len(clips), _vp(src_table), _vp(src_pool),
                                                tp.src_pool.size, _vp(out_table), _vp(pool[tp.out_floats:]), tp.points_floats, _vp(boxes), tp.n_boxes,
                                                _vp(frames), fp.n_out, _vp(pool), tp.out_floats, _vp(canon)), "parc_augment_terrains")
    got = pool.cpu().numpy()
    for n in range(fp.V):
        X, Y = tp.shapes[n]
        off = tp.hf_entries[n].off_hf
        if n != n_bad:
            assert np.array_equal(got[off:off + X * Y], clean.pool[off:off + X * Y]), n
    # (variant n_bad's first frame is finite, so its heights are too, except where a NaN frame centres a box - it has none: HEIGHT_SCALE)
    assert np.isfinite(got[:tp.out_floats]).all()


def test_70000_one_cell_variants(hostlib):
    """no grid-dimension limit: 70 000 variants of one frame and one cell each through all three kernels, equal to the host build"""
    from parc_amd import _hip, _hip_augment, _hip_moopt
    V = 70000
    rng = np.random.default_rng(7)
    hf = rng.uniform(-1, 1, size=(9, 11)).astype(np.float32)
    src_frames = rng.uniform(-2, 2, size=(16, 34)).astype(np.float32)
    src_contacts = (rng.uniform(size=(16, 15)) > 0.5).astype(np.float32)
    ft = np.zeros(V, dtype=np.dtype(_hip_augment.AugFramesS))
    ang = rng.uniform(-np.pi, np.pi, size=V)
    ft["src_off"], ft["src_len"], ft["start"], ft["length"], ft["out_off"] = 0, 16, rng.integers(0, 16, size=V), 1, np.arange(V)
    ft["cos_h"], ft["sin_h"], ft["qz"], ft["qw"] = np.cos(ang), np.sin(ang), np.sin(ang / 2), np.cos(ang / 2)
    ft["sx"], ft["sy"] = rng.uniform(0.8, 1.2, size=V), rng.uniform(0.8, 1.2, size=V)
    L = ah.host_lib(hostlib)
    h_frames, h_contacts, h_bounds = np.zeros((V, 34), np.float32), np.zeros((V, 15), np.float32), np.zeros((V, 4), np.float32)
    assert L.augment_frames_host(V, 16, 15, ah._p(src_frames), ah._p(src_contacts), ah._p(ft), V, ah._p(h_frames), ah._p(h_contacts), ah._p(h_bounds)) == 0
    st = np.zeros(1, dtype=np.dtype(_hip_augment.AugTerrainS))
    st["dim_x"], st["dim_y"], st["min_x"], st["min_y"], st["dx"], st["dy"] = 9, 11, -1.6, -2.0, 0.4, 0.4
    ot = np.zeros(V, dtype=np.dtype(_hip_augment.AugTerrainS))
    ot["off_hf"], ot["off_x"], ot["off_y"], ot["dim_x"], ot["dim_y"] = np.arange(V), 2 * np.arange(V), 2 * np.arange(V) + 1, 1, 1
    ot["dx"], ot["dy"] = 0.4, 0.4
    points = np.ascontiguousarray((np.round((h_frames[:, 0:2] - st["min_x"][0]) / 0.4) * 0.4 + st["min_x"][0]).astype(np.float32)).reshape(-1)
    ot["min_x"], ot["min_y"] = points[0::2], points[1::2]
    vt = np.zeros(V, dtype=np.dtype(_hip_augment.AugVariantS))
    vt["pad"], vt["mode"], vt["slice"], vt["frame_off"], vt["frame_len"], vt["scale"] = 1, _hip_augment.MODE_HEIGHT_SCALE, 1, np.arange(V), 1, 0.5
    cells = np.arange(V + 1, dtype=np.int64)
    hft = np.zeros(V, dtype=np.dtype(_hip_moopt.MooptTerrainS))
    hft["ox"], hft["oy"] = ot["min_x"], ot["min_y"]
    h_pool, h_canon, h_hft, h_loc = np.zeros(V, np.float32), np.zeros((V, 3), np.float32), hft.copy(), h_frames.copy()
    assert L.augment_terrains_host(V, V, ah._p(cells), ah._p(vt), 1, ah._p(st), ah._p(hf), hf.size, ah._p(ot), ah._p(points), points.size, None, 0,
                                   ah._p(h_loc), V, ah._p(h_pool), V, ah._p(h_canon)) == 0
    assert L.augment_localize_host(V, ah._p(vt), ah._p(h_canon), ah._p(h_loc), V, ah._p(h_hft)) == 0
    # (the one cell of a variant is the cell under its first frame: its height is 0 after re-centring, and canon z carries the lookup)
    assert np.all(h_pool == 0.0) and len(np.unique(h_canon[:, 2])) > 20

    def up(a):
        return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(DEV)
    d = {k: up(a) for k, a in dict(src_frames=src_frames, src_contacts=src_contacts, ft=ft, st=st, hf=hf, ot=ot, points=points, vt=vt, cells=cells,
                                   hft=hft).items()}
    frames = torch.zeros((V, 34), dtype=torch.float32, device=DEV)
    contacts = torch.zeros((V, 15), dtype=torch.float32, device=DEV)
    bounds, pool, canon = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((V, 4), (V,), (V, 3)))
    lib, stream = _hip.lib(), _hip.stream()
    _hip.check(lib.parc_augment_frames(stream, V, 16, 15, _vp(d["src_frames"]), _vp(d["src_contacts"]), _vp(d["ft"]), V, _vp(frames), _vp(contacts),
                                       _vp(bounds)), "parc_augment_frames")
    # the device's own xy are the host's bit for bit (separately rounded products), so the same points serve both
    assert np.array_equal(frames[:, 0:3].cpu().numpy(), h_frames[:, 0:3]) and np.array_equal(bounds.cpu().numpy(), h_bounds)
    _hip.check(lib.parc_augment_terrains(stream, V, V, _vp(d["cells"]), _vp(d["vt"]), 1, _vp(d["st"]), _vp(d["hf"]), hf.size, _vp(d["ot"]), _vp(d["points"]),
                                         points.size, None, 0, _vp(frames), V, _vp(pool), V, _vp(canon)), "parc_augment_terrains")
    _hip.check(lib.parc_augment_localize(stream, V, _vp(d["vt"]), _vp(canon), _vp(frames), V, _vp(d["hft"])), "parc_augment_localize")
    torch.cuda.synchronize()
    assert np.array_equal(pool.cpu().numpy(), h_pool) and np.array_equal(canon.cpu().numpy(), h_canon)
    assert np.array_equal(frames[:, 0:3].cpu().numpy(), h_loc[:, 0:3]) and np.array_equal(contacts.cpu().numpy(), h_contacts)
    assert d["hft"].cpu().numpy().tobytes() == h_hft.tobytes()
    assert np.array_equal(frames[-1, 0:2].cpu().numpy(), np.zeros(2, np.float32))          # the last variant was reached and localised


def test_add_boxes_on_a_device_tensor_equals_g31(g31):
    from parc_amd.util import terrain_util
    z, meta, _ = g31
    cfg = meta["box_cfg"]
    for k in (2, 3, 7, 9):
        v = meta["variants"][k]
        c = v["clip"]
        base = ar.build_terrain64(z["v%d_transformed" % k], z["c%d_hf" % c], z["c%d_min_point" % c], z["c%d_dxdy" % c], v["pad"], v["slice"],
                                  z["v%d_dims" % k], z["v%d_grid_min" % k], "NONE")["hf"]
        hf = torch.tensor(base.astype(np.float32), device=DEV)
        random.seed(v["seed"])
        torch.manual_seed(v["seed"])
        terrain_util.add_boxes_to_hf_at_xy_points(torch.tensor(z["v%d_box_centers" % k], device=DEV), hf, cfg["min_h"], cfg["max_h"], cfg["min_len"],
                                                  cfg["max_len"], cfg["min_angle"], cfg["max_angle"])
        safe = ~ar.variant64(z, meta, k)[2]["unsafe"]
        got, want = hf.cpu().numpy(), z["v%d_hf" % k]
        # (variant 9 has a box centred outside the grid that reaches into it)
        assert (got != base.astype(np.float32)).sum() > 4 and safe.mean() >= 0.98
        assert np.array_equal(got[safe].view(np.uint32), want[safe].view(np.uint32)), k


def test_augment_dataset_end_to_end(km, g31, tmp_path):
    """3 variants from G31's seeds, 10 iterations, opt_batch_size 3: the descent inside augment_dataset against per-variant
    motion_contact_optimization on the same prepared inputs (bound of tests/test_motion_opt_batch_gpu.py, "each motion alone against inside
    the batch": 2e-3 of the first total, on every iteration's total), and the written files read back."""
    from parc_amd.tools.motion_opt import augment_motions as am
    from parc_amd.tools.motion_opt import motion_optimization as mo
    from parc_amd.zmotion_editing_tools import motion_edit_lib
    z, meta, clips = g31
    pts, _, w, max_jerk = _problem(golden("g20_motion_opt"))
    cfg = dict(meta["runs"][1]["cfg"])
    cfg.update(device=DEV, num_new_motions=3, output_folder_path=str(tmp_path / "out") + "/", num_iters=10, step_size=0.001, opt_batch_size=3,
               use_wandb=False, max_jerk=max_jerk, **{k: w[k] for k in w if k != "w_body_constraints"})
    random.seed(77)
    torch.manual_seed(77)
    traces = []
    paths = am.augment_dataset(cfg, clips=clips, char_model=km, body_points=pts, verbose=False, loss_trace=traces)
    assert len(paths) == 3 and len(traces) == 1 and traces[0].shape == (10, 3)
    inside = traces[0].cpu().numpy()
    random.seed(77)
    torch.manual_seed(77)
    specs = am.draw_variants(cfg, clips)
    frames, contacts, terrains = am.prepare_variants(specs, clips, DEV, cfg["terrain_padding_size"], cfg["slice_terrain"])
    assert [os.path.basename(p) for p in paths] == [s.name + ".pkl" for s in specs]
    for n, s in enumerate(specs):
        trace = []
        single = mo.motion_contact_optimization(src_frames=frames[n], contacts=contacts[n], body_points=pts, terrain=terrains[n], char_model=km, num_iters=10,
                                                step_size=0.001, body_constraints=None, max_jerk=max_jerk, exp_name=None, use_wandb=False, log_file=None,
                                                use_graph=True, verbose=False, loss_trace=trace, **am.loss_weights(cfg))
        alone = trace[0].cpu().numpy()
        diff = np.abs(alone - inside[:, n]).max()
        print("variant {} alone vs inside augment_dataset {:.3e} bound {:.3e}".format(n, diff, 2e-3 * inside[0, n]))
        assert np.isfinite(inside[:, n]).all() and diff <= 2e-3 * inside[0, n], (n, diff)
        md = motion_edit_lib.load_motion_file(paths[n])
        assert os.path.exists(os.path.join(cfg["output_folder_path"], "log", "log_" + s.name + ".txt"))
        assert md.get_fps() == 30 and md.get_loop_mode() == "CLAMP"
        assert tuple(md.get_frames().shape) == (s.length, 34) == tuple(single.shape) and tuple(md.get_contacts().shape) == (s.length, 15)
        ter = md.get_terrain()
        X, Y = terrains[n].hf.shape
        assert tuple(ter.hf.shape) == (X, Y) and tuple(ter.hf_mask.shape) == (X, Y) and tuple(ter.hf_maxmin.shape) == (X, Y, 2)
        assert np.array_equal(ter.hf.numpy(), terrains[n].hf.cpu().numpy()) and np.array_equal(ter.min_point.numpy(), terrains[n].min_point.cpu().numpy())
        assert np.array_equal(ter.dims.numpy(), [X, Y]) and np.array_equal(md.get_contacts().numpy(), contacts[n].cpu().numpy())
        moved = np.abs(md.get_frames().numpy() - frames[n].cpu().numpy()).max()
        assert 0 < moved < 0.1          # ten steps of 1e-3
