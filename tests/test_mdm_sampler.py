"""The generator's training-batch sampler without a GPU: the host build of the kernels' shared header parc_mdm_batch_core.h
(tests/tools/mdm_batch_host.cpp) and the sampler's loop path on the CPU, against fixture G32 (the reference's own sampler, run by
tests/golden/gen_mdm_sampler.py) and against the float64 restatement tests/mdm_sampler_ref.py.

Bounds.  e-bar is the largest |reference fp32 - float64| over the fixture's motion tensors, targets and heights (measured by
tests/mdm_sampler_ref.py, recorded in DESIGN.md).  Every build is held within 2 e-bar of the restatement and within 2 e-bar of G32: the
same fp32 expression chain evaluated by another libm's sin / cos / sqrt / acos / atan2 is one more fp32 evaluation of the same thing.
Exact: contacts at on-frame start times, center_h, the grid's dims, the mask, the terrain cell each local point reads, the
pre-augmentation heights and band, and (host build and loop path against G32) the heights.  Heights are compared on every cell except
those within 1e-4 cells of a box edge under the restatement; a sample may exclude at most 2 % of its cells.
"""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import mdm_batch_host as mh      # noqa: E402
import mdm_sampler_ref as msr    # noqa: E402

EBAR_RECORDED = 1.800167e-05       # python tests/mdm_sampler_ref.py


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return mh.build_host(str(tmp_path_factory.mktemp("mdm_host")))


@pytest.fixture(scope="module")
def g32():
    z, meta = msr.load()
    return z, meta, mh.Dataset(z, meta)


@pytest.fixture(scope="module")
def ref64(g32):
    """the float64 restatement of every case, computed once"""
    z, meta, _ = g32
    model, clips = msr.model_tables(z), msr.clip_tables(z, meta)
    return [msr.case64(z, meta, k, model, clips) for k in range(len(meta["cases"]))]


@pytest.fixture(scope="module")
def ebar(g32):
    e = msr.measure_ebar(g32[0], g32[1])
    assert abs(e - EBAR_RECORDED) <= 1e-9, e          # the recorded figure is the fixture's
    return e


@pytest.fixture(scope="module")
def host_runs(hostlib, g32):
    z, meta, ds = g32
    return [mh.run_host(hostlib, ds, mh.Case(z, meta, k)) for k in range(len(meta["cases"]))]


@pytest.fixture(scope="module")
def cpu_dataset(tmp_path_factory, g32):
    from parc_amd.anim import kin_char_model
    from parc_amd.diffusion.motion_sampler import TorchMotionLib
    ypath = mh.write_dataset(g32[0], g32[1], str(tmp_path_factory.mktemp("mdm_data")))
    km = kin_char_model.KinCharModel("cpu")
    km.load_char_file(kin_char_model.default_char_file())
    return ypath, TorchMotionLib(ypath, km, "cpu", contact_info=True)


check_case = mh.check_case


def test_host_build_equals_g32_and_float64(host_runs, g32, ref64, ebar):
    z, meta, _ = g32
    for k, out in enumerate(host_runs):
        a, (o64, _) = msr.case_arrays(z, k), ref64[k]
        check_case(k, out, a, o64, 2 * ebar, "host", exact_hfs=True)
        assert np.array_equal(out["pre"], a["pre"]), k
        assert np.array_equal(out["cell_code"] & ((1 << 30) - 1), o64["cell"]) and np.array_equal((out["cell_code"] >> 30) & 1, o64["masked"]), k
        assert out["hfs"].shape[1:] == (len(a["grid_x"]), len(a["grid_y"]))


def test_fixture_covers_the_edge_cases(g32, ref64):
    """the edge cases G32 is built to hold (tests/golden/gen_mdm_sampler.py), checked on the fixture itself"""
    z, meta, _ = g32
    grids, modes, seq, prev, orders, nboxes = set(), set(), set(), set(), set(), set()
    seen = dict(outside=False, past=False, clamp=False, wrap=False, r0=False, rbig=False, on=False, off=False, empty=False, masked=False, long_box=False)
    for k, cs in enumerate(meta["cases"]):
        a, (o64, infos) = msr.case_arrays(z, k), ref64[k]
        c = cs["cfg"]
        X, Y = len(a["grid_x"]), len(a["grid_y"])
        grids.add((X, Y)), modes.add((c["mode"], c["z_style"])), seq.add(len(a["motion_times"])), prev.add(c["num_prev"])
        seen["masked"] |= bool(o64["masked"].any()) and not bool(o64["masked"].all())
        for s, info in enumerate(infos):
            seen["outside"] |= info["outside"]
            seen["past"] |= info["window_past_end"]
            seen["wrap" if a["ids"][s] == 1 else "clamp"] |= info["future_past_end"]
            if c["mode"] == "MAXPOOL_AND_BOXES":
                used = a["pool_kind"][s] >= 0
                seen["on"] |= bool(used.all())
                seen["off"] |= not used.any()
                seen["r0"] |= bool(np.any(used & (a["pool_r"][s] == 0)))
                seen["rbig"] |= bool(np.any(used & (a["pool_r"][s] >= max(X, Y))))
                if used.all():
                    orders.add(tuple(a["pool_kind"][s]))
                nboxes.add(int(a["nboxes"][s]))
                seen["long_box"] |= bool(np.any(a["boxes"][s, :a["nboxes"][s], 2:4] > max(X, Y)))
    for c in range(meta["clips"]):
        seen["empty"] |= bool(np.any(np.diff(z["c%d_cell_start" % c]) == 0))
    assert {(9, 7), (1, 1), (31, 31)} <= grids and len(modes) == 6 and {1, 15} <= seq and {1, 2} <= prev, (grids, modes, seq, prev)
    assert all(seen.values()) and len(orders) == 6 and {0, 1, 4} <= nboxes, (seen, orders, nboxes)
    assert z["c2_root_pos"].shape[0] == meta["S15"] and z["c3_hf"].shape == (1, 1)
    assert os.path.getsize(msr.FIXTURE) < 600 * 1024


def test_loop_path_on_the_cpu_equals_g32(cpu_dataset, g32, ref64, ebar):
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    z, meta, _ = g32
    for k, cs in enumerate(meta["cases"]):
        s = ms.MDMHeightfieldContactMotionSampler(mh.sampler_cfg(cs["cfg"], cpu_dataset[1], "cpu"))
        assert s._path == "loop"
        a = msr.case_arrays(z, k)
        out = s.run_batch(torch.tensor(a["ids"]), torch.tensor(a["starts"]), mh.case_draws(a, "cpu"))
        check_case(k, {key: v.numpy() for key, v in out.items()}, a, ref64[k][0], 2 * ebar, "loop", exact_hfs=True)


def test_seeded_cpu_sampler_reproduces_the_drawn_runs(cpu_dataset, g32, ref64, ebar):
    """the trainer's calling sequence with the fixture's seeds: the same clips, start times and draws as the reference made, exactly,
    and its outputs within the bound"""
    from parc_amd.diffusion import diffusion_util as du
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    z, meta, _ = g32
    drawn = [k for k, cs in enumerate(meta["cases"]) if cs["drawn"]]
    assert len(drawn) == 2
    for k in drawn:
        cs = meta["cases"][k]
        a = msr.case_arrays(z, k)
        s = ms.MDMHeightfieldContactMotionSampler(mh.sampler_cfg(cs["cfg"], cpu_dataset[1], "cpu"))
        for attempt in ("draws", "outputs"):
            random.seed(cs["seed"])
            torch.manual_seed(cs["seed"])
            ids = s._mlib.sample_motions(cs["n"])
            starts = s._sample_motion_start_times(ids, s._sample_seq_time)
            assert np.array_equal(ids.numpy(), a["ids"]) and np.array_equal(starts.numpy(), a["starts"]), k
            if attempt == "draws":
                d = s.make_draws(ids, starts)
                if cs["cfg"]["mode"] == "MAXPOOL_AND_BOXES":
                    for f, g in (("change_height", "change"), ("new_height", "new_h"), ("pool_kind", "pool_kind"), ("pool_radius", "pool_r"),
                                 ("num_boxes", "nboxes"), ("boxes", "boxes")):
                        assert np.array_equal(getattr(d, f), a[g]), (k, f)
                else:
                    assert np.array_equal(d.noise.numpy(), a["noise"]), k
                assert np.array_equal(d.future_time.numpy(), a["future_time"]) and np.array_equal(d.future_noise.numpy(), a["future_noise"]), k
            else:
                motion, hfs, target = s.sample_motion_data(motion_ids=ids, motion_start_times=starts)
                got = dict(root_pos=motion[du.MDMFrameType.ROOT_POS], root_rot=motion[du.MDMFrameType.ROOT_ROT], body_pos=motion[du.MDMFrameType.JOINT_POS],
                           joint_rot=motion[du.MDMFrameType.JOINT_ROT], contacts=motion[du.MDMFrameType.CONTACTS], hfs=hfs,
                           future_pos=target.future_pos, future_rot=target.future_rot, center_h=torch.tensor(a["center_h"]))
                check_case(k, {key: v.numpy() for key, v in got.items()}, a, ref64[k][0], 2 * ebar, "seeded", exact_hfs=True)
                assert list(motion.keys()) == [du.MDMFrameType[c] for c in ("ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS")]
                only = s.sample_motion_data(motion_ids=ids, motion_start_times=starts, ret_hf_obs=False, ret_target_info=False)
                assert isinstance(only, dict) and torch.equal(only[du.MDMFrameType.JOINT_ROT], motion[du.MDMFrameType.JOINT_ROT])


def test_sanitized_program_runs_the_cases(tmp_path, g32, host_runs):
    """parc_mdm_batch_core.h under AddressSanitizer and UBSan in a stand-alone program (its own main, run as a child process): every
    fixture case through both entry points; its results equal the plain host build's bit for bit."""
    z, meta, ds = g32
    exe = mh.build_program(str(tmp_path), sanitize=True)
    for k in range(len(meta["cases"])):
        case = mh.Case(z, meta, k)
        f, o = str(tmp_path / ("k%d.case" % k)), str(tmp_path / ("k%d.out" % k))
        mh.dump(f, ds, case)
        res = subprocess.run([exe, f, o], capture_output=True, text=True)
        assert res.returncode == 0 and "mdm batch ok" in res.stdout, (k, res.returncode, res.stderr[-2000:])
        got = mh.read_program_output(o, ds, case)
        for key in mh.OUT_KEYS:
            assert np.array_equal(got[key], host_runs[k][key]), (k, key)


def test_argument_rules_through_the_library():
    """both entry points answer before any HIP call: no GPU is needed to be refused (or to be told there is nothing to do)"""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_mdm_batch as mb
    from parc_amd.diffusion import batch_tables
    L = _hip.lib()
    assert L.parc_mdm_batch_abi() == 1 and L.parc_abi_version() == 1
    d = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused, or has nothing to launch
    ml = _hip.MotionLibS(2, 15, 28, 112, 60, 63, 78, 81, 84, d, d, d, d, d, d)
    km = _hip.CharModelS()
    km.num_bodies = 15

    def cfg(S=15, ref=1, xn=3, yn=2, X=9, Y=7, z=0, mode=1, boxes=4):
        return batch_tables.make_cfg(S, ref, xn, yn, X, Y, z, mode, boxes, 30, 3.0)

    h_names = ("ids", "starts", "times", "gx", "gy", "clips", "pool", "cell_start", "cells", "draws", "boxes", "noise", "hfs", "center")

    def hf(c=None, n=2, n_clips=2, pf=8, ncs=4, nc=4, mc=64, ml_=ml, **null):
        a = {k: (None if k in null else d) for k in h_names}
        return L.parc_mdm_heightfields(None, ml_, c or cfg(), n, a["ids"], a["starts"], a["times"], a["gx"], a["gy"], n_clips, a["clips"], a["pool"], pf,
                                       a["cell_start"], ncs, a["cells"], nc, mc, a["draws"], a["boxes"], a["noise"], a["hfs"], a["center"], None, None)

    for kw in ("n", "n_clips", "pf", "ncs", "nc", "mc"):
        assert hf(**{kw: -1}) == -1, kw
    for bad in (cfg(S=0), cfg(ref=15), cfg(ref=-1), cfg(X=0), cfg(Y=0), cfg(xn=9), cfg(yn=-1), cfg(z=2), cfg(mode=3), cfg(boxes=-1)):
        assert hf(bad) == -1
    assert hf(cfg(X=64, Y=33, xn=0, yn=0)) == -2 and hf(cfg(X=64, Y=32, xn=0, yn=0), n=0) == 0          # 2112 > 2048 cells; 2048 is in
    assert hf(cfg(boxes=mb.MAX_BOXES + 1)) == -2 and hf(cfg(S=mb.MAX_SEQ_LEN + 1)) == -2 and hf(mc=mb.MAX_TERRAIN_CELLS + 1) == -2
    assert hf(mc=mb.MAX_TERRAIN_CELLS, n=0) == 0
    assert hf(n=0) == 0 and hf(n=0, ids=None, hfs=None) == 0
    for name in ("ids", "starts", "times", "gx", "gy", "clips", "pool", "cell_start", "cells", "draws", "boxes", "hfs", "center"):
        assert hf(**{name: None}) == -1, name
    assert hf(cfg(mode=0), noise=None) == -1 and hf(cfg(mode=0, boxes=0), n=0, noise=None) == 0
    assert hf(cfg(mode=2, boxes=0), n=0, draws=None, boxes=None, noise=None) == 0
    bad_ml = _hip.MotionLibS(2, 15, 28, 112, 60, 63, 78, 81, 84, d, d, None, d, d, d)
    assert hf(ml_=bad_ml) == -1

    w_names = ("ids", "starts", "times", "center", "ftime", "fnoise", "rp", "rr", "bp", "jr", "con", "fp", "fr")

    def win(c=None, n=2, km_=km, ml_=ml, **null):
        a = {k: (None if k in null else d) for k in w_names}
        return L.parc_mdm_windows(None, km_, ml_, c or cfg(), n, a["ids"], a["starts"], a["times"], a["center"], a["ftime"], a["fnoise"], a["rp"], a["rr"],
                                  a["bp"], a["jr"], a["con"], a["fp"], a["fr"])

    assert win(n=-1) == -1 and win(cfg(S=0)) == -1 and win(cfg(S=mb.MAX_SEQ_LEN + 1)) == -2 and win(n=0) == 0
    assert win(cfg(S=1024, ref=0), n=2 ** 31 - 1) == -2                        # n * S lanes do not fit a launch
    for name in ("ids", "starts", "times", "rp", "rr", "bp", "jr", "con"):
        assert win(**{name: None}) == -1, name
    for name in ("ftime", "fnoise", "fp", "fr"):                              # the target: all four or none
        assert win(**{name: None}) == -1, name
    km0, km17 = _hip.CharModelS(), _hip.CharModelS()
    km17.num_bodies = 17
    assert win(km_=km0) == -1 and win(km_=km17) == -1 and win(ml_=bad_ml) == -1


def test_exports_sizes_and_documentation(hostlib):
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_mdm_batch as mb
    with open(os.path.join(REPO, "include", "parc_mdm_batch.h")) as f:
        header = f.read()
    names = sorted(set(re.findall(r"\b(parc_mdm_[a-z0-9_]+)\s*\(", header)))
    assert names == ["parc_mdm_batch_abi", "parc_mdm_heightfields", "parc_mdm_windows"]
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    L = _hip.lib()
    for n in names:
        assert n in _hip.EXPORTED and hasattr(L, n) and n in doc, n
    assert "parc_mdm_batch.hip" in _hip.SOURCES and "-ffp-contract=off" in _hip.OPT_LEVEL["parc_mdm_batch.hip"]
    assert "types=" in doc and "diffusion.diffusion_util" in doc
    from parc_amd import _ALIASES
    assert not any("diffusion" in k for k in _ALIASES)                       # the reference's own diffusion package stays importable beside this one
    # ctypes struct sizes equal the header's, and the caps the Python side names are the header's
    sizes = (ctypes.c_int * 6)()
    assert mh.host_lib(hostlib).mdm_struct_sizes(sizes) == 6
    assert list(sizes) == [ctypes.sizeof(s) for s in (mb.MdmCfgS, mb.MdmClipS, mb.MdmDrawS, mb.MdmBoxS, _hip.MotionLibS, _hip.CharModelS)]
    for name, value in (("PARC_MDM_MAX_LOCAL_CELLS", mb.MAX_LOCAL_CELLS), ("PARC_MDM_MAX_TERRAIN_CELLS", mb.MAX_TERRAIN_CELLS),
                        ("PARC_MDM_MAX_BOXES", mb.MAX_BOXES), ("PARC_MDM_MAX_SEQ_LEN", mb.MAX_SEQ_LEN)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value, name


def test_motion_lib_fills_hf_mask_inds(tmp_path, g32):
    """MotionLib(init_type="motion_file") keeps the per-frame cell lists of a file written by save_motion_data(..., hf_mask_inds=...);
    a file without them gives None.  (Read through the CPU subclass: the loader is MotionLib's own.)"""
    from parc_amd.anim import kin_char_model
    from parc_amd.diffusion.motion_sampler import TorchMotionLib
    z, meta, ds = g32
    ypath = mh.write_dataset(z, meta, str(tmp_path), skip_lists=1)
    km = kin_char_model.KinCharModel("cpu")
    km.load_char_file(kin_char_model.default_char_file())
    m = TorchMotionLib(ypath, km, "cpu", contact_info=True)
    assert isinstance(m._hf_mask_inds, list) and len(m._hf_mask_inds) == m.num_motions() == meta["clips"]
    assert m._hf_mask_inds[1] is None
    for i in (0, 2, 3, 4):
        lists = m._hf_mask_inds[i]
        assert len(lists) == int(m._motion_num_frames[i])
        for f, t in enumerate(lists):
            assert t.dtype == torch.int64 and t.dim() == 2 and t.shape[1] == 2 and t.device.type == "cpu"
            assert np.array_equal(t.numpy(), ds.mask_lists[i][f]), (i, f)


def test_dataset_without_bands_or_cell_lists_is_refused(tmp_path, g32):
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    z, meta, _ = g32
    c = meta["cases"][0]["cfg"]
    for what, kw in (("hf_mask_inds", dict(skip_lists=2)), ("hf_maxmin", dict(skip_band=0))):
        d = tmp_path / what
        d.mkdir()
        ypath = mh.write_dataset(z, meta, str(d), **kw)
        with pytest.raises(ValueError) as e:
            ms.MDMHeightfieldContactMotionSampler(mh.sampler_cfg(c, ypath, "cpu"))
        assert what in str(e.value) and ("clip2.pkl" if what == "hf_mask_inds" else "clip0.pkl") in str(e.value)


def test_shipped_config_keys_floor_heights_and_types(cpu_dataset):
    """the sampler keys of the shipped PARC/train_gen_default.yaml construct a sampler as they are; FLOOR_HEIGHTS raises; types= swaps
    the key and return classes"""
    import enum
    import types as pytypes
    from parc_amd.anim import kin_char_model
    from parc_amd.diffusion import diffusion_util as du
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    shipped = {"features": {"frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"], "canonicalize_samples": True},
               "autoregressive": True, "sequence_duration": 0.5, "sequence_fps": 30, "num_prev_states": 2, "use_heightmap_obs": True,
               "use_saved_heightmaps": True, "use_hf_augmentation": True, "relative_z_style": "RELATIVE_TO_ROOT", "hf_augmentation_mode": "MAXPOOL_AND_BOXES",
               "max_num_boxes": 4, "box_min_len": 2, "box_max_len": 12, "hf_maxpool_chance": 0.15, "hf_max_maxpool_size": 10, "hf_change_height_chance": 0.1,
               "angle_noise_scale": 0.01, "pos_noise_scale": 0.01, "future_pos_noise_scale": 0.05,
               "heightmap": {"horizontal_scale": 0.2, "local_grid": {"num_x_neg": 10, "num_x_pos": 20, "num_y_neg": 15, "num_y_pos": 15}, "max_h": 3.0},
               "future_window_min": 0.4, "future_window_max": 1.5}
    cfg = dict(shipped, device="cpu", char_file=kin_char_model.default_char_file(), motion_lib_file=cpu_dataset[1])
    s = ms.MDMHeightfieldContactMotionSampler(cfg)
    assert (s._grid_dim_x, s._grid_dim_y) == (31, 31) and s.get_seq_len() == s._motion_times.shape[0] and s._mlib is cpu_dataset[1]
    assert s._kin_char_model.get_num_joints() == 15 and s._hf_augmentation_mode == ms.HFAugmentationMode.MAXPOOL_AND_BOXES
    random.seed(5)
    torch.manual_seed(5)
    motion, hfs, target = s.sample_motion_data(num_samples=3)
    S = s.get_seq_len()
    assert motion[du.MDMFrameType.ROOT_POS].shape == (3, S, 3) and motion[du.MDMFrameType.JOINT_POS].shape == (3, S, 14, 3)
    assert hfs.shape == (3, 31, 31) and float(hfs.abs().max()) <= 3.0 and isinstance(target, du.TargetInfo) and target.future_rot.shape == (3, 4)
    s.update_old_sampler()
    assert s._relative_z_style == du.RelativeZStyle.RELATIVE_TO_ROOT
    # the reference's names and values
    assert [(m.name, m.value) for m in du.MDMFrameType] == [("ROOT_POS", 0), ("ROOT_ROT", 1), ("JOINT_POS", 2), ("JOINT_VEL", 3), ("JOINT_ROT", 4),
                                                            ("CONTACTS", 5), ("FLOOR_HEIGHTS", 6)]
    assert [(m.name, m.value) for m in du.RelativeZStyle] == [("RELATIVE_TO_ROOT", 0), ("RELATIVE_TO_ROOT_FLOOR", 1)]
    assert [(m.name, m.value) for m in ms.HFAugmentationMode] == [("NOISE", 0), ("MAXPOOL_AND_BOXES", 1), ("NONE", 2)]

    with pytest.raises(NotImplementedError, match="FLOOR_HEIGHTS"):
        ms.MDMHeightfieldContactMotionSampler(dict(cfg, features={"frame_components": ["ROOT_POS", "FLOOR_HEIGHTS"], "canonicalize_samples": True}))
    # JOINT_VEL yields no entry, as in the reference
    s2 = ms.MDMHeightfieldContactMotionSampler(dict(cfg, features={"frame_components": ["ROOT_POS", "JOINT_VEL"], "canonicalize_samples": True}))
    assert list(s2.sample_motion_data(num_samples=2, ret_hf_obs=False, ret_target_info=False).keys()) == [du.MDMFrameType.ROOT_POS]

    class OtherFrameType(enum.Enum):
        ROOT_POS = 0
        ROOT_ROT = 1
        JOINT_POS = 2
        JOINT_VEL = 3
        JOINT_ROT = 4
        CONTACTS = 5
        FLOOR_HEIGHTS = 6

    class OtherZ(enum.Enum):
        RELATIVE_TO_ROOT = 0
        RELATIVE_TO_ROOT_FLOOR = 1

    class OtherTarget:
        def __init__(self, future_pos, future_rot):
            self.future_pos, self.future_rot = future_pos, future_rot

    other = pytypes.SimpleNamespace(MDMFrameType=OtherFrameType, RelativeZStyle=OtherZ, TargetInfo=OtherTarget)
    s3 = ms.MDMHeightfieldContactMotionSampler(dict(cfg, relative_z_style="RELATIVE_TO_ROOT_FLOOR"), types=other)
    motion, hfs, target = s3.sample_motion_data(num_samples=2)
    assert set(motion.keys()) == {OtherFrameType.ROOT_POS, OtherFrameType.ROOT_ROT, OtherFrameType.JOINT_POS, OtherFrameType.JOINT_ROT,
                                  OtherFrameType.CONTACTS}
    assert isinstance(target, OtherTarget) and s3._relative_z_style is OtherZ.RELATIVE_TO_ROOT_FLOOR
