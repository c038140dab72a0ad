"""The batch sampler's kernels behind one interface for tests/test_mdm_sampler*.py -- TEST INFRASTRUCTURE.

Fixture G32's clips and cases as the tables the entry points of include/parc_mdm_batch.h read (packed by parc_amd.diffusion.batch_tables,
as the sampler packs them), run through the host build of parc_mdm_batch_core.h (mdm_batch_host.cpp, compiled here) or through the
stand-alone program built from the same file with -DMDM_BATCH_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the
case from a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
from parc_amd import _hip, _hip_mdm_batch as mb      # noqa: E402
from parc_amd.anim.motion_lib import _row_layout      # noqa: E402
from parc_amd.diffusion import batch_tables           # noqa: E402
import mdm_sampler_ref as msr                         # noqa: E402

SOURCE = os.path.join(HERE, "mdm_batch_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
OUT_KEYS = ("root_pos", "root_rot", "body_pos", "joint_rot", "contacts", "future_pos", "future_rot", "hfs", "center_h")


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_mdm_batch_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "mdm_batch_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DMDM_BATCH_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


def _p(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(ctypes.c_void_p)
    return ctypes.cast(a, ctypes.c_void_p)


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        for name, args in (("mdm_heightfields_host", mb.HEIGHTFIELDS_ARGTYPES[1:]), ("mdm_windows_host", mb.WINDOWS_ARGTYPES[1:])):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = args
        L.mdm_struct_sizes.restype = ctypes.c_int
        L.mdm_struct_sizes.argtypes = [ctypes.c_void_p]
        _libs[path] = L
    return _libs[path]


class Dataset:
    """fixture G32's clips as the host-side tables: the motion library's rows and struct, the character, the clip tables"""

    def __init__(self, z, meta):
        self.clips = msr.clip_tables(z, meta)
        self.model = msr.model_tables(z)
        B = len(self.model["parent"])
        D = 28
        self.B = B
        lay = _row_layout(B, D)
        nf = np.array([c["root_pos"].shape[0] for c in self.clips], np.int32)
        self.num_frames = nf
        self.start_idx = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int32)
        self.total = int(nf.sum())
        rows = np.zeros((self.total, lay["row_stride"]), np.float32)
        at = 0
        for c in self.clips:
            T = c["root_pos"].shape[0]
            rows[at:at + T, 0:4] = c["root_rot"]
            rows[at:at + T, 4:4 * B] = c["joint_rot"].reshape(T, -1)
            rows[at:at + T, lay["off_pos"]:lay["off_pos"] + 3] = c["root_pos"]
            rows[at:at + T, lay["off_contacts"]:lay["off_contacts"] + B] = c["contacts"]
            at += T
        self.rows = rows
        self.length = np.array([c["length"] for c in self.clips], np.float32)
        self.loop = np.array([c["loop"] for c in self.clips], np.int32)
        self.pos_delta = np.stack([c["pos_delta"] for c in self.clips]).astype(np.float32)
        self.ml = _hip.MotionLibS(len(self.clips), B, D, lay["row_stride"], lay["off_pos"], lay["off_contacts"], lay["off_root_vel"],
                                  lay["off_root_ang_vel"], lay["off_dof_vel"], _p(self.num_frames), _p(self.start_idx), _p(self.length), _p(self.loop),
                                  _p(self.pos_delta), _p(self.rows))
        km = _hip.CharModelS()
        km.num_bodies, km.dof_size, km.max_depth = B, D, 0
        for b in range(B):
            km.parent[b] = int(self.model["parent"][b])
            for e in range(3):
                km.local_translation[b][e] = float(self.model["local_translation"][b][e])
            for e in range(4):
                km.local_rotation[b][e] = float(self.model["local_rotation"][b][e])
        self.km = km
        terrains = [(c["hf"], c["hf_maxmin"], c["min_point"], c["dxdy"]) for c in self.clips]
        lists = []
        for c in self.clips:
            Y = c["hf"].shape[1]
            cs = c["cell_start"]
            lists.append([np.stack([c["cells"][cs[f]:cs[f + 1]] // Y, c["cells"][cs[f]:cs[f + 1]] % Y], -1) for f in range(len(cs) - 1)])
        self.mask_lists = lists
        self.clip_table, self.pool, self.cell_start, self.cells, self.mask_cells = batch_tables.pack_clip_tables(terrains, lists)


class Case:
    """case k of G32 as the entry points' arguments"""

    def __init__(self, z, meta, k):
        self.cfg64 = msr.case_cfg(meta, z, k)
        a = self.a = msr.case_arrays(z, k)
        c = meta["cases"][k]["cfg"]
        self.n = len(a["ids"])
        self.cfg = batch_tables.make_cfg(len(a["motion_times"]), c["ref_idx"], c["grid"][0], c["grid"][2], len(a["grid_x"]), len(a["grid_y"]),
                                         msr.Z_STYLES[c["z_style"]], msr.MODES[c["mode"]], c["max_num_boxes"] if c["mode"] == "MAXPOOL_AND_BOXES" else 0,
                                         c["fps"], c["max_h"])
        self.floor = c["z_style"] == "RELATIVE_TO_ROOT_FLOOR"
        self.ids = np.ascontiguousarray(a["ids"], np.int64)
        self.starts = np.ascontiguousarray(a["starts"], np.float32)
        self.draw_table = self.box_table = None
        if c["mode"] == "MAXPOOL_AND_BOXES":
            raw, off = batch_tables.pack_draws(a["change"], a["new_h"], a["pool_kind"], a["pool_r"], a["nboxes"], a["boxes"], c["max_num_boxes"])
            self.draw_table, self.box_table = raw[:off].copy(), raw[off:].copy()
        self.noise = np.ascontiguousarray(a["noise"], np.float32) if c["mode"] == "NOISE" else None


def run_host(lib, ds, case, debug=True):
    """case through both host entry points -> dict of outputs (+ pre, cell_code)"""
    L = host_lib(lib)
    n, cfg, a = case.n, case.cfg, case.a
    S, X, Y, B = cfg.seq_len, cfg.dim_x, cfg.dim_y, ds.B
    f = lambda *shape: np.full(shape, -7.0, np.float32)       # noqa: E731
    out = dict(root_pos=f(n, S, 3), root_rot=f(n, S, 4), body_pos=f(n, S, B - 1, 3), joint_rot=f(n, S, B - 1, 4), contacts=f(n, S, B),
               future_pos=f(n, 3), future_rot=f(n, 4), hfs=f(n, X, Y), center_h=f(n), pre=f(n, 3, X, Y), cell_code=np.full((n, X, Y), -7, np.int32))
    mt, gx, gy = (np.ascontiguousarray(a[k], np.float32) for k in ("motion_times", "grid_x", "grid_y"))
    rc = L.mdm_heightfields_host(ds.ml, cfg, n, _p(case.ids), _p(case.starts), _p(mt), _p(gx), _p(gy), len(ds.clips), _p(ds.clip_table), _p(ds.pool),
                                 ds.pool.size, _p(ds.cell_start), ds.cell_start.size, _p(ds.cells), ds.cells.size, ds.mask_cells, _p(case.draw_table),
                                 _p(case.box_table), _p(case.noise), _p(out["hfs"]), _p(out["center_h"]), _p(out["pre"]) if debug else None,
                                 _p(out["cell_code"]) if debug else None)
    assert rc == 0, rc
    ft, fn = np.ascontiguousarray(a["future_time"], np.float32), np.ascontiguousarray(a["future_noise"], np.float32)
    rc = L.mdm_windows_host(ds.km, ds.ml, cfg, n, _p(case.ids), _p(case.starts), _p(mt), _p(out["center_h"]) if case.floor else None, _p(ft), _p(fn),
                            _p(out["root_pos"]), _p(out["root_rot"]), _p(out["body_pos"]), _p(out["joint_rot"]), _p(out["contacts"]),
                            _p(out["future_pos"]), _p(out["future_rot"]))
    assert rc == 0, rc
    return out


def dump(path, ds, case):
    """the case file of the stand-alone program"""
    a, cfg, n = case.a, case.cfg, case.n
    with open(path, "wb") as f:
        f.write(np.array([n, len(ds.clips), ds.pool.size, ds.cell_start.size, ds.cells.size, ds.mask_cells, ds.total, case.draw_table is not None,
                          case.noise is not None, case.floor, 0, 0], np.int64).tobytes())
        f.write(bytes(cfg))
        f.write(bytes(ds.km))
        f.write(bytes(ds.ml))
        for arr in (ds.num_frames, ds.start_idx, ds.length, ds.loop, ds.pos_delta, ds.rows, case.ids, case.starts, a["motion_times"].astype(np.float32),
                    a["grid_x"].astype(np.float32), a["grid_y"].astype(np.float32)):
            f.write(np.ascontiguousarray(arr).tobytes())
        f.write(bytes(ds.clip_table)[:len(ds.clips) * ctypes.sizeof(mb.MdmClipS)])
        f.write(ds.pool.tobytes())
        f.write(ds.cell_start.tobytes())
        f.write(ds.cells.tobytes())
        if case.draw_table is not None:
            f.write(case.draw_table.tobytes())
            f.write(case.box_table.tobytes())
        if case.noise is not None:
            f.write(case.noise.tobytes())
        f.write(a["future_time"].astype(np.float32).tobytes())
        f.write(a["future_noise"].astype(np.float32).tobytes())


def read_program_output(path, ds, case):
    raw = np.fromfile(path, dtype=np.float32)
    n, S, X, Y, B = case.n, case.cfg.seq_len, case.cfg.dim_x, case.cfg.dim_y, ds.B
    shapes = [(n, S, 3), (n, S, 4), (n, S, B - 1, 3), (n, S, B - 1, 4), (n, S, B), (n, 3), (n, 4), (n, X, Y), (n,)]
    sizes = [int(np.prod(s)) for s in shapes]
    assert raw.size == sum(sizes), (raw.size, sizes)
    parts = np.split(raw, np.cumsum(sizes)[:-1])
    return {k: p.reshape(s) for k, p, s in zip(OUT_KEYS, parts, shapes)}


# ---------------------------------------------------------------------------------------------------------- the sampler over fixture G32
def write_dataset(z, meta, out_dir, skip_band=None, skip_lists=None):
    """fixture G32's clips as motion files + a dataset yaml, written with the package's own save_motion_data; returns the yaml's path"""
    import torch
    import yaml
    from parc_amd.util import terrain_util
    from parc_amd.zmotion_editing_tools import motion_edit_lib
    entries = []
    for i, c in enumerate(msr.clip_tables(z, meta)):
        ter = terrain_util.SubTerrain.from_arrays(c["hf"], c["min_point"], c["dxdy"], hf_maxmin=None if skip_band == i else c["hf_maxmin"], device="cpu")
        Y, cs = c["hf"].shape[1], c["cell_start"]
        extra = {}
        if skip_lists != i:
            extra["hf_mask_inds"] = [torch.tensor(np.stack([c["cells"][cs[f]:cs[f + 1]] // Y, c["cells"][cs[f]:cs[f + 1]] % Y], -1), dtype=torch.int64)
                                     for f in range(len(cs) - 1)]
        path = os.path.join(out_dir, "clip%d.pkl" % i)
        motion_edit_lib.save_motion_data(path, z["c%d_frames" % i], z["c%d_contacts" % i], ter, int(c["fps"]), "WRAP" if c["loop"] == 1 else "CLAMP",
                                         **extra)
        entries.append(dict(file=path, weight=0.0 if i == 4 else 1.0))      # clip 4 is not drawn (tests/golden/gen_mdm_sampler.py)
    ypath = os.path.join(out_dir, "dataset.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(dict(motions=entries), f)
    return ypath


def sampler_cfg(c, motion_lib, device):
    """the sampler's config keys from a fixture case's cfg (the generator's sampler_cfg)"""
    from parc_amd.anim import kin_char_model
    return {"device": device, "char_file": kin_char_model.default_char_file(), "motion_lib_file": motion_lib,
            "features": {"canonicalize_samples": True, "frame_components": ["ROOT_POS", "ROOT_ROT", "JOINT_POS", "JOINT_ROT", "CONTACTS"]},
            "sequence_fps": c["fps"], "autoregressive": c["autoregressive"], "sequence_duration": (c["S"] - 0.5) / c["fps"],
            "num_prev_states": c["num_prev"], "future_pos_noise_scale": c["noise_scale"], "use_saved_heightmaps": True,
            "relative_z_style": c["z_style"], "hf_augmentation_mode": c["mode"],
            "heightmap": {"horizontal_scale": c["dx"], "max_h": c["max_h"],
                          "local_grid": {"num_x_neg": c["grid"][0], "num_x_pos": c["grid"][1], "num_y_neg": c["grid"][2], "num_y_pos": c["grid"][3]}},
            "use_hf_augmentation": True, "max_num_boxes": c["max_num_boxes"], "box_min_len": c["box_min_len"], "box_max_len": c["box_max_len"],
            "hf_maxpool_chance": c["maxpool_chance"], "hf_max_maxpool_size": c["max_maxpool"], "hf_change_height_chance": c["change_chance"],
            "angle_noise_scale": 0.01, "pos_noise_scale": 0.01, "future_window_min": c["fmin"], "future_window_max": c["fmax"]}


def case_draws(a, device, rows=None):
    """the recorded draws of a case as SamplerDraws (rows: an index array that picks / repeats samples)"""
    import torch
    from parc_amd.diffusion.mdm_heightfield_contact_motion_sampler import SamplerDraws
    r = np.arange(len(a["ids"])) if rows is None else np.asarray(rows)
    t = lambda x: torch.tensor(np.ascontiguousarray(x[r])).to(device)      # noqa: E731
    return SamplerDraws(change_height=a["change"][r], new_height=a["new_h"][r], pool_kind=a["pool_kind"][r], pool_radius=a["pool_r"][r],
                        num_boxes=a["nboxes"][r], boxes=a["boxes"][r], noise=t(a["noise"]), future_time=t(a["future_time"]),
                        future_noise=t(a["future_noise"]))


def check_case(k, got, a, o64, tol, what, exact_hfs):
    """one case's outputs against G32 (a) and the restatement (o64)"""
    for key in msr.COMPARED:
        g = np.asarray(got[key], np.float64)
        assert g.shape == a[key].shape, (what, k, key, g.shape)
        dg, dr = np.abs(g - a[key]), np.abs(g - o64[key])
        if key == "hfs":
            share = o64["unsafe"].reshape(len(g), -1).mean(axis=1)
            assert np.all(share <= msr.EDGE_SHARE), (what, k, share)
            dg, dr = np.where(o64["unsafe"], 0.0, dg), np.where(o64["unsafe"], 0.0, dr)
            if exact_hfs:
                assert dg.max() == 0.0, (what, k, dg.max())
        assert dg.max() <= tol and dr.max() <= tol, (what, k, key, dg.max(), dr.max(), tol)
    assert np.array_equal(np.asarray(got["center_h"], np.float32), a["center_h"]), (what, k)
    on_frame = np.abs(a["starts"] * 30.0 - np.rint(a["starts"] * 30.0)) < 1e-4
    ids30 = np.isin(a["ids"], [0, 2, 3, 4])              # the clips recorded at the sampler's 30 fps
    rows = on_frame & ids30
    assert np.array_equal(np.asarray(got["contacts"], np.float32)[rows], a["contacts"][rows]), (what, k)
