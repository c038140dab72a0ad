"""The dataset augmentation behind one interface for tests/test_augment*.py -- TEST INFRASTRUCTURE.

The plans of parc_amd.tools.motion_opt.augment_motions (FramesPlan, TerrainPlan: pure host code) run through the host build of
parc_augment_core.h (augment_host.cpp, compiled here), or through the stand-alone program built from the same file with
-DAUGMENT_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the case from a file.  Also here: fixture G31 as seed clips
and variant specs.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from parc_amd import _hip_augment, _hip_moopt      # noqa: E402

SOURCE = os.path.join(HERE, "augment_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_augment_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "augment_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DAUGMENT_HOST_MAIN"] + FLAGS +
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
        for name, args in (("augment_frames_host", _hip_augment.FRAMES_ARGTYPES[1:]), ("augment_terrains_host", _hip_augment.TERRAINS_ARGTYPES[1:]),
                           ("augment_localize_host", _hip_augment.LOCALIZE_ARGTYPES[1:])):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = args
        _libs[path] = L
    return _libs[path]


# ---------------------------------------------------------------------------------------------------------- fixture G31
def fixture_clips(z, meta):
    """the seed clips of G31 as augment_motions.SeedClip"""
    from parc_amd.tools.motion_opt import augment_motions as am
    from parc_amd.util import terrain_util
    clips = []
    for c in range(meta["clips"]):
        ter = terrain_util.SubTerrain.from_arrays(z["c%d_hf" % c], z["c%d_min_point" % c], z["c%d_dxdy" % c], device="cpu")
        clips.append(am.SeedClip("clip%d" % c, z["c%d_frames" % c], z["c%d_contacts" % c], ter, meta["fps"]))
    return clips


def fixture_spec(z, meta, k):
    """variant k of G31 as augment_motions.VariantSpec (its draws as the fixture recorded them)"""
    import torch
    from parc_amd.tools.motion_opt import augment_motions as am
    v = meta["variants"][k]
    kw = {}
    if v["mode"] == "HEIGHT_SCALE":
        kw["height_scale"] = v["height_scale"]
    elif v["mode"] == "BOXES_ALONG_PATH":
        kw.update(frame_inds=torch.tensor(z["v%d_frame_inds" % k], dtype=torch.int64), box_len=torch.tensor(z["v%d_box_len" % k]),
                  box_angle=z["v%d_box_angle" % k].tolist(), box_h=z["v%d_box_h" % k].tolist())
    return am.VariantSpec(v["clip"], "v%d" % k, v["start"], v["length"], v["heading"], v["sx"], v["sy"], am.TerrainAugmentationType[v["mode"]], **kw)


def setting_groups(meta):
    """fixture variants grouped by what one prepare_variants call shares: {(pad, slice): [k, ...]}"""
    groups = {}
    for k, v in enumerate(meta["variants"]):
        groups.setdefault((v["pad"], bool(v["slice"])), []).append(k)
    return groups


# ---------------------------------------------------------------------------------------------------------- running plans
class HostRun:
    """specs through the three host entry points, as prepare_variants drives the device ones"""

    def __init__(self, lib, specs, clips, pad, slice_terrain):
        from parc_amd.tools.motion_opt import augment_motions as am
        L = host_lib(lib)
        fp = self.fp = am.FramesPlan(specs, clips)
        V, C = fp.V, fp.contact_width
        self.frames = np.full((fp.n_out, _hip_augment.FRAME_DIM), -7.0, np.float32)
        self.contacts = np.full((fp.n_out, C), -7.0, np.float32)
        self.bounds = np.full((V, 4), -7.0, np.float32)
        rc = L.augment_frames_host(V, fp.src_frames.shape[0], C, _p(fp.src_frames), _p(fp.src_contacts), _p(fp.table), fp.n_out, _p(self.frames),
                                   _p(self.contacts), _p(self.bounds))
        assert rc == 0, rc
        self.transformed = self.frames.copy()
        tp = self.tp = am.TerrainPlan(specs, clips, self.bounds, fp, pad, slice_terrain)
        self.pool = tp.pool.copy()
        self.canon = np.full((V, 3), np.nan, np.float32)
        self.hf_entries = (_hip_moopt.MooptTerrainS * max(V, 1)).from_buffer_copy(bytes(tp.hf_entries))
        points = self.pool[tp.out_floats:]
        rc = L.augment_terrains_host(V, tp.n_cells, _p(tp.cell_start), _p(tp.vars), len(clips), _p(tp.src_table), _p(tp.src_pool), tp.src_pool.size,
                                     _p(tp.out_table), _p(points) if tp.points_floats else None, tp.points_floats, _p(tp.boxes), tp.n_boxes,
                                     _p(self.frames), fp.n_out, _p(self.pool), tp.out_floats, _p(self.canon))
        assert rc == 0, rc
        rc = L.augment_localize_host(V, _p(tp.vars), _p(self.canon), _p(self.frames), fp.n_out, _p(self.hf_entries))
        assert rc == 0, rc

    def variant_frames(self, k, transformed=False):
        o, n = self.fp.out_off[k], self.fp.lengths[k]
        return (self.transformed if transformed else self.frames)[o:o + n]

    def variant_contacts(self, k):
        o, n = self.fp.out_off[k], self.fp.lengths[k]
        return self.contacts[o:o + n]

    def variant_hf(self, k):
        X, Y = self.tp.shapes[k]
        off = self.tp.hf_entries[k].off_hf
        return self.pool[off:off + X * Y].reshape(X, Y)

    def variant_min_point(self, k):
        return np.array([self.hf_entries[k].ox, self.hf_entries[k].oy], np.float32)


def dump(path, fp, tp, n_sources):
    """the case file of the stand-alone program"""
    with open(path, "wb") as f:
        f.write(np.array([fp.V, fp.src_frames.shape[0], fp.contact_width, fp.n_out, n_sources, tp.src_pool.size, tp.out_floats, tp.points_floats,
                          tp.n_boxes, tp.n_cells, 0, 0], np.int64).tobytes())
        f.write(fp.src_frames.tobytes())
        f.write(fp.src_contacts.tobytes())
        f.write(bytes(fp.table)[:fp.V * ctypes.sizeof(_hip_augment.AugFramesS)])
        f.write(bytes(tp.src_table)[:n_sources * ctypes.sizeof(_hip_augment.AugTerrainS)])
        f.write(tp.src_pool.tobytes())
        f.write(bytes(tp.out_table)[:fp.V * ctypes.sizeof(_hip_augment.AugTerrainS)])
        f.write(bytes(tp.vars)[:fp.V * ctypes.sizeof(_hip_augment.AugVariantS)])
        f.write(bytes(tp.boxes)[:tp.n_boxes * ctypes.sizeof(_hip_augment.AugBoxS)])
        f.write(tp.cell_start.tobytes())
        f.write(tp.pool.tobytes())
        f.write(bytes(tp.hf_entries)[:fp.V * ctypes.sizeof(_hip_moopt.MooptTerrainS)])


def read_program_output(path, fp, tp):
    raw = np.fromfile(path, dtype=np.float32)
    C, V = fp.contact_width, fp.V
    sizes = [fp.n_out * _hip_augment.FRAME_DIM, fp.n_out * C, V * 4, tp.out_floats, V * 3, V * ctypes.sizeof(_hip_moopt.MooptTerrainS) // 4]
    assert raw.size == sum(sizes), (raw.size, sizes)
    parts = np.split(raw, np.cumsum(sizes)[:-1])
    return dict(frames=parts[0].reshape(fp.n_out, _hip_augment.FRAME_DIM), contacts=parts[1].reshape(fp.n_out, C), bounds=parts[2].reshape(V, 4),
                pool=parts[3], canon=parts[4].reshape(V, 3), hf_table=parts[5].view(np.uint8))
