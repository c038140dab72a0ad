"""The generator guidance step's kernel behind one interface for tests/test_mdm_guide*.py -- TEST INFRASTRUCTURE.

A case of fixture G35 as the arguments parc_mdm_guide_step reads (built by parc_amd.diffusion.mdm_guidance.MDMGuidance, as apply_guidance
builds them), run through the host build of parc_mdm_guide_core.h (mdm_guide_host.cpp, compiled here) or through the stand-alone program
built from the same file with -DMDM_GUIDE_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the case from a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
from parc_amd import _hip, _hip_mdm_guide as H                         # noqa: E402
from parc_amd.diffusion import diffusion_util, mdm_guidance            # noqa: E402
import mdm_guide_ref as mgr                                            # noqa: E402
from mdm_loss_host import FLAGS, SANITIZE                              # noqa: E402

SOURCE = os.path.join(HERE, "mdm_guide_host.cpp")
K = diffusion_util.MDMKeyType


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_mdm_guide_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "mdm_guide_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DMDM_GUIDE_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        L.mdm_guide_step_host.restype = ctypes.c_int
        L.mdm_guide_step_host.argtypes = H.STEP_ARGTYPES[1:]
        L.mdm_guide_lds_bytes_host.restype = ctypes.c_int64
        L.mdm_guide_lds_bytes_host.argtypes = [_hip.CharModelS, H.MdmGuideCfgS]
        L.mdm_guide_struct_sizes.restype = ctypes.c_int
        L.mdm_guide_struct_sizes.argtypes = [ctypes.c_void_p]
        _libs[path] = L
    return _libs[path]


def gen_cfg(case, device="cpu", rot_type="DEFAULT"):
    """the generator's configuration keys of a fixture case"""
    xn, xp, yn, yp = case["grid"]
    return {"device": device, "features": {"frame_components": list(case["components"]), "rot_type": rot_type}, "sequence_fps": case["fps"],
            "num_prev_states": case["num_prev_states"], "use_pos_loss": False, "use_hf_collision_loss": False, "use_target_loss": False,
            "heightmap": {"local_grid": {"num_x_neg": xn, "num_x_pos": xp, "num_y_neg": yn, "num_y_pos": yp}, "horizontal_scale": case["dx"],
                          "max_h": case["max_h"]}}


def make_guide(km, case, z, device="cpu", path=None, types=None):
    n = case["name"]
    return mdm_guidance.MDMGuidance(gen_cfg(case, device), km, torch.tensor(z[n + "_mean"]), torch.tensor(z[n + "_std"]), types=types, path=path)


def body_points(case, z, device="cpu"):
    pts = mgr.case_points(case, z)
    return None if pts is None else [p.to(device) for p in pts]


def guidance_inputs(case, z, device="cpu", points=None, B=None, key_type=K, params_type=diffusion_util.MDMCustomGuidance):
    """(conds, guidance parameters) of a fixture case, verbose off; B: repeat the case's samples up to a batch of B"""
    n = case["name"]
    rep = lambda a: torch.tensor(a if B is None else np.concatenate([a] * (B // len(a) + 1))[:B]).to(device)
    gp = params_type()
    gp.verbose = False
    gp.guidance_str = case["guidance_str"]
    gp.target_xy = rep(z[n + "_target_xy"]) if "target" in case["terms"] else None
    gp.body_points = (points if points is not None else body_points(case, z, device)) if "hf" in case["terms"] else None
    gp.w_target_loss, gp.w_hf_loss, gp.w_speed, gp.w_acc, gp.w_jerk = case["w"]
    gp.guide_speed, gp.guide_acc, gp.guide_jerk = "speed" in case["terms"], "acc" in case["terms"], "jerk" in case["terms"]
    gp.max_speed, gp.max_acc, gp.max_jerk = case["max_rate"]
    conds = {key_type.GUIDANCE_PARAMS: gp}
    if "hf" in case["terms"]:
        conds[key_type.OBS_KEY] = rep(z[n + "_hfs"])
    return conds, gp


def batch_x(case, z, B):
    x = z[case["name"] + "_x"]
    return np.ascontiguousarray(np.concatenate([x] * (B // len(x) + 1))[:B])


class Args:
    """the entry point's arguments of a fixture case as host arrays; x may be replaced"""

    def __init__(self, km, case, z, x=None):
        n = case["name"]
        G = make_guide(km, case, z)
        conds, gp = guidance_inputs(case, z)
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.x = f32(z[n + "_x"] if x is None else x)
        self.B, self.S, self.D = self.x.shape
        enabled = G._enabled(gp, conds)
        hf, tgt = bool(enabled & 2), bool(enabled & 1)
        points, start, P = G.pack_points(gp.body_points) if hf else (None, None, 0)
        self.cfg = G.device_cfg(self.S, gp, enabled, P)
        self.model = km.c_struct()
        X, Y = self.cfg.dim_x, self.cfg.dim_y
        gx, gy = G._grid_points() if hf else (None, None)
        self.mean, self.std = f32(z[n + "_mean"][:self.S]), f32(z[n + "_std"][:self.S])
        self.hfs = f32(z[n + "_hfs"]).reshape(self.B, X, Y) if hf else None
        self.target = f32(z[n + "_target_xy"]).reshape(self.B, 2) if tgt else None
        self.grid_x, self.grid_y = (f32(gx), f32(gy)) if hf else (None, None)
        self.points = f32(points) if hf else None
        self.start = np.ascontiguousarray(start.numpy().astype(np.int32)) if hf else None

    def only(self, b):
        """the same case with sample b alone"""
        import copy
        a = copy.copy(self)
        a.B, a.x = 1, np.ascontiguousarray(self.x[b:b + 1])
        a.hfs = None if self.hfs is None else np.ascontiguousarray(self.hfs[b:b + 1])
        a.target = None if self.target is None else np.ascontiguousarray(self.target[b:b + 1])
        return a

    def tail(self):
        """the arguments after x, mean, std"""
        return [self.hfs, self.target, self.grid_x, self.grid_y, self.points, self.start]


def _p(arr):
    return None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)


def run_host(lib_path, a, in_place=False):
    """-> (terms [5, B], x_out [B, S, D]); a.x is left as it was"""
    L = host_lib(lib_path)
    terms = np.full((H.TERMS, a.B), np.nan, np.float32)
    x = a.x.copy()
    x_out = x if in_place else np.full(a.x.shape, np.nan, np.float32)
    rc = L.mdm_guide_step_host(a.model, a.cfg, a.B, _p(x), _p(a.mean), _p(a.std), *[_p(t) for t in a.tail()], _p(x_out), _p(terms))
    assert rc == 0, rc
    return terms, x_out


def dump(path, a, in_place):
    with open(path, "wb") as f:
        f.write(np.array([a.B, 1 if a.hfs is not None else 0, 1 if a.target is not None else 0, 1 if in_place else 0], np.int64).tobytes())
        f.write(bytes(a.cfg))
        f.write(bytes(a.model))
        for arr in (a.x, a.mean, a.std, a.hfs, a.grid_x, a.grid_y, a.points, a.start, a.target):
            if arr is not None:
                f.write(arr.tobytes())


def read_program_output(path, a):
    raw = np.fromfile(path, dtype=np.float32)
    n = H.TERMS * a.B
    assert raw.size == n + a.x.size, raw.size
    return raw[:n].reshape(H.TERMS, a.B), raw[n:].reshape(a.x.shape)
