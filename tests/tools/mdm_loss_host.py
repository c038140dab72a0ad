"""The generator loss's kernels behind one interface for tests/test_mdm_loss*.py -- TEST INFRASTRUCTURE.

A case of fixture G33 as the arguments the entry points of include/parc_mdm_loss.h read (built by parc_amd.diffusion.mdm_loss.MDMMotionLoss,
as the trainer's call builds them), run through the host build of parc_mdm_loss_core.h (mdm_loss_host.cpp, compiled here) or through the
stand-alone program built from the same file with -DMDM_LOSS_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the case
from a file.
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
from parc_amd import _hip, _hip_mdm_loss as H                      # noqa: E402
from parc_amd.diffusion import diffusion_util, mdm_loss            # noqa: E402
import mdm_loss_ref as mlr                                         # noqa: E402

SOURCE = os.path.join(HERE, "mdm_loss_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-parameter", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
T = diffusion_util.MDMFrameType


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_mdm_loss_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "mdm_loss_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DMDM_LOSS_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        for name, args in (("mdm_loss_forward_host", H.FORWARD_ARGTYPES[1:]), ("mdm_loss_backward_host", H.BACKWARD_ARGTYPES[1:])):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = args
        L.mdm_loss_lds_bytes_host.restype = ctypes.c_int64
        L.mdm_loss_lds_bytes_host.argtypes = [_hip.CharModelS, H.MdmLossCfgS]
        L.mdm_loss_struct_sizes.restype = ctypes.c_int
        L.mdm_loss_struct_sizes.argtypes = [ctypes.c_void_p]
        _libs[path] = L
    return _libs[path]


def loss_cfg(case, device="cpu"):
    """the generator's configuration keys of a fixture case"""
    xn, xp, yn, yp = case["grid"]
    cfg = {"device": device, "features": {"frame_components": list(case["components"]), "rot_type": case.get("rot_type", "DEFAULT")}, "sequence_fps": case["fps"],
           "num_prev_states": case["num_prev_states"], "use_pos_loss": case["use_pos_loss"], "use_hf_collision_loss": case["use_hf_collision_loss"],
           "use_target_loss": case["use_target_loss"], "target_type": "XY_DIR", "target_dir_len_eps": case["target_dir_len_eps"],
           "heightmap": {"local_grid": {"num_x_neg": xn, "num_x_pos": xp, "num_y_neg": yn, "num_y_pos": yp}, "horizontal_scale": case["dx"],
                         "max_h": case["max_h"]}}
    cfg.update(case["weights"])
    return cfg


def make_loss(km, case, z, device="cpu", path=None):
    n = case["name"]
    return mdm_loss.MDMMotionLoss(loss_cfg(case, device), km, torch.tensor(z[n + "_mean"]), torch.tensor(z[n + "_std"]), path=path)


def true_data(km, case, device="cpu"):
    """the case's true motion data as the sampler returns it (JOINT_POS from the CPU chain of the package)"""
    tw = mlr.true_windows(case)
    out = {T.ROOT_POS: torch.tensor(tw["ROOT_POS"]), T.ROOT_ROT: torch.tensor(tw["ROOT_ROT"]), T.JOINT_ROT: torch.tensor(tw["JOINT_ROT"])}
    if "CONTACTS" in case["components"]:
        out[T.CONTACTS] = torch.tensor(tw["CONTACTS"])
    out = {k: v.to(device) for k, v in out.items()}
    if "JOINT_POS" in case["components"]:          # km lives on `device`
        out[T.JOINT_POS] = km.forward_kinematics_torch(out[T.ROOT_POS], out[T.ROOT_ROT], out[T.JOINT_ROT])[0][..., 1:, :].contiguous()
    return out


class Args:
    """the entry points' arguments of a fixture case as host arrays; x and g_losses may be replaced"""

    def __init__(self, km, case, z, x=None):
        n = case["name"]
        L = make_loss(km, case, z)
        tab = L._tables()
        true = true_data(km, case)
        self.B, self.S, self.D = z[n + "_x"].shape
        self.cfg = L._device_cfg(self.S, {"squared_l2": 0, "pseudo_huber": 1}[case["loss_fn"]], L._enabled_terms(true))
        self.model = km.c_struct()
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.x = f32(z[n + "_x"] if x is None else x)
        X, Y = self.cfg.dim_x, self.cfg.dim_y
        self.arrays = [f32(z[n + "_mean"][:self.S]), f32(z[n + "_std"][:self.S]), f32(true[T.ROOT_POS]), f32(true[T.ROOT_ROT]), f32(true[T.JOINT_ROT]),
                       f32(true[T.CONTACTS]) if T.CONTACTS in true else None, f32(z[n + "_hfs"]).reshape(self.B, X, Y),
                       f32(z[n + "_target_dir"]).reshape(self.B, 2), f32(tab["grid_x"]), f32(tab["grid_y"]), f32(tab["points"]),
                       np.ascontiguousarray(tab["start"].numpy().astype(np.int32))]
        self.enabled = self.cfg.enabled
        self.keys = [mlr.TERM_ORDER[t] for t in range(H.TERMS) if (self.enabled >> t) & 1]

    def ptrs(self):
        return [a.ctypes.data_as(ctypes.c_void_p) if a is not None else None for a in self.arrays]

    def cotangent(self, ood_mask=None):
        """d(reduce)/d(losses): 1 / B for every enabled term, 0 where the ood mask zeroes it"""
        g = np.zeros((H.TERMS, self.B), np.float32)
        for t in range(H.TERMS):
            if (self.enabled >> t) & 1:
                g[t] = np.float32(1.0) / np.float32(self.B)
                if ood_mask is not None and mlr.TERM_ORDER[t] not in mlr.UNMASKED:
                    g[t][np.asarray(ood_mask, bool)] = 0.0
        return g


def run_host(lib_path, a, g_losses=None):
    """-> (dict name -> [B] of the enabled terms, g_x or None)"""
    L = host_lib(lib_path)
    losses = np.full((H.TERMS, a.B), np.nan, np.float32)
    p = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    rc = L.mdm_loss_forward_host(a.model, a.cfg, a.B, p(a.x), *a.ptrs(), p(losses))
    assert rc == 0, rc
    out = {mlr.TERM_ORDER[t]: losses[t] for t in range(H.TERMS) if (a.enabled >> t) & 1}
    g_x = None
    if g_losses is not None:
        g_x = np.full(a.x.shape, np.nan, np.float32)
        g = np.ascontiguousarray(g_losses, dtype=np.float32)
        rc = L.mdm_loss_backward_host(a.model, a.cfg, a.B, p(a.x), *a.ptrs(), p(g), p(g_x))
        assert rc == 0, rc
    return out, g_x, losses


def dump(path, a, g_losses):
    with open(path, "wb") as f:
        f.write(np.array([a.B, 1 if a.arrays[5] is not None else 0, 0, 0], np.int64).tobytes())
        f.write(bytes(a.cfg))
        f.write(bytes(a.model))
        f.write(a.x.tobytes())
        for arr in a.arrays:
            if arr is not None:
                f.write(arr.tobytes())
        f.write(np.ascontiguousarray(g_losses, dtype=np.float32).tobytes())


def read_program_output(path, a):
    raw = np.fromfile(path, dtype=np.float32)
    n = H.TERMS * a.B
    assert raw.size == n + a.x.size, raw.size
    return raw[:n].reshape(H.TERMS, a.B), raw[n:].reshape(a.x.shape)
