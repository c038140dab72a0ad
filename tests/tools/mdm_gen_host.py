"""The generator call's kernels behind one interface for tests/test_mdm_gen*.py -- TEST INFRASTRUCTURE.

A case of fixture G36 as the arguments parc_mdm_gen_encode / parc_mdm_gen_decode read (built by parc_amd.diffusion.gen_util.MDMGenIO, as
encode and decode build them), run through the host build of parc_mdm_gen_core.h (mdm_gen_host.cpp, compiled here) or through the
stand-alone program built from the same file with -DMDM_GEN_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the
case from a file.
"""
import copy
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
from parc_amd import _hip, _hip_mdm_gen as H                           # noqa: E402
from parc_amd.diffusion import diffusion_util, gen_util                # noqa: E402
from parc_amd.util import terrain_util                                 # noqa: E402
from parc_amd.util.motion_util import MotionFrames                     # noqa: E402
from mdm_loss_host import FLAGS, SANITIZE                              # noqa: E402

SOURCE = os.path.join(HERE, "mdm_gen_host.cpp")
ENC_OUT = ("frame", "root_pos", "root_rot", "body_pos", "hf_z", "target", "target_dir", "prev_state", "obs")
DEC_OUT = ("root_pos", "root_rot", "joint_rot", "contacts", "frames")


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_mdm_gen_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "mdm_gen_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DMDM_GEN_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        L.mdm_gen_encode_host.restype = ctypes.c_int
        L.mdm_gen_encode_host.argtypes = H.ENCODE_ARGTYPES[1:]
        L.mdm_gen_decode_host.restype = ctypes.c_int
        L.mdm_gen_decode_host.argtypes = H.DECODE_ARGTYPES[1:]
        L.mdm_gen_lds_bytes_host.restype = ctypes.c_int64
        L.mdm_gen_lds_bytes_host.argtypes = [_hip.CharModelS, H.MdmGenCfgS]
        L.mdm_gen_struct_sizes.restype = ctypes.c_int
        L.mdm_gen_struct_sizes.argtypes = [ctypes.c_void_p]
        _libs[path] = L
    return _libs[path]


def gen_cfg(case, device="cpu", rot_type="DEFAULT", z_style=None, **extra):
    """the generator's configuration keys of a fixture case"""
    xn, xp, yn, yp = case["grid"]
    cfg = {"device": device, "features": {"frame_components": list(case["components"]), "rot_type": rot_type}, "sequence_fps": case["fps"],
           "num_prev_states": case["num_prev_states"], "use_pos_loss": False, "use_hf_collision_loss": False, "use_target_loss": False,
           "relative_z_style": z_style or case["z_style"],
           "heightmap": {"local_grid": {"num_x_neg": xn, "num_x_pos": xp, "num_y_neg": yn, "num_y_pos": yp}, "horizontal_scale": case["dx"],
                         "max_h": case["max_h"]}}
    cfg.update(extra)
    return cfg


def make_io(km, case, z, device="cpu", path=None, types=None, z_style=None, **extra):
    n = case["name"]
    return gen_util.MDMGenIO(gen_cfg(case, device, z_style=z_style, **extra), km, torch.tensor(z[n + "_mean"]), torch.tensor(z[n + "_std"]), types=types,
                             path=path)


def fixture_terrain(z, device="cpu"):
    return terrain_util.SubTerrain.from_arrays(z["terrain_hf"], z["terrain_min_point"], z["terrain_dxdy"], device=device)


def rep(a, B):
    """the case's samples repeated up to a batch of B (None: as they are)"""
    a = np.asarray(a)
    return a if B is None else np.ascontiguousarray(np.concatenate([a] * (B // len(a) + 1))[:B])


def call_inputs(case, z, device="cpu", B=None):
    """(target_world, prev_frames, settings) of a fixture case as gen_mdm_motion takes them"""
    n = case["name"]
    t = lambda a: torch.tensor(rep(a, B)).to(device)
    prev = MotionFrames(root_pos=t(z[n + "_prev_root_pos"]), root_rot=t(z[n + "_prev_root_rot"]), joint_rot=t(z[n + "_prev_joint_rot"]),
                        contacts=t(z[n + "_prev_contacts"]))
    s = gen_util.MDMGenSettings()
    s.use_prev_state = t(z[n + "_use_prev_state"]) if isinstance(case["use_prev_state"], list) else case["use_prev_state"]
    s.target_guidance = case["target_guidance"]
    return t(z[n + "_target_world"]), prev, s


def stand_in(case, z, device="cpu", B=None, components=False):
    """a model object with the attributes gen_mdm_motion reads off a reference MDM and a sampling loop that records its conds and
    returns the case's seeded sample (feature mode), or with gen_sequence_with_contacts alone (component mode)"""
    n = case["name"]
    xn, xp, yn, yp = case["grid"]
    m = types.SimpleNamespace(
        _device=torch.device(device), _sequence_fps=case["fps"], _num_prev_states=case["num_prev_states"], _seq_len=case["S"],
        _frame_components=[diffusion_util.MDMFrameType[c] for c in case["components"]], _target_type=types.SimpleNamespace(name="XY_DIR"),
        _relative_z_style=diffusion_util.RelativeZStyle[case["z_style"]], _dx=case["dx"], _dy=case["dx"], _num_x_neg=xn, _num_x_pos=xp,
        _num_y_neg=yn, _num_y_pos=yp, _max_h=case["max_h"], _min_h=-case["max_h"], _mdm_features_mean=torch.tensor(z[n + "_mean"]).to(device),
        _mdm_features_std=torch.tensor(z[n + "_std"]).to(device), _diffusion_timesteps=1000, calls=[])
    x = torch.tensor(rep(z[n + "_x"], B)).to(device)
    if components:
        def gen_sequence_with_contacts(conds, ddim_stride=None, mode=None):
            m.calls.append(("components", conds, ddim_stride, mode))
            return m.components_out
        m.gen_sequence_with_contacts = gen_sequence_with_contacts
    else:
        m.ddim_inference = lambda conds, stride: (m.calls.append(("ddim", conds, stride)), x.clone())[1]
        m.reverse_diffusion = lambda conds, start_timestep: (m.calls.append(("reverse", conds, start_timestep)), x.clone())[1]
    return m


class Args:
    """the entry points' arguments of a fixture case as host arrays"""

    def __init__(self, km, case, z, z_style=None, features=True):
        n = case["name"]
        f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        io = make_io(km, case, z, z_style=z_style)
        self.case, self.model = case, km.c_struct()
        self.root_pos, self.root_rot = f32(z[n + "_prev_root_pos"]), f32(z[n + "_prev_root_rot"])
        self.joint_rot, self.contacts = f32(z[n + "_prev_joint_rot"]), f32(z[n + "_prev_contacts"])
        self.target_world = f32(z[n + "_target_world"])
        self.B, self.T = self.root_pos.shape[:2]
        self.S, self.P = case["S"], case["num_prev_states"]
        self.cfg_enc, self.cfg_dec = io.device_cfg(self.T, self.T), io.device_cfg(self.S, self.S)
        self.D, self.X, self.Y = self.cfg_enc.feat_dim, self.cfg_enc.dim_x, self.cfg_enc.dim_y
        self.J, self.nb, self.dofs = km.get_num_joints() - 1, km.get_num_joints(), km.get_dof_size()
        gx, gy = io._grid_points()
        self.grid_x, self.grid_y = f32(gx), f32(gy)
        self.mean, self.std = f32(z[n + "_mean"]), f32(z[n + "_std"])
        self.hf = f32(z["terrain_hf"])
        self.terrain = _hip.TerrainS(self.hf.ctypes.data_as(ctypes.c_void_p), self.hf.shape[0], self.hf.shape[1], float(z["terrain_min_point"][0]),
                                     float(z["terrain_min_point"][1]), float(z["terrain_dxdy"][0]), float(z["terrain_dxdy"][1]))
        self.features = features
        self.x = f32(z[n + "_x"])
        self.keep = np.ascontiguousarray(np.asarray(z[n + "_use_prev_state"], dtype=np.uint8)) if features and case["mode"] == "feature" else None

    def only(self, b):
        """the same case with sample b alone"""
        a = copy.copy(self)
        a.B = 1
        for k in ("root_pos", "root_rot", "joint_rot", "contacts", "target_world", "x", "keep"):
            v = getattr(self, k)
            setattr(a, k, None if v is None else np.ascontiguousarray(v[b:b + 1]))
        return a

    def enc_shapes(self):
        B, T, J, X, Y, P, D = self.B, self.T, self.J, self.X, self.Y, self.P, self.D
        s = {"frame": (B, 8), "root_pos": (B, T, 3), "root_rot": (B, T, 4), "body_pos": (B, T, J, 3), "hf_z": (B, X, Y), "target": (B, 2),
             "target_dir": (B, 2)}
        if self.features:
            s.update(prev_state=(B, P, D), obs=(B, X, Y))
        return s

    def dec_shapes(self):
        B, S, J = self.B, self.S, self.J
        s = {"root_pos": (B, S, 3), "root_rot": (B, S, 4), "joint_rot": (B, S, J, 4)}
        if self.cfg_dec.off_contacts >= 0:
            s["contacts"] = (B, S, self.nb)
        s["frames"] = (B, S, 6 + self.dofs)
        return s


def _p(arr):
    return None if arr is None else arr.ctypes.data_as(ctypes.c_void_p)


def run_encode(lib_path, a):
    """-> dict of the encode outputs (ENC_OUT; prev_state and obs with a.features)"""
    L = host_lib(lib_path)
    out = {k: np.full(s, np.nan, np.float32) for k, s in a.enc_shapes().items()}
    rc = L.mdm_gen_encode_host(a.model, a.cfg_enc, a.terrain, a.B, _p(a.root_pos), _p(a.root_rot), _p(a.joint_rot), _p(a.contacts), _p(a.target_world),
                               _p(a.grid_x), _p(a.grid_y), _p(a.mean), _p(a.std), *[_p(out.get(k)) for k in ENC_OUT])
    assert rc == 0, rc
    return out


def run_decode(lib_path, a, enc, x=None, frames=True):
    """-> dict of the decode outputs (DEC_OUT; without `frames` where not asked for) for the sample a.x, with the encode outputs `enc`"""
    L = host_lib(lib_path)
    out = {k: np.full(s, np.nan, np.float32) for k, s in a.dec_shapes().items() if frames or k != "frames"}
    keep = a.keep
    rc = L.mdm_gen_decode_host(a.model, a.cfg_dec, a.B, _p(a.x if x is None else x), _p(enc["prev_state"]) if keep is not None else None, _p(keep),
                               _p(a.mean), _p(a.std), _p(enc["frame"]), *[_p(out.get(k)) for k in DEC_OUT])
    assert rc == 0, rc
    return out


def dump(path, a):
    """the case file of the stand-alone program (mdm_gen_host.cpp)"""
    decode = a.case["mode"] == "feature"
    rows = a.S if decode else a.P
    with open(path, "wb") as f:
        f.write(np.array([a.B, 1 if a.features else 0, 1 if decode else 0, 1 if (decode and a.keep is not None) else 0], np.int64).tobytes())
        f.write(bytes(a.cfg_enc))
        f.write(bytes(a.cfg_dec))
        f.write(bytes(a.model))
        f.write(np.array(a.hf.shape, np.int32).tobytes())
        f.write(np.array([a.terrain.min_x, a.terrain.min_y, a.terrain.dx, a.terrain.dy], np.float32).tobytes())
        for arr in (a.hf, a.root_pos, a.root_rot, a.joint_rot, a.contacts, a.target_world, a.grid_x, a.grid_y, a.mean[:rows], a.std[:rows]):
            f.write(np.ascontiguousarray(arr).tobytes())
        if decode:
            f.write(a.x.tobytes())
            if a.keep is not None:
                f.write(a.keep.tobytes())


def read_program_output(path, a):
    """-> (encode outputs, decode outputs or None)"""
    raw = np.fromfile(path, dtype=np.float32)
    pos, enc, dec = 0, {}, None
    for k, s in a.enc_shapes().items():
        n = int(np.prod(s))
        enc[k], pos = raw[pos:pos + n].reshape(s), pos + n
    if a.case["mode"] == "feature":
        dec = {}
        for k, s in a.dec_shapes().items():
            n = int(np.prod(s))
            dec[k], pos = raw[pos:pos + n].reshape(s), pos + n
    assert pos == raw.size, (pos, raw.size)
    return enc, dec
