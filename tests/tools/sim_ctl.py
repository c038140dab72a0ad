"""The simulator in every control mode (PARC_SIM_CTL_*) behind one interface, for tests/test_control_modes*.py -- TEST INFRASTRUCTURE.

Three formulations of the same step: "core" (parc_sim_core.h, one env per lane) and "bpl" (parc_sim_bpl.h, the body-per-lane kernel under
the lane emulation of oracle/sim_host_bpl.cpp), both compiled here for the host from sim_ctl_host_core.cpp / sim_ctl_host_bpl.cpp, and
"device" (sim_step_bpl_kernel / sim_step_bpl_ctl_kernel through parc_sim_step_ctl of the C ABI).

    python tests/tools/sim_ctl.py --smoke LIB     one step of every mode on both host formulations (the sanitizer child of the tests)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SOURCES = [os.path.join(HERE, "sim_ctl_host_core.cpp"), os.path.join(HERE, "sim_ctl_host_bpl.cpp")]
MODES = {"pd": 0, "vel": 1, "torque": 2, "pd_exp": 3, "pd_1d": 4}
FLAGS = ["-fPIC", "-shared", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"]
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_host(out_dir, sanitize=False):
    """Compile the host builds of both formulations into out_dir; returns the library path."""
    lib = os.path.join(out_dir, "libparc_sim_ctl_host{}.so".format("_asan" if sanitize else ""))
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx] + (SANITIZE if sanitize else ["-O2"]) + FLAGS + ["-o", lib] + SOURCES + ["-lm"])
    return lib


class TerrainS(ctypes.Structure):
    _fields_ = [("hf", ctypes.c_void_p), ("dim_x", ctypes.c_int32), ("dim_y", ctypes.c_int32), ("min_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("dx", ctypes.c_float), ("dy", ctypes.c_float)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        args = [ctypes.c_void_p, TerrainS, ctypes.c_int] + [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                                                                   ctypes.c_void_p]
        for fn in (L.sim_ctl_host_step, L.sim_ctl_host_step_bpl):
            fn.restype, fn.argtypes = ctypes.c_int, args
        _libs[path] = L
    return _libs[path]


class CtlSim:
    """State arrays in the Isaac Gym layouts, stepped by one formulation in any control mode.  variant: "core" / "bpl" (lib = the host
    library of build_host) or "device"."""

    def __init__(self, model_struct, n, variant, lib=None, hf=None, min_point=(-4.0, -4.0), dxdy=(0.4, 0.4)):
        self.m, self.n, self.variant, self.lib = model_struct, n, variant, lib
        self.B, self.D = int(model_struct.num_bodies), int(model_struct.dof_size)
        self.hf = np.ascontiguousarray(np.full((20, 20), -100.0, np.float32) if hf is None else hf, dtype=np.float32)
        self.min_point, self.dxdy = [float(v) for v in min_point], [float(v) for v in dxdy]
        self.root_state = np.zeros((n, 13), np.float32)
        self.root_state[:, 6] = 1.0
        self.dof_state = np.zeros((n, self.D, 2), np.float32)
        self.rigid_body_state = np.zeros((n, self.B, 13), np.float32)
        self.contact_forces = np.zeros((n, self.B, 3), np.float32)
        self.env_offsets = np.zeros((n, 3), np.float32)
        self.act_lo = np.full(self.D, -10.0, np.float32)
        self.act_hi = np.full(self.D, 10.0, np.float32)

    def step(self, action, mode, n_sub=4, h=1.0 / 120.0, hold=2):
        """One control step; returns the dof torque [n, D] of the step's last hold (torque / pd_exp / pd_1d), else None."""
        mode = MODES[mode] if isinstance(mode, str) else int(mode)
        action = np.ascontiguousarray(np.broadcast_to(action, (self.n, self.D)), dtype=np.float32)
        tq = np.full((self.n, self.D), np.nan, np.float32) if mode in (2, 3, 4) else None
        if self.variant == "device":
            self._step_device(action, mode, n_sub, h, hold, tq)
        else:
            L = host_lib(self.lib)
            fn = L.sim_ctl_host_step if self.variant == "core" else L.sim_ctl_host_step_bpl
            ter = TerrainS(_p(self.hf), self.hf.shape[0], self.hf.shape[1], self.min_point[0], self.min_point[1], self.dxdy[0], self.dxdy[1])
            rc = fn(ctypes.byref(self.m), ter, self.n, _p(self.root_state), _p(self.dof_state), _p(self.rigid_body_state),
                    _p(self.contact_forces), _p(self.env_offsets), _p(action), _p(self.act_lo), _p(self.act_hi), int(n_sub), float(h), int(hold),
                    mode, _p(tq) if tq is not None else None)
            assert rc == 0, rc
        return tq

    def _step_device(self, action, mode, n_sub, h, hold, tq):
        import torch
        from parc_amd import _hip
        dev = "cuda:0"

        def up(a):
            t = torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
            return t if t.numel() else torch.zeros(4, device=dev)
        m = torch.frombuffer(bytearray(bytes(self.m)), dtype=torch.uint8).to(dev)
        hf = torch.tensor(self.hf, device=dev)
        ter = _hip.terrain_struct(hf, self.min_point, self.dxdy)
        rs, ds, rb, cf = up(self.root_state), up(self.dof_state), up(self.rigid_body_state), up(self.contact_forces)
        eo, act, lo, hi = up(self.env_offsets), up(action), up(self.act_lo), up(self.act_hi)
        dt = up(tq) if tq is not None else None
        p = _hip.ptr
        _hip.check(_hip.lib().parc_sim_step_ctl(_hip.stream(), _hip.c_vp(m.data_ptr()), ter, self.n, p(rs), p(ds), p(rb), p(cf), p(eo), p(act),
                                                p(lo), p(hi), int(n_sub), float(h), int(hold), int(mode), p(dt) if dt is not None else None,
                                                None, None, 0.0), "parc_sim_step_ctl")
        torch.cuda.synchronize()
        self.root_state[:] = rs.cpu().numpy()
        self.dof_state[:] = ds.cpu().numpy()
        self.rigid_body_state[:] = rb.cpu().numpy()
        self.contact_forces[:] = cf.cpu().numpy()
        if tq is not None:
            tq[:] = dt.cpu().numpy()


def humanoid_struct():
    sys.path.insert(0, REPO)
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    from parc_amd.sim_model import SimModel
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    return km, SimModel(km)


def _smoke(lib):
    """One step of every mode on both host formulations from a perturbed standing pose (the sanitizer build's workload)."""
    _, sm = humanoid_struct()
    rng = np.random.default_rng(0)
    for variant in ("core", "bpl"):
        for mode in MODES:
            sim = CtlSim(sm.struct, 2, variant, lib=lib, hf=np.zeros((20, 20), np.float32))
            sim.root_state[:, 2] = 0.95
            sim.dof_state[..., 0] = rng.normal(0.0, 0.2, sim.dof_state.shape[:2])
            tq = sim.step(rng.normal(0.0, 0.5, (2, sim.D)), mode, n_sub=4, hold=2)
            assert np.isfinite(sim.dof_state).all() and np.isfinite(sim.rigid_body_state).all(), (variant, mode)
            assert tq is None or np.isfinite(tq).all(), (variant, mode)
    print("smoke ok")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--smoke"]:
        _smoke(sys.argv[2])
