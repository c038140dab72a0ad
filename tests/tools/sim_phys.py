"""The simulator with per-env physics parameters (parc_sim_step_phys) behind the interface of tests/tools/sim_ctl.py, for
tests/test_phys_params*.py -- TEST INFRASTRUCTURE.

"core" / "bpl": the host builds sim_phys_host_core.cpp / sim_phys_host_bpl.cpp (which include the control-mode host builds, so the same
library also steps without a table); "device": sim_step_bpl_phys_kernel through parc_sim_step_phys of the C ABI.

    python tests/tools/sim_phys.py --smoke LIB     one pushed, randomised step of every mode on both host formulations (sanitizer child)
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sim_ctl  # noqa: E402

SOURCES = [os.path.join(HERE, "sim_phys_host_core.cpp"), os.path.join(HERE, "sim_phys_host_bpl.cpp")]
# parc_sim_env_params_t (include/parc_sim.h): one 64-byte row
ROW = np.dtype([("gravity", "<f4"), ("friction_mu", "<f4"), ("contact_kn", "<f4"), ("contact_cn", "<f4"), ("contact_ct", "<f4"),
                ("mass_scale", "<f4"), ("kp_scale", "<f4"), ("kd_scale", "<f4"), ("push_force", "<f4", (3,)), ("push_steps_left", "<i4"),
                ("push_next_in", "<i4"), ("_pad", "<i4", (3,))])
assert ROW.itemsize == 64


def build_host(out_dir, sanitize=False):
    lib = os.path.join(out_dir, "libparc_sim_phys_host{}.so".format("_asan" if sanitize else ""))
    cxx = os.environ.get("CXX", "g++")
    subprocess.check_call([cxx] + (sim_ctl.SANITIZE if sanitize else ["-O2"]) + sim_ctl.FLAGS + ["-o", lib] + SOURCES + ["-lm"])
    return lib


def neutral_rows(model_struct, n):
    """the table that changes nothing: the model's own constants, scales 1, no push"""
    t = np.zeros(n, ROW)
    for f in ("gravity", "friction_mu", "contact_kn", "contact_cn", "contact_ct"):
        t[f] = getattr(model_struct, f)
    t["mass_scale"] = t["kp_scale"] = t["kd_scale"] = 1.0
    return t


_declared = set()


def phys_lib(path):
    L = sim_ctl.host_lib(path)
    if path not in _declared:
        args = [ctypes.c_void_p, sim_ctl.TerrainS, ctypes.c_int] + [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_float, ctypes.c_int,
                                                                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        for fn in (L.sim_phys_host_step, L.sim_phys_host_step_bpl):
            fn.restype, fn.argtypes = ctypes.c_int, args
        L.sim_phys_host_check.restype, L.sim_phys_host_check.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
        _declared.add(path)
    return L


class PhysSim(sim_ctl.CtlSim):
    """CtlSim with a table: `params` [n] rows (numpy, dtype ROW), neutral at construction.  step() goes through the table's entry point,
    step_plain() through the entry points without one (parc_sim_step / parc_sim_step_ctl or their host builds)."""

    def __init__(self, model_struct, n, variant, lib=None, **kw):
        super().__init__(model_struct, n, variant, lib=lib, **kw)
        self.params = neutral_rows(model_struct, n)

    def step_plain(self, action, mode, n_sub=4, h=1.0 / 120.0, hold=2):
        return sim_ctl.CtlSim.step(self, action, mode, n_sub=n_sub, h=h, hold=hold)

    def step(self, action, mode, n_sub=4, h=1.0 / 120.0, hold=None, expect=0):
        hold = (2 if n_sub % 2 == 0 else 1) if hold is None else hold
        mode = sim_ctl.MODES[mode] if isinstance(mode, str) else int(mode)
        action = np.ascontiguousarray(np.broadcast_to(action, (self.n, self.D)), dtype=np.float32)
        tq = np.full((self.n, self.D), np.nan, np.float32) if mode in (2, 3, 4) else None
        if self.variant == "device":
            rc = self._step_device_phys(action, mode, n_sub, h, hold, tq)
        else:
            L = phys_lib(self.lib)
            fn = L.sim_phys_host_step if self.variant == "core" else L.sim_phys_host_step_bpl
            p = sim_ctl._p
            ter = sim_ctl.TerrainS(p(self.hf), self.hf.shape[0], self.hf.shape[1], self.min_point[0], self.min_point[1], self.dxdy[0], self.dxdy[1])
            rc = fn(ctypes.byref(self.m), ter, self.n, p(self.root_state), p(self.dof_state), p(self.rigid_body_state), p(self.contact_forces),
                    p(self.env_offsets), p(action), p(self.act_lo), p(self.act_hi), int(n_sub), float(h), int(hold), mode,
                    p(tq) if tq is not None else None, p(self.params))
        assert rc == expect, rc
        return tq

    def _step_device_phys(self, action, mode, n_sub, h, hold, tq):
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
        table = torch.frombuffer(bytearray(self.params.tobytes()), dtype=torch.uint8).to(dev)
        p = _hip.ptr
        rc = _hip.lib().parc_sim_step_phys(_hip.stream(), _hip.c_vp(m.data_ptr()), ter, self.n, p(rs), p(ds), p(rb), p(cf), p(eo), p(act), p(lo),
                                           p(hi), int(n_sub), float(h), int(hold), _hip.c_vp(table.data_ptr()), int(mode),
                                           p(dt) if dt is not None else None, None, None, 0.0)
        torch.cuda.synchronize()
        if rc != 0:
            return rc
        self.root_state[:] = rs.cpu().numpy()
        if self.dof_state.size:                      # (a body without dofs uploads a placeholder)
            self.dof_state[:] = ds.cpu().numpy()
        self.rigid_body_state[:] = rb.cpu().numpy()
        self.contact_forces[:] = cf.cpu().numpy()
        self.params[:] = np.frombuffer(table.cpu().numpy().tobytes(), ROW)
        if tq is not None:
            tq[:] = dt.cpu().numpy()
        return 0

    def state(self):
        return [a.copy() for a in (self.root_state, self.dof_state, self.rigid_body_state, self.contact_forces)]


def _smoke(lib):
    """One step of every mode on both host formulations with a non-neutral, pushed table (the sanitizer build's workload)."""
    _, sm = sim_ctl.humanoid_struct()
    rng = np.random.default_rng(0)
    for variant in ("core", "bpl"):
        for mode in sim_ctl.MODES:
            sim = PhysSim(sm.struct, 2, variant, lib=lib, hf=np.zeros((20, 20), np.float32))
            sim.params["gravity"], sim.params["friction_mu"], sim.params["contact_kn"] = [3.7, 12.0], [0.5, 1.5], [1e4, 1.6e5]
            sim.params["mass_scale"], sim.params["kp_scale"], sim.params["kd_scale"] = [0.7, 1.4], [0.5, 2.0], [0.0, 2.0]
            sim.params["push_force"], sim.params["push_steps_left"] = [[100.0, -50.0, 20.0], [0.0, 0.0, 0.0]], [2, 0]
            sim.root_state[:, 2] = 0.95
            sim.dof_state[..., 0] = rng.normal(0.0, 0.2, sim.dof_state.shape[:2])
            tq = sim.step(rng.normal(0.0, 0.5, (2, sim.D)), mode, n_sub=4, hold=2)
            assert np.isfinite(sim.dof_state).all() and np.isfinite(sim.rigid_body_state).all(), (variant, mode)
            assert tq is None or np.isfinite(tq).all(), (variant, mode)
            assert list(sim.params["push_steps_left"]) == [1, 0]
    print("smoke ok")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--smoke"]:
        _smoke(sys.argv[2])
