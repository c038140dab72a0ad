"""The motion scorer behind one interface for tests/test_motion_score*.py -- TEST INFRASTRUCTURE.

A `Case` holds everything one parc_motion_score call reads, as numpy arrays.  It is scored by the host build of parc_score_core.h
(score_host.cpp, compiled here; body poses from the torch forward kinematics on the CPU), by the device (parc_motion_score of the C
ABI), or by the stand-alone program built from the same file with -DSCORE_HOST_MAIN (plain or with -fsanitize=address,undefined),
which reads the case from a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from parc_amd import _hip_score      # noqa: E402

SOURCE = os.path.join(HERE, "score_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
HOST_ARGTYPES = [ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                                                    _hip_score.ScoreTerrainS] + [ctypes.c_float] * 5 + [ctypes.c_void_p] * 3


def build_host(out_dir):
    """the shared library with score_host()"""
    lib = os.path.join(out_dir, "libparc_score_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "score_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DSCORE_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        L.score_host.restype = ctypes.c_int
        L.score_host.argtypes = HOST_ARGTYPES
        _libs[path] = L
    return _libs[path]


def linspace_grid(n, d):
    """torch.linspace(0, (n - 1) * d, n) in fp32: what HfGrid hands the kernels"""
    import torch
    return torch.linspace(0.0, (n - 1.0) * float(d), n).numpy().astype(np.float32)


class Case:
    """root_pos [B,F,3], root_rot [B,F,4], joint_rot [B,F,Bd-1,4], contacts [B,F,Bd]; local [P,3], start [Bd+1]; hf [X,Y]"""

    def __init__(self, km, root_pos, root_rot, joint_rot, contacts, local, start, hf, min_point, dxdy, num_frames=None, w_contact=1.0, w_pen=1.0,
                 dt=1.0 / 30.0, max_jerk=np.inf):
        f32 = np.float32
        self.km, self.Bd = km, km.get_num_joints()
        self.root_pos, self.root_rot = np.array(root_pos, f32, order="C"), np.array(root_rot, f32, order="C")          # copies: tests edit them
        self.joint_rot, self.contacts = np.array(joint_rot, f32, order="C"), np.array(contacts, f32, order="C")
        self.B, self.F = self.root_pos.shape[0], self.root_pos.shape[1]
        self.local, self.start = np.ascontiguousarray(local, f32).reshape(-1, 3), np.ascontiguousarray(start, np.int32)
        self.P = self.local.shape[0]
        self.hf = np.ascontiguousarray(hf, f32)
        self.min_point, self.dxdy = [float(f32(v)) for v in min_point], [float(f32(v)) for v in dxdy]
        self.xs, self.ys = linspace_grid(self.hf.shape[0], self.dxdy[0]), linspace_grid(self.hf.shape[1], self.dxdy[1])
        self.num_frames = None if num_frames is None else np.ascontiguousarray(num_frames, np.int32)
        self.base_z = float(f32(self.hf.min()) - f32(10.0))
        self.w_contact, self.w_pen, self.dt, self.max_jerk = float(w_contact), float(w_pen), float(dt), float(max_jerk)

    def terrain_struct(self, hf_ptr, xs_ptr, ys_ptr):
        return _hip_score.ScoreTerrainS(hf_ptr, self.hf.shape[0], self.hf.shape[1], self.min_point[0], self.min_point[1], self.dxdy[0], self.dxdy[1],
                                        xs_ptr, ys_ptr)

    def body_poses(self):
        """fp32 forward kinematics with torch ops on the CPU -> body_pos [B,F,Bd,3], body_rot [B,F,Bd,4]"""
        import torch
        bp, br = self.km.forward_kinematics_torch(torch.tensor(self.root_pos), torch.tensor(self.root_rot), torch.tensor(self.joint_rot))
        return np.ascontiguousarray(bp.numpy(), np.float32), np.ascontiguousarray(br.numpy(), np.float32)

    def float64(self, ref):
        """the float64 restatement (tests/motion_score_ref.py)"""
        return ref.score64(ref.model_tables(self.km), self.root_pos, self.root_rot, self.joint_rot, self.contacts, self.local, self.start, self.hf,
                           self.min_point, self.dxdy, self.num_frames, self.w_contact, self.w_pen, self.dt, self.max_jerk)

    # ------------------------------------------------------------------ the three ways to score it
    def score_host(self, lib, jerk=True):
        bp, br = self.body_poses()
        terms = np.full((self.B, self.F, 2), -7.0, np.float32)
        losses, jk = np.zeros((self.B, 3), np.float32), np.zeros((self.B, 2), np.float32)
        rc = host_lib(lib).score_host(self.Bd, self.B, self.F, _p(self.num_frames), _p(bp), _p(br), _p(self.contacts), self.P, _p(self.local),
                                      _p(self.start), self.terrain_struct(self.hf.ctypes.data, self.xs.ctypes.data, self.ys.ctypes.data), self.base_z,
                                      self.w_contact, self.w_pen, self.dt, self.max_jerk, _p(terms), _p(losses), _p(jk) if jerk else None)
        return dict(rc=rc, frame_terms=terms, losses=losses, jerk=jk if jerk else None)

    def score_device(self, jerk=True, guard=64):
        """parc_motion_score on the GPU.  `guard` float words before and behind every output (and the workspace), filled with a pattern; they
        come back as out["guard"] (a list of arrays) next to out["pattern"]."""
        import torch
        from parc_amd import _hip
        dev = "cuda:0"

        def up(a):
            return None if a is None else torch.tensor(a, device=dev)
        t = [up(a) for a in (self.num_frames, self.root_pos, self.root_rot, self.joint_rot, self.contacts, self.local, self.start, self.hf, self.xs, self.ys)]
        pattern = -1234.5
        sizes = [self.B * self.F * self.Bd * 3, self.B * self.F * 2, self.B * 3, self.B * 2]
        bufs = [torch.full((n + 2 * guard,), pattern, dtype=torch.float32, device=dev) for n in sizes]
        outs = [b[guard:] for b in bufs]          # (a view: data_ptr() is that of its first element)

        def p(t_):
            return None if t_ is None else ctypes.c_void_p(t_.data_ptr())
        rc = _hip.lib().parc_motion_score(_hip.stream(), self.km.c_struct(), self.B, self.F, p(t[0]), p(t[1]), p(t[2]), p(t[3]), p(t[4]), self.P, p(t[5]),
                                          p(t[6]), self.terrain_struct(t[7].data_ptr(), t[8].data_ptr(), t[9].data_ptr()), self.base_z, self.w_contact,
                                          self.w_pen, self.dt, self.max_jerk, p(outs[0]) if jerk else None, p(outs[1]), p(outs[2]),
                                          p(outs[3]) if jerk else None)
        torch.cuda.synchronize()
        whole = [b.cpu().numpy() for b in bufs]
        host = [w[guard:] for w in whole]
        return dict(rc=rc, body_pos=host[0][:sizes[0]].reshape(self.B, self.F, self.Bd, 3), frame_terms=host[1][:sizes[1]].reshape(self.B, self.F, 2),
                    losses=host[2][:sizes[2]].reshape(self.B, 3), jerk=host[3][:sizes[3]].reshape(self.B, 2) if jerk else None,
                    guard=[np.concatenate([w[:guard], w[guard + n:]]) for w, n in zip(whole, sizes)], pattern=np.float32(pattern))

    def dump(self, path):
        """the case file of the stand-alone program"""
        bp, br = self.body_poses()
        with open(path, "wb") as f:
            f.write(np.array([self.Bd, self.B, self.F, self.P, self.hf.shape[0], self.hf.shape[1], self.num_frames is not None], np.int32).tobytes())
            f.write(np.array(self.min_point + self.dxdy + [self.base_z, self.w_contact, self.w_pen, self.dt, self.max_jerk], np.float32).tobytes())
            for a in (self.num_frames, self.start, bp, br, self.contacts, self.local, self.hf, self.xs, self.ys):
                if a is not None:
                    f.write(a.tobytes())

    def read_program_output(self, path):
        raw = np.fromfile(path, dtype=np.float32)
        n = self.B * self.F * 2
        assert raw.size == n + self.B * 5
        return dict(frame_terms=raw[:n].reshape(self.B, self.F, 2), losses=raw[n:n + self.B * 3].reshape(self.B, 3), jerk=raw[n + self.B * 3:].reshape(self.B, 2))


def fixture_case(km, fx, cands=None, num_frames=None, **kw):
    """G28 (tests/motion_score_ref.load_fixture) as one Case over the candidates `cands` (default all)"""
    s = slice(None) if cands is None else list(cands)
    return Case(km, fx["root_pos"][s], fx["root_rot"][s], fx["joint_rot"][s], fx["contacts"][s], fx["pts"], fx["start"], fx["hf"], fx["min_point"],
                fx["dxdy"], num_frames=num_frames, **kw)
