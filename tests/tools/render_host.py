"""The ray caster behind one interface for tests/test_render*.py -- TEST INFRASTRUCTURE.

A `Scene` holds everything one parc_render call reads, as numpy arrays.  It is drawn by the host build of parc_render_core.h
(render_host.cpp, compiled here), by the device (parc_render of the C ABI), or by the stand-alone program built from the same file with
-DRENDER_HOST_MAIN (plain or with -fsanitize=address,undefined), which reads the scene from a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from parc_amd import _hip_render, render      # noqa: E402
from parc_amd._hip import TerrainS      # noqa: E402

SOURCE = os.path.join(HERE, "render_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_host(out_dir):
    """the shared library with render_host()"""
    lib = os.path.join(out_dir, "libparc_render_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog scene_file [out_file]`"""
    exe = os.path.join(out_dir, "render_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DRENDER_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        L.render_host.restype = ctypes.c_int
        L.render_host.argtypes = _hip_render.RENDER_ARGTYPES[1:] + [ctypes.c_void_p]
        _libs[path] = L
    return _libs[path]


class Scene:
    """prims: list of PrimS.  body_pos [N,B,3] / body_rot [N,B,4] (x y z w) of the simulated character, ref_pos / ref_rot of the
    reference character (or None), contact_forces [N,B,3] (or None), env_offsets [N,3], views: list of ViewS, hf [dim_x, dim_y]."""

    def __init__(self, prims, num_bodies, body_pos, body_rot, hf, min_point, dxdy, views, width=32, height=24, ref_pos=None, ref_rot=None,
                 contact_forces=None, env_offsets=None, **scene_kw):
        f32 = np.float32
        self.prims, self.B = list(prims), int(num_bodies)
        self.body_pos = np.ascontiguousarray(body_pos, f32).reshape(-1, self.B, 3)
        self.N = self.body_pos.shape[0]
        self.body_rot = np.ascontiguousarray(body_rot, f32).reshape(self.N, self.B, 4)
        self.rigid_body_state = np.zeros((self.N, self.B, 13), f32)
        self.rigid_body_state[..., 0:3], self.rigid_body_state[..., 3:7] = self.body_pos, self.body_rot
        self.root_state = np.ascontiguousarray(self.rigid_body_state[:, 0, :])
        self.ref_pos = None if ref_pos is None else np.ascontiguousarray(ref_pos, f32).reshape(self.N, self.B, 3)
        self.ref_rot = None if ref_rot is None else np.ascontiguousarray(ref_rot, f32).reshape(self.N, self.B, 4)
        self.contact_forces = None if contact_forces is None else np.ascontiguousarray(contact_forces, f32).reshape(self.N, self.B, 3)
        self.env_offsets = np.zeros((self.N, 3), f32) if env_offsets is None else np.ascontiguousarray(env_offsets, f32).reshape(self.N, 3)
        self.hf = np.ascontiguousarray(hf, f32)
        self.min_point, self.dxdy = [float(np.float32(v)) for v in min_point], [float(np.float32(v)) for v in dxdy]
        self.views, self.width, self.height = list(views), int(width), int(height)
        self.scene_kw = dict(scene_kw)
        self._prim_buf = np.frombuffer(render.prims_bytes(self.prims) or b"\0" * 64, dtype=np.uint8).copy()
        self._view_buf = np.frombuffer(b"".join(bytes(v) for v in self.views) or b"\0" * 64, dtype=np.uint8).copy()

    def with_scene(self, **kw):
        """a shallow copy with other scene scalars (shadows=..., show_contacts=..., ref_char_offset=...)"""
        import copy
        s = copy.copy(self)
        s.scene_kw = dict(self.scene_kw, **kw)
        return s

    def with_views(self, views, width=None, height=None):
        import copy
        s = copy.copy(self)
        s.views = list(views)
        s._view_buf = np.frombuffer(b"".join(bytes(v) for v in s.views) or b"\0" * 64, dtype=np.uint8).copy()
        s.width, s.height = int(width or self.width), int(height or self.height)
        return s

    def scene_struct(self, prims_ptr):
        return render.make_scene(len(self.prims), self.B, prims_ptr, **self.scene_kw)

    def terrain_struct(self, hf_ptr):
        return TerrainS(hf_ptr, self.hf.shape[0], self.hf.shape[1], self.min_point[0], self.min_point[1], self.dxdy[0], self.dxdy[1])

    # ------------------------------------------------------------------ the three ways to draw it
    def render_host(self, lib):
        """-> dict(rc, rgba uint8 [V,H,W,4], depth, ids, normals)"""
        V, H, W = len(self.views), self.height, self.width
        rgba = np.zeros((V, H, W), np.uint32)
        depth, ids, normals = np.zeros((V, H, W), np.float32), np.zeros((V, H, W), np.int32), np.zeros((V, H, W, 3), np.float32)
        sc = self.scene_struct(self._prim_buf.ctypes.data)
        rc = host_lib(lib).render_host(self.terrain_struct(self.hf.ctypes.data), ctypes.byref(sc), V, _p(self._view_buf), W, H, _p(self.root_state),
                                       _p(self.rigid_body_state), _p(self.ref_pos), _p(self.ref_rot), _p(self.contact_forces), _p(self.env_offsets),
                                       self.N, _p(rgba), _p(depth), _p(ids), _p(normals))
        return dict(rc=rc, rgba=rgba.view(np.uint8).reshape(V, H, W, 4), depth=depth, ids=ids, normals=normals)

    def render_device(self, guard=0):
        """parc_render on the GPU.  guard > 0: that many int32 words behind every output plane, filled with a pattern; they come back as
        out["guard"] (a list of arrays) for the caller to check."""
        import torch
        from parc_amd import _hip
        dev = "cuda:0"
        V, H, W = len(self.views), self.height, self.width
        n = V * H * W

        def up(a):
            return None if a is None else torch.tensor(a, device=dev)
        prims, views, hf = up(self._prim_buf), up(self._view_buf), up(self.hf)
        t = [up(a) for a in (self.root_state, self.rigid_body_state, self.ref_pos, self.ref_rot, self.contact_forces, self.env_offsets)]
        pattern = 0x5A5A5A5A
        planes = [torch.full((n + guard,), pattern, dtype=torch.int32, device=dev) for _ in range(3)]
        depth = planes[1].view(torch.float32)
        sc = self.scene_struct(prims.data_ptr())
        p = _hip.ptr
        rc = _hip.lib().parc_render(_hip.stream(), self.terrain_struct(hf.data_ptr()), ctypes.byref(sc), V, p(views), W, H, p(t[0]), p(t[1]), p(t[2]),
                                    p(t[3]), p(t[4]), p(t[5]), self.N, p(planes[0]), p(depth), p(planes[2]))
        torch.cuda.synchronize()
        host = [pl.cpu().numpy() for pl in planes]
        return dict(rc=rc, rgba=host[0][:n].copy().view(np.uint8).reshape(V, H, W, 4), depth=host[1][:n].copy().view(np.float32).reshape(V, H, W),
                    ids=host[2][:n].reshape(V, H, W), guard=[h[n:] for h in host], pattern=np.int32(pattern))

    def dump(self, path):
        """the scene file of the stand-alone program"""
        has_ref, has_cf = self.ref_pos is not None, self.contact_forces is not None
        with open(path, "wb") as f:
            f.write(np.array([self.width, self.height, len(self.views), self.N, has_ref, has_cf, self.hf.shape[0], self.hf.shape[1]], np.int32).tobytes())
            f.write(np.array(self.min_point + self.dxdy, np.float32).tobytes())
            f.write(bytes(self.scene_struct(None)))
            f.write(render.prims_bytes(self.prims))
            f.write(b"".join(bytes(v) for v in self.views))
            for a in (self.hf, self.root_state, self.rigid_body_state, self.ref_pos, self.ref_rot, self.contact_forces, self.env_offsets):
                if a is not None:
                    f.write(a.tobytes())

    def read_program_output(self, path):
        V, H, W = len(self.views), self.height, self.width
        n = V * H * W
        raw = np.fromfile(path, dtype=np.uint32)
        assert raw.size == 3 * n
        return dict(rgba=raw[:n].copy().view(np.uint8).reshape(V, H, W, 4), ids=raw[n:2 * n].view(np.int32).reshape(V, H, W),
                    depth=raw[2 * n:].view(np.float32).reshape(V, H, W))


def humanoid():
    """(KinCharModel on the CPU, prims)"""
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    km = KinCharModel("cpu")
    km.load_char_file(humanoid_spec.write_mjcf())
    return km, render.scene_prims(km)
