"""ctypes declarations of the renderer entry points (include/parc_render.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32

MAX_PRIMS = 32
SPHERE, CAPSULE, BOX = 0, 1, 2
CAMERA_MODES = {"still": 0, "track": 1}       # the reference's CameraMode enum (envs/ig_char_env.py:27-29)


class PrimS(ctypes.Structure):
    """parc_render_prim_t: one geom in its body's frame (64 bytes)"""
    _fields_ = [("body", c_i32), ("type", c_i32), ("a", c_f * 3), ("b", c_f * 3), ("radius", c_f), ("q", c_f * 4), ("_pad", c_f * 3)]


class SceneS(ctypes.Structure):
    """parc_render_scene_t"""
    _fields_ = [("prims", c_vp), ("n_prims", c_i32), ("num_bodies", c_i32), ("light_dir", c_f * 3), ("ambient", c_f),
                ("sim_color", c_f * 3), ("ref_color", c_f * 3), ("ref_char_offset", c_f * 3), ("shadows", c_i32), ("show_contacts", c_i32),
                ("contact_eps", c_f)]


class ViewS(ctypes.Structure):
    """parc_render_view_t: one 64-byte row per view"""
    _fields_ = [("env", c_i32), ("mode", c_i32), ("fov_y", c_f), ("vec", c_f * 3), ("target", c_f * 3), ("_pad", c_f * 7)]


assert ctypes.sizeof(PrimS) == 64 and ctypes.sizeof(ViewS) == 64

RENDER_ARGTYPES = [c_vp, _hip.TerrainS, ctypes.POINTER(SceneS), c_int, c_vp, c_int, c_int] + [c_vp] * 6 + [c_int, c_vp, c_vp, c_vp]


def declare(L):
    L.parc_render_abi.restype = c_int
    L.parc_render.restype = c_int
    L.parc_render.argtypes = RENDER_ARGTYPES
