"""ctypes declarations of the motion scorer's entry points (include/parc_score.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32

TILE = 16       # PARC_SCORE_TILE: frames per workgroup of the frame kernel


class ScoreTerrainS(ctypes.Structure):
    """parc_score_terrain_t"""
    _fields_ = [("hf", c_vp), ("dim_x", c_i32), ("dim_y", c_i32), ("min_x", c_f), ("min_y", c_f), ("dx", c_f), ("dy", c_f),
                ("x_points", c_vp), ("y_points", c_vp)]


SCORE_ARGTYPES = [c_vp, _hip.CharModelS, c_int, c_int] + [c_vp] * 5 + [c_int, c_vp, c_vp, ScoreTerrainS] + [c_f] * 5 + [c_vp] * 4


def declare(L):
    L.parc_score_abi.restype = c_int
    L.parc_motion_score.restype = c_int
    L.parc_motion_score.argtypes = SCORE_ARGTYPES
