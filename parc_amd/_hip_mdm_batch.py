"""ctypes declarations of the batch sampler's entry points (include/parc_mdm_batch.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32, ctypes.c_int64

MAX_LOCAL_CELLS = 2048          # PARC_MDM_MAX_LOCAL_CELLS
MAX_TERRAIN_CELLS = 131072      # PARC_MDM_MAX_TERRAIN_CELLS
MAX_BOXES = 64                  # PARC_MDM_MAX_BOXES
MAX_SEQ_LEN = 1024              # PARC_MDM_MAX_SEQ_LEN
Z_ROOT, Z_ROOT_FLOOR = 0, 1
AUG_NOISE, AUG_MAXPOOL_AND_BOXES, AUG_NONE = 0, 1, 2
POOL_UNUSED, POOL_2D, POOL_X, POOL_Y = -1, 0, 1, 2
EUNSUPPORTED = -2


class MdmCfgS(ctypes.Structure):
    """parc_mdm_cfg_t"""
    _fields_ = [("seq_len", c_i32), ("ref_idx", c_i32), ("num_x_neg", c_i32), ("num_y_neg", c_i32), ("dim_x", c_i32), ("dim_y", c_i32),
                ("z_style", c_i32), ("mode", c_i32), ("max_boxes", c_i32), ("dt", c_f), ("min_h", c_f), ("max_h", c_f)]


class MdmClipS(ctypes.Structure):
    """parc_mdm_clip_t"""
    _fields_ = [("off_hf", c_i32), ("off_band", c_i32), ("dim_x", c_i32), ("dim_y", c_i32), ("min_x", c_f), ("min_y", c_f), ("dx", c_f),
                ("dy", c_f), ("frame_off", c_i32), ("num_frames", c_i32)]


class MdmDrawS(ctypes.Structure):
    """parc_mdm_draw_t"""
    _fields_ = [("change_height", c_i32), ("new_height", c_f), ("pool_kind", c_i32 * 3), ("pool_radius", c_i32 * 3), ("num_boxes", c_i32)]


class MdmBoxS(ctypes.Structure):
    """parc_mdm_box_t"""
    _fields_ = [("cx", c_f), ("cy", c_f), ("lx", c_f), ("ly", c_f), ("angle", c_f), ("h", c_f)]


HEIGHTFIELDS_ARGTYPES = [c_vp, _hip.MotionLibS, MdmCfgS, c_int] + [c_vp] * 5 + [c_int, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_int] + [c_vp] * 7
WINDOWS_ARGTYPES = [c_vp, _hip.CharModelS, _hip.MotionLibS, MdmCfgS, c_int] + [c_vp] * 13


def declare(L):
    L.parc_mdm_batch_abi.restype = c_int
    for name, args in (("parc_mdm_heightfields", HEIGHTFIELDS_ARGTYPES), ("parc_mdm_windows", WINDOWS_ARGTYPES)):
        fn = getattr(L, name)
        fn.restype = c_int
        fn.argtypes = args
