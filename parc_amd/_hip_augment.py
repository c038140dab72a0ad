"""ctypes declarations of the dataset augmentation's entry points (include/parc_augment.h)."""
import ctypes

c_vp, c_int, c_f, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32, ctypes.c_int64

FRAME_DIM = 34      # PARC_AUG_FRAME_DIM
MODE_NONE, MODE_HEIGHT_SCALE, MODE_BOXES_ALONG_PATH = 0, 1, 2


class AugFramesS(ctypes.Structure):
    """parc_augment_frames_t"""
    _fields_ = [("src_off", c_i32), ("src_len", c_i32), ("start", c_i32), ("length", c_i32), ("out_off", c_i32),
                ("cos_h", c_f), ("sin_h", c_f), ("qz", c_f), ("qw", c_f), ("sx", c_f), ("sy", c_f)]


class AugTerrainS(ctypes.Structure):
    """parc_augment_terrain_t"""
    _fields_ = [("off_hf", c_i32), ("off_x", c_i32), ("off_y", c_i32), ("dim_x", c_i32), ("dim_y", c_i32),
                ("min_x", c_f), ("min_y", c_f), ("dx", c_f), ("dy", c_f)]


class AugVariantS(ctypes.Structure):
    """parc_augment_variant_t"""
    _fields_ = [("src", c_i32), ("pad", c_i32), ("mode", c_i32), ("slice", c_i32), ("box_off", c_i32), ("box_count", c_i32),
                ("frame_off", c_i32), ("frame_len", c_i32), ("scale", c_f)]


class AugBoxS(ctypes.Structure):
    """parc_augment_box_t"""
    _fields_ = [("frame_ind", c_i32), ("len_x", c_f), ("len_y", c_f), ("angle", c_f), ("cos_a", c_f), ("sin_a", c_f), ("h", c_f)]


FRAMES_ARGTYPES = [c_vp, c_int, c_int, c_int, c_vp, c_vp, c_vp, c_int, c_vp, c_vp, c_vp]
TERRAINS_ARGTYPES = [c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_int, c_vp, c_int, c_vp, c_i64, c_vp]
LOCALIZE_ARGTYPES = [c_vp, c_int, c_vp, c_vp, c_vp, c_int, c_vp]


def declare(L):
    L.parc_augment_abi.restype = c_int
    for name, args in (("parc_augment_frames", FRAMES_ARGTYPES), ("parc_augment_terrains", TERRAINS_ARGTYPES),
                       ("parc_augment_localize", LOCALIZE_ARGTYPES)):
        fn = getattr(L, name)
        fn.restype = c_int
        fn.argtypes = args
