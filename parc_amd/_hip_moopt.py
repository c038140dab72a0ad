"""ctypes declarations of the batched motion optimiser's entry points (include/parc_moopt.h)."""
import ctypes

c_vp, c_int, c_f, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32, ctypes.c_int64

SUM_LANES = 256     # PARC_MOOPT_SUM_LANES


class MooptTerrainS(ctypes.Structure):
    """parc_moopt_terrain_t"""
    _fields_ = [("off_hf", c_i32), ("off_x", c_i32), ("off_y", c_i32), ("dim_x", c_i32), ("dim_y", c_i32), ("ox", c_f), ("oy", c_f),
                ("half_x", c_f), ("half_y", c_f), ("base_z", c_f)]


RAGGED_ARGTYPES = [c_vp, c_i64, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_f, c_vp, c_vp]
RAGGED_GRAD_ARGTYPES = [c_vp, c_i64, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_int, c_vp, c_vp, c_vp]
TT_SEG_ARGTYPES = [c_vp, c_int, c_int, c_int] + [c_vp] * 7 + [c_f] * 3 + [c_vp]
TT_SEG_GRAD_ARGTYPES = [c_vp, c_int, c_int, c_int] + [c_vp] * 7 + [c_f] * 3 + [c_vp] * 3
SEGMENT_SUMS_ARGTYPES = [c_vp, c_int, c_int, c_int, c_int, c_vp, c_vp, c_vp]


def declare(L):
    L.parc_moopt_abi.restype = c_int
    for name, args in (("parc_points_hf_sdf_ragged", RAGGED_ARGTYPES), ("parc_points_hf_sdf_ragged_grad", RAGGED_GRAD_ARGTYPES),
                       ("parc_temporal_terms_seg", TT_SEG_ARGTYPES), ("parc_temporal_terms_seg_grad", TT_SEG_GRAD_ARGTYPES),
                       ("parc_segment_sums", SEGMENT_SUMS_ARGTYPES)):
        fn = getattr(L, name)
        fn.restype = c_int
        fn.argtypes = args
