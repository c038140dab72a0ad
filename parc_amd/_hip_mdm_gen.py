"""ctypes declarations of the generator call's entry points (include/parc_mdm_gen.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32

Z_ROOT, Z_ROOT_FLOOR = 0, 1                     # PARC_MDM_GEN_Z_*
ROT_DEFAULT, ROT_EXP_MAP, ROT_QUAT = 0, 1, 2    # PARC_MDM_GEN_ROT_*
FRAME = 8                                       # PARC_MDM_GEN_FRAME
MAX_LDS = 65536                                 # PARC_MDM_GEN_MAX_LDS
EINVAL, EUNSUPPORTED = -1, -2


class MdmGenCfgS(ctypes.Structure):
    """parc_mdm_gen_cfg_t"""
    _fields_ = [("num_frames", c_i32), ("seq_len", c_i32), ("num_prev_states", c_i32), ("feat_dim", c_i32),
                ("off_root_pos", c_i32), ("off_root_rot", c_i32), ("off_joint_pos", c_i32), ("off_joint_rot", c_i32), ("off_contacts", c_i32),
                ("dim_x", c_i32), ("dim_y", c_i32), ("z_style", c_i32), ("rot_type", c_i32), ("min_h", c_f), ("max_h", c_f)]


ENCODE_ARGTYPES = [c_vp, _hip.CharModelS, MdmGenCfgS, _hip.TerrainS, c_int] + [c_vp] * 18
DECODE_ARGTYPES = [c_vp, _hip.CharModelS, MdmGenCfgS, c_int] + [c_vp] * 11


def declare(L):
    L.parc_mdm_gen_abi.restype = c_int
    L.parc_mdm_gen_encode.restype = c_int
    L.parc_mdm_gen_encode.argtypes = ENCODE_ARGTYPES
    L.parc_mdm_gen_decode.restype = c_int
    L.parc_mdm_gen_decode.argtypes = DECODE_ARGTYPES
