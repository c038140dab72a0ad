"""ctypes declarations of the generator guidance step's entry points (include/parc_mdm_guide.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_d, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_int32, ctypes.c_int64

TERMS = 5                       # PARC_MDM_GUIDE_TERMS
TARGET, HF, SPEED, ACC, JERK = range(TERMS)
MAX_LDS = 65536                 # PARC_MDM_GUIDE_MAX_LDS
EINVAL, EUNSUPPORTED = -1, -2


class MdmGuideCfgS(ctypes.Structure):
    """parc_mdm_guide_cfg_t"""
    _fields_ = [("seq_len", c_i32), ("feat_dim", c_i32),
                ("off_root_pos", c_i32), ("off_root_rot", c_i32), ("off_joint_pos", c_i32), ("off_joint_rot", c_i32), ("off_contacts", c_i32),
                ("dim_x", c_i32), ("dim_y", c_i32), ("enabled", c_i32), ("num_points", c_i32),
                ("ox", c_f), ("oy", c_f), ("half_x", c_f), ("half_y", c_f), ("max_h", c_f), ("base_z", c_f), ("guidance_str", c_f),
                ("w", c_f * TERMS), ("dt", c_d), ("max_rate", c_d * 3)]


STEP_ARGTYPES = [c_vp, _hip.CharModelS, MdmGuideCfgS, c_int] + [c_vp] * 11


def lds_formula(S, nb, D, XY, P):
    """the byte formula of include/parc_mdm_guide.h"""
    n, J = S * nb, nb - 1
    return 4 * (XY + 7 * n + 4 * S * J + 7 * n + 4 * S * J + S * D + 5 * 16 + S * P + (S * P + 1) // 2)


def declare(L):
    L.parc_mdm_guide_abi.restype = c_int
    L.parc_mdm_guide_lds_bytes.restype = c_i64
    L.parc_mdm_guide_lds_bytes.argtypes = [_hip.CharModelS, MdmGuideCfgS]
    L.parc_mdm_guide_step.restype = c_int
    L.parc_mdm_guide_step.argtypes = STEP_ARGTYPES
