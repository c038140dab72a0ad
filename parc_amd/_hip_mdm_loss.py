"""ctypes declarations of the generator loss's entry points (include/parc_mdm_loss.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f, c_i32, c_i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int32, ctypes.c_int64

TERMS = 14                      # PARC_MDM_LOSS_TERMS
SQUARED_L2, PSEUDO_HUBER = 0, 1
MAX_LDS = 65536                 # PARC_MDM_LOSS_MAX_LDS
EUNSUPPORTED = -2
(VEL_ROOT_POS, VEL_ROOT_ROT, VEL_JOINT_ROT, SIMPLE_ROOT_POS, SIMPLE_ROOT_ROT, SIMPLE_JOINT_ROT, SIMPLE_CONTACT, SIMPLE_BODY_POS, FK_BODY_POS,
 FK_BODY_ROT, BODY_POS_CONSISTENCY, VEL_FK_BODY_POS, HF_COLLISION, TARGET) = range(TERMS)


class MdmLossCfgS(ctypes.Structure):
    """parc_mdm_loss_cfg_t"""
    _fields_ = [("seq_len", c_i32), ("feat_dim", c_i32), ("ref_idx", c_i32),
                ("off_root_pos", c_i32), ("off_root_rot", c_i32), ("off_joint_pos", c_i32), ("off_joint_rot", c_i32), ("off_contacts", c_i32),
                ("dim_x", c_i32), ("dim_y", c_i32), ("loss_fn", c_i32), ("enabled", c_i32), ("num_points", c_i32),
                ("ox", c_f), ("oy", c_f), ("half_x", c_f), ("half_y", c_f), ("max_h", c_f), ("base_z", c_f), ("dt", c_f), ("target_eps", c_f),
                ("w", c_f * TERMS)]


FORWARD_ARGTYPES = [c_vp, _hip.CharModelS, MdmLossCfgS, c_int] + [c_vp] * 14
BACKWARD_ARGTYPES = [c_vp, _hip.CharModelS, MdmLossCfgS, c_int] + [c_vp] * 15


def declare(L):
    L.parc_mdm_loss_abi.restype = c_int
    L.parc_mdm_loss_lds_bytes.restype = c_i64
    L.parc_mdm_loss_lds_bytes.argtypes = [_hip.CharModelS, MdmLossCfgS]
    for name, args in (("parc_mdm_loss_forward", FORWARD_ARGTYPES), ("parc_mdm_loss_backward", BACKWARD_ARGTYPES)):
        fn = getattr(L, name)
        fn.restype = c_int
        fn.argtypes = args
