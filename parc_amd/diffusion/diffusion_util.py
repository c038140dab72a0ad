"""Names the sampler and the loss share with the reference's trainer (reference diffusion/diffusion_util.py:6-17,65-69 and
diffusion/mdm.py:39-55, :63-67): same members, same values."""
import enum


class RelativeZStyle(enum.Enum):
    RELATIVE_TO_ROOT = 0
    RELATIVE_TO_ROOT_FLOOR = 1


class MDMFrameType(enum.Enum):
    ROOT_POS = 0
    ROOT_ROT = 1
    JOINT_POS = 2
    JOINT_VEL = 3
    JOINT_ROT = 4
    CONTACTS = 5
    FLOOR_HEIGHTS = 6


class MDMKeyType(enum.Enum):
    """keys of the sampler's `conds` dictionary (reference diffusion/diffusion_util.py:19-36; 7 and 13 are unused there too)"""
    OBS_KEY = 0
    PREV_STATE_KEY = 1
    PREV_STATE_FLAG_KEY = 2
    TARGET_KEY = 3
    TARGET_FLAG_KEY = 4
    FINAL_STATE_KEY = 5
    PREV_STATE_NOISE_IND_KEY = 6
    OBS_FLAG_KEY = 8
    GUIDANCE_PARAMS = 9
    NOISE_IND_KEY = 10
    CANON_FRAME_IDX = 11
    CLEAN_STATE_KEY = 12
    FEATURE_VECTOR_KEY = 14
    FEATURE_VECTOR_FLAG_KEY = 15
    IN_PAINT_PARAMS = 16


class GenerationMode(enum.Enum):
    """reference diffusion/mdm.py:57-61"""
    MODE_REVERSE_DIFFUSION = 0
    MODE_DDIM = 1
    MODE_ECM = 2
    NONE = 3


class MDMCustomGuidance:
    """what conds[GUIDANCE_PARAMS] carries (reference diffusion/diffusion_util.py:38-57): class attributes as defaults"""
    obs_cfg_scale = None
    guidance_str = 0.1
    target_xy = None
    target_floor_height = None
    w_target_loss = 1.0
    w_hf_loss = 10.0
    body_points = None          # list over the bodies of [num points of body b, 3]
    verbose = True
    strong_hf_guidance = False

    guide_speed = False
    guide_acc = False
    guide_jerk = False
    max_speed = 16.1498
    max_acc = 343.0243
    max_jerk = 14062.6680
    w_speed = 1.0 / 16.1498
    w_acc = 1.0 / 343.0243
    w_jerk = 1.0 / 14062.6680


class TargetInfo:
    def __init__(self, future_pos, future_rot):
        self.future_pos = future_pos
        self.future_rot = future_rot


class LossType(enum.Enum):
    SIMPLE_ROOT_POS_LOSS = 0
    SIMPLE_ROOT_ROT_LOSS = 1
    SIMPLE_JOINT_ROT_LOSS = 2
    SIMPLE_CONTACT_LOSS = 3
    VEL_ROOT_POS_LOSS = 4
    VEL_ROOT_ROT_LOSS = 5
    VEL_JOINT_ROT_LOSS = 6
    FK_BODY_POS_LOSS = 7
    FK_BODY_ROT_LOSS = 8
    FOOT_CONTACT_LOSS = 9
    TARGET_LOSS = 10
    HF_COLLISION_LOSS = 11
    SIMPLE_FLOOR_HEIGHT_LOSS = 12
    SIMPLE_BODY_POS_LOSS = 13
    BODY_POS_CONSISTENCY_LOSS = 14
    VEL_FK_BODY_POS_LOSS = 15
