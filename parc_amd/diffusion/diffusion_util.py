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
