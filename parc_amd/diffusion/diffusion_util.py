"""Names the sampler shares with the reference's trainer (reference diffusion/diffusion_util.py:6-17,65-69): same members, same values."""
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
