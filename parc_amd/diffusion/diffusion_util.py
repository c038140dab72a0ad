"""Names the sampler and the loss share with the reference's trainer (reference diffusion/diffusion_util.py:6-17,65-69 and
diffusion/mdm.py:39-55, :63-67): same members, same values.  Below them, what the callers of the generator's device kernels share when
they fill a configuration structure and its tables (include/parc_mdm_loss.h, parc_mdm_guide.h, parc_mdm_gen.h)."""
import enum

import numpy as np
import torch


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


# ---------------------------------------------------------------------- tables of the device kernels
def set_feature_layout(c, features):
    """feat_dim and the five slice offsets of a parc_mdm_{loss,guide,gen}_cfg_t, from the MDMMotionLoss that registered the features; a
    component the layout does not have is -1"""
    c.feat_dim = features._motion_frame_dof
    off = lambda name: features._feature_slices[features.MDMFrameType[name]].start if name in features._component_names else -1
    c.off_root_pos, c.off_root_rot, c.off_joint_rot = off("ROOT_POS"), off("ROOT_ROT"), off("JOINT_ROT")
    c.off_joint_pos, c.off_contacts = off("JOINT_POS"), off("CONTACTS")


def set_local_grid(c, features):
    """ox, oy, half_x, half_y of a parc_mdm_{loss,guide}_cfg_t: the reference's float32 arithmetic on the cell size"""
    dx = np.float32(features._dx)
    c.ox, c.oy = float(-dx * np.float32(features._num_x_neg)), float(-dx * np.float32(features._num_y_neg))
    c.half_x = c.half_y = float(dx / np.float32(2.0))


def local_grid_axes(features):
    """(grid_x [X], grid_y [Y]) on the features' device: the host's linspace, copied"""
    X, Y = features._grid_dim_x, features._grid_dim_y
    return (torch.linspace(0.0, (X - 1.0) * features._dxdy[0].item(), X).to(features._device),
            torch.linspace(0.0, (Y - 1.0) * features._dxdy[1].item(), Y).to(features._device))


def pack_body_points(body_points, device):
    """per-body list of [num points of body b, 3] -> (points [max(P, 1), 3], point_start [nb + 1] int32, P) on the device"""
    counts = [int(p.shape[0]) for p in body_points]
    start = torch.zeros(len(counts) + 1, dtype=torch.int32)
    start[1:] = torch.cumsum(torch.tensor(counts), 0)
    P = int(start[-1])
    pts = torch.cat([p.detach().to(device="cpu", dtype=torch.float32).reshape(-1, 3) for p in body_points]) if P else torch.zeros((1, 3))
    return pts.contiguous().to(device), start.to(device), P
