"""ctypes declarations of the simulator entry points (include/parc_sim.h)."""
import ctypes

from . import _hip

c_vp, c_int, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


c_i32 = ctypes.c_int32


class EnvParamsS(ctypes.Structure):
    """parc_sim_env_params_t: one 64-byte row of the per-env physics table"""
    _fields_ = [("gravity", c_f), ("friction_mu", c_f), ("contact_kn", c_f), ("contact_cn", c_f), ("contact_ct", c_f), ("mass_scale", c_f),
                ("kp_scale", c_f), ("kd_scale", c_f), ("push_force", c_f * 3), ("push_steps_left", c_i32), ("push_next_in", c_i32),
                ("_pad", c_i32 * 3)]


# the randomisable fields in the order of the row (= bit order of parc_phys_ranges_t.field_mask) and which of them are drawn log-uniformly
PHYS_FIELDS = ("gravity", "friction_mu", "contact_kn", "contact_cn", "contact_ct", "mass_scale", "kp_scale", "kd_scale")
PHYS_LOG_FIELDS = ("contact_kn", "contact_cn", "contact_ct", "mass_scale")
PHYS_ROW_WORDS = ctypes.sizeof(EnvParamsS) // 4
PHYS_COLUMN = {f: i for i, f in enumerate(PHYS_FIELDS)}       # word of the row that holds the field
PHYS_COLUMN.update({"push_force": 8, "push_steps_left": 11, "push_next_in": 12})


class PhysRangesS(ctypes.Structure):
    """parc_phys_ranges_t"""
    _fields_ = [(f, c_f * 2) for f in PHYS_FIELDS] + [("push_force", c_f * 2), ("push_interval", c_i32 * 2), ("push_duration", c_i32 * 2),
                                                      ("push_tick", c_i32), ("field_mask", ctypes.c_uint32)]


def declare(L):
    L.parc_sim_abi.restype = c_int
    # stream, model, terrain, n_envs, the four state tensors, env offsets, action, its two bounds, n_substeps, h
    step = [c_vp, c_vp, _hip.TerrainS, c_int] + [c_vp] * 8 + [c_int, c_f]
    clock = [c_vp, c_vp, c_f]                 # timestep_buf, time_buf, step_dt
    L.parc_sim_step.restype = c_int
    L.parc_sim_step.argtypes = step
    L.parc_sim_step_tick.restype = c_int
    L.parc_sim_step_tick.argtypes = step + clock
    L.parc_sim_refresh_bodies.restype = c_int
    L.parc_sim_refresh_bodies.argtypes = [c_vp, c_vp, c_int, c_vp, c_int, c_vp, c_vp, c_vp, c_vp]
    L.parc_sim_refresh_bodies_masked.restype = c_int
    L.parc_sim_refresh_bodies_masked.argtypes = [c_vp, c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_vp]
    L.parc_sim_step_ctl.restype = c_int
    L.parc_sim_step_ctl.argtypes = step + [c_int, c_int, c_vp] + clock
    L.parc_sim_step_phys.restype = c_int
    L.parc_sim_step_phys.argtypes = step + [c_int, c_vp, c_int, c_vp] + clock
    L.parc_sim_env_params_check.restype = c_int
    L.parc_sim_env_params_check.argtypes = [c_vp, c_vp, c_int]
    L.parc_phys_rand.restype = c_int
    L.parc_phys_rand.argtypes = [c_vp, c_int, c_vp, ctypes.POINTER(PhysRangesS), ctypes.c_uint64, c_vp, c_vp]


# control modes of parc_sim_step_ctl (include/parc_sim.h PARC_SIM_CTL_*), numbered like the reference's ControlMode enum
CONTROL_MODES = {"pd": 0, "vel": 1, "torque": 2, "pd_exp": 3, "pd_1d": 4}
