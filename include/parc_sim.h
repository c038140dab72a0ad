/*
 * parc_sim.h -- C-ABI of the articulated-body simulator inside libparc_hip.so.
 *
 * Stands in for the Isaac Gym calls of the reference's env step (paths relative to the reference root):
 *   gym.set_dof_position_target_tensor      envs/ig_char_env.py:489-495   (PD targets = clipped action)
 *   gym.simulate x sim_steps                envs/ig_env.py:830-837        (substeps from the YAML `sim:` block)
 *   gym.refresh_*_tensor                    envs/ig_env.py:850-860        (state published in the same tensors)
 * The state tensors ARE the simulator state (as with Isaac Gym): writing root_state / dof_state rows and
 * stepping is all a reset needs (envs/ig_env.py:693-721).
 * Dynamics parity is unpinned (no arithmetic reference exists outside the Isaac Gym binary); see DESIGN.md.
 */
#ifndef PARC_SIM_H
#define PARC_SIM_H

#include "parc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PARC_SIM_MAX_BODIES 16
#define PARC_SIM_MAX_DOFS 64
#define PARC_SIM_MAX_SPHERES 64

/* Character dynamics model, built on the host from the MJCF (data/assets/humanoid.xml): masses from geom
 * densities, PD gains = joint stiffness/damping, armature, limits (radians), motor gears as torque limits. */
typedef struct {
    int32_t num_bodies, dof_size, num_spheres, _pad;
    int32_t parent[PARC_SIM_MAX_BODIES];
    int32_t joint_type[PARC_SIM_MAX_BODIES];
    int32_t dof_idx[PARC_SIM_MAX_BODIES];
    float local_translation[PARC_SIM_MAX_BODIES][3];
    float local_rotation[PARC_SIM_MAX_BODIES][4];
    float joint_axis[PARC_SIM_MAX_BODIES][3];
    float mass[PARC_SIM_MAX_BODIES];
    float com[PARC_SIM_MAX_BODIES][3];          /* body frame */
    float inertia_o[PARC_SIM_MAX_BODIES][6];    /* about the body ORIGIN: xx xy xz yy yz zz */
    float kp[PARC_SIM_MAX_DOFS], kd[PARC_SIM_MAX_DOFS], armature[PARC_SIM_MAX_DOFS];
    float limit_lo[PARC_SIM_MAX_DOFS], limit_hi[PARC_SIM_MAX_DOFS], effort[PARC_SIM_MAX_DOFS];
    int32_t sph_body[PARC_SIM_MAX_SPHERES];      /* collision sample spheres */
    float sph_pos[PARC_SIM_MAX_SPHERES][3];
    float sph_radius[PARC_SIM_MAX_SPHERES];
    float gravity;                               /* 9.81 */
    float contact_kn, contact_cn, contact_ct, friction_mu, contact_max_pen;
    float limit_kp, limit_kd, max_angular_velocity;
    float angular_damping;                       /* 1/s, per link (asset_options.angular_damping, envs/ig_char_env.py:141): a couple
                                                    -c * I_com * omega on every body, i.e. d(omega)/dt = -c * omega for a free body */
    /* self-collision (Isaac Gym creates the actor with collision filter 0, envs/ig_char_env.py:105-113: links of one character
     * collide with each other except across a joint): one capsule per body (segment cap_p0..cap_p1 in the body frame, radius
     * cap_radius; <= 0 = none) and, per body, the set of bodies it is tested against (bit j of self_mask[b]) */
    float cap_p0[PARC_SIM_MAX_BODIES][3], cap_p1[PARC_SIM_MAX_BODIES][3], cap_radius[PARC_SIM_MAX_BODIES];
    uint32_t self_mask[PARC_SIM_MAX_BODIES];
} parc_sim_model_t;

/* One control step for n_envs environments: n_substeps semi-implicit Euler substeps of length h with PD
 * targets = clamp(action, action_low, action_high).  model is a DEVICE pointer to a parc_sim_model_t.
 * root_state [N,13], dof_state [N,D,2], rigid_body_state [N,B,13], contact_forces [N,B,3] (mean over the
 * substeps, env frame), env_offsets [N,3], action [N,D], action_low/high [D]. */
int parc_sim_step(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                  float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                  const float *action, const float *action_low, const float *action_high, int n_substeps, float h);

/* The same step, followed by IGEnv._update_time (envs/ig_env.py:862-865) inside the launch: timestep_buf[e] += 1 (int32),
 * time_buf[e] = timestep_buf[e] * step_dt.  */
int parc_sim_step_tick(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                       float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                       const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                       int32_t *timestep_buf, float *time_buf, float step_dt);

/* Control modes of parc_sim_step_ctl, numbered like the reference's ControlMode enum (envs/ig_char_env.py:20-25). */
#define PARC_SIM_CTL_PD 0       /* implicit position drive, targets = clamp(action): what parc_sim_step does */
#define PARC_SIM_CTL_VEL 1      /* implicit velocity drive (stiffness ignored), velocity targets = clamp(action) */
#define PARC_SIM_CTL_TORQUE 2   /* joint torque = clamp(action) */
#define PARC_SIM_CTL_PD_EXP 3   /* explicit PD on the relative joint rotation, targets = action (unclamped), held per hold */
#define PARC_SIM_CTL_PD_1D 4    /* explicit PD on the raw dof difference (1-D joints), targets = action (unclamped) */

/* One control step in any control mode (envs/ig_char_env.py:378-420,489-504).  The n_substeps substeps form
 * n_substeps / substeps_per_hold holds (one hold = one gym.simulate of substeps_per_hold PhysX substeps,
 * envs/ig_env.py:830-837); the explicit modes (pd_exp, pd_1d) compute their torque at the start of every hold and keep
 * it for the hold.  dof_torque [N,D] (optional; NULL for pd and vel) receives the torque of the last hold (torque,
 * pd_exp, pd_1d).  timestep_buf / time_buf: both NULL, or both given (IGEnv._update_time as in parc_sim_step_tick).
 * PARC_EINVAL for a mode out of range, n_substeps not a multiple of substeps_per_hold, only one of the clock buffers,
 * or dof_torque given for pd / vel. */
int parc_sim_step_ctl(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                      float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                      const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                      int substeps_per_hold, int control_mode, float *dof_torque, int32_t *timestep_buf, float *time_buf,
                      float step_dt);

/* Per-env physics parameters of parc_sim_step_phys: one row per env, N rows on the device.  The first five fields replace the model
 * struct's constants of the same name for that env; the scales multiply what the model holds.
 *   mass_scale      every link's mass and inertia (not armature, gains or effort)
 *   kp_scale/kd_scale  the drive gains m.kp / m.kd in every control mode (not the limit springs)
 *   push_force      world-frame force at the root link's centre of mass, applied in every substep while push_steps_left > 0;
 *                   the step decrements push_steps_left once per launch (= one control step)
 *   push_next_in    control steps until the sampler (parc_phys_rand) draws the next push; the step does not read it */
typedef struct {
    float gravity;
    float friction_mu;
    float contact_kn, contact_cn, contact_ct;
    float mass_scale;
    float kp_scale, kd_scale;
    float push_force[3];
    int32_t push_steps_left;
    int32_t push_next_in;
    int32_t _pad[3];                               /* rows are 64 bytes */
} parc_sim_env_params_t;

/* parc_sim_step_ctl with the per-env table env_params [N] (a DEVICE pointer): every control mode, pd included, runs
 * sim_step_bpl_phys_kernel<MODE>.  A table filled with the model's own constants, scales 1 and no push reproduces parc_sim_step /
 * parc_sim_step_ctl bit for bit.  PARC_EINVAL for what parc_sim_step_ctl refuses, for a NULL table, and for a row with a non-finite
 * or non-positive mass_scale, contact_kn or kp_scale, a negative (or NaN) friction_mu, contact_cn, contact_ct or kd_scale, a
 * non-finite gravity or push_force, or a negative push_steps_left.  The rows are checked by a small launch over the table in front
 * of the step whose one-word verdict the call waits for; while `stream` is being captured into a hipGraph nothing can be waited
 * for, so there the check is skipped and the table is the caller's responsibility (the env validates what it writes). */
int parc_sim_step_phys(void *stream, const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state,
                       float *dof_state, float *rigid_body_state, float *contact_forces, const float *env_offsets,
                       const float *action, const float *action_low, const float *action_high, int n_substeps, float h,
                       int substeps_per_hold, parc_sim_env_params_t *env_params, int control_mode, float *dof_torque,
                       int32_t *timestep_buf, float *time_buf, float step_dt);

/* The verdict alone: PARC_OK, or PARC_EINVAL if any of the n_envs rows breaks the rules above (waits for the stream). */
int parc_sim_env_params_check(void *stream, const parc_sim_env_params_t *env_params, int n_envs);

/* Ranges of the device-side sampler, [lo, hi] each; lo == hi fixes the value.  contact_kn / contact_cn / contact_ct / mass_scale are
 * drawn log-uniformly, the others uniformly.  Push: every push_interval (control steps, uniform integer in [lo, hi]) a horizontal
 * force of magnitude in push_force, uniform direction, for push_duration control steps; push_interval[1] <= 0 = no pushes. */
typedef struct {
    float gravity[2], friction_mu[2], contact_kn[2], contact_cn[2], contact_ct[2], mass_scale[2], kp_scale[2], kd_scale[2];
    float push_force[2];
    int32_t push_interval[2], push_duration[2];
    int32_t push_tick;                             /* != 0: this launch counts the push schedule down (one control step) */
    uint32_t field_mask;                           /* bit k set: field k (order above, gravity = bit 0 .. kd_scale = bit 7) is redrawn at a reset */
} parc_phys_ranges_t;

/* One launch per control step, capturable: for the envs whose reset_mask[e] != 0 (NULL = none) redraw the fields of field_mask, end a
 * running push and draw the interval to the next one; for every other env, if push_tick, count push_next_in down and, at 0, draw a
 * push (direction, magnitude, duration) and the next interval.  PARC_EINVAL for a NULL pointer, lo > hi, a non-finite bound, a
 * non-positive lower bound of a log-uniform field, or a push duration / interval below 1 when pushes are on.  Random numbers: Philox4x32-10 keyed by
 * `seed`, counter = (env, stream id, rng_state[0] lo, hi); rng_state[0] is the launch counter, advanced by the launch's last
 * workgroup, rng_state[1] its ticket (as parc_rng_step).  ranges is passed by value (host memory). */
int parc_phys_rand(void *stream, int n_envs, const int32_t *reset_mask, const parc_phys_ranges_t *ranges, uint64_t seed,
                   uint64_t *rng_state, parc_sim_env_params_t *env_params);

/* Recompute rigid_body_state (poses, velocities) from root_state / dof_state for the listed envs and zero
 * their contact forces: what the reference gets from refresh_rigid_body_state_tensor after a reset
 * (envs/ig_env.py:850-860).  env_ids int64 device pointer, NULL = all. */
int parc_sim_refresh_bodies(void *stream, const parc_sim_model_t *model, int n_envs, const int64_t *env_ids, int n_sel,
                            const float *root_state, const float *dof_state, float *rigid_body_state, float *contact_forces);

/* Same for every env whose mask[e] != 0 (device-side reset, no index list). */
int parc_sim_refresh_bodies_masked(void *stream, const parc_sim_model_t *model, int n_envs, const int32_t *mask,
                                   const float *root_state, const float *dof_state, float *rigid_body_state, float *contact_forces);

int parc_sim_abi(void);

#ifdef __cplusplus
}
#endif
#endif
