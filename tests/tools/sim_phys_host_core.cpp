// HOST build of the simulator core (parc_amd/csrc/parc_sim_core.h) with per-env physics parameters -- TEST INFRASTRUCTURE ONLY
// (tests/test_phys_params.py builds it with the host compiler).  Includes the control-mode host build, so that one library holds the
// step without a table (sim_ctl_host_step) and the step with one (sim_phys_host_step), the two sides of the bit-equality checks.
#include "sim_ctl_host_core.cpp"

// the argument rules of parc_sim_step_phys that concern the table (the host build sees the rows directly)
extern "C" int sim_phys_host_check(const parc_sim_env_params_t *env_params, int n_envs) {
    if (!env_params || n_envs < 0) return PARC_EINVAL;
    for (int e = 0; e < n_envs; ++e)
        if (!parc_sim::env_params_valid(env_params[e])) return PARC_EINVAL;
    return PARC_OK;
}

extern "C" int sim_phys_host_step(const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state, float *dof_state,
                                  float *rigid_body_state, float *contact_forces, const float *env_offsets, const float *action,
                                  const float *action_low, const float *action_high, int n_substeps, float h, int hold, int mode,
                                  float *dof_torque, parc_sim_env_params_t *env_params) {
    if (hold <= 0 || n_substeps % hold != 0) return PARC_EINVAL;
    if (sim_phys_host_check(env_params, n_envs) != PARC_OK) return PARC_EINVAL;
    return parc_sim::ctl_dispatch(mode, [&](auto m) {
        step_core<decltype(m)::value, true>(model, terrain, n_envs, root_state, dof_state, rigid_body_state, contact_forces, env_offsets, action,
                                            action_low, action_high, n_substeps, h, hold, dof_torque, env_params);
    }) ? 0 : PARC_EINVAL;
}
