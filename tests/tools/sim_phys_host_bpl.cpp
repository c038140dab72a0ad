// HOST build of the body-per-lane kernel (parc_amd/csrc/parc_sim_bpl.h) with per-env physics parameters, under the 16-fiber lane
// emulation of oracle/sim_host_bpl.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_phys_params.py).  Includes the control-mode host build
// (sim_ctl_host_step_bpl: the step without a table).
#include "sim_ctl_host_bpl.cpp"

namespace {
struct PhysArgs {
    CtlArgs c;
    const parc_sim_env_params_t *ep;        // this env's row, as the kernel's LDS copy
};
template <int MODE>
void phys_lane(int lane, const PhysArgs &p) {
    const EnvArgs &a = p.c.a;
    parc_sim_bpl::step_lane<MODE, true>(*a.m, *a.ter, lane, a.root_state, a.dof_state, a.rigid_body_state, a.contact_forces, a.env_offset,
                                        a.action, a.lo, a.hi, a.n_sub, a.h, a.lds, a.cc + lane * (BPL_CC_SLOTS * BPL_CC_FLOATS + 1), p.c.hold,
                                        p.c.dof_torque, p.ep);
}
void phys_lane_body(int lane, void *q) {
    const PhysArgs &p = *(const PhysArgs *)q;
    (void)parc_sim::ctl_dispatch(p.c.mode, [&](auto m) { phys_lane<decltype(m)::value>(lane, p); });      // (the entry point has refused any other mode)
}
}  // namespace

extern "C" int sim_phys_host_step_bpl(const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state, float *dof_state,
                                      float *rigid_body_state, float *contact_forces, const float *env_offsets, const float *action,
                                      const float *action_low, const float *action_high, int n_substeps, float h, int hold, int mode,
                                      float *dof_torque, parc_sim_env_params_t *env_params) {
    const int B = model->num_bodies, D = model->dof_size;
    if (B > lane_emu::LANES) return -2;
    if (hold <= 0 || n_substeps % hold != 0 || mode < PARC_SIM_CTL_PD || mode > PARC_SIM_CTL_PD_1D) return PARC_EINVAL;
    if (!env_params) return PARC_EINVAL;
    for (int e = 0; e < n_envs; ++e)
        if (!parc_sim::env_params_valid(env_params[e])) return PARC_EINVAL;
    for (int e = 0; e < n_envs; ++e) {
        float lds[BPL_G * BPL_CONTRIB];
        float cc[lane_emu::LANES * (BPL_CC_SLOTS * BPL_CC_FLOATS + 1)];
        memset(lds, g_fill < 0 ? 0 : g_fill, sizeof lds);
        memset(cc, g_fill < 0 ? 0 : g_fill, sizeof cc);
        const parc_sim_env_params_t row = env_params[e];          // the kernel stages the row before the step, and so does this
        PhysArgs p{CtlArgs{EnvArgs{model, &terrain, root_state + 13 * (size_t)e, dof_state + 2 * (size_t)D * e,
                                   rigid_body_state + 13 * (size_t)B * e, contact_forces + 3 * (size_t)B * e, env_offsets + 3 * (size_t)e,
                                   action + (size_t)D * e, action_low, action_high, n_substeps, h, lds, cc},
                           hold, mode, dof_torque ? dof_torque + (size_t)D * e : nullptr},
                   &row};
        lane_emu::run(phys_lane_body, &p);
        if (row.push_steps_left > 0) env_params[e].push_steps_left = row.push_steps_left - 1;      // as sim_step_bpl_phys_kernel
    }
    return 0;
}
