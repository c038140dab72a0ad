// HOST build of the body-per-lane kernel (parc_amd/csrc/parc_sim_bpl.h) in every control mode, under the 16-fiber lane emulation of
// oracle/sim_host_bpl.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_control_modes.py builds it with the host compiler).
#include "../../oracle/sim_host_bpl.cpp"

namespace {
struct CtlArgs {
    EnvArgs a;
    int hold, mode;
    float *dof_torque;
};
template <int MODE>
void ctl_lane(int lane, const CtlArgs &c) {
    const EnvArgs &a = c.a;
    parc_sim_bpl::step_lane<MODE>(*a.m, *a.ter, lane, a.root_state, a.dof_state, a.rigid_body_state, a.contact_forces, a.env_offset, a.action,
                                  a.lo, a.hi, a.n_sub, a.h, a.lds, a.cc + lane * (BPL_CC_SLOTS * BPL_CC_FLOATS + 1), c.hold, c.dof_torque);
}
void ctl_lane_body(int lane, void *p) {
    const CtlArgs &c = *(const CtlArgs *)p;
    (void)parc_sim::ctl_dispatch(c.mode, [&](auto m) { ctl_lane<decltype(m)::value>(lane, c); });      // (the entry point has refused any other mode)
}
}  // namespace

extern "C" int sim_ctl_host_step_bpl(const parc_sim_model_t *model, parc_terrain_t terrain, int n_envs, float *root_state, float *dof_state,
                                     float *rigid_body_state, float *contact_forces, const float *env_offsets, const float *action,
                                     const float *action_low, const float *action_high, int n_substeps, float h, int hold, int mode,
                                     float *dof_torque) {
    const int B = model->num_bodies, D = model->dof_size;
    if (B > lane_emu::LANES) return -2;
    if (hold <= 0 || n_substeps % hold != 0 || mode < PARC_SIM_CTL_PD || mode > PARC_SIM_CTL_PD_1D) return PARC_EINVAL;
    for (int e = 0; e < n_envs; ++e) {
        float lds[BPL_G * BPL_CONTRIB];
        float cc[lane_emu::LANES * (BPL_CC_SLOTS * BPL_CC_FLOATS + 1)];
        memset(lds, g_fill < 0 ? 0 : g_fill, sizeof lds);
        memset(cc, g_fill < 0 ? 0 : g_fill, sizeof cc);
        CtlArgs c{EnvArgs{model, &terrain, root_state + 13 * (size_t)e, dof_state + 2 * (size_t)D * e, rigid_body_state + 13 * (size_t)B * e,
                          contact_forces + 3 * (size_t)B * e, env_offsets + 3 * (size_t)e, action + (size_t)D * e, action_low, action_high,
                          n_substeps, h, lds, cc},
                  hold, mode, dof_torque ? dof_torque + (size_t)D * e : nullptr};
        lane_emu::run(ctl_lane_body, &c);
    }
    return 0;
}
