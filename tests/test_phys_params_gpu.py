"""Per-env physics parameters on the DEVICE: the checks of tests/test_phys_params.py on sim_step_bpl_phys_kernel through
parc_sim_step_phys, the neutral table against parc_sim_step / parc_sim_step_ctl bit for bit on the bench workload, the argument
checks on device rows, the sampler parc_phys_rand, and the env (YAML gravity, `physics_rand`, setters, captured rollout)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import sim_ctl  # noqa: E402
import sim_phys  # noqa: E402
import test_control_modes as cm  # noqa: E402
import test_phys_params as pp  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def humanoid():
    return sim_ctl.humanoid_struct()


def test_neutral_table_is_bitwise_the_plain_step_on_the_device(humanoid):
    pp.check_neutral_table_is_bitwise_the_plain_step(humanoid, "device", None)


def test_rows_are_independent_on_the_device(humanoid):
    pp.check_rows_are_independent(humanoid, "device", None)


def test_free_fall_follows_the_rows_gravity_on_the_device(humanoid):
    pp.check_free_fall_follows_the_rows_gravity(humanoid, "device", None)


def test_friction_per_env_on_the_device(humanoid):
    pp.check_friction_per_env(humanoid, "device", None)


def test_rest_depth_per_env_on_the_device(humanoid):
    pp.check_rest_depth_per_env(humanoid, "device", None)


def test_oscillator_with_scales_on_the_device(humanoid):
    pp.check_oscillator_with_scales(humanoid, "device", None)


def test_explicit_pd_and_vel_with_gain_scales_on_the_device(humanoid):
    pp.check_explicit_pd_and_vel_with_gain_scales(humanoid, "device", None)


def test_push_delivers_its_momentum_on_the_device(humanoid):
    pp.check_push_delivers_its_momentum(humanoid, "device", None)


def test_push_on_the_humanoid_on_the_device(humanoid):
    pp.check_push_on_the_humanoid(humanoid, "device", None)


def _neutral_table(env, n):
    from parc_amd import _hip_sim
    st = env._sim_model.struct
    row = _hip_sim.EnvParamsS(gravity=st.gravity, friction_mu=st.friction_mu, contact_kn=st.contact_kn, contact_cn=st.contact_cn,
                              contact_ct=st.contact_ct, mass_scale=1.0, kp_scale=1.0, kd_scale=1.0)
    return torch.frombuffer(bytearray(bytes(row)), dtype=torch.float32).to(DEV).repeat(n, 1).contiguous()


@pytest.mark.parametrize("mode", ["pd", "vel", "torque", "pd_exp", "pd_1d"])
def test_neutral_table_on_the_bench_workload_is_bitwise(mode):
    """4096 envs of boxes_64clips, 32 steps from the reset state: parc_sim_step_phys with the neutral table == parc_sim_step (pd) /
    parc_sim_step_ctl (the other modes), every state tensor and the torque output bit for bit.  (pd_1d steps the humanoid only as a
    kernel workload, as tools/bench_sim_modes.py does.)"""
    from parc_amd import _hip, _hip_sim, workloads
    N = 4096
    env, _, _ = workloads.build_env("boxes_64clips", N, DEV, seed=0)
    env.reset()
    c = env._core
    D = env._cfg.dof_size
    table = _neutral_table(env, N)
    gen = torch.Generator(device=DEV).manual_seed(0)
    eff = torch.tensor([env._sim_model.struct.effort[d] for d in range(D)], device=DEV)
    lo, hi = env._action_bound_low, env._action_bound_high
    if mode == "vel":
        lo, hi = torch.full((D,), -2 * np.pi, device=DEV), torch.full((D,), 2 * np.pi, device=DEV)
        acts = [(torch.rand((N, D), device=DEV, generator=gen) * 2 - 1) * 0.5 for _ in range(32)]
    elif mode == "torque":
        lo, hi = -eff, eff
        acts = [(torch.rand((N, D), device=DEV, generator=gen) * 2 - 1) * 0.1 * eff for _ in range(32)]
    else:
        acts = [env._ref_dof_pos.clone() + 0.1 * torch.randn((N, D), device=DEV, generator=gen) for _ in range(32)]
    m = _hip_sim.CONTROL_MODES[mode]
    has_tq = mode in ("torque", "pd_exp", "pd_1d")
    tensors = (c.root_state, c.dof_state, c.rigid_body_state, c.contact_forces)
    start = [t.clone() for t in tensors]
    res = []
    for phys in (False, True):
        for t, s in zip(tensors, start):
            t.copy_(s)
        tq = torch.full((N, D), float("nan"), device=DEV) if has_tq else None
        for a in acts:
            args = (_hip.stream(), env._sim_model.device_ptr(DEV), c._terrain_struct, N, _hip.ptr(c.root_state), _hip.ptr(c.dof_state),
                    _hip.ptr(c.rigid_body_state), _hip.ptr(c.contact_forces), _hip.ptr(c.env_offsets), _hip.ptr(a), _hip.ptr(lo), _hip.ptr(hi),
                    env._sim_steps * env._substeps, env._sim_h)
            if phys:
                rc = _hip.lib().parc_sim_step_phys(*args, env._substeps, _hip.ptr(table), m, _hip.ptr(tq), None, None, 0.0)
            elif mode == "pd":
                rc = _hip.lib().parc_sim_step(*args)
            else:
                rc = _hip.lib().parc_sim_step_ctl(*args, env._substeps, m, _hip.ptr(tq), None, None, 0.0)
            _hip.check(rc, "step")
        torch.cuda.synchronize()
        res.append([t.clone() for t in tensors] + ([tq] if has_tq else []))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert not torch.equal(res[0][1], start[1]) and torch.isfinite(res[0][1]).all()


def test_device_refuses_bad_rows(humanoid):
    """every rule of the table on DEVICE rows: parc_sim_step_phys returns PARC_EINVAL and launches no step; parc_sim_env_params_check
    gives the verdict alone"""
    from parc_amd import _hip
    _, sm = humanoid
    for field, val in pp.BAD_ROWS:
        sim = pp.make_body(sm.struct, 300, "device", None)
        sim.params[field][257] = val
        before = sim.state()
        sim.step(pp.NO_ACT, "pd", expect=-1)
        for a, b in zip(sim.state(), before):
            np.testing.assert_array_equal(a, b)
        t = torch.frombuffer(bytearray(sim.params.tobytes()), dtype=torch.uint8).to(DEV)
        assert _hip.lib().parc_sim_env_params_check(_hip.stream(), _hip.c_vp(t.data_ptr()), 300) == -1, field
        assert _hip.lib().parc_sim_env_params_check(_hip.stream(), _hip.c_vp(t.data_ptr()), 257) == 0, field
    sim = pp.make_body(sm.struct, 3, "device", None)
    sim.params["friction_mu"], sim.params["contact_cn"], sim.params["contact_ct"], sim.params["kd_scale"] = 0.0, 0.0, 0.0, 0.0
    sim.step(pp.NO_ACT, "pd")


def test_device_matches_the_host_build_with_a_table(humanoid, tmp_path):
    """one step with non-neutral, pushed rows: the device kernel and the host build of the same header agree (the bounds of
    test_control_modes_gpu.test_device_matches_the_host_build_in_every_mode)"""
    import copy
    _, sm = humanoid
    lib = sim_phys.build_host(str(tmp_path))
    rng = np.random.default_rng(11)
    n = 8
    dof = rng.normal(0.0, 0.3, (n, 28)).astype(np.float32)
    vel = rng.normal(0.0, 1.0, (n, 28)).astype(np.float32)
    act = rng.normal(0.0, 0.5, (n, 28)).astype(np.float32)
    for mode in sim_ctl.MODES:
        out = []
        for variant in ("bpl", "device"):
            sim = sim_phys.PhysSim(copy.deepcopy(sm.struct), n, variant, lib=lib)
            sim.params["gravity"] = np.linspace(0.0, 12.0, n)
            sim.params["mass_scale"], sim.params["kp_scale"], sim.params["kd_scale"] = np.linspace(0.6, 1.5, n), np.linspace(0.5, 2.0, n), np.linspace(0.0, 2.0, n)
            sim.params["push_force"][:, 0], sim.params["push_steps_left"] = np.linspace(-100.0, 100.0, n), 1
            sim.root_state[:, 2] = 3.0
            sim.dof_state[..., 0], sim.dof_state[..., 1] = dof, vel
            sim.step(act, mode, n_sub=2, hold=2)
            out.append((sim.dof_state.copy(), sim.root_state.copy()))
        np.testing.assert_allclose(out[1][0], out[0][0], rtol=2e-4, atol=2e-4, err_msg=mode)
        np.testing.assert_allclose(out[1][1], out[0][1], rtol=2e-4, atol=2e-4, err_msg=mode)


# ---------------------------------------------------------------------------------------------------------------------- sampler
def _ranges(**kw):
    from parc_amd import _hip_sim
    rg = _hip_sim.PhysRangesS()
    for k, f in enumerate(_hip_sim.PHYS_FIELDS):
        if f in kw:
            getattr(rg, f)[0], getattr(rg, f)[1] = kw[f]
            rg.field_mask |= 1 << k
    return rg


def _rand(n, mask, rg, seed, state, table):
    from parc_amd import _hip
    _hip.check(_hip.lib().parc_phys_rand(_hip.stream(), n, _hip.ptr(mask), rg, seed, _hip.ptr(state), _hip.ptr(table)), "parc_phys_rand")
    torch.cuda.synchronize()


RANGES = dict(gravity=(8.0, 11.0), friction_mu=(0.5, 1.5), contact_kn=(1e4, 1.6e5), contact_cn=(5e2, 2e3), contact_ct=(1.5e3, 6e3),
              mass_scale=(0.8, 1.25), kp_scale=(0.5, 2.0), kd_scale=(0.0, 2.0))


def test_sampler_draws_in_range_log_uniform_masked_and_reproducible():
    """parc_phys_rand at a reset: every drawn value lies in its range; the log-uniform fields fill 16 bins of equal RATIO evenly and
    the uniform ones 16 bins of equal width (chi^2 with 15 degrees of freedom over N = 65536 draws, fixed seed: bound 44.3, the
    1 - 1e-4 quantile - and, against a uniform draw of a log field, bins 1 and 16 of a 16x band would hold 4.3x / 0.27x the even
    share, chi^2 ~ N); only masked envs are redrawn, the others stay bit for bit; two launches from the same generator state agree
    bit for bit, two consecutive ones do not."""
    from parc_amd import _hip_sim
    N = 65536
    col = _hip_sim.PHYS_COLUMN
    table = torch.zeros((N, 16), dtype=torch.float32, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    ones = torch.ones(N, dtype=torch.int32, device=DEV)
    rg = _ranges(**RANGES)
    _rand(N, ones, rg, 1234, state, table)
    assert state.tolist() == [1, 0]
    t = table.cpu().numpy().astype(np.float64)
    for f, (lo, hi) in RANGES.items():
        v = t[:, col[f]]
        assert v.min() >= np.float32(lo) and v.max() <= np.float32(hi), f
        u = np.log(v / lo) / np.log(hi / lo) if f in _hip_sim.PHYS_LOG_FIELDS else (v - lo) / (hi - lo)
        counts = np.histogram(u, bins=16, range=(0.0, 1.0))[0]
        chi2 = ((counts - N / 16.0) ** 2 / (N / 16.0)).sum()
        assert chi2 < 44.3, (f, chi2, counts)
    assert np.all(t[:, 8:] == 0.0)                                # no push configured: the push words stay untouched
    # the fields are independent draws
    assert abs(np.corrcoef(t[:, col["contact_kn"]], t[:, col["friction_mu"]])[0, 1]) < 0.02
    # same generator state -> same rows; the next launch -> other rows
    first = table.clone()
    state.zero_()
    table.zero_()
    _rand(N, ones, rg, 1234, state, table)
    assert torch.equal(table, first)
    _rand(N, ones, rg, 1234, state, table)
    assert not torch.equal(table[:, :8], first[:, :8]) and state.tolist() == [2, 0]
    # masked
    mask = (torch.arange(N, device=DEV) % 3 == 0).to(torch.int32)
    before = table.clone()
    _rand(N, mask, rg, 1234, state, table)
    keep = mask == 0
    assert torch.equal(table[keep], before[keep])
    assert (table[~keep][:, :8] != before[~keep][:, :8]).all(dim=1).float().mean() > 0.99
    # a field outside field_mask is never written
    rg2 = _ranges(contact_kn=(1e4, 1.6e5))
    before = table.clone()
    _rand(N, ones, rg2, 1234, state, table)
    others = [i for i in range(16) if i != col["contact_kn"]]
    assert torch.equal(table[:, others], before[:, others]) and not torch.equal(table, before)
    _rand(N, None, rg, 1234, state, table.clone())               # no mask: nothing is redrawn, the launch still counts
    assert state.tolist()[0] == 5


def test_sampler_push_schedule():
    """Pushes: an env that restarts is unpushed and gets an interval in [lo, hi]; every launch with push_tick counts it down; at 0 a
    push is drawn - horizontal, magnitude and duration in range - with the next interval; the gap between two draws of an env is the
    interval drawn at the first.  Directions cover the circle.  Without push_tick nothing moves."""
    from parc_amd import _hip_sim
    N = 4096
    col = _hip_sim.PHYS_COLUMN
    table = torch.zeros((N, 16), dtype=torch.float32, device=DEV)
    ti = table.view(torch.int32)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    rg = _ranges()
    rg.push_interval[0], rg.push_interval[1] = 3, 6
    rg.push_duration[0], rg.push_duration[1] = 1, 2
    rg.push_force[0], rg.push_force[1] = 50.0, 200.0
    ti[:, col["push_steps_left"]] = 7                             # a running push ends with the episode
    _rand(N, torch.ones(N, dtype=torch.int32, device=DEV), rg, 99, state, table)
    nxt = ti[:, col["push_next_in"]].cpu().numpy().copy()
    assert nxt.min() == 3 and nxt.max() == 6 and (ti[:, col["push_steps_left"]] == 0).all()
    assert np.bincount(nxt)[3:].min() > 0.8 * N / 4
    before = table.clone()
    _rand(N, None, rg, 99, state, table)                          # push_tick = 0
    assert torch.equal(table, before)
    rg.push_tick = 1
    due = nxt.copy()                                              # launches until the env's next draw
    draws = 0
    angles = []
    for launch in range(40):
        prev = table.clone()
        _rand(N, None, rg, 99, state, table)
        due -= 1
        fired = due == 0
        left = ti[:, col["push_steps_left"]].cpu().numpy()
        now_next = ti[:, col["push_next_in"]].cpu().numpy()
        f = table[:, 8:11].cpu().numpy().astype(np.float64)
        # envs that were not due: only the countdown moved
        quiet = torch.tensor(~fired, device=DEV)
        assert torch.equal(table[quiet][:, :12], prev[quiet][:, :12])
        assert np.array_equal(now_next[~fired], due[~fired])
        if fired.any():
            mag = np.linalg.norm(f[fired, 0:2], axis=1)
            assert np.all(f[fired, 2] == 0.0) and mag.min() >= 50.0 * (1 - 1e-6) and mag.max() <= 200.0 * (1 + 1e-6)
            assert left[fired].min() >= 1 and left[fired].max() <= 2
            assert now_next[fired].min() >= 3 and now_next[fired].max() <= 6
            angles.append(np.arctan2(f[fired, 1], f[fired, 0]))
            due[fired] = now_next[fired]
            draws += int(fired.sum())
        ti[:, col["push_steps_left"]] = torch.clamp(ti[:, col["push_steps_left"]] - 1, min=0)      # what the step does per launch
    assert draws > 6 * N
    counts = np.histogram(np.concatenate(angles), bins=8, range=(-np.pi, np.pi))[0]
    assert counts.min() > 0.9 * counts.mean() and counts.max() < 1.1 * counts.mean()


# ---------------------------------------------------------------------------------------------------------------------- env
def _com_velocity(env, e=0):
    sm = env._sim_model
    rb = env._core.rigid_body_state.view(env._num_envs, -1, 13)[e].cpu().numpy().astype(np.float64)
    P = np.zeros(3)
    for b in range(rb.shape[0]):
        R = cm._rotm(rb[b, 3:7])
        P += sm.body_mass[b] * (rb[b, 7:10] + np.cross(rb[b, 10:13], R @ sm.body_com[b]))
    return P / sm.body_mass.sum()


@pytest.mark.parametrize("gz", [None, -3.7])
def test_yaml_gravity_z_reaches_the_kernel(gz):
    """`env.gravity_z` (ig_env.py:139-142; -9.81 when absent) without a `physics_rand` block: the model struct carries it and a
    character lifted off the ground falls with it: after one control step from rest its centre of mass moves at gravity_z dt (to the
    integrator's momentum bound of the invariant tests, 4 %)."""
    from parc_amd import workloads
    N = 64
    env, _, _ = workloads.build_env("flat_1clip", N, DEV, seed=0, env_overrides={} if gz is None else {"gravity_z": gz})
    g = 9.81 if gz is None else -gz
    assert env._sim_model.struct.gravity == np.float32(g) and env.get_physics_params() is None
    env.reset()
    c = env._core
    c.root_state[:, 2] += 3.0
    c.root_state[:, 7:13] = 0.0
    c.dof_state.view(N, -1, 2)[..., 1] = 0.0
    env.step(env._char_dof_pos.clone())
    v = _com_velocity(env)
    assert abs(v[2] + g * env._timestep) < 0.04 * g * env._timestep, (v, g * env._timestep)
    assert np.abs(v[0:2]).max() < 0.04 * g * env._timestep


PHYS_RAND = {"friction_mu": [0.5, 1.5], "contact_kn": [1e4, 1.6e5], "mass_scale": [0.8, 1.25], "kp_scale": [0.8, 1.2], "kd_scale": 1.5,
             "gravity": [9.0, 10.5]}


def test_env_with_physics_rand_redraws_only_at_resets():
    """`physics_rand` in the YAML: the table exists, a scalar fixes its field, pairs are drawn per env at the first reset and redrawn
    exactly for the rows that restart (reset_done under the restart chain's mask, and reset(env_ids)); info["physics_params"] are views
    of the table and change at no other time."""
    from parc_amd import workloads
    N = 256
    torch.manual_seed(0)
    env, _, _ = workloads.build_env("boxes_64clips", N, DEV, seed=0, env_overrides={"physics_rand": PHYS_RAND})
    obs, info = env.reset()
    pr = info["physics_params"]
    assert pr is env.get_physics_params() and pr["contact_kn"].data_ptr() == env._phys_table[:, 2].data_ptr()
    assert (pr["kd_scale"] == 1.5).all() and (pr["contact_cn"] == env._sim_model.struct.contact_cn).all()
    for f in ("friction_mu", "contact_kn", "mass_scale", "kp_scale", "gravity"):
        lo, hi = PHYS_RAND[f]
        assert pr[f].min() >= np.float32(lo) and pr[f].max() <= np.float32(hi) and pr[f].unique().numel() > 0.9 * N, f
    restarts = 0
    gen = torch.Generator(device=DEV).manual_seed(1)
    for step in range(60):
        before = env._phys_table.clone()
        a = env._ref_dof_pos + 0.6 * torch.randn((N, 28), device=DEV, generator=gen)       # noisy enough to fall now and then
        obs, r, done, info = env.step(a)
        assert torch.equal(env._phys_table, before)               # a step changes no parameter (no pushes configured)
        assert torch.isfinite(obs).all() and torch.isfinite(r).all()
        d = (done != 0)
        if step % 2 == 0:
            env.reset_done()
        elif d.any():
            env.reset(torch.nonzero(d).flatten())
        after = env._phys_table
        assert torch.equal(after[~d], before[~d])
        if d.any():
            assert (after[d][:, 2] != before[d][:, 2]).float().mean() > 0.95
            restarts += int(d.sum())
        assert info["physics_params"]["contact_kn"].data_ptr() == env._phys_table[:, 2].data_ptr()
    assert restarts > 10


def test_setters_switch_the_env_to_the_table_and_sweep_a_parameter():
    """No `physics_rand`: the env steps without a table until a setter is called; set_physics_params(env_ids, contact_kn=grid) then makes
    a deterministic sweep a three-line script, values are checked on the host, apply_push shoves the chosen envs for num_steps steps."""
    from parc_amd import workloads
    N = 64
    env, _, _ = workloads.build_env("flat_1clip", N, DEV, seed=0)
    env.reset()
    assert env.get_physics_params() is None and "physics_params" not in env._info
    sig0 = env.host_step_signature()
    ids = torch.arange(N, device=DEV)
    grid = torch.logspace(4, np.log10(1.6e5), N)
    env.set_physics_params(ids, contact_kn=grid)
    pr = env.get_physics_params()
    assert torch.equal(pr["contact_kn"].cpu(), grid) and (pr["mass_scale"] == 1.0).all() and env.host_step_signature() != sig0
    with pytest.raises(AssertionError):
        env.set_physics_params(ids[:2], mass_scale=0.0)
    with pytest.raises(AssertionError):
        env.set_physics_params(None, friction_mu=-1.0)
    with pytest.raises(AssertionError):
        env.set_physics_params(None, restitution=0.5)
    env.set_physics_params(None, friction_mu=0.7)
    assert (pr["friction_mu"] == np.float32(0.7)).all()
    # standing characters sink m g / kn into the spring: softer ground, lower root
    for _ in range(20):
        obs, r, done, info = env.step(env._ref_dof_pos.clone())
    assert "physics_params" in info and torch.isfinite(obs).all()
    # push: env 3 is shoved along +x for 2 control steps, env 4 is not
    env.reset()
    v0 = env._char_root_vel.clone()
    env.apply_push(torch.tensor([3], device=DEV), [1500.0, 0.0, 0.0], 2)
    left = []
    for _ in range(3):
        env.step(env._ref_dof_pos.clone())
        left.append(int(pr["push_steps_left"][3].item()))
    assert left == [1, 0, 0] and (pr["push_steps_left"][4] == 0).all()
    # 1500 N for 2 steps of 1/30 s on a ~50 kg character: its centre of mass gains 2 m/s; the pelvis gains at least half of that over
    # anything the unpushed neighbours (same clip, other phases) did in the same three steps
    dv = (env._char_root_vel - v0)[:, 0]
    others = torch.cat([dv[:3], dv[4:]])
    assert dv[3] > others.max() + 1.0, (dv[3], others.max())


def _replay_kernel_names(agent):
    """kernel names of one replay of the agent's captured rollout step"""
    from torch.profiler import ProfilerActivity, profile
    (g, _), = list(agent._graphs.values())[:1]
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        g.replay()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name]
    ev.sort(key=lambda e: e.time_range.start)
    return [e.name for e in ev]


def _trained_agent(env_overrides):
    from parc_amd import workloads
    from parc_amd.learning.dm_ppo_agent import AgentMode
    torch.manual_seed(0)
    env, _, _ = workloads.build_env("flat_1clip", 64, DEV, seed=0, env_overrides=env_overrides)
    agent = workloads.build_agent(env, DEV, steps_per_iter=8, update_epochs=1, batch_size=2)
    assert agent._device_tick()
    agent._curr_obs, agent._curr_info = env.reset()
    agent._init_train()
    return env, agent, AgentMode


def test_graph_rollout_with_physics_rand_writes_the_same_rows_as_the_eager_rollout():
    """(the pattern of test_learner_gpu.test_graph_rollout_writes_the_same_rows_as_the_eager_rollout, with a `physics_rand` block and
    pushes) the captured training step and the eager one fill the experience rows consistently; the captured step launches the table's
    kernel and the sampler; the parameters of a row change only where the row restarted; the sampler's generator moved on once per
    launch (its cells were not allocated inside the capture)."""
    rand = dict(PHYS_RAND, push={"interval_s": [0.2, 0.4], "force": [50.0, 150.0], "duration_s": [0.1, 0.2]})
    env, agent, AgentMode = _trained_agent({"physics_rand": rand})
    for it in range(3):
        if it < 2:
            info = agent._train_iter()
            assert np.isfinite(info["critic_loss"].item())
        else:
            agent._exp_buffer.reset()
            agent.eval()
            agent.set_mode(AgentMode.TRAIN)
            kn0 = env._phys_table[:, 2].clone()
            ep0 = env._ep_num_buf.clone()
            agent._rollout_train(agent._steps_per_iter)
            assert agent._graphs
            same = env._ep_num_buf == ep0
            assert torch.equal(env._phys_table[:, 2][same], kn0[same])
            assert (env._phys_table[:, 2][~same] != kn0[~same]).all()
        eb = agent._exp_buffer
        ts = eb.get_data("timestep").cpu().numpy()
        ep = eb.get_data("ep_num").cpu().numpy()
        assert (eb.get_data("env_id").cpu().numpy() == np.arange(64)[None, :]).all()
        d_ts, d_ep = np.diff(ts, axis=0), np.diff(ep, axis=0)
        done = eb.get_data("done").cpu().numpy()[:-1] != 0
        assert np.all(np.where(done, ts[1:] == 1, d_ts == 1)) and np.all(np.where(done, d_ep == 1, d_ep == 0))
        obs, nxt = eb.get_data("obs"), eb.get_data("next_obs")
        keep = ~torch.tensor(done, device=DEV)
        assert torch.equal(obs[1:][keep], nxt[:-1][keep])
        assert torch.isfinite(eb.get_data("action")).all() and torch.isfinite(obs).all()
    # 24 rollout steps, each with one push tick and one reset redraw, plus the first reset's draw
    assert int(env._phys_rng_state[0].item()) == 1 + 2 * 24 and int(env._phys_rng_state[1].item()) == 0
    assert (env.get_physics_params()["push_force"].abs().sum(dim=1) > 0).any()
    names = _replay_kernel_names(agent)
    assert sum("sim_step_bpl_phys_kernel" in n for n in names) == 1 and sum("phys_rand_kernel" in n for n in names) == 2, names
    assert not any("sim_step_bpl_kernel" in n or "sim_step_bpl_ctl_kernel" in n for n in names), names
    assert len(names) == 20, names


def test_graph_rollout_without_physics_rand_launches_what_it_always_did():
    """No `physics_rand`, no setter: the captured rollout step is the 18 kernel nodes of DESIGN section 3, in that order - the pd
    simulator kernel among them, nothing of the table's."""
    env, agent, AgentMode = _trained_agent({})
    for it in range(3):
        agent._train_iter()
    assert agent._graphs and env.get_physics_params() is None
    names = _replay_kernel_names(agent)
    assert len(names) == 18, names
    assert not any("phys" in n for n in names), names
    order = ["rng_step", "obs_ingest", "moments_final", None, None, None, None, "action_head", "sim_step_bpl_kernel", "track_post", "step_tail",
             "return_tracker", "return_tracker", "record", "reset_sample_apply", None, "sim_refresh", "track_post"]
    for n, want in zip(names, order):
        assert want is None or want in n, (n, want, names)
