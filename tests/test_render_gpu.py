"""parc_render on the device: the scenes of tests/test_render.py through the C ABI, against the float64 reference (ids exact, depth within
4 x the measured fp32-vs-float64 error: the device contracts to fma and has other division and sqrt sequences) and against the host build
of the same header (ids exact), on the safe pixels; edge workgroups with guard words; two envs in one launch; and an IGParkourEnv in TEST
mode with a renderer and a writer attached."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_ref as rr
from render_ref import rh
from test_render import check_against_reference, reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEPTH_TOL_GPU = 4.0 * rr.MEASURED_DEPTH_ERR

SCENES = [("sphere", rr.scene_sphere), ("flat", rr.scene_flat), ("raised", rr.scene_raised), ("capsule_box", rr.scene_capsule_box),
          ("occlusion", rr.scene_occlusion), ("shadows", rr.scene_shadows), ("contacts", rr.scene_contacts),
          ("track", lambda: rr.scene_track((0.25, 0.5))), ("humanoid", rr.scene_humanoid)]


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return rh.build_host(str(tmp_path_factory.mktemp("render_host")))


@pytest.mark.parametrize("name,make", SCENES, ids=[n for n, _ in SCENES])
def test_scene_against_reference_and_host_build(name, make, hostlib):
    s = make()
    out, host = s.render_device(guard=64), s.render_host(hostlib)
    assert out["rc"] == 0
    for g in out["guard"]:
        assert (g == out["pattern"]).all()
    for k in range(len(s.views)):
        ref = reference(name, make, k)
        check_against_reference(out, ref, k, DEPTH_TOL_GPU, name + " (device)")
        safe = ~ref["unsafe"]
        assert np.array_equal(out["ids"][k][safe], host["ids"][k][safe])
        # colours: the same shading from (nearly) the same normals - a rounding step of one level at the most, away from shadow edges
        calm = safe & ~ref["shadow_unsafe"]
        assert np.abs(out["rgba"][k][calm].astype(int) - host["rgba"][k][calm].astype(int)).max() <= 1


def test_shadows_and_contacts_on_the_device():
    s = rr.scene_shadows()
    on, off = s.render_device(), s.with_scene(shadows=False).render_device()
    ref = reference("shadows", rr.scene_shadows)
    differ = (on["rgba"][0] != off["rgba"][0]).any(axis=-1)
    terrain = (ref["ids"] >= 2 * s.B) & ~ref["shadow_unsafe"]
    assert np.array_equal(differ[terrain], ref["lit_occluded"][terrain])
    c = rr.scene_contacts()
    plain, tinted = c.render_device(), c.with_scene(show_contacts=True, contact_eps=0.1).render_device()
    changed = (plain["rgba"][0] != tinted["rgba"][0]).any(axis=-1)
    assert np.array_equal(changed, plain["ids"][0] == 1) and changed.sum() > 10


def test_track_equals_still_on_the_device():
    from parc_amd import render
    s = rr.scene_track((0.5, 0.375))
    track = s.render_device()
    still = s.with_views([render.make_view(1, "still", (0.5 - 0.5, 0.375 + 0.25 - 5.0, 3.0), (0.5 - 0.5, 0.375 + 0.25, 1.0))]).render_device()
    for key in ("rgba", "ids", "depth"):
        assert np.array_equal(track[key], still[key]), key


def test_edge_workgroups_and_guard_words(hostlib):
    """37 x 21 pixels: 3 x 2 workgroups per view whose last column and row are partly outside the image; the words behind every plane stay
    as they were; two views of different envs in one launch"""
    base = rr.scene_humanoid()
    s = base.with_views(base.views, width=37, height=21)
    out, host = s.render_device(guard=257), s.render_host(hostlib)
    assert out["rc"] == 0
    for g in out["guard"]:
        assert g.size == 257 and (g == out["pattern"]).all()
    assert (out["rgba"][..., 3] == 255).all()          # every pixel of the image was written
    assert s.views[0].env == 0 and s.views[1].env == 1
    for k in range(2):
        ref = rr.Reference(s).view(k)
        check_against_reference(out, ref, k, DEPTH_TOL_GPU, "humanoid 37x21 (device)")
        assert np.array_equal(out["ids"][k][~ref["unsafe"]], host["ids"][k][~ref["unsafe"]])
    # the two views show different envs: each equals the launch that draws it alone
    for k in range(2):
        alone = s.with_views([s.views[k]]).render_device()
        for key in ("rgba", "ids", "depth"):
            assert np.array_equal(alone[key][0], out[key][k]), (k, key)


def test_malformed_views_on_the_device():
    s = rr.scene_malformed()
    out = s.render_device(guard=64)
    assert out["rc"] == 0
    for g in out["guard"]:
        assert (g == out["pattern"]).all()
    assert (out["rgba"][..., 3] == 255).all()
    assert not np.isnan(out["depth"]).any() and (out["depth"] > 0).all()
    assert ((out["ids"] >= -1) & (out["ids"] < 2 * s.B + s.hf.size)).all()


def test_argument_errors_return_without_a_launch():
    from parc_amd import _hip
    s = rr.scene_humanoid()
    L = _hip.lib()
    V, H, W = 2, s.height, s.width
    t = {k: torch.tensor(getattr(s, k), device=DEV) for k in ("root_state", "rigid_body_state", "ref_pos", "ref_rot", "contact_forces", "env_offsets", "hf")}
    prims, views = torch.tensor(s._prim_buf, device=DEV), torch.tensor(s._view_buf, device=DEV)
    rgba = torch.full((V, H, W), 0x01020304, dtype=torch.int32, device=DEV)
    p = _hip.ptr

    def call(**kw):
        sc = s.scene_struct(prims.data_ptr())
        sc.n_prims = kw.get("n_prims", sc.n_prims)
        ter = s.terrain_struct(t["hf"].data_ptr())
        ter.dx, ter.dim_y = kw.get("dx", ter.dx), kw.get("dim_y", ter.dim_y)
        a = dict(views=views, rgba=rgba, rigid_body_state=t["rigid_body_state"], ref_pos=t["ref_pos"], ref_rot=t["ref_rot"])
        a.update({k: v for k, v in kw.items() if k in a})
        return L.parc_render(_hip.stream(), ter, ctypes.byref(sc), kw.get("n_views", V), p(a["views"]), kw.get("width", W), kw.get("height", H),
                             p(t["root_state"]), p(a["rigid_body_state"]), p(a["ref_pos"]), p(a["ref_rot"]), p(t["contact_forces"]),
                             p(t["env_offsets"]), kw.get("n_envs", s.N), p(a["rgba"]), None, None)
    for kw in (dict(width=0), dict(height=-1), dict(n_views=-1), dict(n_envs=0), dict(views=None), dict(rgba=None), dict(rigid_body_state=None),
               dict(ref_pos=None), dict(ref_rot=None), dict(n_prims=33), dict(dx=0.0), dict(dim_y=0), dict(n_views=65536), dict(n_views=0)):
        assert call(**kw) == (0 if kw == dict(n_views=0) else -1), kw
    torch.cuda.synchronize()
    assert (rgba == 0x01020304).all()          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (rgba != 0x01020304).all()


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name]
    ev.sort(key=lambda e: e.time_range.start)
    return [e.name for e in ev]


def test_env_with_renderer_and_writer(tmp_path):
    """A 4-env IGParkourEnv on the synthetic workload in TEST mode: 3 steps with a renderer and a writer attached write the frames, the
    ids plane shows both characters and terrain, and observations, rewards and done flags are bit-equal to the same 3 steps without a
    renderer; an eager step without a renderer launches what it launched before (no render kernel, no extra launch)."""
    from PIL import Image
    from parc_amd import render, workloads
    from parc_amd.envs import base_env

    def rollout(with_renderer):
        torch.manual_seed(0)
        env, _, _ = workloads.build_env("boxes_64clips", 4, DEV, seed=0)
        env.set_mode(base_env.EnvMode.TEST)
        r = w = None
        if with_renderer:
            with pytest.raises(RuntimeError, match="TEST mode"):
                env.set_mode(base_env.EnvMode.TRAIN) or env.set_renderer(object())
            env.set_mode(base_env.EnvMode.TEST)
            r = render.Renderer(env, 48, 32, [0, 2], with_depth=True, with_ids=True)
            w = render.FrameWriter(str(tmp_path / "frames"), env_ids=[0, 2], chunk=3)
            env.set_renderer(r, w)
        torch.manual_seed(1)
        env.reset()
        res = []
        for _ in range(3):
            obs, rew, done, _ = env.step(env._ref_dof_pos.clone())
            res.append((obs.clone(), rew.clone(), done.clone()))
        return env, r, w, res
    env, r, w, with_r = rollout(True)
    _, _, _, without = rollout(False)
    for a, b in zip(with_r, without):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    ids = r.ids.cpu().numpy()
    B = env._cfg.num_bodies
    for v in range(2):
        assert ((ids[v] >= 0) & (ids[v] < B)).any() and ((ids[v] >= B) & (ids[v] < 2 * B)).any() and (ids[v] >= 2 * B).any()
    assert torch.isfinite(r.depth[r.ids >= 0]).all() and r.rgba.shape == (2, 32, 48, 4)
    last = r.rgba.cpu().numpy()
    w.close()
    for e in (0, 2):          # the reset's frame and the three steps'
        names = sorted(os.listdir(tmp_path / "frames" / "env{:04d}".format(e)))
        assert names == ["frame{:06d}.png".format(k) for k in range(4)]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "frames" / "env0002" / "frame000003.png")), last[1])
    # the launches of an eager step: with the renderer two more (forward kinematics of the reference pose + render_kernel); detached, and
    # on an env that never had one, the same list
    act = env._ref_dof_pos.clone()
    names_with = _kernel_names(lambda: env.step(act))
    env.set_renderer(None)
    names_detached = _kernel_names(lambda: env.step(act))
    env2, _, _, _ = rollout(False)
    names_never = _kernel_names(lambda: env2.step(act))
    assert sum("render_kernel" in n for n in names_with) == 1 and len(names_with) == len(names_never) + 2, (names_with, names_never)
    assert names_detached == names_never and not any("render" in n for n in names_never)


def test_one_frame_per_step_through_the_agent(tmp_path):
    """agent.test_model resets the finished envs after every step (mostly an empty list): the writer still gets one frame for the
    rollout's full reset and one per step.  A still camera is placed anew at that full reset: 5 m behind the character in y, 3 m up,
    looking at (root xy, 0) as the reference's _init_camera does."""
    from parc_amd import _hip_render, render, workloads
    from parc_amd.envs import base_env
    torch.manual_seed(0)
    env, _, _ = workloads.build_env("boxes_64clips", 4, DEV, seed=0)
    agent = workloads.build_agent(env, DEV, steps_per_iter=4, update_epochs=1, batch_size=2)
    env.set_mode(base_env.EnvMode.TEST)
    r = render.Renderer(env, 48, 32, [1], camera_mode="still")
    w = render.FrameWriter(str(tmp_path / "frames"), env_ids=[1], chunk=16)
    env.set_renderer(r, w)
    r.render()
    views_before = r._views
    steps, resets = [0], []
    step, reset = env.step, env.reset

    def counted_step(action):
        steps[0] += 1
        return step(action)

    def counted_reset(env_ids=None):
        resets.append(None if env_ids is None else len(env_ids))
        return reset(env_ids)
    env.step, env.reset = counted_step, counted_reset
    agent.test_model(num_episodes=4)
    w.close()
    assert steps[0] >= 2 and resets[0] is None and len(resets) == 1 + steps[0]
    names = sorted(os.listdir(tmp_path / "frames" / "env0001"))
    assert names == ["frame{:06d}.png".format(k) for k in range(1 + steps[0])]
    assert r._views is not None and r._views is not views_before
    v = _hip_render.ViewS.from_buffer_copy(r._views.cpu().numpy().tobytes())
    assert v.env == 1 and v.mode == 0 and v.target[2] == 0.0 and v.vec[2] == 3.0
    assert v.vec[0] == v.target[0] and abs((v.vec[1] - v.target[1]) + 5.0) < 1e-5
