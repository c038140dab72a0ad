"""The offscreen ray caster (include/parc_render.h) on the CPU: the host build of parc_render_core.h (tests/tools/render_host.cpp)
against the float64 brute-force ray caster of tests/render_ref.py, on 32 x 24 pixels over an 8 x 8 terrain.

ids are compared exactly and depth within 2 x the measured fp32-vs-float64 error (render_ref.MEASURED_DEPTH_ERR) on the "safe" pixels;
at most 2 % of a view's pixels may be unsafe (asserted: a test cannot pass by leaving its failures out).  tests/test_render_gpu.py runs
the same scenes through parc_render on the device."""
import os
import subprocess

import numpy as np
import pytest

import render_ref as rr
from render_ref import rh

DEPTH_TOL = 2.0 * rr.MEASURED_DEPTH_ERR


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return rh.build_host(str(tmp_path_factory.mktemp("render_host")))


_refs = {}


def reference(name, make, k=0):
    """the float64 planes of view k of a scene, computed once per session"""
    if (name, k) not in _refs:
        _refs[(name, k)] = rr.Reference(make()).view(k)
    return _refs[(name, k)]


def check_against_reference(out, ref, k, tol, what):
    """ids exact and depth within tol on the safe pixels of view k; the unsafe ones are at most MAX_UNSAFE of the view"""
    unsafe = ref["unsafe"]
    assert unsafe.mean() <= rr.MAX_UNSAFE, (what, unsafe.mean())
    safe = ~unsafe
    bad = safe & (out["ids"][k] != ref["ids"])
    assert not bad.any(), (what, np.argwhere(bad)[:5], out["ids"][k][bad][:5], ref["ids"][bad][:5])
    hit = safe & np.isfinite(ref["t"])
    assert np.isinf(out["depth"][k][safe & ~hit]).all() and (out["depth"][k][safe & ~hit] > 0).all(), what
    err = np.abs(out["depth"][k][hit].astype(np.float64) - ref["t"][hit]).max() if hit.any() else 0.0
    print("{} view {}: unsafe {:.2%}, max depth error {:.3e} (bound {:.3e})".format(what, k, unsafe.mean(), err, tol))
    assert err <= tol, (what, err, tol)


def test_sphere_on_the_optical_axis(hostlib):
    d, r = 4.0, 0.5
    s = rr.scene_sphere(d, r)
    out = s.render_host(hostlib)
    assert out["rc"] == 0
    ref = reference("sphere", rr.scene_sphere)
    check_against_reference(out, ref, 0, DEPTH_TOL, "sphere")
    # the centre pixel looks along the axis: it sees the sphere at d - r
    H, W = s.height, s.width
    ang = ref["angle"]
    assert ang[H // 2, W // 2] < 1e-7 and out["ids"][0][H // 2, W // 2] == 0
    assert abs(out["depth"][0][H // 2, W // 2] - (d - r)) <= DEPTH_TOL
    # the silhouette: inside asin(r / d) minus one pixel every ray hits, outside it plus one pixel every ray misses
    pix = 2.0 * np.tan(0.5 * s.views[0].fov_y) / H          # angle of one pixel at the image centre (the largest)
    lim = np.arcsin(r / d)
    ids = out["ids"][0]
    assert (ids[ang < lim - pix] == 0).all() and (ang < lim - pix).sum() > 10
    assert (ids[ang > lim + pix] != 0).all() and (ang > lim + pix).sum() > 100


def test_flat_terrain_from_above(hostlib):
    h, z = 0.25, 5.0
    s = rr.scene_flat(h, z)
    out = s.render_host(hostlib)
    ref = reference("flat", rr.scene_flat)
    check_against_reference(out, ref, 0, DEPTH_TOL, "flat")
    hit = np.isfinite(ref["t"]) & ~ref["unsafe"]
    assert hit.mean() > 0.8
    # depth = (z - h) / cos(theta)
    assert np.abs(out["depth"][0][hit] - (z - h) / np.cos(ref["angle"][hit])).max() <= DEPTH_TOL
    # the id is the cell that hf_lookup's rint((p - min) / dx) gives for the float64 hit point
    assert (out["ids"][0][hit] == ref["owner"][hit]).all() and (ref["owner"][hit] >= 2).all()
    assert len(np.unique(out["ids"][0][hit])) > 30          # (most of the 64 cells are in view)


def test_raised_cell_from_the_side(hostlib):
    s = rr.scene_raised()
    out = s.render_host(hostlib)
    B, ny = 1, 8
    cell = 2 * B + 4 * ny + 3
    for k in range(2):          # view 0 starts outside the grid's bounding box, view 1 inside it
        ref = reference("raised", rr.scene_raised, k)
        check_against_reference(out, ref, k, DEPTH_TOL, "raised")
        safe = ~ref["unsafe"]
        on = safe & (out["ids"][k] == cell)
        wall = on & (np.abs(ref["normal"][..., 1]) > 0.5)
        assert wall.sum() > 8, wall.sum()
        # the wall facing the camera (-y) is what is seen of the cell: its normal is the wall's axis, in both builds
        assert np.array_equal(out["normals"][k][wall], np.broadcast_to(np.float32([0, -1, 0]), out["normals"][k][wall].shape))
        assert np.allclose(ref["normal"][wall], [0, -1, 0])
        # the wall is hit before the top behind it: where the wall is seen, depth is the distance to the plane y = wall
        y_wall = s.min_point[1] + (3 - 0.5) * s.dxdy[1]
        e, o, d = rr.Reference(s).rays(s.views[k])
        t_plane = ((y_wall - o[:, 1]) / d[:, 1]).reshape(s.height, s.width)
        assert np.abs(out["depth"][k][wall] - t_plane[wall]).max() <= DEPTH_TOL
        assert np.array_equal(out["normals"][k][safe & (out["ids"][k] >= 2)], ref["normal"][safe & (out["ids"][k] >= 2)].astype(np.float32))
    eye_in = np.array(s.views[1].vec[:])
    assert -1.6 < eye_in[0] < 1.6 and -1.6 < eye_in[1] < 1.6 and not (-1.6 < s.views[0].vec[1] < 1.6)


def test_capsule_and_oriented_box(hostlib):
    s = rr.scene_capsule_box()
    out = s.render_host(hostlib)
    for k in range(2):
        ref = reference("capsule_box", rr.scene_capsule_box, k)
        check_against_reference(out, ref, k, DEPTH_TOL, "capsule_box")
        assert ((out["ids"][k] == 1) & ~ref["unsafe"]).sum() > 20          # the box is in both views
    assert (out["ids"][0] == 0).sum() > 10                                  # the capsule in the first
    # view 1 starts inside the box's bounding sphere (and outside the box)
    box = s.prims[1]
    R = rr.qmat(s.body_rot[0, 1])
    centre = s.body_pos[0, 1] + R @ np.array(box.a[:])
    eye = np.array(s.views[1].vec[:])
    assert np.linalg.norm(eye - centre) < np.linalg.norm(box.b[:])
    local = (R @ rr.qmat(box.q[:])).T @ (eye - centre)
    assert (np.abs(local) > np.array(box.b[:])).any()


def test_occlusion_and_ref_char_offset(hostlib):
    out = rr.scene_occlusion().render_host(hostlib)
    ref = reference("occlusion", rr.scene_occlusion)
    check_against_reference(out, ref, 0, DEPTH_TOL, "occlusion")
    ids, B = out["ids"][0], 2
    assert ((ids >= 0) & (ids < B)).sum() > 20 and ((ids >= B) & (ids < 2 * B)).sum() > 10
    # without the simulated character in front, more of the reference character is seen: it IS partly hidden
    alone = rr.scene_occlusion()
    alone.rigid_body_state[..., 0:3] += rr.FAR
    alone.body_pos = alone.body_pos + rr.FAR
    alone.root_state = np.ascontiguousarray(alone.rigid_body_state[:, 0, :])
    ids_alone = alone.render_host(hostlib)["ids"][0]
    assert ((ids_alone >= B) & (ids_alone < 2 * B)).sum() > ((ids >= B) & (ids < 2 * B)).sum()
    # ref_char_offset moves the reference character by that offset
    off = (-0.9, 0.2, 0.3)

    def moved():
        return rr.scene_occlusion(ref_char_offset=off)
    out2 = moved().render_host(hostlib)
    ref2 = reference("occlusion_offset", moved)
    check_against_reference(out2, ref2, 0, DEPTH_TOL, "occlusion with ref_char_offset")
    shifted = rr.scene_occlusion()
    shifted.ref_pos = shifted.ref_pos + np.float32(off)
    assert np.array_equal(shifted.render_host(hostlib)["ids"], out2["ids"])
    assert not np.array_equal(out2["ids"], out["ids"])


def test_shadows(hostlib):
    s = rr.scene_shadows()
    on, off = s.render_host(hostlib), s.with_scene(shadows=False).render_host(hostlib)
    ref = reference("shadows", rr.scene_shadows)
    check_against_reference(on, ref, 0, DEPTH_TOL, "shadows")
    assert np.array_equal(on["ids"], off["ids"]) and np.array_equal(on["depth"], off["depth"])
    differ = (on["rgba"][0] != off["rgba"][0]).any(axis=-1)
    assert ref["shadow_unsafe"].mean() <= rr.MAX_UNSAFE, ref["shadow_unsafe"].mean()
    terrain = (ref["ids"] >= 2 * s.B) & ~ref["shadow_unsafe"]
    assert np.array_equal(differ[terrain], ref["lit_occluded"][terrain])
    assert ref["lit_occluded"][terrain].sum() > 15 and (~ref["lit_occluded"][terrain]).sum() > 100
    assert (on["rgba"][0][differ] <= off["rgba"][0][differ]).all()         # a shadow only darkens


def test_show_contacts(hostlib):
    s = rr.scene_contacts()
    plain, tinted = s.render_host(hostlib), s.with_scene(show_contacts=True, contact_eps=0.1).render_host(hostlib)
    check_against_reference(plain, reference("contacts", rr.scene_contacts), 0, DEPTH_TOL, "contacts")
    assert np.array_equal(plain["ids"], tinted["ids"])
    changed = (plain["rgba"][0] != tinted["rgba"][0]).any(axis=-1)
    # body 1 carries 5 N, body 0 0.05 N (under contact_eps), body 2 nothing
    assert np.array_equal(changed, plain["ids"][0] == 1) and changed.sum() > 10
    # a higher threshold: nothing is tinted
    assert np.array_equal(s.with_scene(show_contacts=True, contact_eps=6.0).render_host(hostlib)["rgba"], plain["rgba"])


def test_track_mode_is_the_reference_camera_update(hostlib):
    """_init_camera / _update_camera (envs/ig_char_env.py:512-541) on the host, in float64: the camera starts 5 m behind the character in y and
    3 m up, keeps its xy distance to the character and its height, and looks at (root xy, 1.0); env offsets are added.  The track view
    equals the still view from that camera, for two consecutive root positions.  (The positions are binary fractions, so the fp32
    sums of the kernel are exact and the images must be equal bit for bit.)"""
    from parc_amd import render
    roots = [(0.25, 0.5), (0.5, 0.375)]
    off = np.array([-0.5, 0.25, 0.0])
    char0 = np.array([roots[0][0], roots[0][1], 0.9]) + off
    cam_pos, prev = char0 + np.array([0.0, -5.0, 0.0]), char0.copy()          # _init_camera: (x, y - 5, 3)
    cam_pos[2] = 3.0
    for root in roots:
        root_pos = np.array([root[0], root[1], 0.9]) + off
        delta = cam_pos - prev
        cam_pos = np.array([root_pos[0] + delta[0], root_pos[1] + delta[1], cam_pos[2]])
        target = np.array([root_pos[0], root_pos[1], 1.0])
        prev = root_pos.copy()
        assert np.allclose(cam_pos[:2] - root_pos[:2], [0.0, -5.0]) and cam_pos[2] == 3.0          # delta and height are kept
        s = rr.scene_track(root)
        track = s.render_host(hostlib)
        still = s.with_views([render.make_view(1, "still", cam_pos, target)]).render_host(hostlib)
        for key in ("rgba", "ids", "depth"):
            assert np.array_equal(track[key], still[key]), key
        assert (track["ids"][0] == 0).sum() > 5 and (track["ids"][0] >= 2).sum() > 50
    check_against_reference(rr.scene_track((0.25, 0.5)).render_host(hostlib), reference("track", lambda: rr.scene_track((0.25, 0.5))), 0, DEPTH_TOL, "track")


def test_whole_humanoid_on_stepped_terrain(hostlib):
    s = rr.scene_humanoid()
    assert len(s.prims) >= 15 and s.B == 15
    out = s.render_host(hostlib)
    for k in range(2):
        check_against_reference(out, reference("humanoid", rr.scene_humanoid, k), k, DEPTH_TOL, "humanoid")
        ids = out["ids"][k]
        assert ((ids >= 0) & (ids < s.B)).sum() > 15 and ((ids >= s.B) & (ids < 2 * s.B)).sum() > 15 and (ids >= 2 * s.B).sum() > 100
        assert len(np.unique(ids[(ids >= 0) & (ids < s.B)])) >= 8          # most bodies are seen


def _einval_cases(s, call):
    """every PARC_EINVAL rule of include/parc_render.h; call(scene, **overrides) -> rc"""
    assert call(s) == 0
    for kw in (dict(width=0), dict(height=-1), dict(n_views=-1), dict(n_views=65536), dict(n_envs=0), dict(n_envs=-2), dict(views=None), dict(rgba=None),
               dict(rigid_body_state=None), dict(ref_pos=None), dict(ref_rot=None), dict(n_prims=33), dict(dx=0.0), dict(dy=-0.4), dict(dim_x=0),
               dict(dim_y=-8)):
        assert call(s, **kw) == -1, kw


def _call_host(hostlib):
    import ctypes
    L = rh.host_lib(hostlib)

    def call(s, **kw):
        V, H, W = len(s.views), s.height, s.width
        rgba = np.full((V, H, W), 0x01020304, np.uint32)
        sc = s.scene_struct(s._prim_buf.ctypes.data)
        sc.n_prims = kw.get("n_prims", sc.n_prims)
        ter = s.terrain_struct(s.hf.ctypes.data)
        ter.dx, ter.dy = kw.get("dx", ter.dx), kw.get("dy", ter.dy)
        ter.dim_x, ter.dim_y = kw.get("dim_x", ter.dim_x), kw.get("dim_y", ter.dim_y)
        arr = dict(views=s._view_buf, rgba=rgba, rigid_body_state=s.rigid_body_state, ref_pos=s.ref_pos, ref_rot=s.ref_rot)
        arr.update({k: v for k, v in kw.items() if k in arr})
        rc = L.render_host(ter, ctypes.byref(sc), kw.get("n_views", V), rh._p(arr["views"]), kw.get("width", W), kw.get("height", H),
                           rh._p(s.root_state), rh._p(arr["rigid_body_state"]), rh._p(arr["ref_pos"]), rh._p(arr["ref_rot"]), rh._p(s.contact_forces),
                           rh._p(s.env_offsets), kw.get("n_envs", s.N), rh._p(arr["rgba"]), None, None, None)
        if rc != 0 or kw.get("n_views", V) == 0:
            assert arr["rgba"] is None or (rgba == 0x01020304).all()          # nothing was written
        return rc
    return call


def test_argument_errors(hostlib):
    s = rr.scene_humanoid()
    call = _call_host(hostlib)
    _einval_cases(s, call)
    assert call(s, n_views=0) == 0
    # the library itself answers the same before any launch (no GPU is needed to be refused)
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    L = _hip.lib()
    assert L.parc_render_abi() == 1
    dummy = ctypes.c_void_p(0x1000)          # never dereferenced: every call below is refused, or has no view to draw

    def call_lib(s, **kw):
        sc = s.scene_struct(0x1000)
        sc.n_prims = kw.get("n_prims", sc.n_prims)
        ter = s.terrain_struct(0x1000)
        ter.dx, ter.dy = kw.get("dx", ter.dx), kw.get("dy", ter.dy)
        ter.dim_x, ter.dim_y = kw.get("dim_x", ter.dim_x), kw.get("dim_y", ter.dim_y)
        ptr = {k: (None if k in kw and kw[k] is None else dummy) for k in ("views", "rgba", "rigid_body_state", "ref_pos", "ref_rot")}
        assert kw, "only refused calls go to the library here"
        return L.parc_render(None, ter, ctypes.byref(sc), kw.get("n_views", 2), ptr["views"], kw.get("width", 32), kw.get("height", 24), dummy,
                             ptr["rigid_body_state"], ptr["ref_pos"], ptr["ref_rot"], dummy, dummy, kw.get("n_envs", 2), ptr["rgba"], None, None)
    _einval_cases(s, lambda sc, **kw: call_lib(sc, **kw) if kw else 0)
    assert call_lib(s, n_views=0) == 0


def test_malformed_views_give_a_finite_image(hostlib):
    s = rr.scene_malformed()
    out = s.render_host(hostlib)
    assert out["rc"] == 0
    assert (out["rgba"][..., 3] == 255).all()                 # every pixel was written
    assert not np.isnan(out["depth"]).any() and (out["depth"] > 0).all()
    n_cells = s.hf.size
    assert ((out["ids"] >= -1) & (out["ids"] < 2 * s.B + n_cells)).all()
    assert (out["ids"][0] == -1).mean() > 0.5                  # far outside the grid: mostly sky


def test_scene_comes_from_the_mjcf_geoms():
    """the scene is built from the geoms sim_model.py reads - one primitive per geom, capsules and boxes as such - not from the simulator's
    sample spheres"""
    from parc_amd import _hip_render
    from parc_amd.anim.kin_char_model import GeomType
    from parc_amd.sim_model import SimModel
    km, prims = rh.humanoid()
    geoms = [(b, g) for b in range(km.get_num_joints()) for g in km.get_geoms(b)]
    assert len(prims) == len(geoms) <= _hip_render.MAX_PRIMS and len(prims) < SimModel(km).struct.num_spheres
    kinds = {GeomType.SPHERE: 0, GeomType.CAPSULE: 1, GeomType.BOX: 2}
    for p, (b, g) in zip(prims, geoms):
        assert p.body == b and p.type == kinds[g._shape_type]
        assert np.allclose(p.a[:], g._offset)
        if g._shape_type == GeomType.CAPSULE:
            assert np.allclose(np.array(p.b[:]) - np.array(p.a[:]), g._dims, atol=1e-6) and np.isclose(p.radius, g._radius)
    assert {p.type for p in prims} >= {0, 1, 2} or {p.type for p in prims} >= {0, 1}


def test_sanitized_program_renders_the_scenes(tmp_path, hostlib):
    """parc_render_core.h under AddressSanitizer and UBSan in a stand-alone program (its own main): scenes 3, 4, 9 and the malformed views
    of test 10; its images equal the plain build's."""
    exe = rh.build_program(str(tmp_path), sanitize=True)
    for name, make in (("raised", rr.scene_raised), ("capsule_box", rr.scene_capsule_box), ("humanoid", rr.scene_humanoid), ("malformed", rr.scene_malformed)):
        s = make()
        f, o = str(tmp_path / (name + ".scene")), str(tmp_path / (name + ".out"))
        s.dump(f)
        res = subprocess.run([exe, f, o], capture_output=True, text=True)
        assert res.returncode == 0 and "render ok" in res.stdout, (name, res.returncode, res.stderr[-2000:])
        got, want = s.read_program_output(o), s.render_host(hostlib)
        for key in ("rgba", "ids"):
            assert np.array_equal(got[key], want[key]), (name, key)
        assert np.array_equal(got["depth"], want["depth"], equal_nan=True), name


# ------------------------------------------------------------------------------------------------------ host layer
def test_frame_writer_files_reread_pixel_equal(tmp_path):
    import torch
    from parc_amd import render
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (5, 2, 6, 9, 4), dtype=np.uint8)
    frames[..., 3] = 255
    w = render.FrameWriter(str(tmp_path / "f"), every=2, chunk=2, env_ids=[3, 11], gif=True)
    for k in range(5):
        w.add(torch.tensor(frames[k]))
    assert len(w.paths) == 2 * 2          # frames 0 and 2 went out with the full chunk, frame 4 waits for close()
    w.close()
    from PIL import Image
    for v, e in enumerate((3, 11)):
        for n, k in enumerate((0, 2, 4)):
            path = tmp_path / "f" / "env{:04d}".format(e) / "frame{:06d}.png".format(n)
            assert path.exists()
            img = np.asarray(Image.open(path))
            assert img.shape == (6, 9, 4) and np.array_equal(img, frames[k, v])
        gif = Image.open(tmp_path / "f" / "env{:04d}.gif".format(e))
        assert gif.n_frames == 3 and gif.size == (9, 6)
    assert sorted(os.listdir(tmp_path / "f" / "env0003")) == ["frame000000.png", "frame000001.png", "frame000002.png"]


def test_frame_writer_falls_back_to_ppm_without_pil(tmp_path, monkeypatch):
    import sys
    import torch
    from parc_amd import render
    monkeypatch.setitem(sys.modules, "PIL", None)          # `from PIL import Image` raises ImportError
    frame = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(1, 2, 3, 4)
    w = render.FrameWriter(str(tmp_path), gif=True)
    w.add(torch.tensor(frame))
    w.close()
    path = tmp_path / "env0000" / "frame000000.ppm"
    raw = path.read_bytes()
    assert raw.startswith(b"P6\n3 2\n255\n") and raw[len(b"P6\n3 2\n255\n"):] == frame[0, :, :, :3].tobytes()
    assert os.listdir(tmp_path) == ["env0000"]


def test_set_renderer_refuses_train_mode_and_is_off_by_default():
    from parc_amd.envs import base_env
    from parc_amd.envs.ig_parkour.ig_parkour_env import IGParkourEnv
    env = IGParkourEnv.__new__(IGParkourEnv)
    env._mode, env._renderer, env._frame_writer = base_env.EnvMode.TRAIN, None, None
    marker = object()
    with pytest.raises(RuntimeError, match="TEST mode"):
        env.set_renderer(marker)
    assert env._renderer is None
    env.set_mode(base_env.EnvMode.TEST)
    env.set_renderer(marker)
    assert env._renderer is marker
    with pytest.raises(RuntimeError, match="detach the renderer"):
        env.set_mode(base_env.EnvMode.TRAIN)
    env.set_renderer(None)
    env.set_mode(base_env.EnvMode.TRAIN)
    assert env._mode == base_env.EnvMode.TRAIN and env._renderer is None and env._frame_writer is None
    # visualize=True raises what it raised, before anything else is looked at
    with pytest.raises(NotImplementedError, match="the MI355X build has no viewer"):
        IGParkourEnv(None, 1, "cpu", True)
    # a frame goes from the renderer to the writer; without a writer it is only drawn
    class R:
        n = 0

        def render(self):
            self.n += 1
            return "frame"

        def on_full_reset(self):
            pass

    class W:
        def __init__(self):
            self.got = []

        def add(self, f):
            self.got.append(f)
    env.set_mode(base_env.EnvMode.TEST)
    r, w = R(), W()
    env.set_renderer(r, w)
    env._render_frame()
    env.set_renderer(r)
    env._render_frame()
    assert r.n == 2 and w.got == ["frame"]


def test_run_py_render_flags():
    from parc_amd import render, run
    assert render.parse_size("640x360") == (640, 360) and render.parse_size("37X21") == (37, 21)
    with pytest.raises(ValueError):
        render.parse_size("0x10")
    args = run.load_args(["run.py", "--mode", "test", "--render_dir", "out/frames", "--render_envs", "0,2", "--render_size", "320x200"])
    assert args.parse_string("render_dir", "") == "out/frames" and args.parse_string("render_envs", "0") == "0,2"
    assert run.load_args(["run.py", "--mode", "test"]).parse_string("render_dir", "") == ""          # no flag: nothing is attached

    class Env:
        def set_renderer(self, r, w):
            self.got = (r, w)
    made = {}
    orig = render.Renderer
    try:
        render.Renderer = lambda env, w, h, ids: made.setdefault("r", (w, h, ids))
        env = Env()
        writer = render.attach_from_args(env, "d", "0,2", "320x200")
    finally:
        render.Renderer = orig
    assert made["r"] == (320, 200, [0, 2]) and env.got == (made["r"], writer) and writer.env_ids == [0, 2] and writer.directory == "d"
