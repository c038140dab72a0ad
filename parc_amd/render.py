"""Offscreen rendering of test / record rollouts (include/parc_render.h): what the reference shows in its viewer - the simulated
character, the reference character at `ref_char_offset` and the terrain (envs/ig_env.py `_render`, envs/ig_char_env.py:512-541) - as image
sequences, because the MI355X machines have no display.

    renderer = Renderer(env, 640, 360, env_ids=[0])
    env.set_renderer(renderer, FrameWriter("out/frames"))      # TEST mode only: the captured training step is never touched

`Renderer.render()` is one launch of `parc_render` on the current stream and no host synchronisation; `FrameWriter` keeps frames on the
device and brings them over a chunk at a time.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _hip, _hip_render
from .anim.kin_char_model import GeomType

DEFAULT_FOV_Y = math.radians(50.0)
TRACK_DELTA = (0.0, -5.0, 3.0)        # _init_camera (envs/ig_char_env.py:512-520): 5 m behind the character in y, 3 m up


def scene_prims(kin_char_model):
    """The character's collision geoms as parc_render_prim_t rows, from the MJCF geoms that sim_model.py reads (not from the simulator's
    sample spheres)."""
    km = kin_char_model
    rows = []
    for b in range(km.get_num_joints()):
        for g in km.get_geoms(b):
            p = _hip_render.PrimS()
            p.body = b
            p.q[3] = 1.0
            off = np.asarray(g._offset, np.float64)
            if g._shape_type == GeomType.SPHERE:
                p.type, p.radius = _hip_render.SPHERE, float(np.atleast_1d(g._dims)[0])
                a, bb = off, np.zeros(3)
            elif g._shape_type == GeomType.CAPSULE:
                p.type, p.radius = _hip_render.CAPSULE, float(g._radius)
                a, bb = off, off + np.asarray(g._dims, np.float64)
            elif g._shape_type == GeomType.BOX:
                p.type = _hip_render.BOX
                a, bb = off, np.asarray(g._dims, np.float64)
                if g._quat is not None:
                    for k in range(4):
                        p.q[k] = float(g._quat[k])
            else:
                raise NotImplementedError(g._shape_type)
            for k in range(3):
                p.a[k], p.b[k] = float(a[k]), float(bb[k])
            rows.append(p)
    if len(rows) > _hip_render.MAX_PRIMS:
        raise ValueError("the character has {} geoms, parc_render stages at most {}".format(len(rows), _hip_render.MAX_PRIMS))
    return rows


def prims_bytes(rows):
    return b"".join(bytes(r) for r in rows)


def make_scene(n_prims, num_bodies, prims_ptr=None, light_dir=(0.35, -0.45, 0.82), ambient=0.35, sim_color=(0.85, 0.55, 0.25),
               ref_color=(0.30, 0.55, 0.90), ref_char_offset=(0.0, 0.0, 0.0), shadows=True, show_contacts=False, contact_eps=0.1):
    s = _hip_render.SceneS()
    s.prims = prims_ptr
    s.n_prims, s.num_bodies = int(n_prims), int(num_bodies)
    for k in range(3):
        s.light_dir[k], s.sim_color[k], s.ref_color[k] = float(light_dir[k]), float(sim_color[k]), float(ref_color[k])
        s.ref_char_offset[k] = float(ref_char_offset[k])
    s.ambient, s.shadows, s.show_contacts, s.contact_eps = float(ambient), int(bool(shadows)), int(bool(show_contacts)), float(contact_eps)
    return s


def make_view(env, mode, vec, target=(0.0, 0.0, 0.0), fov_y=DEFAULT_FOV_Y):
    v = _hip_render.ViewS()
    v.env, v.mode, v.fov_y = int(env), _hip_render.CAMERA_MODES[mode] if isinstance(mode, str) else int(mode), float(fov_y)
    for k in range(3):
        v.vec[k], v.target[k] = float(vec[k]), float(target[k])
    return v


class Renderer:
    """Draws the envs `env_ids` of an IGParkourEnv, one view each.  camera_mode: "track" (the reference's _update_camera: the camera
    keeps its xy distance to the character and its height) or "still" (the camera of _init_camera stays where the character was at the first frame after a full reset);
    default the env's `camera_mode` key.  `rgba` [V,H,W,4] uint8, `depth` [V,H,W] float32 and `ids` [V,H,W] int32 (with_depth /
    with_ids) are device tensors overwritten by every render()."""

    def __init__(self, env, width, height, env_ids, camera_mode=None, shadows=True, show_contacts=False, with_depth=False, with_ids=False,
                 fov_y=DEFAULT_FOV_Y):
        env_cfg = env._config["env"]
        camera_mode = env_cfg.get("camera_mode", "track") if camera_mode is None else camera_mode
        if camera_mode not in _hip_render.CAMERA_MODES:
            raise ValueError("Unsupported camera mode {}".format(camera_mode))
        self._env, self._core, self._km = env, env._core, env._kin_char_model
        self.width, self.height = int(width), int(height)
        self.env_ids = [int(e) for e in env_ids]
        N, n_dm = env.get_num_envs(), env._num_dm_envs
        if not self.env_ids or min(self.env_ids) < 0 or max(self.env_ids) >= N:
            raise ValueError("env_ids must be a non-empty list of env indices below {}".format(N))
        in_dm = [e < n_dm for e in self.env_ids]
        if any(in_dm) and not all(in_dm):
            raise ValueError("the envs of one Renderer share a terrain: take rows of the dataset sub-env or of the generator sub-env")
        self._dm_rows = all(in_dm)
        dev = env._device
        self.camera_mode = camera_mode
        B = self._km.get_num_joints()
        rows = scene_prims(self._km)
        self._prims = torch.frombuffer(bytearray(prims_bytes(rows)), dtype=torch.uint8).to(dev)
        self._scene = make_scene(len(rows), B, self._prims.data_ptr(), ref_char_offset=env_cfg.get("ref_char_offset", [0.0, 0.0, 0.0]),
                                 shadows=shadows, show_contacts=show_contacts, contact_eps=float(env._cfg.struct.contact_eps))
        self._fov_y = float(fov_y)
        self._views = None          # built by the first render(): a still camera is placed where the character is then
        V = len(self.env_ids)
        self._rgba = torch.zeros((V, self.height, self.width), dtype=torch.int32, device=dev)
        self.rgba = self._rgba.view(torch.uint8).view(V, self.height, self.width, 4)
        self.depth = torch.zeros((V, self.height, self.width), dtype=torch.float32, device=dev) if with_depth else None
        self.ids = torch.zeros((V, self.height, self.width), dtype=torch.int32, device=dev) if with_ids else None
        N = env.get_num_envs()
        self._ref_body_pos = torch.zeros((N, B, 3), dtype=torch.float32, device=dev)
        self._ref_body_rot = torch.zeros((N, B, 4), dtype=torch.float32, device=dev)

    def _build_views(self):
        """The reference's initial camera (_init_camera, envs/ig_char_env.py:512-520) for every drawn env: 5 m behind the character in y,
        3 m up.  track: the kernel keeps that xy distance and height and looks at (root xy, 1.0) like _update_camera.  still: the camera
        stays where the character was at the first render() after the latest full reset, looking at (root xy, 0.0) as _init_camera does
        (this placement reads the root positions back once)."""
        views = []
        if self.camera_mode == "track":
            views = [make_view(e, "track", TRACK_DELTA, fov_y=self._fov_y) for e in self.env_ids]
        else:
            p = (self._core.root_state[:, 0:3] + self._core.env_offsets).cpu().numpy()
            for e in self.env_ids:
                views.append(make_view(e, "still", (p[e, 0] + TRACK_DELTA[0], p[e, 1] + TRACK_DELTA[1], TRACK_DELTA[2]), (p[e, 0], p[e, 1], 0.0),
                                       fov_y=self._fov_y))
        self._views = torch.frombuffer(bytearray(b"".join(bytes(v) for v in views)), dtype=torch.uint8).to(self._env._device)

    def on_full_reset(self):
        """called by the env after a full reset, before its frame: a still camera is placed anew"""
        if self.camera_mode == "still":
            self._views = None

    def _terrain_struct(self):
        return self._core._terrain_struct if self._dm_rows else self._env._mgdm_env.terrain_struct()

    def render(self):
        """One frame of every view from the state tensors as they are now -> uint8 [V,H,W,4] (the renderer's own buffer)."""
        c, L, p = self._core, _hip.lib(), _hip.ptr
        N = self._env.get_num_envs()
        if self._views is None:
            self._build_views()
        # the tracker core keeps the reference pose as root + joint rotations: body poses by forward kinematics
        _hip.check(L.parc_forward_kinematics(_hip.stream(), self._km.c_struct(), N, p(c.ref_root_pos), p(c.ref_root_rot), p(c.ref_joint_rot),
                                             p(self._ref_body_pos), p(self._ref_body_rot)), "parc_forward_kinematics")
        _hip.check(L.parc_render(_hip.stream(), self._terrain_struct(), ctypes.byref(self._scene), len(self.env_ids), p(self._views), self.width,
                                 self.height, p(c.root_state), p(c.rigid_body_state), p(self._ref_body_pos), p(self._ref_body_rot),
                                 p(c.contact_forces), p(c.env_offsets), N, p(self._rgba), p(self.depth), p(self.ids)), "parc_render")
        return self.rgba


def _write_image(path_no_ext, frame):
    """frame uint8 [H,W,4] -> PNG with PIL, PPM (RGB) without it; returns the path written"""
    try:
        from PIL import Image
    except ImportError:
        path = path_no_ext + ".ppm"
        with open(path, "wb") as f:
            f.write("P6\n{} {}\n255\n".format(frame.shape[1], frame.shape[0]).encode())
            f.write(np.ascontiguousarray(frame[..., :3]).tobytes())
        return path
    path = path_no_ext + ".png"
    Image.fromarray(frame, "RGBA").save(path)
    return path


class FrameWriter:
    """Writes `directory/env%04d/frame%06d.png` (PPM without PIL).  Every `every`-th frame given to add() is copied into a device-side
    chunk of `chunk` frames; a full chunk comes over in one copy.  close() flushes; gif=True also writes `env%04d.gif` per env at
    close() (PIL only).  env_ids names the directories (default 0..V-1)."""

    def __init__(self, directory, every=1, chunk=32, env_ids=None, gif=False, gif_fps=10):
        assert every >= 1 and chunk >= 1
        self.directory, self.every, self.chunk, self.env_ids, self.gif, self.gif_fps = directory, int(every), int(chunk), env_ids, gif, gif_fps
        self._buf = None
        self._fill = 0
        self._seen = 0
        self._written = 0
        self._gif_frames = None
        self.paths = []

    def add(self, rgba):
        """rgba: uint8 [V,H,W,4] tensor (a Renderer's buffer: it is copied here, on its device)"""
        take = self._seen % self.every == 0
        self._seen += 1
        if not take:
            return
        if self._buf is None:
            self._buf = torch.empty((self.chunk,) + tuple(rgba.shape), dtype=torch.uint8, device=rgba.device)
        self._buf[self._fill].copy_(rgba)
        self._fill += 1
        if self._fill == self.chunk:
            self.flush()

    def flush(self):
        if self._fill == 0:
            return
        host = self._buf[:self._fill].cpu().numpy()        # one copy for the chunk
        V = host.shape[1]
        ids = list(range(V)) if self.env_ids is None else list(self.env_ids)
        if self.gif and self._gif_frames is None:
            self._gif_frames = [[] for _ in range(V)]
        for k in range(self._fill):
            for v in range(V):
                d = os.path.join(self.directory, "env{:04d}".format(ids[v]))
                os.makedirs(d, exist_ok=True)
                self.paths.append(_write_image(os.path.join(d, "frame{:06d}".format(self._written)), host[k, v]))
                if self.gif:
                    self._gif_frames[v].append(host[k, v, :, :, :3].copy())
            self._written += 1
        self._fill = 0

    def close(self):
        self.flush()
        if self.gif and self._gif_frames:
            try:
                from PIL import Image
            except ImportError:
                return
            ids = list(range(len(self._gif_frames))) if self.env_ids is None else list(self.env_ids)
            for v, frames in enumerate(self._gif_frames):
                if frames:
                    imgs = [Image.fromarray(f, "RGB") for f in frames]
                    path = os.path.join(self.directory, "env{:04d}.gif".format(ids[v]))
                    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=int(1000 / self.gif_fps), loop=0)
                    self.paths.append(path)
            self._gif_frames = None


def parse_size(text):
    """"640x360" -> (640, 360)"""
    w, h = text.lower().split("x")
    w, h = int(w), int(h)
    if w <= 0 or h <= 0:
        raise ValueError("render size must be positive: {}".format(text))
    return w, h


def attach_from_args(env, render_dir, render_envs="0", render_size="640x360"):
    """What run.py's --render_dir / --render_envs / --render_size do: a Renderer + FrameWriter on `env`; returns the writer (close() it)."""
    ids = [int(x) for x in str(render_envs).split(",") if x != ""]
    w, h = parse_size(render_size)
    writer = FrameWriter(render_dir, env_ids=ids)
    env.set_renderer(Renderer(env, w, h, ids), writer)
    return writer
