"""Float64 brute-force ray caster and the test scenes of tests/test_render.py / test_render_gpu.py -- TEST INFRASTRUCTURE (not collected).

An independent formulation of what parc_render draws: per ray a slab test against EVERY terrain column as an axis-aligned box and the
closed-form primitive intersections (capsules in their own axis frame, boxes with a rotation matrix), no DDA, no bounding spheres.  For
every pixel it also reports whether the pixel is "unsafe", i.e. whether a rounding error could change WHICH surface the pixel shows:
    gap     nearest hit and the nearest hit of another id are closer than GAP_EPS (m along the ray)
    border  a terrain hit lies closer than BORDER_EPS (m) to a cell boundary
    graze   a surface in front of the nearest hit is passed or entered at less than GRAZE_EPS (m): |distance to a sphere centre or
            capsule axis - r|, or the length of the chord through a box or column
The thresholds are three orders of magnitude above the fp32 rounding of the scenes' coordinates (|x| < 32 m: ulp 2e-6 m).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import render_host as rh      # noqa: E402
from parc_amd import _hip_render, render      # noqa: E402

GAP_EPS = 1e-3
BORDER_EPS = 1e-3
GRAZE_EPS = 1e-3
SHADOW_BIAS = 1e-3          # parc_render_core.h kShadowBias
MAX_UNSAFE = 0.02           # at most this fraction of a view's pixels may be left out
DEEP = -1.0e6               # bottom of a column


def qmat(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=np.float64)


def quat_axis_angle(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([a * np.sin(0.5 * angle), [np.cos(0.5 * angle)]])


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _slab(o, d, lo, hi):
    """rays [P,3] against boxes [K,3]..[K,3] -> tnear, tfar, axis of tnear, sign of the normal on that axis ([P,K] each)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (lo[None] - o[:, None]) / d[:, None]
        t2 = (hi[None] - o[:, None]) / d[:, None]
    par = (d == 0)[:, None, :] & np.ones_like(t1, bool)
    inside = (o[:, None] > lo[None]) & (o[:, None] < hi[None])
    ta, tb = np.minimum(t1, t2), np.maximum(t1, t2)
    ta = np.where(par, np.where(inside, -np.inf, np.inf), ta)          # parallel to the slab: inside it for all t, or for none
    tb = np.where(par, np.where(inside, np.inf, -np.inf), tb)
    axis = np.argmax(ta, axis=2)
    tnear, tfar = np.max(ta, axis=2), np.min(tb, axis=2)
    sgn = -np.sign(np.take_along_axis(np.broadcast_to(d[:, None], ta.shape), axis[..., None], axis=2)[..., 0])
    return tnear, tfar, axis, sgn


class Reference:
    def __init__(self, scene):
        s = self.s = scene
        f8 = np.float64
        self.B = s.B
        kw = dict(light_dir=(0.35, -0.45, 0.82), ref_char_offset=(0.0, 0.0, 0.0), show_contacts=False, contact_eps=0.1, shadows=True)
        kw.update(s.scene_kw)
        self.kw = kw
        light = np.asarray(np.float32(kw["light_dir"]), f8)
        self.light = light / np.linalg.norm(light)
        hf = s.hf.astype(f8)
        nx, ny = hf.shape
        dx, dy = [f8(v) for v in s.dxdy]
        mx, my = [f8(v) for v in s.min_point]
        ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        self.col_lo = np.stack([mx + (ii - 0.5) * dx, my + (jj - 0.5) * dy, np.full(ii.shape, DEEP)], -1).reshape(-1, 3)
        self.col_hi = np.stack([mx + (ii + 0.5) * dx, my + (jj + 0.5) * dy, hf], -1).reshape(-1, 3)
        self.col_id = (2 * self.B + ii * ny + jj).reshape(-1)

    def world_prims(self, env):
        """[(type, id, a, b, radius, R)] in world space, float64, from the float32 inputs"""
        s, f8 = self.s, np.float64
        out = []
        off = s.env_offsets[env].astype(f8)
        chars = [(s.body_pos, s.body_rot, off, 0)]
        if s.ref_pos is not None:
            chars.append((s.ref_pos, s.ref_rot, off + np.asarray(np.float32(self.kw["ref_char_offset"]), f8), self.B))
        for pos, rot, shift, base in chars:
            for p in s.prims:
                b = min(max(int(p.body), 0), self.B - 1)
                R = qmat(rot[env, b].astype(f8))
                x = pos[env, b].astype(f8) + shift
                a = x + R @ np.array(p.a[:], f8)
                if p.type == _hip_render.CAPSULE:
                    bb = x + R @ np.array(p.b[:], f8)
                else:
                    bb = np.array(p.b[:], f8)
                out.append((int(p.type), base + b, a, bb, float(p.radius), R @ qmat(np.array(p.q[:], f8))))
        return out

    def camera(self, view):
        """eye, fwd, right, up, tan_half in float64 from the view row (the arithmetic of _update_camera for mode track)"""
        s, f8 = self.s, np.float64
        e = min(max(int(view.env), 0), s.N - 1)
        eye, tar = np.array(view.vec[:], f8), np.array(view.target[:], f8)
        if view.mode == 1:
            r = s.root_state[e, 0:2].astype(f8) + s.env_offsets[e, 0:2].astype(f8)
            eye = np.array([r[0] + view.vec[0], r[1] + view.vec[1], view.vec[2]], f8)
            tar = np.array([r[0], r[1], 1.0], f8)
        fwd = (tar - eye) / np.linalg.norm(tar - eye)
        r = np.cross(fwd, [0.0, 0.0, 1.0])
        if r @ r <= 1e-6:
            r = np.cross(fwd, [0.0, 1.0, 0.0])
        r = r / np.linalg.norm(r)
        return e, eye, fwd, r, np.cross(r, fwd), np.tan(0.5 * f8(view.fov_y))

    def rays(self, view):
        s = self.s
        e, eye, fwd, right, up, th = self.camera(view)
        W, H = s.width, s.height
        px, py = np.meshgrid(np.arange(W), np.arange(H))
        sx = (2.0 * (px + 0.5) / W - 1.0) * th * (np.float64(W) / H)
        sy = (1.0 - 2.0 * (py + 0.5) / H) * th
        d = fwd[None, None] + sx[..., None] * right + sy[..., None] * up
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        return e, np.broadcast_to(eye, d.shape).reshape(-1, 3).copy(), d.reshape(-1, 3)

    def cast(self, env, o, d):
        """-> t [P], id [P], normal [P,3], unsafe [P], hit point [P,3]"""
        P = o.shape[0]
        T, ID, NRM, GRZ, GT = [], [], [], [], []      # per candidate: entry t, id, normal, graze margin and where along the ray it applies

        def add(t, ident, n, graze, graze_t):
            T.append(t)
            ID.append(np.broadcast_to(ident, t.shape))
            NRM.append(n)
            GRZ.append(graze)
            GT.append(graze_t)

        def sphere(c, r, ident):
            oc = o - c
            b = np.einsum("pk,pk->p", oc, d)
            rho2 = np.einsum("pk,pk->p", oc, oc) - b * b              # squared distance of the centre to the line
            h = r * r - rho2
            t = np.where(h > 0, -b - np.sqrt(np.maximum(h, 0)), np.inf)
            t = np.where(t > 0, t, np.inf)
            n = (oc + np.where(np.isfinite(t), t, 0)[:, None] * d) / r
            add(t, ident, n, np.abs(np.sqrt(np.maximum(rho2, 0)) - r), -b)

        # terrain: every column as a box
        tn, tf, ax, sg = _slab(o, d, self.col_lo, self.col_hi)
        hit = (tn < tf) & (tn > 0)
        n = np.zeros((P, tn.shape[1], 3))
        np.put_along_axis(n, ax[..., None], sg[..., None], axis=2)
        for k in range(tn.shape[1]):
            add(np.where(hit[:, k], tn[:, k], np.inf), self.col_id[k], n[:, k], np.where(tf[:, k] > 0, np.abs(tf[:, k] - tn[:, k]), np.inf), tn[:, k])
        for typ, ident, a, b, r, R in self.world_prims(env):
            if typ == _hip_render.SPHERE:
                sphere(a, r, ident)
            elif typ == _hip_render.CAPSULE:
                sphere(a, r, ident)
                sphere(b, r, ident)
                # the side, in the frame whose z axis is the capsule's axis
                L = np.linalg.norm(b - a)
                z = (b - a) / L
                x = np.cross(z, [1.0, 0, 0] if abs(z[0]) < 0.9 else [0, 1.0, 0])
                x /= np.linalg.norm(x)
                F = np.stack([x, np.cross(z, x), z])            # world -> axis frame
                ol, dl = (o - a) @ F.T, d @ F.T
                qa = dl[:, 0] ** 2 + dl[:, 1] ** 2
                qb = ol[:, 0] * dl[:, 0] + ol[:, 1] * dl[:, 1]
                qc = ol[:, 0] ** 2 + ol[:, 1] ** 2 - r * r
                with np.errstate(divide="ignore", invalid="ignore"):
                    h = qb * qb - qa * qc
                    t = np.where((h > 0) & (qa > 0), (-qb - np.sqrt(np.maximum(h, 0))) / qa, np.inf)
                    zz = ol[:, 2] + np.where(np.isfinite(t), t, 0) * dl[:, 2]
                    t = np.where((t > 0) & (zz > 0) & (zz < L), t, np.inf)
                    tca = np.where(qa > 0, -qb / qa, 0.0)          # closest approach of the two lines
                    rho = np.sqrt(np.maximum(qc + r * r - np.where(qa > 0, qb * qb / qa, 0.0), 0))
                    zca = ol[:, 2] + tca * dl[:, 2]
                pl = ol + np.where(np.isfinite(t), t, 0)[:, None] * dl
                nl = np.stack([pl[:, 0], pl[:, 1], np.zeros(P)], -1) / r
                graze = np.where((zca > -r) & (zca < L + r), np.abs(rho - r), np.inf)
                add(t, ident, nl @ F, graze, tca)
            else:
                ol, dl = (o - a) @ R, d @ R                  # R^T (o - a)
                tn1, tf1, ax1, sg1 = _slab(ol, dl, -b[None], b[None])
                tn1, tf1, ax1, sg1 = tn1[:, 0], tf1[:, 0], ax1[:, 0], sg1[:, 0]
                hit1 = (tn1 < tf1) & (tn1 > 0)
                nl = np.zeros((P, 3))
                nl[np.arange(P), ax1] = sg1
                add(np.where(hit1, tn1, np.inf), ident, nl @ R.T, np.where(tf1 > 0, np.abs(tf1 - tn1), np.inf), tn1)
        T, ID, NRM, GRZ, GT = np.stack(T, 1), np.stack(ID, 1), np.stack(NRM, 1), np.stack(GRZ, 1), np.stack(GT, 1)
        k = np.argmin(T, axis=1)
        rows = np.arange(P)
        t = T[rows, k]
        ident = np.where(np.isfinite(t), ID[rows, k], -1)
        nrm = NRM[rows, k]
        other = np.where(ID != ident[:, None], T, np.inf).min(axis=1)
        with np.errstate(invalid="ignore"):
            unsafe = np.isfinite(t) & (other - t < GAP_EPS)
        # grazes in front of the nearest hit (a graze behind it changes nothing)
        relevant = (GT > -GRAZE_EPS) & (GT < np.where(np.isfinite(t), t, np.inf)[:, None] + 10 * GRAZE_EPS)
        unsafe |= (np.where(relevant, GRZ, np.inf) < GRAZE_EPS).any(axis=1)
        p = o + np.where(np.isfinite(t), t, 0)[:, None] * d
        ter = ident >= 2 * self.B
        s = self.s
        u = (p[:, 0] - np.float64(s.min_point[0])) / np.float64(s.dxdy[0]) + 0.5
        v = (p[:, 1] - np.float64(s.min_point[1])) / np.float64(s.dxdy[1]) + 0.5
        top = ter & (nrm[:, 2] > 0.5)
        wall_x, wall_y = ter & (np.abs(nrm[:, 0]) > 0.5), ter & (np.abs(nrm[:, 1]) > 0.5)
        du = np.abs(u - np.rint(u)) * np.float64(s.dxdy[0])
        dv = np.abs(v - np.rint(v)) * np.float64(s.dxdy[1])
        unsafe |= (top | wall_y) & (du < BORDER_EPS)
        unsafe |= (top | wall_x) & (dv < BORDER_EPS)
        return t, ident, nrm, unsafe, p

    def view(self, k):
        """dict(t, ids, normal, unsafe, lit_occluded, shadow_unsafe, owner) as [H,W] planes for view k; owner = the hf_lookup cell
        rint((p - min) / dx) of every top-of-terrain hit point as an id (else -2)"""
        s = self.s
        e, o, d = self.rays(s.views[k])
        t, ident, nrm, unsafe, p = self.cast(e, o, d)
        lit = np.isfinite(t) & (nrm @ self.light > 0)
        occ, sh_unsafe = np.zeros(len(t), bool), np.zeros(len(t), bool)
        if lit.any():
            res = []
            for bias in (0.5 * SHADOW_BIAS, SHADOW_BIAS, 2.0 * SHADOW_BIAS):
                ts, _, _, us, _ = self.cast(e, p[lit] + bias * nrm[lit], np.broadcast_to(self.light, p[lit].shape).copy())
                res.append((np.isfinite(ts), us))
            occ[lit] = res[1][0]
            sh_unsafe[lit] = (res[0][0] != res[1][0]) | (res[2][0] != res[1][0]) | res[1][1]
        i = np.rint((p[:, 0] - np.float64(s.min_point[0])) / np.float64(s.dxdy[0])).astype(int)
        j = np.rint((p[:, 1] - np.float64(s.min_point[1])) / np.float64(s.dxdy[1])).astype(int)
        owner = np.where((ident >= 2 * self.B) & (nrm[:, 2] > 0.5), 2 * self.B + i * s.hf.shape[1] + j, -2)
        sh = (s.height, s.width)
        return dict(t=t.reshape(sh), ids=ident.reshape(sh), normal=nrm.reshape(sh + (3,)), unsafe=unsafe.reshape(sh), lit_occluded=occ.reshape(sh),
                    shadow_unsafe=(sh_unsafe | unsafe).reshape(sh), owner=owner.reshape(sh), angle=np.arccos(np.clip(d @ self.camera(s.views[k])[2], -1, 1)).reshape(sh))


# ------------------------------------------------------------------------------------------------------ scenes
IDENT = (0.0, 0.0, 0.0, 1.0)
FAR = 50.0        # a body parked here (below the terrain's bounding box, far off) is out of every view


def prim(body, kind, a=(0, 0, 0), b=(0, 0, 0), radius=0.0, q=IDENT):
    p = _hip_render.PrimS()
    p.body, p.type, p.radius = body, {"sphere": 0, "capsule": 1, "box": 2}[kind], radius
    for k in range(3):
        p.a[k], p.b[k] = a[k], b[k]
    for k in range(4):
        p.q[k] = q[k]
    return p


def flat(h=0.0, n=8):
    return np.full((n, n), h, np.float32)


GRID = dict(min_point=(-1.4, -1.4), dxdy=(0.4, 0.4))        # 8 x 8 cells of 0.4 m around the origin: x, y in [-1.6, 1.6]


def scene_sphere(d=4.0, r=0.5):
    """1: one sphere on the optical axis at distance d, terrain far below; 33 x 25 pixels, so that one pixel looks along the axis"""
    return rh.Scene([prim(0, "sphere", radius=r)], 1, [[[0.07, d, 3.0]]], [[IDENT]], flat(-20.0), views=[render.make_view(0, "still", (0.07, 0, 3.0), (0.07, 1.0, 3.0))],
                    width=33, height=25, shadows=False, **GRID)


def scene_flat(h=0.25, z=5.0):
    """2: flat terrain at height h, camera straight down from z; the one body is out of view"""
    return rh.Scene([prim(0, "sphere", radius=0.1)], 1, [[[FAR, FAR, -5.0]]], [[IDENT]], flat(h),
                    views=[render.make_view(0, "still", (0.07, 0.04, z), (0.07, 0.04, 0.0), fov_y=np.radians(30.0))], shadows=False, **GRID)


def scene_raised():
    """3: one raised cell seen from the side, from outside the grid's bounding box (view 0) and from inside it (view 1)"""
    hf = flat(0.0)
    hf[4, 3] = 0.6
    return rh.Scene([prim(0, "sphere", radius=0.1)], 1, [[[FAR, FAR, -5.0]]], [[IDENT]], hf,
                    views=[render.make_view(0, "still", (0.17, -3.0, 0.45), (0.21, 0.0, 0.3)), render.make_view(0, "still", (0.23, -1.3, 0.4), (0.19, 0.0, 0.3))],
                    shadows=False, **GRID)


def scene_capsule_box():
    """4: a capsule and an oriented box on two bodies at rotated poses; view 1 starts inside the box's bounding sphere"""
    q0 = quat_axis_angle((1.0, 2.0, 0.5), 0.9)
    q1 = quat_axis_angle((0.3, -1.0, 1.0), 2.1)
    prims = [prim(0, "capsule", (0.05, -0.3, 0.02), (0.1, 0.35, 0.12), 0.17), prim(1, "box", (0.1, 0.0, -0.05), (0.45, 0.2, 0.3), q=quat_axis_angle((0, 1, 1), 0.6))]
    return rh.Scene(prims, 2, [[[-0.6, 0.2, 1.0], [0.65, 0.1, 0.9]]], [[q0, q1]], flat(0.0),
                    views=[render.make_view(0, "still", (0.15, -2.6, 1.5), (0.0, 0.0, 0.9)), render.make_view(0, "still", (0.244, -0.037, 1.141), (0.8, 0.3, 0.85), fov_y=np.radians(70.0))],
                    shadows=False, **GRID)


def scene_occlusion(ref_char_offset=(0.0, 0.0, 0.0)):
    """5: the reference character (same shapes, other pose) stands behind the simulated one"""
    prims = [prim(0, "capsule", (0, 0, -0.3), (0, 0, 0.3), 0.2), prim(1, "sphere", (0, 0, 0), radius=0.22)]
    pos = [[[0.0, 0.0, 0.8], [0.0, 0.0, 1.45]]]
    rpos = [[[0.25, 0.9, 0.85], [0.3, 0.9, 1.5]]]
    rot = [[quat_axis_angle((0, 1, 0), 0.2), IDENT]]
    return rh.Scene(prims, 2, pos, rot, flat(0.0), views=[render.make_view(0, "still", (0.1, -2.8, 1.3), (0.1, 0.0, 1.0))], ref_pos=rpos, ref_rot=rot,
                    shadows=False, ref_char_offset=ref_char_offset, **GRID)


def scene_shadows():
    """6: a box and a sphere over a stepped terrain, light from the side"""
    hf = flat(0.0)
    hf[2, :] = 0.35
    hf[5, 5] = 0.5
    prims = [prim(0, "box", (0, 0, 0), (0.45, 0.35, 0.2), q=quat_axis_angle((0, 0, 1), 0.5)), prim(1, "sphere", radius=0.35)]
    return rh.Scene(prims, 2, [[[0.1, 0.2, 0.9], [0.7, -0.5, 0.6]]], [[IDENT, IDENT]], hf,
                    views=[render.make_view(0, "still", (0.4, -3.6, 3.0), (0.0, 0.0, 0.2))], shadows=True, **GRID)


def scene_contacts():
    """7: three bodies, one of them over contact_eps"""
    prims = [prim(b, "sphere", radius=0.25) for b in range(3)]
    cf = [[[0.0, 0.0, 0.05], [3.0, 0.0, 4.0], [0.0, 0.0, 0.0]]]
    return rh.Scene(prims, 3, [[[-0.7, 0, 0.5], [0.0, 0, 0.5], [0.7, 0, 0.5]]], [[IDENT] * 3], flat(0.0),
                    views=[render.make_view(0, "still", (0.0, -3.5, 1.5), (0.0, 0.0, 0.5))], contact_forces=cf, shadows=False, **GRID)


def scene_track(root_xy):
    """8: two envs with offsets; env 1 is drawn by a tracking camera"""
    prims = [prim(0, "capsule", (0, 0, -0.2), (0, 0, 0.3), 0.2)]
    pos = [[[0.0, 0.0, 0.9]], [[root_xy[0], root_xy[1], 0.9]]]
    off = [[0.0, 0.0, 0.0], [-0.5, 0.25, 0.0]]
    return rh.Scene(prims, 1, pos, [[IDENT], [IDENT]], flat(0.0), views=[render.make_view(1, "track", render.TRACK_DELTA)], env_offsets=off,
                    shadows=True, **GRID)


def humanoid_pose(km, root_pos, root_quat, joint_angle=0.25, seed=0):
    """body poses [B,3], [B,4] of the humanoid for seeded joint rotations (tree walk in float64)"""
    B = km.get_num_joints()
    par = km._parent_indices.cpu().numpy()
    lt = km._local_translation.cpu().numpy().astype(np.float64)
    lr = km._local_rotation.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(seed)
    pos, rot = np.zeros((B, 3)), np.zeros((B, 4))
    pos[0], rot[0] = root_pos, root_quat
    for b in range(1, B):
        jr = quat_axis_angle(rng.normal(size=3), joint_angle * rng.uniform(-1, 1))
        rot[b] = qmul(qmul(rot[par[b]], lr[b]), jr)
        rot[b] /= np.linalg.norm(rot[b])
        pos[b] = pos[par[b]] + qmat(rot[par[b]]) @ lt[b]
    return pos, rot


def scene_humanoid():
    """9: the whole humanoid (every MJCF geom) in its init pose with bent joints on a stepped terrain, its reference character beside it, two
    envs, two views"""
    km, prims = rh.humanoid()
    B = km.get_num_joints()
    hf = flat(0.0)
    hf[:, 5:] = 0.3
    hf[6, :] = 0.55
    hf[1, 2] = 0.2
    p0, r0 = humanoid_pose(km, (0.0, -0.2, 0.95), IDENT, seed=1)
    p1, r1 = humanoid_pose(km, (0.1, 0.0, 1.0), quat_axis_angle((0, 0, 1), 0.7), seed=2)
    q0, s0 = humanoid_pose(km, (0.5, 0.3, 1.25), quat_axis_angle((0, 0, 1), -0.4), joint_angle=0.1, seed=3)
    q1, s1 = humanoid_pose(km, (-0.5, 0.5, 1.25), IDENT, joint_angle=0.1, seed=4)
    cf = np.zeros((2, B, 3))
    cf[0, B - 1, 2] = 50.0
    views = [render.make_view(0, "still", (1.0, -2.6, 1.7), (0.2, 0.0, 0.9)), render.make_view(1, "track", (-1.8, -2.3, 1.9))]
    return rh.Scene(prims, B, [p0, p1], [r0, r1], hf, views=views, ref_pos=[q0, q1], ref_rot=[s0, s1], contact_forces=cf,
                    env_offsets=[[0.0, 0.0, 0.0], [0.2, -0.1, 0.0]], shadows=True, show_contacts=True, **GRID)


def scene_malformed():
    """10: an env index out of range and cameras far outside the grid, a NaN eye, eye == target, a wild field of view"""
    s = scene_humanoid()
    nan = float("nan")
    views = [render.make_view(7, "still", (900.0, -700.0, 300.0), (0, 0, 0)), render.make_view(-3, "track", (1e6, 1e6, -1e6)),
             render.make_view(0, "still", (nan, 0.0, 1.0), (0, 0, 0)), render.make_view(1, "still", (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), fov_y=nan),
             render.make_view(2 ** 31 - 1, 5, (0.0, -2.0, 1.0), (0, 0, 1.0), fov_y=1e9), render.make_view(0, "still", (0.0, 0.0, 30.0), (0, 0, 0), fov_y=-1.0)]
    return s.with_views(views)


DEPTH_SCENES = dict(sphere=scene_sphere, flat=scene_flat, raised=scene_raised, capsule_box=scene_capsule_box, occlusion=scene_occlusion,
                    shadows=scene_shadows, contacts=scene_contacts, track=lambda: scene_track((0.25, 0.5)), humanoid=scene_humanoid)

# Largest |depth(fp32 host build) - depth(float64 reference)| over the safe pixels of DEPTH_SCENES, measured with
# `python tests/render_ref.py` (it prints the figure per scene); the CPU tests allow 2x, the GPU tests 4x (Rendering).
MEASURED_DEPTH_ERR = 1.39e-4      # (1.389e-4: humanoid, view 1, at depths up to 4.9 m)


def measure(lib):
    worst = 0.0
    for name, make in DEPTH_SCENES.items():
        s = make()
        out = s.render_host(lib)
        ref = Reference(s)
        for k in range(len(s.views)):
            r = ref.view(k)
            safe = ~r["unsafe"]
            hit = safe & np.isfinite(r["t"])
            bad = int((out["ids"][k][safe] != r["ids"][safe]).sum())
            err = float(np.abs(out["depth"][k][hit].astype(np.float64) - r["t"][hit]).max()) if hit.any() else 0.0
            print("{:12s} view {}: unsafe {:5.2f} %  id mismatches on safe pixels {}  max depth err {:.3e}  (max depth {:.2f})".format(
                name, k, 100.0 * r["unsafe"].mean(), bad, err, float(r["t"][hit].max()) if hit.any() else 0.0))
            worst = max(worst, err)
    print("largest depth error: {:.3e}".format(worst))
    return worst


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        measure(rh.build_host(tmp))
