"""Plain numpy references for the per-step bookkeeping whose results are integers or exact copies: the time -> frame-pair lookup (make_query,
parc_motion_query.h), the cumulative clip weights and their inversion (parc_reset_sample_apply, parc_kin.hip) and the heightmap rows
(parc_refresh_ray_obs_hfs / parc_refresh_obs_hfs, parc_hfgather.hip).  No GPU, no torch.  tests/test_bookkeeping_ref_cpu.py pins these functions on the
fixtures, tests/test_bookkeeping_gpu.py compares the kernels with them."""
import numpy as np

f32 = np.float32


# ---------------------------------------------------------------------------------------------- frame lookup
def frame_query_ref(lengths, loop_modes, num_frames, ids, times):
    """MotionLib.calc_motion_phase / _calc_frame_blend (anim/motion_lib.py:443-456,527-538, oracle/parc_oracle.c:374-399) in float32,
    operation for operation: divide, floor, subtract, clamp, multiply by nf - 1, truncate.  The mapping truncates and the reference
    evaluates it in fp32, so next to a frame time fp32 is the yardstick (float64 legitimately picks the neighbouring frame there).
    -> i0, i1 (frame indices inside the clip), blend, loop_phase (floor(time / len), what the wrap offset is multiplied by)."""
    ids = np.asarray(ids, np.int64)
    ln = np.asarray(lengths, f32)[ids]
    t = np.asarray(times, f32)
    nf = np.asarray(num_frames, np.int64)[ids]
    wrap = np.asarray(loop_modes)[ids] == 1
    phase = t / ln
    assert phase.dtype == f32
    loop_phase = np.floor(phase)
    phase = np.where(wrap, phase - np.floor(phase), phase)
    phase = np.minimum(np.maximum(phase, f32(0.0)), f32(1.0))
    fp = phase * (nf - 1).astype(f32)
    assert fp.dtype == f32
    i0 = fp.astype(np.int64)                                    # .long(): truncation
    i1 = np.minimum(i0 + 1, nf - 1)
    blend = fp - i0.astype(f32)
    assert blend.dtype == f32
    return i0, i1, blend, loop_phase


def frame_query_f64(lengths, loop_modes, num_frames, ids, times):
    """The same mapping in float64 on the same fp32 inputs.  -> i0, and the distance of the frame position from the nearest integer
    (queries far from an integer must get the same frame in both precisions: a blunder shared by a kernel and its fp32 restatement
    would move the index everywhere, rounding moves it only next to an integer)."""
    ids = np.asarray(ids, np.int64)
    ln = np.asarray(lengths, f32)[ids].astype(np.float64)
    t = np.asarray(times, f32).astype(np.float64)
    nf = np.asarray(num_frames, np.int64)[ids]
    wrap = np.asarray(loop_modes)[ids] == 1
    phase = t / ln
    phase = np.where(wrap, phase - np.floor(phase), phase)
    phase = np.clip(phase, 0.0, 1.0)
    fp = phase * (nf - 1)
    return fp.astype(np.int64), np.abs(fp - np.rint(fp))


# ---------------------------------------------------------------------------------------------- reset sampler
def clip_products(weights, fail_rates, min_w):
    """fp32 products max(fail_rate, min_w) * weight (1 * weight without fail rates): what the sampler accumulates"""
    w = np.asarray(weights, f32)
    if fail_rates is None:
        return w.copy()
    p = np.maximum(np.asarray(fail_rates, f32), f32(min_w)) * w
    assert p.dtype == f32
    return p


def cdf_ref(weights, fail_rates, min_w):
    """float64 cumulative sum of the fp32 products"""
    return np.cumsum(clip_products(weights, fail_rates, min_w).astype(np.float64))


def select_ref(table, x):
    """first index k with table[k] > x, clamped to M - 1: a linear scan straight from that definition (no searchsorted: the table
    under test need not be sorted)"""
    table = np.asarray(table)
    x = np.atleast_1d(np.asarray(x))
    M = table.shape[0]
    out = np.empty(x.shape[0], np.int64)
    for a in range(0, x.shape[0], 1024):                        # blocks of queries: every entry of the table against every query
        gt = table[None, :] > x[a:a + 1024, None]
        out[a:a + 1024] = np.where(gt.any(axis=1), gt.argmax(axis=1), M)       # argmax of booleans: the first True
    return np.minimum(out, M - 1)


# ---------------------------------------------------------------------------------------------- heightmap rows
def heading_of_quat(q):
    """atan2 of the x axis rotated by q = (x, y, z, w)  (util/torch_util.py calc_heading), float64"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.arctan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def hf_cell_coords(ray_xy, root_xyz, heading, min_point, dxdy):
    """-> [N, P, 2] float64 cell coordinates of every query before rounding (the grid covers [-0.5, dim - 0.5) on each axis)"""
    ray = np.asarray(ray_xy, np.float64)
    root = np.asarray(root_xyz, np.float64)
    hd = np.asarray(heading, np.float64)
    mn = np.asarray(min_point, np.float64)
    d = np.asarray(dxdy, np.float64)
    c, s = np.cos(hd)[:, None], np.sin(hd)[:, None]
    x, y = ray[None, :, 0], ray[None, :, 1]
    px = x * c - y * s + root[:, 0:1]
    py = x * s + y * c + root[:, 1:2]
    return np.stack([(px - mn[0]) / d[0], (py - mn[1]) / d[1]], -1)


def hf_ref(ray_xy, root_xyz, heading, hf, min_point, dxdy, min_h, max_h):
    """util/terrain_util.py:107-126 behind RefCharEnv._refresh_ray_obs_hfs in float64: rotate the ray by the heading, add the root,
    subtract the min point, divide by the cell size, round half to even, clamp to the grid, gather, subtract root z, clamp to
    [min_h, max_h].  ray_xy [P, 2], root_xyz [N, 3], heading [N], hf [dim_x, dim_y].
    -> heights [N, P] (float32: exact copies of hf minus z), distance [N, P] in cells of every query from the nearest rounding boundary"""
    root = np.asarray(root_xyz, np.float64)
    hf = np.asarray(hf)
    u = hf_cell_coords(ray_xy, root_xyz, heading, min_point, dxdy)
    dist = np.abs(u - np.floor(u) - 0.5).min(-1)
    g = np.rint(u).astype(np.int64)                             # half to even, like torch.round
    gi = np.clip(g[..., 0], 0, hf.shape[0] - 1)
    gj = np.clip(g[..., 1], 0, hf.shape[1] - 1)
    # the kernels subtract in fp32 (one rounding of an exact copy); on fp32 inputs the float64 difference rounded once is that value
    v = (hf[gi, gj].astype(np.float64) - root[:, 2:3]).astype(f32)
    return np.clip(v, f32(min_h), f32(max_h)), dist


def hf_ref_from_state(ray_xy, root_state, env_offsets, hf, min_point, dxdy, min_h, max_h):
    """the from-state entry (IGParkourEnv._refresh_obs_hfs): global root = root position + env offset, each summed in fp32 as the env
    does; heading = atan2 of the rotated x axis"""
    rs = np.asarray(root_state, f32)
    glob = rs[:, 0:3] + np.asarray(env_offsets, f32)
    assert glob.dtype == f32
    return hf_ref(ray_xy, glob, heading_of_quat(rs[:, 3:7]), hf, min_point, dxdy, min_h, max_h)
