"""Exact edge-case tests of the per-step bookkeeping whose results are integers or bit copies - which clip, tile, frame and grid cell an env
sees: the device reset sampler (parc_reset_sample_apply, parc_kin.hip), the time -> frame-pair lookup (make_query of parc_motion_query.h,
through parc_calc_motion_frame) and the stand-alone heightmap rows (parc_refresh_ray_obs_hfs / parc_refresh_obs_hfs, parc_hfgather.hip).  Every test calls the C
ABI through parc_amd._hip and compares with the numpy references of tests/tools/bookkeeping_ref.py (pinned on the fixtures by
tests/test_bookkeeping_ref_cpu.py).  An error in this code moves no value by 1e-5: it picks another row, so the comparisons are
exact wherever the operation is."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import bookkeeping_ref as bk  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
EINVAL = -1
ONE_BELOW = np.nextafter(f32(1.0), f32(0.0))


def T(x, dtype=torch.float32):
    return torch.tensor(np.asarray(x), dtype=dtype, device=DEV)


def neighbours(v):
    """v and its two fp32 neighbours"""
    v = np.atleast_1d(np.asarray(v, f32))
    return np.concatenate([np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))])


# =============================================================================================================================
# reset sampler
# =============================================================================================================================
N_ENVS = 300                       # two workgroups; the second is partly empty and selects from its own LDS copy of the table
MIN_W = 0.01
NOISE_SCALE = 0.3
SENT = dict(mask=-5, mid=-7, tid=-8, toff=-9.5, xyoff=-10.5, timestep=77, time=3.25, done=9, ntt=5.5, noise=-11.5, cdf=-1.0)
RESET_CASES = [(M, R, True) for M in (1, 2, 255, 256, 257, 1000, 4096, 4097, 5000) for R in (1, 3)] + [(1000, 3, False), (4097, 3, False)]


def reset_inputs(M, R, with_fr, seed=0):
    """Random weights, about 20 % exactly 0 - among them the first clip of a chunk of the 256-thread table build, the last clip of a
    chunk, a run across a chunk boundary and clip M - 1; clip 0 positive.  Fail rates partly under the floor.  Mixed done flags."""
    rng = np.random.default_rng(1000 * seed + 7 * M + R + (0 if with_fr else 3))
    chunk = (M + 255) // 256
    nch = (M + chunk - 1) // chunk
    w = (rng.random(M) * 0.9 + 0.1).astype(f32)
    zero = rng.random(M) < 0.2
    if nch >= 4:
        zero[(nch // 3) * chunk] = True                                   # first clip of a chunk
        zero[(2 * nch // 3) * chunk + chunk - 1] = True                   # last clip of a chunk
        b = (nch // 2) * chunk
        zero[b - 2:b + 2] = True                                          # a run that spans a chunk boundary
    if M > 1:
        zero[M - 1] = True
    zero[0] = False
    w[zero] = 0.0
    w = (w / w.sum(dtype=np.float64)).astype(f32)
    fr = rng.random(M).astype(f32)
    low = rng.random(M) < 0.15
    fr[low] = (rng.random(int(low.sum())) * 0.009).astype(f32)           # below min_w: floored
    drng = np.random.default_rng(5)                                      # the same mixed done flags in every case
    done = np.where(drng.random(N_ENVS) < 0.75, drng.integers(1, 3, N_ENVS), 0).astype(np.int32)
    done[[0, 255, 256, 299]] = [1, 2, 1, 2]
    done[[1, 257]] = 0
    return dict(M=M, R=R, chunk=chunk, nch=nch, w=w, fr=fr if with_fr else None, zero=zero,
                lengths=(rng.random(M) * 3.0 + 0.5).astype(f32), offs=rng.standard_normal((M, R, 2)).astype(f32), done=done,
                ep0=(100 + 3 * np.arange(N_ENVS)).astype(np.int64), rng=rng)


def reset_launch(inp, U, n=N_ENVS, override=None):
    """One parc_reset_sample_apply launch per batch row of U [B, 5, n]; every output buffer prefilled with its sentinel.  `override`
    replaces arguments by position (argument checks).  -> return codes, outputs [B, ...] as numpy, the published table"""
    from parc_amd import _hip
    B, M, R = U.shape[0], inp["M"], inp["R"]
    d = dict(u=T(U), done_in=T(inp["done"][:n], torch.int32), w=T(inp["w"]), fr=None if inp["fr"] is None else T(inp["fr"]),
             lengths=T(inp["lengths"]), offs=T(np.concatenate([inp["offs"].reshape(-1, 2), np.zeros((1, 2), f32)])))     # + a spare row
    o = dict(mask=torch.full((B, n), SENT["mask"], dtype=torch.int32, device=DEV), mid=torch.full((B, n), SENT["mid"], dtype=torch.int64, device=DEV),
             tid=torch.full((B, n), SENT["tid"], dtype=torch.int64, device=DEV), toff=torch.full((B, n), SENT["toff"], device=DEV),
             xyoff=torch.full((B, n, 2), SENT["xyoff"], device=DEV), timestep=torch.full((B, n), SENT["timestep"], dtype=torch.int32, device=DEV),
             time=torch.full((B, n), SENT["time"], device=DEV), done=torch.full((B, n), SENT["done"], dtype=torch.int32, device=DEV),
             ntt=torch.full((B, n), SENT["ntt"], device=DEV), ep=T(np.tile(inp["ep0"][:n], (B, 1)), torch.int64),
             noise=torch.full((B, n, 2), SENT["noise"], device=DEV), cdf=torch.full((B, M), SENT["cdf"], device=DEV))
    rcs = []
    for b in range(B):
        at = lambda t: _hip.c_vp(t.data_ptr() + b * t[0].numel() * t.element_size())       # noqa: E731  (row b of a [B, ...] buffer)
        args = [_hip.stream(), n, _hip.ptr(d["done_in"]), at(o["mask"]), at(d["u"]), M, _hip.ptr(d["w"]), _hip.ptr(d["fr"]), MIN_W,
                _hip.ptr(d["lengths"]), _hip.ptr(d["offs"]), R, NOISE_SCALE, at(o["cdf"]), at(o["mid"]), at(o["tid"]), at(o["toff"]),
                at(o["xyoff"]), at(o["timestep"]), at(o["time"]), at(o["done"]), at(o["ntt"]), at(o["ep"]), at(o["noise"])]
        for k, v in (override or {}).items():
            args[k] = v
        rcs.append(_hip.lib().parc_reset_sample_apply(*args))
    torch.cuda.synchronize()
    return rcs, {k: v.cpu().numpy() for k, v in o.items()}


_reset_cache = {}


def reset_case(M, R, with_fr):
    """First call: read the cumulative table back (it depends on the weights only).  Second call, in batches of N_ENVS envs: explicit
    uniforms - for the clip 0, the largest fp32 below 1, and for every k next to a clip of weight 0 fl32(table[k] / total) with its two
    fp32 neighbours; for the tile 0, the largest below 1 and the neighbours of j / R, j = 0 .. R; random values elsewhere."""
    key = (M, R, with_fr)
    if key in _reset_cache:
        return _reset_cache[key]
    inp = reset_inputs(M, R, with_fr)
    rng = inp["rng"]
    rc, first = reset_launch(inp, rng.random((1, 5, N_ENVS)).astype(f32))
    assert rc == [0]
    table = first["cdf"][0].copy()
    z = np.nonzero(inp["zero"])[0]
    ks = np.unique(np.clip(np.concatenate([z - 1, z, z + 1]), 0, M - 1)) if z.size else np.zeros(0, np.int64)
    cand = np.concatenate([[f32(0.0), ONE_BELOW], neighbours(table[ks] / table[M - 1])]).astype(f32)
    cand = np.minimum(np.maximum(cand, f32(0.0)), ONE_BELOW)            # uniforms lie in [0, 1)
    fin = np.nonzero(inp["done"] != 0)[0]
    B = max(1, -(-cand.size // fin.size))
    U = rng.random((B, 5, N_ENVS)).astype(f32)
    clip_u = np.concatenate([cand, rng.random(B * fin.size - cand.size).astype(f32)])
    U[:, 0, :][:, fin] = clip_u.reshape(B, fin.size)
    # tile row: j / R with both neighbours for j = 0 .. R.  A correctly rounded fl32(u R) stays below R for every u < 1 (R 2^-24 is at
    # least half the spacing of fp32 below R), so the clamp to R - 1 acts only for u >= 1, outside the documented domain: 1 and its upper
    # neighbour are fed on purpose, the entry must keep them inside the tile table
    tile_c = np.concatenate([[f32(0.0), ONE_BELOW], neighbours(np.arange(0, R + 1, dtype=f32) / f32(R))]).astype(f32)
    for r in (1, 2, 3, 4):                                              # the other rows: their edge values on finished envs of both workgroups
        edge = tile_c if r == 1 else np.array([0.0, ONE_BELOW, 0.5], f32)
        U[:, r, fin[fin < 256][:edge.size]] = edge
        U[:, r, fin[fin >= 256][:edge.size]] = edge[::-1]
    rc, out = reset_launch(inp, U)
    assert rc == [0] * B
    x = (U[:, 0, :] * table[M - 1]).astype(f32)
    c = dict(inp=inp, table=table, U=U, out=out, first=first, fin=inp["done"] != 0, n_adversarial=int(cand.size),
             prod=bk.clip_products(inp["w"], inp["fr"], MIN_W), want_mid=bk.select_ref(table, x.reshape(-1)).reshape(B, N_ENVS))
    _reset_cache[key] = c
    return c


def table_defects(table, prod):
    """(descending steps, clips of product 0 with a strictly positive step) of a cumulative table"""
    step = np.diff(table.astype(np.float64), prepend=0.0)
    return int((step < 0).sum()), int(((step > 0) & (prod == 0))[1:].sum())


reset_param = pytest.mark.parametrize("M,R,with_fr", RESET_CASES)


@reset_param
def test_reset_table_is_the_cumulative_sum(M, R, with_fr):
    """Assertion 1: the published table against the float64 cumulative sum of the fp32 products, within the bound of the kernel's
    order of additions (build_reset_cdf).  Entry k of chunk t is base[t] + run, all additions fp32 round-to-nearest:
      - run and the chunk sums s_0 .. s_t-1 behind base[t] are running sums inside a chunk, at most chunk - 1 roundings each (the first
        addition, to 0, is exact), each by at most half an ulp of a partial sum of THAT chunk: together <= (chunk - 1) 2^-24 (s_0 + .. + s_t);
      - base[t] = ((s_0 + s_1) + ..) + s_t-1 is a chain of t - 1 <= nchunks - 2 roundings, each by at most 2^-24 of a value that is at
        most the last entry (the table is monotonic);
      - base[t] + run is one more such rounding.
    Bound: (chunk + nchunks - 2) 2^-24 table[M - 1]; the factor 1 + 2^-10 covers the second-order terms (s_0 + .. + s_t exceeds the
    last entry by at most nchunks 2^-24 of it)."""
    c = reset_case(M, R, with_fr)
    inp, table = c["inp"], c["table"]
    ref = bk.cdf_ref(inp["w"], inp["fr"], MIN_W)
    bound = (inp["chunk"] + inp["nch"] - 2) * 2.0 ** -24 * float(table[M - 1]) * (1 + 2.0 ** -10)
    err = np.abs(table.astype(np.float64) - ref)
    print("M %d: max table error %.3e, bound %.3e" % (M, err.max(), bound))
    assert err.max() <= bound
    assert np.array_equal(c["out"]["cdf"], np.tile(table, (c["out"]["cdf"].shape[0], 1)))     # the table depends on the weights only


@reset_param
def test_reset_table_is_sorted_and_flat_on_weight_zero(M, R, with_fr):
    """Assertion 2: non-decreasing, and table[k] == table[k - 1] wherever the product of clip k is 0."""
    c = reset_case(M, R, with_fr)
    down, up0 = table_defects(c["table"], c["prod"])
    assert int((c["prod"] == 0).sum()) == int(c["inp"]["zero"].sum()) and (M < 255 or int(c["inp"]["zero"].sum()) > 40)
    assert (down, up0) == (0, 0), "descending steps %d, weight-0 clips with a positive step %d" % (down, up0)


@reset_param
def test_reset_clip_selection_is_the_first_entry_above(M, R, with_fr):
    """Assertions 3 and 4: every finished env, both workgroups, lands on select_ref(table read back, fl32(u * table[M - 1])) exactly,
    and never on a clip whose product is 0."""
    c = reset_case(M, R, with_fr)
    got, want, fin = c["out"]["mid"], c["want_mid"], c["fin"]
    bad = np.argwhere(got[:, fin] != want[:, fin])
    assert bad.size == 0, (len(bad), [(int(b), int(np.nonzero(fin)[0][e]), int(got[b, fin][e]), int(want[b, fin][e])) for b, e in bad[:5]])
    assert fin[256:].sum() > 10 and c["n_adversarial"] >= 2
    on_zero = c["prod"][got[:, fin]] == 0
    assert int(on_zero.sum()) == 0, "%d finished envs start on a clip of weight 0" % int(on_zero.sum())


@reset_param
def test_reset_tile_time_offset_and_noise(M, R, with_fr):
    """Assertions 5-8: tile = min(int(fl32(u R)), R - 1); time offset = fl32(u length[clip]), one multiply; xy offset = a bit copy of the
    tile table's row; noise within 2 * 2^-23 * scale of (2u - 1) scale (two roundings, or one when it contracts to an fma)."""
    c = reset_case(M, R, with_fr)
    inp, U, out, fin = c["inp"], c["U"], c["out"], c["fin"]
    tile = np.minimum((U[:, 1, :] * f32(R)).astype(f32).astype(np.int64), R - 1)
    assert np.array_equal(out["tid"][:, fin], tile[:, fin])
    assert R == 1 or set(np.unique(out["tid"][:, fin])) == set(range(R))
    ut = U[:, 1, :][:, fin]
    assert (ut == ONE_BELOW).any() and (ut == 0).any() and (ut == 1).any() and (ut > 1).any()      # u >= 1: fl32(u R) >= R, the clamp acts
    mid = out["mid"][:, fin]
    toff = (U[:, 2, :][:, fin] * inp["lengths"][mid]).astype(f32)
    assert np.array_equal(out["toff"][:, fin].view(np.uint32), toff.view(np.uint32))
    assert np.array_equal(out["xyoff"][:, fin].view(np.uint32), inp["offs"][mid, out["tid"][:, fin]].view(np.uint32))
    for k in (0, 1):
        want = (2.0 * U[:, 3 + k, :].astype(np.float64) - 1.0) * float(f32(NOISE_SCALE))
        assert np.abs(out["noise"][:, :, k].astype(np.float64) - want)[:, fin].max() <= 2 * 2.0 ** -23 * NOISE_SCALE


@reset_param
def test_reset_counters_and_untouched_envs(M, R, with_fr):
    """Assertions 9 and 10: mask = finished; finished envs get timestep 0, time 0, done NULL, next target time 0, episode number + 1;
    every buffer of every other env keeps its sentinel."""
    c = reset_case(M, R, with_fr)
    inp, out, fin = c["inp"], c["out"], c["fin"]
    B = out["mask"].shape[0]
    assert np.array_equal(out["mask"], np.tile(fin.astype(np.int32), (B, 1)))
    for k, v in (("timestep", 0), ("time", 0.0), ("done", 0), ("ntt", 0.0)):
        assert np.all(out[k][:, fin] == v), k
    assert np.array_equal(out["ep"], np.tile(inp["ep0"] + fin, (B, 1)))
    for k in ("mid", "tid", "toff", "xyoff", "timestep", "time", "done", "ntt", "noise"):
        assert np.all(out[k][:, ~fin] == SENT[k]), k
    assert (~fin).sum() > 30 and (~fin)[256:].sum() > 3


def test_reset_zero_envs_and_argument_checks():
    """Assertions 11 and 12: n_envs = 0 returns 0 and writes nothing; every null or out-of-range argument the entry checks returns
    PARC_EINVAL with all buffers untouched."""
    from parc_amd import _hip
    inp = reset_inputs(257, 3, True)
    U = np.random.default_rng(3).random((1, 5, N_ENVS)).astype(f32)

    def untouched(out):
        for k in ("mask", "mid", "tid", "toff", "xyoff", "timestep", "time", "done", "ntt", "noise", "cdf"):
            assert np.all(out[k] == SENT[k]), k
        assert np.array_equal(out["ep"][0], inp["ep0"])
    rc, out = reset_launch(inp, U, override={1: 0})
    assert rc == [0]
    untouched(out)
    null = _hip.c_vp(0)
    # position in the argument list: n_envs, done_flags, mask, uniforms, n_motions, weights, lengths, terrains_per_motion, cdf, noise
    for pos, val in ((1, -1), (2, null), (3, null), (4, null), (5, 0), (5, -3), (6, null), (9, null), (11, 0), (11, -1), (13, null), (23, null)):
        rc, out = reset_launch(inp, U, override={pos: val})
        assert rc == [EINVAL], (pos, rc)
        untouched(out)


# =============================================================================================================================
# frame lookup
# =============================================================================================================================
FRAME_COUNTS = (2, 3, 17, 34)
CODE = 64                          # marker = 1024 * (column + 1) + CODE * clip + local frame: a small integer, exact in fp32


def frame_clips():
    """16 clips: every frame count in both loop modes and at 30 and 24 fps (a length that fp32 does not represent).  Root positions on a
    dyadic grid (exact pos_delta, non-zero for the wrap clips), every rotation coordinate moving by at least 0.08 rad between
    consecutive frames."""
    clips = []
    for nf in FRAME_COUNTS:
        for loop in (0, 1):
            for fps in (30.0, 24.0):
                c = len(clips)
                k = np.arange(nf)
                fr = np.zeros((nf, 34), f32)
                fr[:, 0], fr[:, 1], fr[:, 2] = 0.25 * k, -0.125 * k, 1.0 + 0.0625 * k
                for d in range(3, 34):
                    fr[:, d] = -0.3 + 0.01 * ((d + c) % 5) + 0.08 * ((k * (1 + (d + c) % 6)) % 7)
                clips.append(dict(frames=fr, contacts=np.zeros((nf, 15), f32), fps=fps, loop=loop))
    return clips


def frame_queries(lengths, fps, num_frames):
    """Per clip, as fp32: -len, -dt / 2, -0.0, 0; every frame time with both fp32 neighbours; len, 1.5 len, 2 len, 3 len with both
    neighbours; 7 len + dt / 3; 1e4.  Interleaved so that neighbouring 16-lane groups hold different clips; the count is no multiple of
    16 (the last workgroup's groups lie partly past the end)."""
    ids, times = [], []
    for c, (ln, f, nf) in enumerate(zip(lengths, fps, num_frames)):
        ln, dt = f32(ln), f32(1.0 / f)
        t = [np.array([-ln, -dt / f32(2), -0.0, 0.0], f32), neighbours((np.arange(nf) / f).astype(f32)),
             neighbours(np.array([ln, f32(1.5) * ln, f32(2) * ln, f32(3) * ln], f32)), np.array([f32(7) * ln + dt / f32(3), 1e4], f32)]
        t = np.concatenate(t).astype(f32)
        ids.append(np.full(t.size, c, np.int64))
        times.append(t)
    within = np.concatenate([np.arange(t.size) for t in times])
    ids, times = np.concatenate(ids), np.concatenate(times)
    ids, times = np.concatenate([ids, ids[5:10]]), np.concatenate([times, times[5:10]])
    within = np.concatenate([within, np.full(5, within.max() + 1)])
    order = np.lexsort((ids, within))
    return ids[order], times[order]


@pytest.fixture(scope="module")
def km():
    from parc_amd.anim.kin_char_model import KinCharModel
    from parc_amd.assets import humanoid_spec
    m = KinCharModel(DEV)
    m.load_char_file(humanoid_spec.write_mjcf())
    return m


@pytest.fixture(scope="module")
def frame_case(km, tmp_path_factory):
    """MotionLib from pickled synthetic clips; then the marker columns of its rows (root position, contacts, root velocity, root angular
    velocity, dof velocity) are overwritten in place with integers that name clip and frame; one parc_calc_motion_frame launch."""
    import pickle
    import yaml
    from parc_amd.anim.motion_lib import MotionLib, LoopMode
    tmp = str(tmp_path_factory.mktemp("bookkeeping_clips"))
    clips = frame_clips()
    entries = []
    for i, c in enumerate(clips):
        p = os.path.join(tmp, "clip_%02d.pkl" % i)
        with open(p, "wb") as f:
            pickle.dump({"fps": c["fps"], "loop_mode": LoopMode(c["loop"]).name, "frames": c["frames"], "contacts": c["contacts"]}, f)
        entries.append({"file": p, "weight": 1.0})
    yp = os.path.join(tmp, "motions.yaml")
    with open(yp, "w") as f:
        yaml.safe_dump({"motions": entries}, f)
    ml = MotionLib(yp, km, DEV, contact_info=True)
    L = ml._layout
    nf = ml._motion_num_frames.cpu().numpy()
    start = ml._motion_start_idx.cpu().numpy()
    assert nf.tolist() == [c["frames"].shape[0] for c in clips]
    rows = ml._rows.cpu().numpy().copy()
    code = np.concatenate([CODE * c + np.arange(n) for c, n in enumerate(nf)]).astype(f32)
    cols = {"pos": (L["off_pos"], 3), "contacts": (L["off_contacts"], 15), "root_vel": (L["off_root_vel"], 3),
            "root_ang_vel": (L["off_root_ang_vel"], 3), "dof_vel": (L["off_dof_vel"], 28)}
    col_id = 0
    for name, (o, w) in cols.items():
        for j in range(w):
            col_id += 1
            rows[:, o + j] = f32(1024 * col_id) + code
    ml._rows.copy_(T(rows))
    torch.cuda.synchronize()
    lengths = ml._motion_lengths.cpu().numpy()
    loops = ml._motion_loop_modes.cpu().numpy()
    ids, times = frame_queries(lengths, [c["fps"] for c in clips], nf)
    assert ids.size % 16 != 0 and np.all(ids[:64:1][1:] != ids[:64][:-1])
    out = ml.calc_motion_frame(T(ids, torch.int64), T(times))
    torch.cuda.synchronize()
    names = ("root_pos", "root_rot", "root_vel", "root_ang_vel", "joint_rot", "dof_vel", "contacts")
    i0, i1, blend, lp = bk.frame_query_ref(lengths, loops, nf, ids, times)
    return dict(ml=ml, rows=rows, cols=cols, ids=ids, times=times, lengths=lengths, loops=loops, nf=nf, start=start,
                out={k: v.cpu().numpy() for k, v in zip(names, out)}, i0=i0, i1=i1, blend=blend, lp=lp,
                delta=ml._motion_root_pos_delta.cpu().numpy())


def test_frame_lookup_row_copies_name_the_frame(frame_case):
    """Root velocity, root angular velocity and dof velocity are bit copies of row i0: they name the chosen frame exactly, at every
    frame time and its fp32 neighbours, at len and its multiples on clamp and wrap clips, for negative times and far past the end."""
    c = frame_case
    r0 = c["rows"][c["start"][c["ids"]] + c["i0"]]
    for name in ("root_vel", "root_ang_vel", "dof_vel"):
        o, w = c["cols"][name]
        got, want = c["out"][name], r0[:, o:o + w]
        bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, (name, len(bad), [(int(c["ids"][q]), float(c["times"][q]), float(got[q, 0]), float(want[q, 0])) for q in bad[:6]])
    # the cases are there: every local frame of every clip is chosen, also as a wrapped one; and truncation, not rounding, chose
    for m, n in enumerate(c["nf"]):
        assert set(c["i0"][c["ids"] == m]) == set(range(n))
    wrap = c["loops"][c["ids"]] == 1
    assert (wrap & (c["lp"] >= 1) & (c["i0"] == 0)).sum() >= 8 and (wrap & (c["lp"] < 0)).sum() >= 8
    assert ((c["blend"] > 0.5) & (c["i1"] > c["i0"])).sum() > 50


def test_frame_lookup_float64_agrees_away_from_frame_times(frame_case):
    """A blunder shared by the kernel and its fp32 restatement would move the index everywhere; rounding moves it only next to an
    integer frame position: the float64 evaluation of the same fp32 inputs picks the same frame wherever that position is more than
    1e-3 from an integer.  That margin presumes the fp32 evaluation itself errs by less: its frame position is
    fl(fl(frac(fl(t / len))) (nf - 1)) - the division rounds by at most 2^-24 |t / len|, the subtraction of the floor is exact, the
    product rounds by at most 2^-24 (nf - 1) - so it errs by at most (nf - 1) 2^-24 (|t / len| + 1) frames.  That is below 4e-5 for
    every query here but t = 1e4 (a phase of 7e3 .. 3e5, up to 0.016 frames: three of those queries sit 0.0065 .. 0.0072 from an
    integer and fp32 legitimately picks the neighbour); there the margin is that bound."""
    c = frame_case
    j0, dist = bk.frame_query_f64(c["lengths"], c["loops"], c["nf"], c["ids"], c["times"])
    ratio = np.abs(c["times"].astype(np.float64) / c["lengths"][c["ids"]].astype(np.float64))
    fp32_err = (c["nf"][c["ids"]] - 1) * 2.0 ** -24 * (ratio + 1.0)
    assert np.all(fp32_err[c["times"] != f32(1e4)] < 1e-3)
    far = dist > np.maximum(1e-3, fp32_err)
    assert far.sum() > 25
    assert np.array_equal(c["i0"][far], j0[far]), np.nonzero(far & (c["i0"] != j0))[0][:10]


def test_frame_lookup_blended_markers_and_wrap_offset(frame_case):
    """Contacts = (1 - blend) a + blend b and root position = the same + loop_phase * pos_delta, of integer markers: three roundings,
    possibly contracted, each at most 2^-23 of the largest magnitude among operands and result; bound 4 * 2^-23 of it.  The z shift of
    a wrap clip is 0 although its frames do rise."""
    c = frame_case
    base = c["start"][c["ids"]]
    r0, r1 = c["rows"][base + c["i0"]].astype(np.float64), c["rows"][base + c["i1"]].astype(np.float64)
    b = c["blend"].astype(np.float64)[:, None]
    o, w = c["cols"]["contacts"]
    want = (1.0 - b) * r0[:, o:o + w] + b * r1[:, o:o + w]
    mag = np.maximum(np.maximum(np.abs(r0[:, o:o + w]), np.abs(r1[:, o:o + w])), np.abs(want))
    assert np.all(np.abs(c["out"]["contacts"] - want) <= 4 * 2.0 ** -23 * mag)
    o, w = c["cols"]["pos"]
    wrap = (c["loops"][c["ids"]] == 1)[:, None]
    shift = np.where(wrap, c["lp"].astype(np.float64)[:, None] * c["delta"][c["ids"]].astype(np.float64), 0.0)
    lerp = (1.0 - b) * r0[:, o:o + w] + b * r1[:, o:o + w]
    want = lerp + shift
    mag = np.max(np.stack([np.abs(r0[:, o:o + w]), np.abs(r1[:, o:o + w]), np.abs(lerp), np.abs(shift), np.abs(want)]), axis=0)
    err = np.abs(c["out"]["root_pos"] - want)
    assert np.all(err <= 4 * 2.0 ** -23 * mag), (float((err / mag).max()), np.argwhere(err > 4 * 2.0 ** -23 * mag)[:5])
    assert np.all(c["delta"][:, 2] == 0) and np.all(shift[:, 2] == 0)
    assert np.all(np.abs(c["delta"][c["loops"] == 1][:, 0:2]) >= 0.125) and np.abs(shift[:, 0]).max() > 1e3
    # and the library was built from frames whose height does change from the first to the last
    assert np.all([cl["frames"][-1, 2] > cl["frames"][0, 2] for cl in frame_clips()])


def test_frame_lookup_rotations_are_the_slerp_of_rows_i0_i1(frame_case):
    """Root and joint rotations against the project's own slerp (util/torch_util.py) in fp32 on the CPU, fed with the DEVICE's stored
    rows i0 and i1 at the reference blend; tolerance of test_g3_motion_lib_build_and_sample (2e-5 absolute + 1e-5 relative).  slerp
    has two value discontinuities in the cosine of the half angle (cos >= 1 -> q0, sin < 1e-3 -> plain average); queries next to
    one would be left out, and the clips are built so that none is: a pair of rows is either the same row twice / a fixed joint
    (bitwise equal quaternions, every branch returns q0) or at least 0.05 rad apart."""
    from parc_amd.util import torch_util
    c = frame_case
    base = c["start"][c["ids"]]
    Q = c["ids"].size
    q0 = c["rows"][base + c["i0"]][:, 0:60].reshape(Q, 15, 4)
    q1 = c["rows"][base + c["i1"]][:, 0:60].reshape(Q, 15, 4)
    same = (q0.view(np.uint32) == q1.view(np.uint32)).all(axis=-1)
    cosv = np.abs((q0.astype(np.float64) * q1.astype(np.float64)).sum(-1))
    sinv = np.sqrt(np.maximum(1.0 - cosv * cosv, 0.0))
    excluded = ~same & ((cosv > 1.0 - 1e-6) | (np.abs(sinv - 1e-3) < 2e-4))
    assert int(excluded.sum()) == 0
    assert float(np.arccos(np.minimum(cosv[~same], 1.0)).min()) >= 0.025          # half angle: frames at least 0.05 rad apart
    assert (~same).sum() > 0.3 * same.size
    want = torch_util.slerp(torch.tensor(q0), torch.tensor(q1), torch.tensor(c["blend"]).unsqueeze(-1)).numpy().astype(np.float64)
    got = np.concatenate([c["out"]["root_rot"][:, None, :], c["out"]["joint_rot"]], axis=1)
    bad = np.abs(got - want) > 2e-5 + 1e-5 * np.abs(want)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - want).max()), np.argwhere(bad)[:5])


# =============================================================================================================================
# heightmap rows
# =============================================================================================================================
HF_DIMS = (7, 5)                   # dim_x != dim_y: a transposed index shows
HF_MIN, HF_D = (-1.0, -0.5), (0.5, 0.25)
HF_MIN_H, HF_MAX_H = -15.5, 12.25
HF_SENT = -77.0
HF_POINTS = (1, 2, 3, 4, 5, 7, 8, 9)          # head 0..3 x tail 0..3 of the float4 rows, rows that are all head included
HF_ENVS = (1, 2, 3, 5)                        # odd counts: the second env slot of the last workgroup is empty


def hf_terrain():
    i, j = np.meshgrid(np.arange(HF_DIMS[0]), np.arange(HF_DIMS[1]), indexing="ij")
    return (10 * i + j).astype(f32)


def hf_inputs(from_state):
    """Seeded rejection loop: 9 rays and 5 envs, kept only if hf_ref puts every query at least 1e-3 cells from a rounding boundary -
    the fp32 compositions of the kernels err by a few 1e-6 cells at these magnitudes, so the float64 reference alone fixes every cell.
    Roots in and around the grid (rays leave it on all four sides); root z next to the height under the root, so that heights come out
    unclamped near it and clamped at min_h and max_h farther away."""
    rng = np.random.default_rng(12 if from_state else 11)
    hf = hf_terrain()
    rays = (rng.uniform(-1.0, 1.0, (9, 2)) * np.array([1.6, 0.7])).astype(f32)
    span = np.array([[HF_MIN[0] - 0.4, HF_MIN[0] + HF_D[0] * HF_DIMS[0] + 0.1], [HF_MIN[1] - 0.3, HF_MIN[1] + HF_D[1] * HF_DIMS[1] + 0.1]])
    sides = np.array([[span[0, 0] - 0.3, 0.1], [span[0, 1] + 0.4, -0.2], [0.7, span[1, 0] - 0.3], [0.2, span[1, 1] + 0.3]])
    envs = []
    while len(envs) < max(HF_ENVS):
        # envs 0..3 stand outside the grid, one beyond each side; the rest anywhere in and around it
        xy = (sides[len(envs)] + rng.uniform(-0.2, 0.2, 2) if len(envs) < 4 else rng.uniform(span[:, 0], span[:, 1])).astype(f32)
        cell = np.clip(np.rint((xy.astype(np.float64) - HF_MIN) / HF_D).astype(int), 0, np.array(HF_DIMS) - 1)
        z = f32(hf[cell[0], cell[1]] + rng.choice([-1.75, 0.25, 2.5]))
        if from_state:
            q = rng.standard_normal(4)
            q = (q / np.linalg.norm(q)).astype(f32)
            off = (rng.uniform(-3.0, 3.0, 3)).astype(f32)
            rs = np.zeros(13, f32)
            rs[0:3] = np.array([xy[0], xy[1], z], f32) - off              # root + offset = the global position (rounded in fp32 by hf_ref too)
            rs[3:7] = q
            rs[7:13] = rng.standard_normal(6)
            _, dist = bk.hf_ref_from_state(rays, rs[None], off[None], hf, HF_MIN, HF_D, HF_MIN_H, HF_MAX_H)
            env = (rs, off)
        else:
            hd = f32(rng.uniform(-np.pi, np.pi))
            root = np.array([xy[0], xy[1], z], f32)
            _, dist = bk.hf_ref(rays, root[None], [hd], hf, HF_MIN, HF_D, HF_MIN_H, HF_MAX_H)
            env = (root, hd)
        if dist.min() >= 1e-3:
            envs.append(env)
    a = np.stack([e[0] for e in envs])
    b = np.stack([e[1] for e in envs]) if from_state else np.array([e[1] for e in envs], f32)
    return hf, rays, a, b


def hf_launch(from_state, rays, a, b, hf_dev, n_envs, n_points, stride, o, rows_extra=2):
    from parc_amd import _hip
    ter = _hip.TerrainS(_hip.ptr(hf_dev), HF_DIMS[0], HF_DIMS[1], HF_MIN[0], HF_MIN[1], HF_D[0], HF_D[1])
    buf = torch.full(((n_envs + rows_extra) * stride + 16,), HF_SENT, device=DEV)
    fn = _hip.lib().parc_refresh_obs_hfs if from_state else _hip.lib().parc_refresh_ray_obs_hfs
    rc = fn(_hip.stream(), n_envs, _hip.ptr(rays), n_points, _hip.ptr(a), _hip.ptr(b), ter, HF_MIN_H, HF_MAX_H,
            _hip.c_vp(buf.data_ptr() + 4 * o), stride)
    assert rc == 0
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def hf_check_buffer(buf, want, n_envs, n_points, stride, o, what):
    exp = np.full(buf.shape, f32(HF_SENT))
    for e in range(n_envs):
        exp[e * stride + o:e * stride + o + n_points] = want[e, :n_points]
    bad = np.nonzero(buf.view(np.uint32) != exp.view(np.uint32))[0]
    assert bad.size == 0, (what, [(int(i), int(i) // stride, (int(i) % stride) - o, float(buf[i]), float(exp[i])) for i in bad[:6]])


@pytest.mark.parametrize("from_state", [False, True], ids=["heading", "from_state"])
def test_heightmap_rows_every_head_body_tail_split(from_state):
    """Both entries at 1..9 points, written at column 0..3 of rows of 16 floats (vector kernel, head = (4 - o) % 4 leading scalars,
    float4 body, 0..3 trailing scalars) and into rows of 13 floats (rows differently aligned: scalar kernel above 3 points), for 1, 2,
    3 and 5 envs: the output equals hf_ref exactly, everything else in the buffer keeps its sentinel."""
    hf, rays, a, b = hf_inputs(from_state)
    if from_state:
        want, dist = bk.hf_ref_from_state(rays, a, b, hf, HF_MIN, HF_D, HF_MIN_H, HF_MAX_H)
        glob = a[:, 0:3] + b
        u = bk.hf_cell_coords(rays, glob, bk.heading_of_quat(a[:, 3:7]), HF_MIN, HF_D)
        assert np.abs(b[:, 0:2]).min() > 0
    else:
        want, dist = bk.hf_ref(rays, a, b, hf, HF_MIN, HF_D, HF_MIN_H, HF_MAX_H)
        u = bk.hf_cell_coords(rays, a, b, HF_MIN, HF_D)
    # the inputs do what they are meant to: rays leave the grid on all four sides, both clamps act, most heights name their cell
    assert dist.min() >= 1e-3
    assert u[..., 0].min() < -0.5 and u[..., 0].max() > HF_DIMS[0] - 0.5 and u[..., 1].min() < -0.5 and u[..., 1].max() > HF_DIMS[1] - 0.5
    assert (want == f32(HF_MIN_H)).any() and (want == f32(HF_MAX_H)).any() and ((want > HF_MIN_H) & (want < HF_MAX_H)).mean() > 0.5
    # the buffer has HF_DIMS[0]^2 floats so that a transposed index still reads inside it
    hf_dev = torch.full((HF_DIMS[0] * HF_DIMS[0],), 1e6, device=DEV)
    hf_dev[:hf.size] = T(hf.reshape(-1))
    d_rays, d_a, d_b = T(rays), T(a), T(b)
    for n_points in HF_POINTS:
        for stride, o in ((16, 0), (16, 1), (16, 2), (16, 3), (13, 0)):
            for n_envs in HF_ENVS:
                buf = hf_launch(from_state, d_rays, d_a, d_b, hf_dev, n_envs, n_points, stride, o)
                hf_check_buffer(buf, want, n_envs, n_points, stride, o, (n_points, stride, o, n_envs))


def test_heightmap_ties_round_to_the_even_cell():
    """Heading 0, rays and root on multiples of 2^-3: both kernels compute k + 0.5 exactly, and 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 in x and
    in y (round half to even, torch.round)."""
    hf = hf_terrain()
    root = np.array([[0.125, -0.125, 12.0]], f32)
    rx = np.array([-0.875, -0.375, 0.125], f32)          # (rx + 0.125 + 1.0) / 0.5   = 0.5, 1.5, 2.5
    ry = np.array([-0.25, 0.0, 0.25], f32)               # (ry - 0.125 + 0.5) / 0.25  = 0.5, 1.5, 2.5
    rays = np.stack([np.repeat(rx, 3), np.tile(ry, 3)], -1)
    u = bk.hf_cell_coords(rays, root, [0.0], HF_MIN, HF_D)[0]
    assert np.array_equal(u, np.stack([np.repeat([0.5, 1.5, 2.5], 3), np.tile([0.5, 1.5, 2.5], 3)], -1))
    cell = np.array([0, 2, 2])
    want = (hf[np.repeat(cell, 3), np.tile(cell, 3)] - f32(12.0))[None]          # -12, -10, 8, 10: inside the clamp and unlike any neighbour cell's
    assert want.min() > HF_MIN_H and want.max() < HF_MAX_H
    ref, _ = bk.hf_ref(rays, root, [0.0], hf, HF_MIN, HF_D, HF_MIN_H, HF_MAX_H)
    assert np.array_equal(ref, want)
    hf_dev = T(hf.reshape(-1))
    for stride, o in ((16, 0), (16, 3), (13, 0)):        # vector kernel at two alignments, scalar kernel
        buf = hf_launch(False, T(rays), T(root), T(np.zeros(1, f32)), hf_dev, 1, 9, stride, o)
        hf_check_buffer(buf, want, 1, 9, stride, o, (stride, o))
