"""The batched motion optimiser on the device: the ragged terrain query, the seamed frame-to-frame terms, and
motion_contact_optimization_batch / compute_approx_body_constraints_batch / the driver's opt_batch_size against the single-motion path
and fixture G20.  The three test motions A, B, C are derived from G20 (tests/tools/moopt_host.three_motions)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden
from test_hip_parity import DEV, T, close, km  # noqa: F401  (km is a fixture)
from test_motion_opt_gpu import _problem, _source_terms

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import moopt_host as mh      # noqa: E402

pytestmark = pytest.mark.gpu

KW = (dict(inverted=True, radius=None), dict(inverted=False, radius=None), dict(inverted=False, radius=0.1))


def _subterrain(hf, mp, dxdy):
    from parc_amd.util import terrain_util
    return terrain_util.SubTerrain.from_arrays(hf, mp, dxdy, device=DEV)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("kw", KW)
def test_ragged_query_values_cells_and_adjoint(oracle, kw):
    from parc_amd.util import terrain_util
    case = mh.RaggedCase()
    ters = [_subterrain(*t) for t in case.terrains]
    table = terrain_util.HfTable(ters, base_z=-10.0, device=DEV)
    rt = torch.tensor(case.row_terrain, device=DEV)
    pts = T(case.points).requires_grad_(True)
    out = terrain_util.points_hf_sdf_ragged(pts, rt, table, **kw)
    out.backward(T(case.g_out))
    _, cell, _ = terrain_util._points_hf_sdf_ragged_launch(pts, rt, table, kw["inverted"], kw["radius"], True)
    got, cell, grad = out.detach().cpu().numpy(), cell.cpu().numpy(), pts.grad.cpu().numpy()
    for t, (rows, want) in case.oracle(oracle, **kw).items():
        ok = ~np.isnan(want)
        err = np.abs(got[rows][ok] - want[ok])
        print("terrain {} rows {} max err {:.3e}".format(t, len(rows), err.max()))
        assert (err <= 1e-6 + 2e-7 * np.abs(want[ok])).all(), (t, err.max())
        assert np.array_equal(np.isnan(got[rows]), np.isnan(want))
        # the per-terrain calls of the existing entry points: same cells, same adjoint
        hf, mp, dxdy = (T(x) for x in case.terrains[t])
        p1 = T(case.points[rows].reshape(1, -1, 3)).requires_grad_(True)
        grid = terrain_util.HfGrid(hf.unsqueeze(0), dxdy, DEV)
        _, cell1 = terrain_util._points_hf_sdf_launch(p1, hf.unsqueeze(0), mp.unsqueeze(0), grid, -10.0, kw["inverted"], kw["radius"], True)
        assert np.array_equal(cell[rows].reshape(-1), cell1.cpu().numpy().reshape(-1)), t
        o1 = terrain_util.points_hf_sdf(p1, hf.unsqueeze(0), mp.unsqueeze(0), dxdy, base_z=-10.0, grid=grid, **kw)
        o1.backward(T(case.g_out[rows].reshape(1, -1)))
        g1 = p1.grad.cpu().numpy().reshape(len(rows), case.K, 3)
        gerr, scale = np.abs(grad[rows] - g1).max(), np.abs(g1).max()
        print("terrain {} adjoint err {:.3e} bound {:.3e}".format(t, gerr, 2e-5 * scale))
        assert gerr <= 2e-5 * scale, (t, gerr, scale)
    for r in case.bad_rows:
        assert np.isnan(got[r]).all() and (cell[r] == -1).all() and (grad[r] == 0.0).all()
    assert np.isnan(got[case.nan_at])


def test_ragged_query_beyond_the_old_row_limit(oracle):
    """70 000 rows of one point each on two terrains (parc_points_hf_sdf takes at most 65 535 rows)"""
    from parc_amd.util import terrain_util
    case = mh.RaggedCase()
    rng = np.random.default_rng(2)
    R = 70000
    pts = np.stack([rng.uniform(-1, 10, size=R), rng.uniform(-1, 5, size=R), rng.uniform(-3, 3, size=R)], axis=-1).astype(np.float32).reshape(R, 1, 3)
    rt = np.where(np.arange(R) % 2 == 0, 0, 2).astype(np.int32)
    table = terrain_util.HfTable([_subterrain(*t) for t in case.terrains], base_z=-10.0, device=DEV)
    out = terrain_util.points_hf_sdf_ragged(T(pts), torch.tensor(rt, device=DEV), table, inverted=True).cpu().numpy().reshape(-1)
    for t in (0, 2):
        rows = np.nonzero(rt == t)[0]
        hf, mp, dxdy = (T(x) for x in case.terrains[t])
        one = terrain_util.points_hf_sdf(T(pts[rows].reshape(1, -1, 3)), hf.unsqueeze(0), mp.unsqueeze(0), dxdy).cpu().numpy().reshape(-1)
        assert np.array_equal(out[rows], one), t
        sub = rows[-1500:]                                      # rows past 65 535 against the oracle
        want = oracle.points_hf_sdf(pts[sub].reshape(1, -1, 3), case.terrains[t][0][None], case.terrains[t][1][None], case.terrains[t][2]).reshape(-1)
        assert sub[-1] >= 69998 and (np.abs(out[sub] - want) <= 1e-6 + 2e-7 * np.abs(want)).all()


def _tt_device(case):
    """the Python surface of the seamed terms on a TtCase -> (sums [3, M], g_pos, g_r) numpy"""
    from parc_amd.tools.motion_opt import motion_optimization as mo
    pos, r = T(case.pos).requires_grad_(True), T(case.r).requires_grad_(True)
    got = mo._TemporalTermsSeg.apply(pos, r, T(case.sv), T(case.keep), T(case.pc), case.lim, torch.tensor(case.ss, device=DEV),
                                     torch.tensor(case.sf, device=DEV))
    got.backward(T(case.w))
    return got.detach().cpu().numpy(), pos.grad.cpu().numpy(), r.grad.cpu().numpy()


@pytest.mark.parametrize("B", [15, 3, 1])
def test_seamed_temporal_terms_device(B):
    """against the torch expressions of the single path, motion by motion, at the tolerances of test_temporal_terms_kernels_equal_torch"""
    lengths = (1, 2, 3, 4, 5, 37, 64, 1, 63)
    case = mh.TtCase(lengths, B, seed=30 + B)
    sums, g_pos, g_r = _tt_device(case)
    c, c2 = mh.C, mh.C2
    for m, T_ in enumerate(lengths):
        s = int(case.ss[m])
        sl = slice(s, s + T_)
        pos, r = T(case.pos[sl]).requires_grad_(True), T(case.r[sl][:T_ - 1]).requires_grad_(True)
        s_bv, keep, pc = T(case.sv[sl][:T_ - 1]), T(case.keep[sl][:T_ - 1]), T(case.pc[sl][:T_ - 1])
        v = pos[1:] - pos[:-1]
        e2 = torch.square(v - s_bv)
        smooth = e2.sum() + r.sum()
        slide = ((torch.sqrt((e2 * keep.unsqueeze(-1)).sum(-1) + c2) - c) * pc).sum() + ((torch.sqrt(r * keep + c2) - c) * pc).sum()
        acc = v[1:] - v[:-1]
        jl = torch.clamp(torch.linalg.vector_norm(acc[1:] - acc[:-1], dim=-1) - case.lim, min=0.0).sum()
        ref = torch.stack([smooth, slide, jl])
        close(T(sums[:, m]), ref.detach().cpu().numpy(), atol=1e-4, rtol=2e-5)
        ref.backward(T(case.w[:, m]))
        for name, a, b in (("g_pos", g_pos[sl], pos.grad.cpu().numpy()), ("g_r", g_r[sl][:T_ - 1], r.grad.cpu().numpy())):
            if b.size:
                err = np.abs(a - b).max()
                assert err <= 3e-5 * max(np.abs(b).max(), 1.0), (m, T_, name, err)
        assert (g_r[s + T_ - 1] == 0.0).all()
        if T_ >= 37:
            assert float(jl.detach()) > 0
    # nothing crosses a seam: motion 5 moved by 100 m (one frame NaN) leaves every other motion bit-identical
    moved = mh.TtCase(lengths, B, seed=30 + B)
    a, b = int(moved.ss[5]), int(moved.ss[6])
    moved.pos[a:b] += np.float32(100.0)
    moved.pos[a + 3] = np.nan
    sums2, g_pos2, g_r2 = _tt_device(moved)
    others = np.arange(len(lengths)) != 5
    assert np.array_equal(sums[:, others], sums2[:, others]) and np.isnan(sums2[:, 5]).any()
    keep_rows = np.ones(case.N, bool)
    keep_rows[a:b] = False
    assert np.array_equal(g_pos[keep_rows], g_pos2[keep_rows]) and np.array_equal(g_r[keep_rows], g_r2[keep_rows])


def test_segment_sums_device_equals_the_host_order():
    """exact for small integers, an empty segment gives 0, and a motion's sum does not depend on where it is packed"""
    from parc_amd.tools.motion_opt import motion_optimization as mo
    rng = np.random.default_rng(3)
    W, ss = 7, [0, 600, 600, 641, 646]
    ints = rng.integers(-8, 9, size=(3, 646, W)).astype(np.float32)
    out = mo.segment_sums(T(ints), torch.tensor(ss, dtype=torch.int32, device=DEV), 4).cpu().numpy()
    for m in range(4):
        assert np.array_equal(out[:, m], ints[:, ss[m]:ss[m + 1]].sum(axis=(1, 2)))
    frac = rng.normal(size=(3, 646, W)).astype(np.float32)
    packed = mo.segment_sums(T(frac), torch.tensor(ss, dtype=torch.int32, device=DEV), 4).cpu().numpy()
    alone = mo.segment_sums(T(frac[:, 600:641]), torch.tensor([0, 41], dtype=torch.int32, device=DEV), 1).cpu().numpy()
    assert np.array_equal(packed[:, 2], alone[:, 0])


# ------------------------------------------------------------------------------------------------------------------ the optimiser
class _Batch:
    """the three test motions as the arguments of the batch functions"""

    def __init__(self, km):
        from parc_amd.tools.motion_opt import motion_optimization as mo
        self.g = g = golden("g20_motion_opt")
        self.pts, _, self.w, self.max_jerk = _problem(g)
        self.mo, self.km = mo, km
        self.motions = mh.three_motions(g)
        self.src = [T(m["frames"]) for m in self.motions]
        self.tgt = [T(m["tgt"]) for m in self.motions]
        self.con = [T(m["contacts"]) for m in self.motions]
        self.ter = [_subterrain(m["hf"], m["min_point"], m["dxdy"]) for m in self.motions]
        self.bc = [mh.constraints_from_rows(m["rows"], km.get_num_joints(), DEV) for m in self.motions]

    def pick(self, ids):
        return dict(src_frames=[self.src[i] for i in ids], contacts=[self.con[i] for i in ids], terrains=[self.ter[i] for i in ids],
                    body_constraints=[self.bc[i] for i in ids])

    def descend(self, ids, use_graph):
        trace = []
        out = self.mo.motion_contact_optimization_batch(body_points=self.pts, char_model=self.km, num_iters=40, step_size=0.001, max_jerk=self.max_jerk,
                                                        exp_names=["m%d" % i for i in ids], use_wandb=False, log_files=[None] * len(ids),
                                                        use_graph=use_graph, verbose=False, loss_trace=trace, **self.pick(ids), **self.w)
        assert len(out) == len(ids) and trace[0].shape == (40, len(ids))
        return [o.cpu().numpy() for o in out], trace[0].cpu().numpy()

    def evaluate(self, tgt):
        totals, terms, grads = self.mo.motion_terrain_contact_loss_batch(tgt, body_points=self.pts, char_model=self.km, max_jerk=self.max_jerk,
                                                                         **self.pick([0, 1, 2]), **self.w)
        return totals.cpu().numpy(), terms.cpu().numpy(), [x.cpu().numpy() for x in grads]


@pytest.fixture(scope="module")
def batch(km):
    return _Batch(km)


@pytest.fixture(scope="module")
def abc_runs(batch):
    """the batch (A, B, C) descended once eagerly and once as a replayed graph - shared, not modified"""
    return {use_graph: batch.descend([0, 1, 2], use_graph) for use_graph in (False, True)}


def test_loss_terms_and_gradient_at_the_start(batch):
    mo, km, g = batch.mo, batch.km, batch.g
    totals, terms, grads = batch.evaluate(batch.tgt)
    assert terms.shape == (9, 3) and totals.shape == (3,)
    for m in range(3):
        a, b, c = (batch.tgt[m][:, 0:3].clone().requires_grad_(True), batch.tgt[m][:, 3:6].clone().requires_grad_(True),
                   batch.tgt[m][:, 6:].clone().requires_grad_(True))
        loss, ld = mo.motion_terrain_contact_loss(a, b, c, *_source_terms(km, batch.src[m]), batch.con[m], batch.ter[m], batch.pts, km,
                                                  body_constraints=batch.bc[m], max_jerk=batch.max_jerk, **batch.w)
        loss.backward()
        for k, key in enumerate(mo._TERM_ORDER):
            r = ld[key]
            print("motion {} {:22s} batch {:.9g} single {:.9g}".format(m, key.name, terms[k, m], r))
            assert abs(terms[k, m] - r) <= 2e-4 * max(abs(r), 1e-2), (m, key, terms[k, m], r)
        assert abs(totals[m] - loss.item()) <= 2e-4 * abs(loss.item()), (m, totals[m], loss.item())
        ref = torch.cat([a.grad, b.grad, c.grad], dim=-1).cpu().numpy()
        err, scale = np.abs(grads[m] - ref).max(), np.abs(ref).max()
        print("motion {} gradient err {:.3e} bound {:.3e}".format(m, err, 3e-5 * scale))
        assert err <= 3e-5 * scale, (m, err, scale)
    # motion A inside the batch against the reference's own terms
    ref_terms = dict(zip([mo.LossType(int(i)) for i in g["full_term_ids"]], g["full_terms"]))
    for k, key in enumerate(mo._TERM_ORDER):
        assert abs(terms[k, 0] - ref_terms[key]) <= 2e-4 * max(abs(ref_terms[key]), 1e-2), (key, terms[k, 0], ref_terms[key])
    assert abs(totals[0] - float(g["full_loss"])) <= 2e-4 * abs(float(g["full_loss"]))


def test_descent_of_40_iterations_eager_and_replayed(batch, abc_runs):
    g = batch.g
    ref = g["opt_loss_trace"]
    moved = np.abs(g["opt_frames"] - g["src_frames"]).max()
    for use_graph, (outs, trace) in abc_runs.items():
        got = trace[:, 0]
        rel = np.abs(got - ref) / ref
        print("graph {} first {:.3e} max {:.3e}".format(use_graph, rel[0], rel.max()))
        assert rel[0] < 2e-4 and rel.max() < 2e-2, (use_graph, rel[0], rel.max())
        d = np.abs(outs[0] - g["opt_frames"])
        assert np.median(d) < 0.05 * moved and np.quantile(d, 0.9) < 0.25 * moved, (use_graph, moved, np.median(d), np.quantile(d, 0.9))
        assert [o.shape for o in outs] == [(40, 34), (12, 34), (4, 34)] and np.isfinite(trace).all()
        assert (trace[-1] < trace[0]).all()
    for m in range(3):
        diff = np.abs(abc_runs[True][1][:, m] - abc_runs[False][1][:, m]).max()
        assert diff <= 2e-3 * abc_runs[False][1][0, m], (m, diff)


def test_motions_descend_independently(batch, abc_runs):
    inside = abc_runs[True][1]
    alone = {}
    for m in range(3):
        alone[m] = batch.descend([m], True)
        diff = np.abs(alone[m][1][:, 0] - inside[:, m]).max()
        print("motion {} alone vs inside {:.3e} bound {:.3e}".format(m, diff, 2e-3 * inside[0, m]))
        assert diff <= 2e-3 * inside[0, m], (m, diff)
    trace = []
    batch.mo.motion_contact_optimization(src_frames=batch.src[0], contacts=batch.con[0], body_points=batch.pts, terrain=batch.ter[0], char_model=batch.km,
                                         num_iters=40, step_size=0.001, body_constraints=batch.bc[0], max_jerk=batch.max_jerk, exp_name="a", use_wandb=False,
                                         log_file=None, use_graph=True, verbose=False, loss_trace=trace, **batch.w)
    single = trace[0].cpu().numpy()
    diff = np.abs(alone[0][1][:, 0] - single).max()
    assert diff <= 2e-3 * single[0], diff
    # two evaluations that differ only in motion C's frames (moved by 100 m, one frame NaN): A and B do not notice
    t1, _, g1 = batch.evaluate(batch.tgt)
    bad = batch.tgt[2].clone()
    bad[:, 0:2] += 100.0
    bad[2] = float("nan")
    t2, terms2, g2 = batch.evaluate([batch.tgt[0], batch.tgt[1], bad])
    assert np.array_equal(g1[0], g2[0]) and np.array_equal(g1[1], g2[1])
    assert np.array_equal(t1[:2], t2[:2]) and np.isnan(t2[2]) and np.isfinite(t1).all()


def _kernel_count(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name])


def test_launches_per_iteration_do_not_depend_on_m(batch):
    """one evaluation (forward, per-motion terms, backward) of (A) and of (A, B, C): the same number of kernel launches"""
    mo = batch.mo
    counts = {}
    for ids in ([0], [0, 1, 2]):
        prob = mo._BatchProblem(char_model=batch.km, body_points=batch.pts, **batch.pick(ids))
        w = mo._weights(**batch.w)
        fr = prob.frames
        params = [fr[:, 0:3].clone().requires_grad_(True), fr[:, 3:6].clone().requires_grad_(True), fr[:, 6:34].clone().requires_grad_(True)]
        terms = torch.zeros((9, len(ids)), device=DEV)
        run = lambda: prob.evaluate(params[0], params[1], params[2], w, batch.max_jerk, terms)
        run()                                                   # makes the constant cotangents, as the warm-up iterations do
        counts[len(ids)] = _kernel_count(run)
    print("kernel launches per evaluation:", counts)
    assert counts[1] == counts[3] and counts[1] > 20, counts


@pytest.mark.parametrize("use_graph", [False, True])
def test_capture_protocol_of_the_shared_driver(use_graph):
    """_descend with a stub iteration that adds 1 to a one-element device counter: the counter ends at num_iters on both sides of the
    three warm-up iterations (3 never captures; 4 captures and replays once) - a capture records and does not run"""
    from parc_amd.tools.motion_opt import motion_optimization as mo
    for num_iters in (0, 1, 3, 4, 10):
        counter = torch.zeros(1, dtype=torch.int64, device=DEV)
        record = torch.zeros((1 + len(mo._TERM_ORDER), 1), dtype=torch.float32, device=DEV)
        mo._descend(lambda: counter.add_(1), num_iters, use_graph, record, [mo.build_logger(None)], False, 0.0)
        assert counter.item() == num_iters, (use_graph, num_iters, counter.item())


def test_logs_go_to_each_motions_own_file(batch, tmp_path):
    files = [str(tmp_path / ("log_%d.txt" % m)) for m in range(3)]
    trace = []
    batch.mo.motion_contact_optimization_batch(body_points=batch.pts, char_model=batch.km, num_iters=30, step_size=0.001, max_jerk=batch.max_jerk,
                                               exp_names=["a", "b", "c"], use_wandb=False, log_files=files, verbose=False, loss_trace=trace,
                                               **batch.pick([0, 1, 2]), **batch.w)
    tr = trace[0].cpu().numpy()
    for m, f in enumerate(files):
        lines = [ln.split("\t") for ln in open(f).read().split("\n") if ln.strip()]
        head = lines[0]
        assert head == ["Iteration", "Time (min)", "TOTAL WEIGHTED LOSS"] + [k.name for k in batch.mo._TERM_ORDER], head      # the single path's keys
        assert [int(float(r[0])) for r in lines[1:]] == [0, 25]
        for row, it in zip(lines[1:], (0, 25)):
            total = float(row[2])
            assert abs(total - tr[it, m]) <= 1e-6 * abs(tr[it, m]), (m, it, total, tr[it, m])
            terms = [float(v) for v in row[3:]]
            w = [batch.w[n] for n in ("w_root_pos", "w_root_rot", "w_joint_rot", "w_smoothness", "w_penetration", "w_contact", "w_sliding", "w_jerk",
                                      "w_body_constraints")]
            assert abs(sum(a * b for a, b in zip(w, terms)) - total) <= 1e-5 * abs(total)


def test_body_constraints_batch(batch):
    from parc_amd.util import torch_util
    mo, km, g = batch.mo, batch.km, batch.g
    ids = [0, 1]
    rp = [batch.src[i][:, 0:3].contiguous() for i in ids]
    rq = [torch_util.exp_map_to_quat(batch.src[i][:, 3:6]) for i in ids]
    jr = [km.dof_to_rot(batch.src[i][:, 6:].contiguous()) for i in ids]
    con = [batch.con[i] for i in ids]
    ter = [batch.ter[i] for i in ids]
    got = mo.compute_approx_body_constraints_batch(rp, rq, jr, con, km, ter)
    rows_of = lambda bc: np.array([[b, c.start_frame_idx, c.end_frame_idx] + c.constraint_point.tolist() for b, lst in enumerate(bc) for c in lst]).reshape(-1, 6)
    for k, i in enumerate(ids):
        one = rows_of(mo.compute_approx_body_constraints(rp[k], rq[k], jr[k], con[k], km, ter[k]))
        have = rows_of(got[k])
        assert have.shape == one.shape and len(one) >= 2
        assert np.array_equal(have[:, 0:3], one[:, 0:3])                  # bodies and frame ranges: exact
        err = np.abs(have[:, 3:6] - one[:, 3:6]).max()
        print("motion {} constraint points err {:.3e}".format(i, err))
        assert err < 2e-4, err
    ref = g["body_constraints"]
    have = rows_of(got[0])
    assert have.shape == ref.shape and np.array_equal(have[:, 0:3], ref[:, 0:3]) and np.abs(have[:, 3:6] - ref[:, 3:6]).max() < 2e-4


def test_driver_with_opt_batch_size(km, tmp_path):
    """opt_batch_size: 2 writes the same files, keys and shapes as the loop, and frames that agree with the loop's in the bulk"""
    import yaml
    from parc_amd import synthetic
    from parc_amd.assets import humanoid_spec
    from parc_amd.tools.motion_opt import optimize_motions
    from parc_amd.util import safe_pickle, terrain_util
    src = tmp_path / "src"
    src.mkdir()
    entries = []
    for k, clip in enumerate(synthetic.make_dataset(num_clips=2, seed=21, frames_range=(40, 50), tile_cells_range=(12, 16))):
        ter = terrain_util.SubTerrain.from_arrays(clip["hf"], clip["min_point"], clip["dxdy"], device="cpu").numpy_copy()
        path = str(src / ("clip_%d.pkl" % k))
        terrain_util.dump_reference_pickle({"fps": 30, "loop_mode": "CLAMP", "frames": clip["frames"], "contacts": clip["contacts"], "terrain": ter}, path)
        entries.append({"file": path, "weight": 1.0})
    (tmp_path / "motions.yaml").write_text(yaml.safe_dump({"motions": entries}))
    outs = {}
    for name, extra in (("loop", {}), ("batch", {"opt_batch_size": 2})):
        cfg = {"motions_yaml_path": str(tmp_path / "motions.yaml"), "device": DEV, "char_model": humanoid_spec.write_mjcf(),
               "output_folder_path": str(tmp_path / name) + "/", "num_iters": 40, "step_size": 0.001, "w_root_pos": 1.0, "w_root_rot": 10.0,
               "w_joint_rot": 1.0, "w_smoothness": 10.0, "w_penetration": 1000.0, "w_contact": 1000.0, "w_sliding": 10.0, "w_body_constraints": 1000.0,
               "w_jerk": 1000.0, "max_jerk": 1000.0, "use_wandb": False, "auto_compute_body_constraints": True, "frame_stride": 1,
               "char_point_samples": {"sphere_num_subdivisions": 0, "box_num_slices": 2, "box_dim_x": 3, "box_dim_y": 6, "capsule_num_circle_points": 4,
                                      "capsule_num_sphere_subdivisions": 0, "capsule_num_cylinder_slices": 4}}
        cfg.update(extra)
        (tmp_path / (name + ".yaml")).write_text(yaml.safe_dump(cfg))
        optimize_motions.main(["optimize_motions.py", "--config", str(tmp_path / (name + ".yaml"))])
        outs[name] = []
        for k in range(2):
            out = tmp_path / name / ("clip_%d_opt.pkl" % k)
            assert out.exists() and (tmp_path / name / "log" / ("log_clip_%d_opt.txt" % k)).exists()
            outs[name].append(safe_pickle.load_motion_file_safe(str(out)))
    for k in range(2):
        a, b = outs["loop"][k], outs["batch"][k]
        assert sorted(a.keys()) == sorted(b.keys()) and "opt:body_constraints" in b
        fa, fb = np.asarray(a["frames"]), np.asarray(b["frames"])
        assert fa.shape == fb.shape and np.asarray(a["contacts"]).shape == np.asarray(b["contacts"]).shape and a["fps"] == b["fps"]
        assert a["terrain"]["hf"].shape == b["terrain"]["hf"].shape
        assert [len(x) for x in a["opt:body_constraints"]] == [len(x) for x in b["opt:body_constraints"]]
        src_frames = safe_pickle.load_motion_file_safe(entries[k]["file"])["frames"]
        moved = np.abs(fa - np.asarray(src_frames)).max()
        d = np.abs(fa - fb)
        assert np.median(d) < 0.05 * moved and np.quantile(d, 0.9) < 0.25 * moved, (k, moved, np.median(d), np.quantile(d, 0.9))
