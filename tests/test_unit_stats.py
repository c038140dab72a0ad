"""The actor unit statistics (include/parc_netstats.h, run mode test2) on the CPU: the host build of parc_netstats_core.h
(tests/tools/netstats_host.cpp) against fixture G29 - the reference's own test_model2 - at every one of its 400 snapshots and against
the float64 restatement of tests/unit_stats_ref.py, the same run under AddressSanitizer / UBSan in a stand-alone program, the rank
figures, the argument rules through the real library, the launcher's argument parsing, and the documentation of the exports.

Tolerances are derived in unit_stats_ref: against float64 twice the bound, against the fixture's fp32 values one bound per side.
tests/test_unit_stats_gpu.py runs the device through the same cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import unit_stats_ref as ref
from unit_stats_ref import nh

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    return nh.build_host(str(tmp_path_factory.mktemp("netstats_host")))


@pytest.fixture(scope="module")
def fx():
    return ref.load_fixture()


def fixture_run(fx):
    """G29 as the arguments of nh.run_host / run_device / dump_case"""
    widths = fx["widths"]
    weights_next = [fx["weight%d" % (l + 1)] for l in range(len(widths))]
    acts = [ref.split(fx["hidden"][k], widths) for k in range(fx["K"])]
    return widths, weights_next, acts, list(fx["mean"])


def check_against_fixture(fx, out, what, ratios=None):
    """every snapshot against float64 (twice the bound) and against the reference's fp32 values (one bound per side); dormant counts
    and never-fired units exact.  `out` holds snapshots per step."""
    widths, N, A, K = fx["widths"], fx["N"], fx["A"], fx["K"]
    d_next = widths[1:] + [A]
    S64 = [ref.abs_colsum64(fx["weight%d" % (l + 1)]) for l in range(len(widths))]
    st = ref.State64(widths, N, A)
    worst = dict(act=0.0, util=0.0, mean=0.0)
    for k in range(K):
        st.step(ref.split(fx["hidden"][k], widths), fx["mean"][k], S64)
        steps = k + 1
        fa, fu = ref.split(fx["activations"][k], widths), ref.split(fx["utility"][k], widths)
        for l in range(len(widths)):
            ba, bu = ref.bound_activations(N, steps), ref.bound_utility(N, d_next[l], steps)
            for got, want, fixt, b, key in ((out["activations"][k][l], st.activations[l], fa[l], ba, "act"), (out["utility"][k][l], st.utility[l], fu[l], bu, "util")):
                want = np.asarray(want)
                live = want > 0
                assert (np.asarray(got)[~live] == 0.0).all() and (fixt[~live] == 0.0).all()
                e64 = np.abs(got[live] - want[live]) / (2 * b * want[live])
                efx = np.abs(got[live].astype(np.float64) - fixt[live]) / (2 * b * want[live])
                worst[key] = max(worst[key], float(e64.max()))
                assert e64.max() <= 1.0 and efx.max() <= 1.0, (what, k, l, key, e64.max(), efx.max())
        bm = ref.bound_mean_net(steps)
        got, want = out["mean_net_acts"][k].astype(np.float64), st.mean_net_acts
        live = want > 0
        assert (got[~live] == 0.0).all()
        e64 = np.abs(got[live] - want[live]) / (2 * bm * want[live])
        efx = np.abs(got[live] - fx["mean_net_acts"][k][live]) / (2 * bm * want[live])
        worst["mean"] = max(worst["mean"], float(e64.max()))
        assert e64.max() <= 1.0 and efx.max() <= 1.0, (what, k, "mean net", e64.max(), efx.max())
    print("{}: largest error / allowed over {} snapshots: activations {:.4f} utility {:.4f} mean net {:.4f}".format(what, K, worst["act"], worst["util"], worst["mean"]))
    if ratios is not None:
        ratios.update(worst)
    # the end of the run: a never-fired unit per layer, dormant and live units in every layer, counts exact (margin asserted in float64)
    for l in range(len(widths)):
        assert (st.activations[l] == 0.0).any()
        n = ref.dormant64(st.activations[l])
        assert 0 < n < widths[l] and n == int((np.asarray(out["activations"][-1][l]) < ref.THRESHOLD).sum())
    return st


def test_host_core_on_fixture_at_every_snapshot(hostlib, fx):
    widths, weights_next, acts, means = fixture_run(fx)
    out = nh.run_host(hostlib, widths, weights_next, acts, means, snapshots=True)
    assert out["rc"] == 0 and out["need"] == sum(widths)
    for l, W in enumerate(weights_next):
        ref.check_rel(out["S"][l], ref.abs_colsum64(W), 2 * W.shape[0] * ref.U, "host S_%d" % l)
    st = check_against_fixture(fx, out, "host build")
    want = [ref.dormant64(a) for a in st.activations] + [ref.dormant64(st.mean_net_acts)]
    assert list(out["counts"]) == want
    assert fx["mean_net_acts"].shape == (fx["K"], fx["N"], fx["A"])          # the reference's value is per env and action


def test_host_core_many_rows_and_layers(hostlib):
    """more than one chunk (rows 130 = 64 + 64 + 2), 8 layers of unequal widths, an all-zero column"""
    rng = np.random.default_rng(5)
    widths, N, A, K = [4, 28, 252, 256, 260, 8, 12, 516], 130, 28, 3
    acts = [[np.maximum(rng.standard_normal((N, d)), 0).astype(np.float32) + np.float32(0.01) for d in widths] for _ in range(K)]
    for k in range(K):
        acts[k][2][:, 7] = 0.0
    means = [rng.standard_normal((N, A)).astype(np.float32) for _ in range(K)]
    weights_next = [rng.standard_normal((dn, d)).astype(np.float32) for d, dn in zip(widths, widths[1:] + [A])]
    out = nh.run_host(hostlib, widths, weights_next, acts, means)
    assert out["rc"] == 0 and out["need"] == 3 * sum(widths)
    S64 = [ref.abs_colsum64(W) for W in weights_next]
    st = ref.State64(widths, N, A)
    for k in range(K):
        st.step(acts[k], means[k], S64)
    for l, d in enumerate(widths):
        ref.check_rel(out["activations"][l], st.activations[l], 2 * ref.bound_activations(N, K), "host rows 130 activations L%d" % l)
        ref.check_rel(out["utility"][l], st.utility[l], 2 * ref.bound_utility(N, weights_next[l].shape[0], K), "host rows 130 utility L%d" % l)
    assert out["activations"][2][7] == 0.0 and out["utility"][2][7] == 0.0
    ref.check_rel(out["mean_net_acts"], st.mean_net_acts, 2 * ref.bound_mean_net(K), "host rows 130 mean net")


def test_sanitized_program_runs_the_fixture(tmp_path, hostlib, fx):
    """parc_netstats_core.h under AddressSanitizer and UBSan in a stand-alone program (its own main): all 400 steps of G29; its
    snapshots equal the plain build's bit for bit."""
    exe = nh.build_program(str(tmp_path), sanitize=True)
    widths, weights_next, acts, means = fixture_run(fx)
    f, o = str(tmp_path / "g29.case"), str(tmp_path / "g29.out")
    nh.dump_case(f, widths, weights_next, acts, means)
    res = subprocess.run([exe, f, o], capture_output=True, text=True)
    assert res.returncode == 0 and "netstats ok" in res.stdout, (res.returncode, res.stderr[-2000:])
    got = nh.read_program_output(o, widths, fx["N"], fx["A"], fx["K"])
    want = nh.run_host(hostlib, widths, weights_next, acts, means, snapshots=True)
    for k in range(fx["K"]):
        assert np.array_equal(got["activations"][k], np.concatenate(want["activations"][k]))
        assert np.array_equal(got["utility"][k], np.concatenate(want["utility"][k]))
        assert np.array_equal(got["mean_net_acts"][k], want["mean_net_acts"][k])
    assert np.array_equal(got["counts"], want["counts"])


def test_rank_figures_on_fixture_and_by_hand(fx):
    import torch
    from parc_amd.learning import unit_stats
    for i in range(len(fx["widths"]) + 1):
        r = unit_stats.rank_figures(torch.tensor(fx["weight%d" % i]))
        S = np.linalg.svd(fx["weight%d" % i].astype(np.float64), compute_uv=False)
        assert r["max_rank"] == int(fx["max_rank"][i]) == len(S)
        assert r["stable_rank"] == int(fx["stable_rank"][i]) == ref.stable_rank64(S)
        assert abs(r["avg_weight_mag"] - float(fx["avg_weight_mag"][i])) <= 1e-12 * float(fx["avg_weight_mag"][i])
    # singular values 50, 30, 15, 4, 1 (sum 100): the cumulative share is 0.5, 0.8, 0.95, 0.99, 1 -> 0.99 is not > 0.99, index 4 crosses
    W = torch.zeros(5, 7, dtype=torch.float64)
    for i, s in enumerate((50.0, 30.0, 15.0, 4.0, 1.0)):
        W[i, i + 1] = -s if i % 2 else s
    r = unit_stats.rank_figures(W)
    assert r == {"max_rank": 5, "stable_rank": 4, "avg_weight_mag": 100.0 / 35.0}
    # 60, 39.5, 0.5: 0.6, 0.995 -> index 1;  one singular value: 1 > 0.99 at index 0
    assert unit_stats.stable_rank([60.0, 39.5, 0.5]) == 1 and unit_stats.stable_rank([3.0]) == 0
    lines = unit_stats.rank_lines({"layers": [r], "mean_net": r})
    assert lines[0] == "Max possible rank of layer 0 : 5" and lines[1] == "Stable rank of layer 0 : 4" and lines[4] == "Stable rank of mean_net: 4"


def test_networks_that_do_not_fit_are_refused():
    import torch
    from parc_amd.learning import dm_ppo_model, unit_stats

    class M:
        pass

    def model(widths, std=dm_ppo_model.StdType.FIXED, extra=None):
        m = M()
        mods, i = [], 12
        for d in widths:
            mods += [torch.nn.Linear(i, d), torch.nn.ReLU()]
            i = d
        m._actor_layers = torch.nn.Sequential(*(mods + ([extra] if extra else [])))
        m._action_dist = M()
        m._action_dist._std_type = std
        m._action_dist._mean_net = torch.nn.Linear(i, 4)
        return m
    unit_stats.check_model(model([20, 12, 8]))
    with pytest.raises(ValueError, match="multiples of 4"):
        unit_stats.check_model(model([20, 10]))
    with pytest.raises(ValueError, match="state-dependent"):
        unit_stats.check_model(model([20, 12], std=dm_ppo_model.StdType.VARIABLE))
    with pytest.raises(ValueError, match="at most 8"):
        unit_stats.check_model(model([8] * 9))
    with pytest.raises(ValueError, match="Linear \\+ ReLU"):
        unit_stats.check_model(model([8, 8], extra=torch.nn.Tanh()))


def test_argument_errors_through_the_library():
    """the entry points answer before any HIP call: no GPU is needed to be refused"""
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip, _hip_netstats as ns
    L = _hip.lib()
    assert L.parc_netstats_abi() == 1 and L.parc_abi_version() == 1
    P = 0x1000          # never dereferenced: every call below is refused

    def table(dims, **ptrs):
        return ns.table([(ptrs.get("act", P), d, ptrs.get("out_abs_sum", P), ptrs.get("activations", P), ptrs.get("utility", P)) for d in dims])

    def update(rows=5, dims=(8, 4), A=4, mean=P, mna=P, ws=P, **ptrs):
        return L.parc_netstats_update(None, rows, table(dims, **ptrs), A, mean, mna, 0.99, 0.01, ws)
    for kw in (dict(rows=0), dict(rows=-3), dict(dims=()), dict(dims=(4,) * 9), dict(dims=(8, 6)), dict(dims=(0,)), dict(dims=(-4,)), dict(A=0),
               dict(mean=None), dict(mna=None), dict(ws=None), dict(ws=P + 4), dict(act=None), dict(act=P + 4), dict(out_abs_sum=None),
               dict(out_abs_sum=P + 8), dict(activations=None), dict(activations=P + 4), dict(utility=None), dict(utility=P + 12)):
        assert update(**kw) == -1, kw
    assert update(rows=64 * 65535 + 1) == -2
    assert L.parc_netstats_workspace_floats(130, table((8, 4))) == 3 * 12 and L.parc_netstats_workspace_floats(64, table((8, 4))) == 12
    assert L.parc_netstats_workspace_floats(0, table((8,))) == -1 and L.parc_netstats_workspace_floats(5, table((6,))) == -1
    assert L.parc_netstats_workspace_floats(5, table(())) == -1
    for args in ((0, 4, P, P), (3, 0, P, P), (3, 4, None, P), (3, 4, P, None)):
        assert L.parc_netstats_abs_colsum(None, *args) == -1, args
    for t, n, m, c in ((table(()), 4, P, P), (table((8,)), -1, P, P), (table((8,)), 4, None, P), (table((8,)), 4, P, None), (table((0,)), 4, P, P),
                       (table((8,), activations=None), 4, P, P), (table((8,)), 2 ** 31, P, P)):
        assert L.parc_netstats_dormant_count(None, t, n, m, 0.01, c) == -1


def test_load_args_accepts_mode_test2():
    from parc_amd import run
    args = run.load_args(["run.py", "--mode", "test2", "--test_episodes", "32", "--num_envs", "8"])
    assert args.parse_string("mode", "train") == "test2" and args.parse_int("test_episodes", 16) == 32


def test_every_export_is_declared_listed_and_documented():
    with open(os.path.join(REPO, "include", "parc_netstats.h")) as f:
        names = sorted(set(re.findall(r"\b(parc_netstats_[a-z_]+)\s*\(", f.read())))
    assert names == ["parc_netstats_abi", "parc_netstats_abs_colsum", "parc_netstats_dormant_count", "parc_netstats_update", "parc_netstats_workspace_floats"]
    import __graft_entry__ as ge
    ge.build()
    from parc_amd import _hip
    L = _hip.lib()
    with open(os.path.join(REPO, "INTEGRATION.md")) as f:
        doc = f.read()
    for n in names:
        assert n in _hip.EXPORTED and hasattr(L, n) and n in doc, n
    assert isinstance(L.parc_netstats_update, ctypes._CFuncPtr) and "parc_netstats.hip" in _hip.SOURCES
