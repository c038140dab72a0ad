"""The actor unit statistics on the GPU: the C ABI of include/parc_netstats.h at the smallest shapes that can break it (rows around the
64-row chunk, widths around the 256-column tile, 1 / 3 / 8 layers of unequal widths in one call, A = 4 and 28) against the float64
restatement of tests/unit_stats_ref.py and against fixture G29 (the reference's own test_model2), then the agent: test_model2,
unit_report, --mode test2 and the log_unit_stats key on a 32-env setup.

Tolerances are derived in unit_stats_ref: against float64 twice the bound, against the fixture's fp32 values one bound per side."""
import os

import numpy as np
import pytest
import torch
import yaml

import unit_stats_ref as ref
from test_unit_stats import check_against_fixture, fixture_run
from unit_stats_ref import nh

pytestmark = pytest.mark.gpu

# rows: 1, 2, 63, 64, 65, 130 (one row; below / at / above one chunk; three chunks with a ragged last one)
# dims: 4, 28, 252, 256, 260, 516 (one float4; below / at / above one 256-column tile; three tiles with a ragged last one)
CASES = [(1, [4], 4), (2, [28], 28), (63, [252], 4), (64, [256], 28), (65, [260], 4), (130, [516], 28),
         (1, [516], 28), (2, [260], 4), (63, [256], 28), (64, [252], 4), (65, [28], 28), (130, [4], 4),
         (65, [260, 28, 516], 28), (130, [4, 256, 252], 4), (64, [516, 4, 260], 4),
         (130, [4, 28, 252, 256, 260, 516, 8, 12], 28), (1, [516, 4, 260, 28, 256, 252, 12, 8], 4), (63, [8, 516, 12, 256, 4, 260, 28, 252], 28)]
K = 5
ZERO_COL = 1


def make_run(N, widths, A, steps=K, seed=0):
    """post-ReLU style activations (non-negative, half of them 0, column ZERO_COL of every layer all 0), clear of the subnormal range"""
    rng = np.random.default_rng(1000 * N + 10 * len(widths) + A + seed)
    acts = []
    for _ in range(steps):
        layer = []
        for d in widths:
            h = np.maximum(rng.standard_normal((N, d)), 0.0).astype(np.float32)
            h[:, 0] += np.float32(0.25)          # a column that fires in every row
            h[:, ZERO_COL] = 0.0
            layer.append(h)
        acts.append(layer)
    means = [rng.standard_normal((N, A)).astype(np.float32) for _ in range(steps)]
    weights_next = [rng.standard_normal((dn, d)).astype(np.float32) for d, dn in zip(widths, widths[1:] + [A])]
    return acts, means, weights_next


@pytest.fixture(scope="module")
def ratios():
    return []


@pytest.mark.parametrize("N,widths,A", CASES, ids=["r%d-%s-a%d" % (n, "x".join(map(str, w)), a) for n, w, a in CASES])
def test_update_against_float64_after_1_and_5_steps(N, widths, A, ratios):
    acts, means, weights_next = make_run(N, widths, A)
    out = nh.run_device(widths, weights_next, acts, means, snapshots=True)
    assert out["rc"] == 0 and out["rc_count"] == 0 and out["need"] == -(-N // 64) * sum(widths)
    S64 = [ref.abs_colsum64(W) for W in weights_next]
    for l, W in enumerate(weights_next):
        ref.check_rel(out["S"][l], S64[l], 2 * W.shape[0] * ref.U, "S_%d" % l, ratios)
    st = ref.State64(widths, N, A)
    for k in range(K):
        st.step(acts[k], means[k], S64)
        if k + 1 not in (1, K):
            continue
        for l in range(len(widths)):
            ref.check_rel(out["activations"][k][l], st.activations[l], 2 * ref.bound_activations(N, k + 1), "step %d activations L%d" % (k + 1, l), ratios)
            ref.check_rel(out["utility"][k][l], st.utility[l], 2 * ref.bound_utility(N, weights_next[l].shape[0], k + 1), "step %d utility L%d" % (k + 1, l),
                          ratios)
            assert out["activations"][k][l][ZERO_COL] == 0.0 and out["utility"][k][l][ZERO_COL] == 0.0        # never fired: exactly 0
            assert out["activations"][k][l][0] > 0.0
        ref.check_rel(out["mean_net_acts"][k], st.mean_net_acts, 2 * ref.bound_mean_net(k + 1), "step %d mean net" % (k + 1), ratios)
    want = [ref.dormant64(a) for a in st.activations] + [ref.dormant64(st.mean_net_acts)]
    assert list(out["counts"]) == want and (out["counts_guard"] == -7).all()
    for g in out["guard"]:
        assert (g == nh.PATTERN).all()          # nothing written before or behind any output, nor around the workspace


def test_fixture_end_to_end(ratios):
    fx = ref.load_fixture()
    widths, weights_next, acts, means = fixture_run(fx)
    out = nh.run_device(widths, weights_next, acts, means, snapshots=True)
    assert out["rc"] == 0
    worst = {}
    st = check_against_fixture(fx, out, "device", worst)
    ratios.extend(worst.values())
    assert list(out["counts"]) == [ref.dormant64(a) for a in st.activations] + [ref.dormant64(st.mean_net_acts)]


def test_two_runs_give_identical_bits():
    N, widths, A = 130, [4, 28, 252, 256, 260, 516, 8, 12], 28
    acts, means, weights_next = make_run(N, widths, A)
    a, b = (nh.run_device(widths, weights_next, acts, means) for _ in range(2))
    for key in ("activations", "utility", "S"):
        for x, y in zip(a[key], b[key]):
            assert x.tobytes() == y.tobytes()
    assert a["mean_net_acts"].tobytes() == b["mean_net_acts"].tobytes() and a["workspace"].tobytes() == b["workspace"].tobytes()


@pytest.mark.parametrize("widths,misalign", [([8, 6], None), ([6], None), ([8, 12], ("act", 1)), ([8, 12], ("out_abs_sum", 0)), ([8, 12], ("activations", 1)),
                                             ([8, 12], ("utility", 0)), ([8, 12], ("workspace", 0))])
def test_refused_calls_write_nothing(widths, misalign):
    """a dim of 6 or a pointer that is not 16-byte aligned: PARC_EINVAL, and neither the outputs, the workspace nor the words around them change"""
    N, A = 65, 4
    acts, means, weights_next = make_run(N, widths, A, steps=1)
    out = nh.run_device(widths, weights_next, acts, means, misalign=misalign, workspace_floats=2 * sum(widths))
    assert out["rc"] == -1
    for g in out["guard"]:
        assert (g == nh.PATTERN).all()
    assert (out["workspace"] == nh.PATTERN).all() and (out["mean_net_acts"] == 0.0).all()
    for v in out["activations"] + out["utility"]:
        assert (v == 0.0).all()


# ------------------------------------------------------------------------------------------------ the agent, on the 32-env setup of the drop-in test
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from parc_amd.assets import humanoid_spec
    from parc_amd.envs.ig_parkour.default_config import default_agent_config, default_env_config
    from test_dropin_gpu import _write_dataset
    tmp = str(tmp_path_factory.mktemp("unit_stats"))
    motions = _write_dataset(tmp)
    env_cfg = default_env_config(char_file=humanoid_spec.write_mjcf(), motion_file=motions, terrain_save_path=os.path.join(tmp, "terrain.pkl"))
    env_yaml = os.path.join(tmp, "dm_env.yaml")
    with open(env_yaml, "w") as f:
        yaml.safe_dump(env_cfg, f)

    def agent_yaml(name, **kw):
        cfg = default_agent_config()
        cfg.update(steps_per_iter=8, update_epochs=1, iters_per_output=1, iters_per_checkpoint=1000, test_episodes=32)
        cfg.update(kw)
        path = os.path.join(tmp, name)
        with open(path, "w") as f:
            yaml.safe_dump(cfg, f)
        return path
    return dict(tmp=tmp, env_yaml=env_yaml, agent_yaml=agent_yaml)


def test_agent_test_model2_report(setup):
    from parc_amd.envs import env_builder
    from parc_amd.learning import agent_builder
    from parc_amd.util import util
    util.set_rand_seed(0)
    env = env_builder.build_env(setup["env_yaml"], 32, "cuda:0", False)
    agent = agent_builder.build_agent(setup["agent_yaml"]("plain.yaml"), env, "cuda:0")
    assert agent.unit_report() is None and agent._unit_stats is None
    tap, kept = [], {}
    agent._unit_stats_tap = tap           # the test-only tap: (hidden activations, mean) of every step
    off = agent._unit_stats_off

    def keep_then_off(ranks=None):
        kept["st"] = agent._unit_stats
        off(ranks)
    agent._unit_stats_off = keep_then_off
    info2 = agent.test_model2(32)
    st = kept["st"]
    rep = agent.unit_report()
    assert agent._unit_stats is None and rep["steps"] == len(tap) == st.steps and len(tap) >= 1
    # the statistics are off again: test_model goes down the path it always took (the tapped forward is never called), and returns the same keys
    agent._model.eval_actor_tapped = None
    del agent._unit_stats_tap
    info = agent.test_model(32)
    assert sorted(info2.keys()) == sorted(info.keys()) and info2["num_eps"] >= 32
    assert agent._unit_stats is None and agent.unit_report() is rep

    # float64 recomputation from what the agent tapped during the run
    widths, N, A, steps = st.widths, 32, st.num_actions, len(tap)
    assert widths == [2048, 1024, 512] and st.mean_net_acts.shape == (N, A)
    lins = [m for m in agent._model._actor_layers if isinstance(m, torch.nn.Linear)] + [agent._model._action_dist._mean_net]
    S64 = [ref.abs_colsum64(lin.weight.detach().cpu().numpy()) for lin in lins[1:]]
    s64 = ref.State64(widths, N, A)
    for acts, mean in tap:
        s64.step([a.cpu().numpy() for a in acts], mean.cpu().numpy(), S64)
    thr = ref.THRESHOLD

    def count_between(v64, got):
        """exact wherever no value sits within 1e-4 of the threshold; the rollout's values are not ours to choose, so a value inside the
        margin may fall on either side"""
        lo, hi = int((v64 < thr * (1 - ref.MARGIN)).sum()), int((v64 < thr * (1 + ref.MARGIN)).sum())
        assert lo <= got <= hi, (lo, got, hi)

    def moments_close(got, v32, what):
        """the report's mean / std / max / min against float64 moments of the SAME fp32 vector: max and min exact, the mean of d
        non-negative fp32 values within (d + 2) u relative, the std within (d + 4) u of the largest value"""
        m = ref.moments64(v32)
        d, top = v32.size, float(np.abs(v32).max())
        assert got["max"] == m["max"] and got["min"] == m["min"], what
        assert abs(got["mean"] - m["mean"]) <= (d + 2) * ref.U * abs(m["mean"]) + 1e-45, (what, got["mean"], m["mean"])
        assert abs(got["std"] - m["std"]) <= (d + 4) * ref.U * top + 1e-45, (what, got["std"], m["std"])
    for l, d in enumerate(widths):
        a32, u32 = st.activations[l].cpu().numpy(), st.utility[l].cpu().numpy()
        ref.check_rel(a32, s64.activations[l], 2 * ref.bound_activations(N, steps), "agent activations L%d" % l)
        ref.check_rel(u32, s64.utility[l], 2 * ref.bound_utility(N, lins[l + 1].weight.shape[0], steps), "agent utility L%d" % l)
        y = rep["layers"][l]
        assert y["num_units"] == d and y["num_dormant"] == int((a32 < np.float32(thr)).sum()) and y["percent_dormant"] == y["num_dormant"] / d * 100.0
        count_between(s64.activations[l], y["num_dormant"])
        moments_close(y["activation"], a32, "activation L%d" % l)
        moments_close(y["utility"], u32, "utility L%d" % l)
    m32 = st.mean_net_acts.cpu().numpy()
    ref.check_rel(m32, s64.mean_net_acts, 2 * ref.bound_mean_net(steps), "agent mean net")
    mn = rep["mean_net"]
    count_between(s64.mean_net_acts, mn["num_dormant"])
    assert mn["num_rows"] == N and mn["num_entries"] == N * A and mn["percent_dormant"] == mn["num_dormant"] / N * 100.0
    assert mn["fraction_dormant"] == mn["num_dormant"] / (N * A) and 0.0 <= mn["fraction_dormant"] <= 1.0
    moments_close(mn["activation"], m32, "mean net")
    # the rank figures, and plain Python numbers all the way down
    for r, lin in zip(rep["ranks"]["layers"] + [rep["ranks"]["mean_net"]], lins):
        S = np.linalg.svd(lin.weight.detach().cpu().numpy().astype(np.float64), compute_uv=False)
        assert r["max_rank"] == len(S) and r["stable_rank"] == ref.stable_rank64(S) and r["avg_weight_mag"] > 0

    def plain(x):
        return all(plain(v) for v in x.values()) if isinstance(x, dict) else all(plain(v) for v in x) if isinstance(x, list) else type(x) in (int, float)
    assert plain(rep)


def _header(path):
    with open(path) as f:
        return f.readline().rstrip("\n").split("\t")


def test_run_main_mode_test2_and_training_log_columns(setup, capsys):
    from parc_amd import run as parc_run
    tmp = setup["tmp"]
    base = ["run.py", "--env_config", setup["env_yaml"], "--num_envs", "32", "--device", "cuda:0", "--visualize", "False", "--rand_seed", "0"]
    parc_run.main(base + ["--agent_config", setup["agent_yaml"]("t2.yaml"), "--mode", "test2", "--test_episodes", "32"])
    text = capsys.readouterr().out
    for line in ("Max possible rank of layer 0 : 1312", "Stable rank of mean_net:", "layer 2", "Percentage dormant units:", "Utility min:",
                 "Mean Net Number of dormant units:", "Mean Return:", "Episodes:"):
        assert line in text, line
    # two training iterations with a test rollout after each: the new columns with the key, exactly the other columns without it
    logs = {}
    for name, kw in (("on", dict(log_unit_stats=True)), ("off", dict()), ("false", dict(log_unit_stats=False))):
        logs[name] = os.path.join(tmp, "log_%s.txt" % name)
        parc_run.main(base + ["--agent_config", setup["agent_yaml"]("train_%s.yaml" % name, **kw), "--mode", "train", "--max_samples", str(2 * 8 * 32),
                              "--out_model_file", os.path.join(tmp, "model_%s.pt" % name), "--log_file", logs[name]])
    new = ["Dormant_Pct_L0", "Act_Mean_L0", "Util_Mean_L0", "Dormant_Pct_L1", "Act_Mean_L1", "Util_Mean_L1", "Dormant_Pct_L2", "Act_Mean_L2",
           "Util_Mean_L2", "Dormant_Pct_MeanNet"]
    on, plain = _header(logs["on"]), _header(logs["off"])
    assert plain == _header(logs["false"]) and not [c for c in plain if c.startswith(("Dormant_", "Act_Mean", "Util_Mean"))]
    assert [c for c in on if c in new] == new and [c for c in on if c not in new] == plain
    rows = np.loadtxt(logs["on"], skiprows=1, ndmin=2)
    assert rows.shape == (2, len(on))
    col = {c: rows[:, i] for i, c in enumerate(on)}
    assert ((col["Dormant_Pct_L0"] >= 0) & (col["Dormant_Pct_L0"] <= 100)).all() and (col["Act_Mean_L0"] > 0).all() and (col["Util_Mean_L2"] > 0).all()
    assert ((col["Dormant_Pct_MeanNet"] >= 0) & (col["Dormant_Pct_MeanNet"] <= 100.0 * 28)).all()
