"""Independent float64 restatement of the actor unit statistics (include/parc_netstats.h; learning/dm_ppo_agent.py:683-736 of the
reference), with plain loops -- TEST INFRASTRUCTURE for tests/test_unit_stats*.py -- and the error bounds the tests hold the code to.

Bounds (derived, not measured).  u = 2^-24.  Every summand is non-negative (post-ReLU activations, absolute weights, running values
that start at 0), so relative errors never cancel:
  * a column mean over N rows errs by at most (N + 1) u relative in any summation order (N - 1 additions, the division, |.| exact);
  * S_l = sum of d_next absolute weights errs by at most d_next u;
  * one running update multiplies the old value by eta and adds: 2 u on the old term per step, hence 2 K u after K steps; the new
    term takes the gain, one or two products and the addition: at most 4 u (activations) or 6 u (utility, with S_l).
So after K steps against float64, relative:  activations (N + 5 + 2 K) u,  utility (N + d_next + 7 + 2 K) u,  and the mean net's running
value (its input |mean| is exact: N = 0) (5 + 2 K) u.  Tests allow TWICE these (second-order terms; eta = 0.99 rounded to fp32 adds
K u).  A comparison of two fp32 evaluations (the fixture) gets one bound per side.  A unit that never fires gives exactly 0.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import netstats_host as nh  # noqa: E402,F401  (the host build and the device call behind one interface)

U = 2.0 ** -24
ETA = 0.99
THRESHOLD = 0.01
MARGIN = 1e-4


def bound_activations(N, K):
    return (N + 5 + 2 * K) * U


def bound_utility(N, d_next, K):
    return (N + d_next + 7 + 2 * K) * U


def bound_mean_net(K):
    return (5 + 2 * K) * U


def abs_colsum64(W):
    """S[j] = sum_i |W[i, j]|"""
    W = np.asarray(W, np.float64)
    S = np.zeros(W.shape[1])
    for i in range(W.shape[0]):
        S = S + np.abs(W[i])
    return S


class State64:
    def __init__(self, widths, N, A):
        self.activations = [np.zeros(d) for d in widths]
        self.utility = [np.zeros(d) for d in widths]
        self.mean_net_acts = np.zeros((N, A))
        self.steps = 0

    def step(self, acts, mean, S):
        """acts[l] [N, d_l], mean [N, A], S[l] [d_l] (float64)"""
        for l, H in enumerate(acts):
            H = np.asarray(H, np.float64)
            total = np.zeros(H.shape[1])
            for r in range(H.shape[0]):
                total = total + H[r]
            m = np.abs(total / H.shape[0])
            self.activations[l] = ETA * self.activations[l] + (1.0 - ETA) * m
            self.utility[l] = ETA * self.utility[l] + ((1.0 - ETA) * m) * S[l]
        self.mean_net_acts = ETA * self.mean_net_acts + (1.0 - ETA) * np.abs(np.asarray(mean, np.float64))
        self.steps += 1


def dormant64(v):
    """count below the threshold, after asserting that no value sits within the margin of it"""
    v = np.asarray(v, np.float64)
    assert (np.abs(v / THRESHOLD - 1.0) > MARGIN).all(), "a value sits within 1e-4 of the threshold: the count is not well defined"
    return int((v < THRESHOLD).sum())


def stable_rank64(S):
    S = [float(s) for s in S]
    total, run = sum(S), 0.0
    for k, s in enumerate(S):
        run += s
        if run / total > 0.99:
            return k
    return 0


def moments64(v):
    v = np.asarray(v, np.float64).ravel()
    return {"mean": float(v.mean()), "std": float(v.std(ddof=1)) if v.size > 1 else float("nan"), "max": float(v.max()), "min": float(v.min())}


def check_rel(got, want, bound, what, ratios=None):
    """|got - want| <= bound * want element-wise (want >= 0); want == 0 demands got == 0.  Prints the largest error-to-bound ratio, and
    appends it to `ratios`."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    zero = want == 0.0
    assert (got[zero] == 0.0).all(), (what, "a unit that never fired is not exactly 0")
    live = ~zero
    assert (want[live] > 1e-30).all(), (what, "inputs must stay clear of the subnormal range")
    ratio = float((np.abs(got[live] - want[live]) / (bound * want[live])).max()) if live.any() else 0.0
    print("{}: largest error / bound = {:.4f} (bound {:.3e} relative)".format(what, ratio, bound))
    if ratios is not None:
        ratios.append(ratio)
    assert ratio <= 1.0, (what, ratio)
    return ratio


_fixture = None


def load_fixture():
    """G29 (tests/golden/gen_unit_stats.py): the reference's own running values after each of 400 steps"""
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(HERE, "golden", "g29_unit_stats.npz"))
        fx = {k: z[k] for k in z.files}
        fx["widths"] = [int(d) for d in fx["widths"]]
        fx["K"], fx["N"], fx["A"] = fx["mean"].shape
        _fixture = fx
    return _fixture


def split(v, widths):
    out, off = [], 0
    for d in widths:
        out.append(np.ascontiguousarray(v[..., off:off + d]))
        off += d
    return out
