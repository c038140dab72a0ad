"""The actor unit statistics behind one interface for tests/test_unit_stats*.py -- TEST INFRASTRUCTURE.

A run is K steps of parc_netstats_update from zero state: `widths` of the hidden layers, `weights_next[l]` = the weight matrix
[d_next, d_l] whose absolute column sums are S_l, `acts[k][l]` [N, d_l] and `means[k]` [N, A] as numpy float32.  It goes through the
host build of parc_netstats_core.h (netstats_host.cpp, compiled here), through the device (the C ABI of include/parc_netstats.h), or
through the stand-alone program built from the same file with -DNETSTATS_HOST_MAIN (plain or with -fsanitize=address,undefined), which
reads the run from a file.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from parc_amd import _hip_netstats as ns      # noqa: E402

SOURCE = os.path.join(HERE, "netstats_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Wno-missing-field-initializers"]
# the sanitizer runtimes are linked statically: the program then runs whatever else the environment preloads
SANITIZE = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
ETA, THRESHOLD = 0.99, 0.01
GAIN = 1.0 - ETA
PATTERN = np.float32(-1234.5)
c_vp, c_i64, c_int, c_f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float


def build_host(out_dir):
    lib = os.path.join(out_dir, "libparc_netstats_host.so")
    # -ffp-contract=off: the host build is the plain-fp32 evaluation of the header (no fused multiply-adds)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-fPIC", "-shared"] + FLAGS + ["-o", lib, SOURCE, "-lm"])
    return lib


def build_program(out_dir, sanitize=True):
    """the stand-alone program (its own main): `prog case_file [out_file]`"""
    exe = os.path.join(out_dir, "netstats_host_main" + ("_asan" if sanitize else ""))
    subprocess.check_call([os.environ.get("CXX", "g++")] + (SANITIZE if sanitize else ["-O2"]) + ["-ffp-contract=off", "-DNETSTATS_HOST_MAIN"] + FLAGS +
                          ["-o", exe, SOURCE, "-lm"])
    return exe


_libs = {}


def host_lib(path):
    if path not in _libs:
        L = ctypes.CDLL(path)
        L.netstats_workspace_floats_host.restype = c_i64
        L.netstats_workspace_floats_host.argtypes = [c_i64, ns.NetstatsTableS]
        L.netstats_update_host.restype = c_int
        L.netstats_update_host.argtypes = [c_i64, ns.NetstatsTableS, c_int, c_vp, c_vp, c_f, c_f, c_vp]
        L.netstats_abs_colsum_host.restype = c_int
        L.netstats_abs_colsum_host.argtypes = [c_int, c_int, c_vp, c_vp]
        L.netstats_dormant_count_host.restype = c_int
        L.netstats_dormant_count_host.argtypes = [ns.NetstatsTableS, c_i64, c_vp, c_f, c_vp]
        _libs[path] = L
    return _libs[path]


def aligned(n, dtype=np.float32, fill=0.0):
    """n elements whose first one sits on a 16-byte boundary"""
    raw = np.full(n + 4, fill, dtype)
    off = (-raw.ctypes.data % 16) // raw.itemsize
    return raw[off:off + n]


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def run_host(lib, widths, weights_next, acts, means, snapshots=False):
    """-> dict(rc, S, activations, utility, mean_net_acts, counts); with snapshots=True the three values are lists over the steps"""
    L = host_lib(lib)
    K, (N, A) = len(means), means[0].shape
    S = [aligned(d) for d in widths]
    for s, W in zip(S, weights_next):
        W = f32(W)
        assert L.netstats_abs_colsum_host(W.shape[0], W.shape[1], W.ctypes.data, s.ctypes.data) == 0
    act, util, mna = [aligned(d) for d in widths], [aligned(d) for d in widths], aligned(N * A)
    inp = [aligned(N * d) for d in widths]
    t = ns.table([(i.ctypes.data, d, s.ctypes.data, a.ctypes.data, u.ctypes.data) for i, d, s, a, u in zip(inp, widths, S, act, util)])
    need = L.netstats_workspace_floats_host(N, t)
    ws = aligned(max(int(need), 4))
    snaps = dict(activations=[], utility=[], mean_net_acts=[])
    rc = 0
    for k in range(K):
        for i, x in zip(inp, acts[k]):
            i[:] = f32(x).ravel()
        m = f32(means[k])
        rc = L.netstats_update_host(N, t, A, m.ctypes.data, mna.ctypes.data, ETA, GAIN, ws.ctypes.data)
        if rc != 0:
            break
        if snapshots:
            snaps["activations"].append([a.copy() for a in act])
            snaps["utility"].append([u.copy() for u in util])
            snaps["mean_net_acts"].append(mna.reshape(N, A).copy())
    counts = np.zeros(len(widths) + 1, np.int32)
    assert L.netstats_dormant_count_host(t, N * A, mna.ctypes.data, THRESHOLD, counts.ctypes.data) == 0
    out = dict(rc=rc, need=int(need), S=S, counts=counts)
    out.update(snaps if snapshots else dict(activations=act, utility=util, mean_net_acts=mna.reshape(N, A)))
    return out


def run_device(widths, weights_next, acts, means, snapshots=False, guard=64, misalign=None, workspace_floats=None):
    """The same run through parc_netstats_* on the GPU.  Every output (and the workspace) has `guard` float words of PATTERN before and
    behind it; they come back as out["guard"].  misalign = (field, layer): that pointer is moved on by one float (field in "act",
    "out_abs_sum", "activations", "utility", "workspace").  The run stops at the first call that does not return 0."""
    import torch
    from parc_amd import _hip
    dev = "cuda:0"
    L = _hip.lib()
    K, (N, A) = len(means), means[0].shape

    def guarded(n, fill=0.0):
        b = torch.full((n + 2 * guard,), float(PATTERN), dtype=torch.float32, device=dev)
        b[guard:guard + n] = fill
        return b

    def shift(field, l):
        return 4 if misalign == (field, l) else 0
    S_buf = [guarded(d + 1) for d in widths]        # (+ 1: room for the shifted pointer of the misaligned cases)
    for b, W, d in zip(S_buf, weights_next, widths):
        W = torch.tensor(f32(W), device=dev)
        assert W.shape[1] == d
        _hip.check(L.parc_netstats_abs_colsum(_hip.stream(), W.shape[0], d, _hip.ptr(W), ctypes.c_void_p(b.data_ptr() + 4 * guard)), "parc_netstats_abs_colsum")
    act_buf, util_buf, mna_buf = [guarded(d + 1) for d in widths], [guarded(d + 1) for d in widths], guarded(N * A)
    base = lambda b: b.data_ptr() + 4 * guard       # noqa: E731

    def table(act_ptrs):
        return ns.table([(p + shift("act", l) if p else 0, d, base(s) + shift("out_abs_sum", l), base(a) + shift("activations", l), base(u) + shift("utility", l))
                         for l, (p, d, s, a, u) in enumerate(zip(act_ptrs, widths, S_buf, act_buf, util_buf))])
    need = int(L.parc_netstats_workspace_floats(N, table([0] * len(widths))))
    n_ws = workspace_floats if workspace_floats is not None else max(need, 4)
    ws_buf = guarded(n_ws + 1, float(PATTERN))
    snaps = dict(activations=[], utility=[], mean_net_acts=[])
    rc = 0
    for k in range(K):
        x = [torch.tensor(np.concatenate([f32(a).ravel(), np.zeros(1, np.float32)]), device=dev) for a in acts[k]]
        m = torch.tensor(f32(means[k]), device=dev)
        rc = L.parc_netstats_update(_hip.stream(), N, table([t.data_ptr() for t in x]), A, _hip.ptr(m), ctypes.c_void_p(base(mna_buf)), ETA, GAIN,
                                    ctypes.c_void_p(base(ws_buf) + shift("workspace", 0)))
        torch.cuda.synchronize()
        if rc != 0:
            break
        if snapshots:
            snaps["activations"].append([b[guard:guard + d].cpu().numpy() for b, d in zip(act_buf, widths)])
            snaps["utility"].append([b[guard:guard + d].cpu().numpy() for b, d in zip(util_buf, widths)])
            snaps["mean_net_acts"].append(mna_buf[guard:guard + N * A].cpu().numpy().reshape(N, A))
    counts = torch.full((len(widths) + 1 + 2,), -7, dtype=torch.int32, device=dev)
    rc_count = L.parc_netstats_dormant_count(_hip.stream(), table([0] * len(widths)), N * A, ctypes.c_void_p(base(mna_buf)), THRESHOLD,
                                             ctypes.c_void_p(counts.data_ptr() + 4)) if misalign is None else 0
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    whole = [b.cpu().numpy() for b in act_buf + util_buf + [mna_buf, ws_buf]]
    sizes = list(widths) + list(widths) + [N * A, n_ws]
    out = dict(rc=rc, rc_count=rc_count, need=need, S=[b[guard:guard + d].cpu().numpy() for b, d in zip(S_buf, widths)], counts=counts[1:-1],
               counts_guard=counts[[0, -1]], guard=[np.concatenate([w[:guard], w[guard + n + 1:]]) for w, n in zip(whole, sizes)],
               workspace=whole[-1][guard:guard + n_ws])
    if snapshots:
        out.update(snaps)
    else:
        n = len(widths)
        out.update(activations=[w[guard:guard + d] for w, d in zip(whole[:n], widths)], utility=[w[guard:guard + d] for w, d in zip(whole[n:2 * n], widths)],
                   mean_net_acts=whole[2 * n][guard:guard + N * A].reshape(N, A))
    return out


def dump_case(path, widths, weights_next, acts, means):
    """the case file of the stand-alone program"""
    K, (N, A) = len(means), means[0].shape
    with open(path, "wb") as f:
        f.write(np.array([len(widths), N, A, K] + list(widths) + [0] * (ns.MAX_LAYERS - len(widths)), np.int32).tobytes())
        f.write(np.array([ETA, GAIN, THRESHOLD], np.float32).tobytes())
        for W in weights_next:
            f.write(f32(W).tobytes())
        for k in range(K):
            for a in acts[k]:
                f.write(f32(a).tobytes())
            f.write(f32(means[k]).tobytes())


def read_program_output(path, widths, N, A, K):
    raw = np.fromfile(path, dtype=np.float32)
    D = sum(widths)
    per = 2 * D + N * A
    assert raw.size == K * per + len(widths) + 1, (raw.size, K, per)
    steps = raw[:K * per].reshape(K, per)
    return dict(activations=steps[:, :D], utility=steps[:, D:2 * D], mean_net_acts=steps[:, 2 * D:].reshape(K, N, A), counts=raw[K * per:].astype(np.int32))
