"""The generator's training-batch sampler on the device: parc_mdm_heightfields and parc_mdm_windows through the sampler's batch path,
against fixture G32 and the float64 restatement with the bounds of tests/test_mdm_sampler.py (2 e-bar each; exact: center_h, the mask,
the terrain cell each local point reads, contacts at on-frame start times), and against the loop path on the same draws."""
import os
import random
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tests", "tools"))
import mdm_batch_host as mh      # noqa: E402
import mdm_sampler_ref as msr    # noqa: E402
from test_mdm_sampler import EBAR_RECORDED      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2 * EBAR_RECORDED
KEYS = mh.OUT_KEYS


@pytest.fixture(scope="module")
def g32():
    return msr.load()


@pytest.fixture(scope="module")
def ref64(g32):
    z, meta = g32
    model, clips = msr.model_tables(z), msr.clip_tables(z, meta)
    return [msr.case64(z, meta, k, model, clips) for k in range(len(meta["cases"]))]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory, g32):
    from parc_amd.anim import kin_char_model, motion_lib
    ypath = mh.write_dataset(g32[0], g32[1], str(tmp_path_factory.mktemp("mdm_data")))
    km = kin_char_model.KinCharModel(DEV)
    km.load_char_file(kin_char_model.default_char_file())
    return motion_lib.MotionLib(ypath, km, DEV, contact_info=True)


def sampler(meta, k, dataset, **over):
    from parc_amd.diffusion import mdm_heightfield_contact_motion_sampler as ms
    return ms.MDMHeightfieldContactMotionSampler(mh.sampler_cfg(dict(meta["cases"][k]["cfg"], **over), dataset, DEV))


def inputs(a, rows=None):
    r = np.arange(len(a["ids"])) if rows is None else np.asarray(rows)
    return torch.tensor(a["ids"][r], device=DEV), torch.tensor(a["starts"][r], device=DEV), mh.case_draws(a, DEV, r)


def host(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def device_runs(g32, dataset):
    """every fixture case through the device entry points, once"""
    z, meta = g32
    runs = []
    for k in range(len(meta["cases"])):
        s = sampler(meta, k, dataset)
        assert s._path == "batch"
        runs.append(host(s.build_batch(*inputs(msr.case_arrays(z, k)), debug=True)))
    return runs


def test_device_equals_g32_and_float64(device_runs, g32, ref64):
    z, meta = g32
    for k, out in enumerate(device_runs):
        a, (o64, _) = msr.case_arrays(z, k), ref64[k]
        mh.check_case(k, out, a, o64, TOL, "device", exact_hfs=False)
        assert np.array_equal(out["cell_code"] & ((1 << 30) - 1), o64["cell"]) and np.array_equal((out["cell_code"] >> 30) & 1, o64["masked"]), k
        assert np.abs(out["pre"] - a["pre"]).max() <= TOL, k
        assert out["hfs"].shape[1:] == (len(a["grid_x"]), len(a["grid_y"]))


@pytest.mark.parametrize("n", [1, 6, 65])
def test_batch_sizes_and_mixed_clips(n, device_runs, g32, dataset):
    """n = 65 crosses a 64-lane boundary of the window kernel; case 0 mixes the four clips (ids 0 1 2 3 0 1): every row of a batch equals
    the row of the six-sample batch it repeats, bit for bit"""
    z, meta = g32
    a = msr.case_arrays(z, 0)
    assert set(a["ids"].tolist()) == {0, 1, 2, 3}
    rows = np.arange(n) % len(a["ids"])
    out = host(sampler(meta, 0, dataset).build_batch(*inputs(a, rows)))
    for key in KEYS:
        assert out[key].shape[0] == n and np.array_equal(out[key], device_runs[0][key][rows]), (n, key)


def test_batch_path_equals_loop_path_on_the_device(device_runs, g32, ref64, dataset):
    z, meta = g32
    for k in (0, 1, 2, 5, 8, 9):              # every mode, both z styles, the 1 x 1 grid excluded (8: 31 x 31, 9: long boxes)
        a = msr.case_arrays(z, k)
        s = sampler(meta, k, dataset)
        loop = host(s.loop_batch(*inputs(a)))
        unsafe = ref64[k][0]["unsafe"]
        for key in KEYS:
            d = np.abs(loop[key].astype(np.float64) - device_runs[k][key])
            if key == "hfs":
                d = np.where(unsafe, 0.0, d)
            assert d.max() <= TOL, (k, key, d.max())


def test_over_cap_batch_takes_the_loop_path(g32, dataset, capsys):
    """more boxes per sample than the kernels hold: PARC_EUNSUPPORTED before any launch, the loop path's result, one line in the log"""
    from parc_amd import _hip_mdm_batch as mb
    z, meta = g32
    s = sampler(meta, 0, dataset, max_num_boxes=mb.MAX_BOXES + 1)
    random.seed(3)
    torch.manual_seed(3)
    ids = torch.tensor([0, 1, 2], device=DEV)
    starts = torch.tensor([0.3, 0.2, 0.0], device=DEV)
    draws = s.make_draws(ids, starts)
    capsys.readouterr()
    got = host(s.run_batch(ids, starts, draws))
    assert s.last_path == "loop"
    s.run_batch(ids, starts, draws)
    assert capsys.readouterr().out.count("loop path") == 1
    want = host(s.loop_batch(ids, starts, draws))
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key
    ok = sampler(meta, 0, dataset, max_num_boxes=mb.MAX_BOXES)
    ok.run_batch(ids, starts, ok.make_draws(ids, starts))
    torch.cuda.synchronize()
    assert ok.last_path == "batch"


def test_two_batches_back_to_back(device_runs, g32, dataset):
    """two batches on one stream without a synchronisation between them give what each gives alone"""
    z, meta = g32
    s0, s3 = sampler(meta, 0, dataset), sampler(meta, 3, dataset)
    in0, in3 = inputs(msr.case_arrays(z, 0)), inputs(msr.case_arrays(z, 3))
    torch.cuda.synchronize()
    o0 = s0.build_batch(*in0)
    o3 = s3.build_batch(*in3)
    o0b = s0.build_batch(*in0)
    o0, o3, o0b = host(o0), host(o3), host(o0b)
    for key in KEYS:
        assert np.array_equal(o0[key], device_runs[0][key]) and np.array_equal(o3[key], device_runs[3][key]) and np.array_equal(o0b[key], o0[key]), key


def test_rows_behind_the_batch_stay_untouched(g32, dataset):
    """every output gets one more row, filled with a sentinel: the kernels leave it alone"""
    z, meta = g32
    for k in (0, 3):
        s = sampler(meta, k, dataset)
        big = []

        def alloc(shape, dtype=torch.float32):
            t = torch.full((shape[0] + 1,) + tuple(shape[1:]), -12345, dtype=dtype, device=DEV)
            big.append(t)
            return t[:shape[0]]

        s._alloc = alloc
        a = msr.case_arrays(z, k)
        out = s.build_batch(*inputs(a), debug=True)
        torch.cuda.synchronize()
        assert len(big) == 11
        for t in big:
            assert bool((t[-1] == -12345).all()) and not bool((t[:-1] == -12345).any())
        assert float(out["hfs"].abs().max()) <= 3.0
