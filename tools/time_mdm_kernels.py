#!/usr/bin/env python
"""Time the motion generator's kernels per launch: parc_mdm_loss_forward / _backward, parc_mdm_guide_step, parc_mdm_gen_encode / _decode
called directly, back to back, between two device events - no Python wrapper between launches, unlike tools/bench_mdm_{loss,guide,gen}.py,
whose host-clock figures are mostly wrapper time.  The workloads are those tools' (their build()).  To compare two revisions, run this
file in a checkout of each, alternately, on one machine.

usage: python tools/time_mdm_kernels.py [--only loss guide gen] [--launches 200] [--repeats 9] [--out times.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="+", default=["loss", "guide", "gen"], choices=["loss", "guide", "gen"])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print(json.dumps({"status": "not measured", "reason": "no device"}))
        return 0
    from parc_amd import _hip
    from parc_amd.diffusion.diffusion_util import MDMFrameType as T
    p, lib, dev, out = _hip.ptr, _hip.lib(), "cuda:0", {}

    def time_it(name, launch):
        for _ in range(30):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        out[name] = {"median_us": round(statistics.median(us), 3), "min_us": round(min(us), 3), "max_us": round(max(us), 3)}
        print(name, out[name], flush=True)

    def checked(fn, *args):
        def launch():
            rc = fn(*args)
            assert rc == 0, rc
        return launch

    def capture(name, call):
        """run call() once with lib.<name> replaced by a recorder -> (the entry point, its arguments, what call() returned: the
        tensors behind the arguments stay alive with it)"""
        real, got = getattr(lib, name), []

        def rec(*args):
            got.append(args)
            return real(*args)
        setattr(lib, name, rec)
        try:
            kept = call()
        finally:
            setattr(lib, name, real)
        assert len(got) == 1, len(got)
        return real, got[0], kept

    if "loss" in a.only:
        import bench_mdm_loss as bl
        for B in (64, 1024):
            L, _, true, x, hfs, td, _ = bl.build(dev, B, 7)
            S, km = int(x.shape[1]), L._char_model
            nb = km.get_num_joints()
            c, tab = L._device_cfg(S, 0, L._enabled_terms(true)), L._tables()
            f32 = lambda t, shape: t.detach().to(device=dev, dtype=torch.float32).reshape(shape).contiguous()
            tensors = (L._mdm_features_mean[:S].contiguous(), L._mdm_features_std[:S].contiguous(), f32(true[T.ROOT_POS], (B, S, 3)),
                       f32(true[T.ROOT_ROT], (B, S, 4)), f32(true[T.JOINT_ROT], (B, S, nb - 1, 4)), f32(true[T.CONTACTS], (B, S, nb)),
                       f32(hfs, (B, c.dim_x, c.dim_y)), f32(td, (B, 2)))
            args = [p(x)] + [p(t) for t in tensors] + [p(tab["grid_x"]), p(tab["grid_y"]), p(tab["points"]), p(tab["start"])]
            losses, g_x = torch.empty((14, B), dtype=torch.float32, device=dev), torch.empty_like(x)
            g = torch.full((14, B), 1.0 / B, dtype=torch.float32, device=dev)
            time_it("loss_fwd_B%d" % B, checked(lib.parc_mdm_loss_forward, _hip.stream(), km.c_struct(), c, B, *args, p(losses)))
            time_it("loss_bwd_B%d" % B, checked(lib.parc_mdm_loss_backward, _hip.stream(), km.c_struct(), c, B, *args, p(g), p(g_x)))
    if "guide" in a.only:
        import bench_mdm_guide as bg
        for B in (1, 64, 1024):
            G, _, x, gp, conds = bg.build(dev, B, 7)
            S, F = int(x.shape[1]), G._features
            reason, call = G._device_call(x, gp, conds, G._enabled(gp, conds))
            assert reason is None, reason
            c, target, hfs, points, start = call
            gx, gy = G._grid_points()
            mean, std = F._mdm_features_mean[:S].contiguous(), F._mdm_features_std[:S].contiguous()
            x_out, terms = torch.empty_like(x), torch.empty((5, B), dtype=torch.float32, device=dev)          # out of place: x stays as it is
            time_it("guide_step_B%d" % B, checked(lib.parc_mdm_guide_step, _hip.stream(), G._char_model.c_struct(), c, B, p(x), p(mean), p(std), p(hfs),
                                                  p(target), p(gx), p(gy), p(points), p(start), p(x_out), p(terms)))
    if "gen" in a.only:
        import bench_mdm_gen as bn
        for B in (1, 32, 4096):
            io, _, target, prev, terrain, settings, x = bn.build(dev, B, 7)
            enc, ea, kept = capture("parc_mdm_gen_encode", lambda: io.encode(target, prev, terrain, settings))
            assert io.last_path == "device", io.last_path_reason
            dec, da, kept2 = capture("parc_mdm_gen_decode", lambda: io.decode(kept[1], x))
            time_it("gen_encode_B%d" % B, checked(enc, *ea))
            time_it("gen_decode_B%d" % B, checked(dec, *da))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "launches": a.launches, "repeats": a.repeats, "per_launch": out}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
