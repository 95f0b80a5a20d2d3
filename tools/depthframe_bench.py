"""The metric-frame launch (rdm_depth_frames, include/rdm_depth.h) against the composed path it replaces, at the native 480x640 frame, B = 1 and
B = 8, both outputs, one process:
  (fused)     one launch: the map placed on the test transform's view of the frame, the DORN counts' scale, exp, float32 and uint16 planes;
  (composed)  the parent's operators: cp.resize of the log map to a float64 (B,1,480,640) frame (rdm_resize_bicubic_f64: the map stretched over
              the whole frame - the composed path has no view), add of the per-sample log scale, exp, cast to float32, divide by the unit, round, clamp
              and the integer cast, each a launch with its float64 intermediate.
Then the fused launch at split = 0 (the library's default) against fixed splits.  Every figure is the time per call of `reps` back-to-back calls
on one stream between two device events (host enqueue included: that is what a caller pays), taken in `rounds` rounds that alternate the
candidates; reported: median, minimum and maximum over the rounds.  Before timing, the fused float32 plane under the FULL view is compared with
the composed one on the timed input (within one float32 ulp) and the uint16 planes within one step.  `bytes` is what each path must move
through memory by its shapes: the fused launch reads the map and the counts and writes 6 bytes per pixel; the composed path also writes and
reads back its float64 intermediates.
One JSON line per figure.  `python tools/depthframe_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import depth, filler  # noqa: E402
from md_rdm_amd.dataloaders import nyu  # noqa: E402
from md_rdm_amd.network import computations as cp  # noqa: E402

H, W, UNIT = 480, 640, 1e-3


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                   # us per call


def alternate(cands, reps, rounds, warmup=3):
    """{name: [us per call, one per round]}: the candidates take turns inside every round."""
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(window(fn, reps))
    return out


def summary(v):
    return {"us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def traffic(B):
    """bytes by shape: (fused, composed)"""
    px, src = B * H * W, B * (128 * 128 * 8 + 64 * 8)
    fused = src + px * (4 + 2)
    composed = (B * 128 * 128 * 8 + px * 8                  # resize: map -> float64 frame
                + px * 16 + px * 16                         # add, exp: float64 in, float64 out
                + px * 12                                   # cast: float64 in, float32 out
                + px * 16 + px * 16 + px * 16               # divide, round, clamp
                + px * 10)                                  # integer cast: float64 in, uint16 out
    return fused, composed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--splits", type=int, nargs="*", default=[1, 2, 4, 8, 16, 32, 64, 128, 240, 480])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    view = nyu.test_view((H, W))
    try:                                                     # the composed path's last cast: uint16 where this torch copies to it, else int32
        torch.zeros(1, dtype=torch.float64, device=dev).to(torch.uint16)
        U = torch.uint16
    except (RuntimeError, TypeError):
        U = torch.int32
    for B in (1, 8):
        m = torch.from_numpy(filler.uniform("depthframe_bench.map/%d" % B, (B, 1, 128, 128), -1.5, 1.5).astype("float64")).to(dev)
        counts = torch.from_numpy((filler.unit("depthframe_bench.counts/%d" % B, B * 64) * 91).astype("int64").reshape(B, 1, 8, 8)).to(dev)
        ls = depth.sid_log_scale(counts)
        unit = torch.full((1,), UNIT, dtype=torch.float64, device=dev)

        def fused(split=0, v=view):
            return depth.metric_frames(m, (H, W), view=v, counts=counts, unit=UNIT, want=("f32", "u16"), split=split)

        def composed():
            d = torch.exp(cp.resize(m, (H, W)) + ls.view(B, 1, 1, 1))
            return d.float(), torch.round(d / unit).clamp(0.0, 65535.0).to(U)

        got, (f, u) = fused(v=None), composed()
        torch.cuda.synchronize()
        steps = (got["f32"].view(torch.int32) - f[:, 0].view(torch.int32)).abs().max().item()
        du = (got["u16"].to(torch.int32) - u[:, 0].to(torch.int32)).abs().max().item()
        assert steps <= 1 and du <= 1, "the fused planes under the full view differ from the composed ones: %d float32 steps, %d uint16 steps" % (steps, du)
        fb, cb = traffic(B)
        t = alternate({"fused": fused, "composed": composed}, args.reps, args.rounds)
        base = {"batch": B, "frame": [H, W], "outputs": ["f32", "u16"]}
        emit({"figure": "rdm_depth_frames, the test transform's view", **base, "bytes": fb, **summary(t["fused"])})
        emit({"figure": "composed: resize, add, exp, cast, divide, round, clamp, cast", **base, "bytes": cb, "last_cast": str(U), **summary(t["composed"])})
        cands = {"split 0": fused}
        for s in args.splits:
            cands["split %d" % s] = (lambda s_: lambda: fused(s_))(s)
        t = alternate(cands, args.reps, args.rounds)
        for k, v in t.items():
            emit({"figure": "rdm_depth_frames, " + k, **base, **summary(v)})
    if args.out:
        with open(args.out, "w") as fh:
            for d_ in lines:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
