"""Depth-map rendering (rdm_viz_rows_u8, md_rdm_amd.viz) at B = 8, 128x128 maps to 480x640, one process:
  one panel    viz.colorize(pred, size=(480, 640))           against the composed path on the same device: cp.resize, amin / amax per image,
               the normalisation, a torch gather from the 256-entry table and the cast to uint8;
  three panels viz.comparison_rows(x, target, pred)          against the same chain for two maps with a joint range, the input scaled and cast,
               and the concatenation of the three panels;
  and the fused launch with a fixed range (no first sweep) and at --split 1 2 4 ... (workgroups per image), automatic range.
Time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included), in `rounds` rounds that alternate
the candidates; reported: median, minimum and maximum over the rounds, and for the fused launch the effective bytes per second (maps read once
+ image written once).  Before timing, fused and composed are compared on the timed input (the composed index is computed in float64 like the
kernel's, so the bytes are equal).  One JSON line per figure.  `timeout 600 python tools/viz_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, filler, viz  # noqa: E402
from md_rdm_amd.network import computations as cp  # noqa: E402

B, H, W = 8, 480, 640


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                   # us per call


def alternate(cands, measure, rounds, warmup=3):
    for fn in cands.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, fn in cands.items():
            out[k].append(measure(fn))
    return out


def summary(v):
    return {"us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def jet_table(dev):
    """the kernel's table, read back through the kernel: the 256 bin centres over [0, 1]"""
    ramp = ((torch.arange(256, dtype=torch.float64, device=dev) + 0.5) / 256.0).reshape(1, 1, 1, 256)
    return viz.colorize(ramp, 0.0, 1.0).reshape(256, 3)


def composed_colour(maps, lut, lo, hi):
    xa = (maps - lo) / (hi - lo) * 256.0
    idx = xa.clamp(0, 255).long()                            # (xa == 256 -> 255, below 0 -> 0; the timed inputs hold no NaN)
    return lut[idx.squeeze(1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    pred = torch.from_numpy(filler.uniform("viz-bench-pred", (B, 1, 128, 128), -1.0, 2.0, dtype=np.float64)).to(dev)
    target = torch.from_numpy(filler.log_uniform("viz-bench-target", (B, 1, 128, 128), 0.2, 4.0, dtype=np.float64)).to(dev)
    x = torch.from_numpy(filler.synthetic_batch(B, H, W)[0]).to(dev)
    lut = jet_table(dev)

    def composed1():
        r = cp.resize(pred, (H, W))
        lo, hi = r.amin(dim=(1, 2, 3), keepdim=True), r.amax(dim=(1, 2, 3), keepdim=True)
        return composed_colour(r, lut, lo, hi)

    def composed3():
        rt, rp = cp.resize(target, (H, W)), cp.resize(pred, (H, W))
        lo = torch.minimum(rt.amin(dim=(1, 2, 3), keepdim=True), rp.amin(dim=(1, 2, 3), keepdim=True))
        hi = torch.maximum(rt.amax(dim=(1, 2, 3), keepdim=True), rp.amax(dim=(1, 2, 3), keepdim=True))
        rgb = (255.0 * x).permute(0, 2, 3, 1).to(torch.uint8)
        return torch.cat([rgb, composed_colour(rt, lut, lo, hi), composed_colour(rp, lut, lo, hi)], dim=2)

    def fused1():
        return viz.colorize(pred, size=(H, W))

    def fused1_fixed():
        return viz.colorize(pred, -1.0, 2.0, size=(H, W))

    def fused3():
        return viz.comparison_rows(x, target, pred)

    emit({"figure": "fused vs composed bytes on the timed input", "batch": B, "one_panel_equal": bool(torch.equal(fused1(), composed1())),
          "three_panels_equal": bool(torch.equal(fused3(), composed3()))})

    def one_split(s):
        return lambda: viz.render_rows(None, None, pred, H, W, split=s)

    cands = {"composed1": composed1, "fused1": fused1, "fused1_fixed": fused1_fixed, "composed3": composed3, "fused3": fused3}
    splits = (1, 2, 4, 8, 16, 32, 64, 128)
    cands.update({"fused1_split%d" % s: one_split(s) for s in splits})
    t = alternate(cands, lambda fn: window(fn, args.reps), args.rounds)
    bytes1 = B * (128 * 128 * 8 + H * W * 3)
    bytes3 = B * (2 * 128 * 128 * 8 + 3 * H * W * 4 + 3 * H * W * 3)
    c1, f1, ff, c3, f3 = (summary(t[k]) for k in ("composed1", "fused1", "fused1_fixed", "composed3", "fused3"))
    emit({"figure": "one panel, composed: resize, amin, amax, normalise, gather, cast", "batch": B, **c1})
    emit({"figure": "one panel, fused launch (automatic range: two sweeps)", "batch": B, **f1, "speedup_vs_composed": round(c1["us"] / f1["us"], 2),
          "effective_GB_per_s": round(bytes1 / f1["us"] * 1e-3, 1)})
    emit({"figure": "one panel, fused launch, fixed range (one sweep)", "batch": B, **ff, "effective_GB_per_s": round(bytes1 / ff["us"] * 1e-3, 1)})
    emit({"figure": "three panels, composed", "batch": B, **c3})
    emit({"figure": "three panels, fused launch (automatic range)", "batch": B, **f3, "speedup_vs_composed": round(c3["us"] / f3["us"], 2),
          "effective_GB_per_s": round(bytes3 / f3["us"] * 1e-3, 1)})
    for s in splits:
        emit({"figure": "one panel, fused launch, automatic range, workgroups per image", "split": s, **summary(t["fused1_split%d" % s])})
    emit({"figure": "launches per call (rdm_launch_count)", "fused": int(_count(fused3))})
    if args.out:
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


def _count(fn):
    L = _lib.lib()
    n = L.rdm_launch_count()
    fn()
    return L.rdm_launch_count() - n


if __name__ == "__main__":
    main()
