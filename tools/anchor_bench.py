"""The three anchor launches (include/rdm_anchor.h: cell sums, fit and field, corrected frames) against the composed torch path they replace, one
process, B = 8 and B = 1, a 480x640 and a 226x226 frame, anchors dense with holes (about 70 % valid) and sparse (about 0.2 % valid):
  (fused)     anchor.fit (rdm_depth_anchor_cells + rdm_depth_anchor_field) and anchor.metric_frames (rdm_depth_frames_corrected), the output
              allocations of the wrappers included, as a caller pays them; the three launches are also timed one by one through the C entry points;
  (composed)  single operators: cp.resize of the log map to a float64 (B,1,h,w) frame, log of the anchors, the validity mask, the residuals,
              avg_pool2d (ceil_mode, divisor 1 = sums) for the cell sums and counts, the mean, the re-centring, two conv2d passes with the Gaussian
              taps (zero padding) on each of the two planes, the division, F.interpolate (bilinear, align_corners=False) of the field to whole cells and a crop to the
              frame, add, exp, cast to float32.
Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included), taken in
`rounds` rounds that alternate the candidates; reported: median, minimum and maximum over the rounds.  Before timing, the fused log scale is
compared with the composed one (1e-9) and the fused float32 plane with the composed one (relative 1e-3 away from the frame's border cells: the
composed bilinear resize clamps like the kernel, but its sums run in another order).
One JSON line per figure.  `python tools/anchor_bench.py [--out profiles/anchor_bench.jsonl]`"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, anchor, filler  # noqa: E402
from md_rdm_amd.network import computations as cp  # noqa: E402

CELL, SIGMA, LAM = 16, 2.0, 1.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    rg = int(math.ceil(3 * SIGMA))
    g = torch.tensor([math.exp(-(k * k) / (2 * SIGMA * SIGMA)) for k in range(-rg, rg + 1)], dtype=torch.float64, device=dev)
    for (h, w) in ((480, 640), (226, 226)):
        for B in (8, 1):
            for density, share in (("dense with holes", 0.7), ("sparse", 0.002)):
                key = "anchor_bench/%d/%d/%d/%s" % (h, w, B, density)
                m = torch.from_numpy(filler.uniform(key + "/map", (B, 1, 128, 128), -1.5, 1.5).astype("float64")).to(dev)
                off = torch.from_numpy(filler.uniform(key + "/off", (B, h, w), -0.2, 0.6).astype("float64")).to(dev)
                keep = torch.from_numpy(filler.unit(key + "/keep", B * h * w).reshape(B, h, w) < share).to(dev)
                a = torch.where(keep, torch.exp(cp.resize(m, (h, w))[:, 0] + off), torch.zeros((), dtype=torch.float64, device=dev)).float()
                prior = torch.full((B,), 0.1, dtype=torch.float64, device=dev)
                gy, gx = -(-h // CELL), -(-w // CELL)

                def fused():
                    f = anchor.fit(m, a, prior=prior, cell=CELL, sigma=SIGMA, lam=LAM)
                    return f, anchor.metric_frames(m, (h, w), f)["f32"]

                def composed():
                    v = cp.resize(m, (h, w))[:, 0]
                    ok = torch.isfinite(a) & (a > 0)
                    r = torch.where(ok, torch.log(torch.where(ok, a, torch.ones_like(a)).double()) - v - prior.view(B, 1, 1), torch.zeros_like(v))
                    pool = lambda t: F.avg_pool2d(t[:, None], CELL, ceil_mode=True, divisor_override=1, count_include_pad=False)
                    s, n = pool(r), pool(ok.double())
                    cnt = n.sum(dim=(1, 2, 3))
                    delta = torch.where(cnt > 0, s.sum(dim=(1, 2, 3)) / cnt.clamp(min=1), torch.zeros_like(cnt))
                    sp = s - n * delta.view(B, 1, 1, 1)
                    sm = lambda t: F.conv2d(F.conv2d(t, g.view(1, 1, 1, -1), padding=(0, rg)), g.view(1, 1, -1, 1), padding=(rg, 0))
                    field = sm(sp) / (sm(n) + LAM)
                    c = F.interpolate(field, size=(gy * CELL, gx * CELL), mode="bilinear", align_corners=False)[:, 0, :h, :w]      # whole cells, so that the scale is 1 / CELL
                    return prior + delta, torch.exp(v + (prior + delta).view(B, 1, 1) + c).float()

                (f, plane), (ls, ref) = fused(), composed()
                torch.cuda.synchronize()
                assert (f["log_scale"] - ls).abs().max().item() < 1e-9, "the fused log scale differs from the composed one"
                inner = (slice(None), slice(CELL, h - 2 * CELL), slice(CELL, w - 2 * CELL))
                rel = ((plane[inner] - ref[inner]).abs() / ref[inner]).max().item()
                assert rel < 1e-3, "the fused float32 plane differs from the composed one by %g" % rel

                n_c = torch.empty(B, gy, gx, dtype=torch.int32, device=dev)
                s_c = torch.empty(B, gy, gx, dtype=torch.float64, device=dev)
                ls_o, cnt_o = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
                fld, out = torch.empty(B, gy, gx, dtype=torch.float64, device=dev), torch.empty(B, h, w, dtype=torch.float32, device=dev)
                st = _lib.stream()
                one = {
                    "rdm_depth_anchor_cells": lambda: _lib.check(L.rdm_depth_anchor_cells(_lib.ptr(m), _lib.ptr(a), _lib.ptr(prior), B, h, w, None, CELL, 0.0, math.inf, math.inf,
                                                                                         _lib.ptr(n_c), _lib.ptr(s_c), st)),
                    "rdm_depth_anchor_field": lambda: _lib.check(L.rdm_depth_anchor_field(_lib.ptr(n_c), _lib.ptr(s_c), _lib.ptr(prior), B, gy, gx, 1, SIGMA, LAM, _lib.ptr(ls_o),
                                                                                         _lib.ptr(cnt_o), _lib.ptr(fld), st)),
                    "rdm_depth_frames_corrected": lambda: _lib.check(L.rdm_depth_frames_corrected(_lib.ptr(m), None, 0, _lib.ptr(ls_o), None, B, h, w, None, 0, 1e-3, _lib.ptr(out),
                                                                                                 None, None, 0, _lib.ptr(fld), gy, gx, CELL, st)),
                }
                for fn in one.values():
                    fn()
                t = alternate({"fused": fused, "composed": composed, **one}, args.reps, args.rounds)
                base = {"batch": B, "frame": [h, w], "anchors": density, "valid": round(keep.double().mean().item(), 4), "cell": CELL, "sigma": SIGMA}
                emit({"figure": "anchor.fit + anchor.metric_frames (three launches)", **base, **summary(t["fused"])})
                emit({"figure": "composed: resize, log, masks, avg_pool2d sums, 4 conv2d, interpolate, add, exp, cast", **base, **summary(t["composed"])})
                for k in one:
                    emit({"figure": k, **base, **summary(t[k])})
    if args.out:
        with open(args.out, "w") as fh:
            for d_ in lines:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
