"""The novel-view call (rdm_depth_warp, include/rdm_warp.h: three launches) against the composed torch path it replaces, one process, four shapes:
B = 8 and B = 1 at the native 480x640 frame, B = 8 at 226x226 (splat 1, no fill), and B = 8 at 480x640 with splat = 2 and fill = 16.  The frame is
a smooth surface between 1.6 and 3.5 m with a depth step every 64 columns and a sixteenth of the pixels without a measurement (16x16 blocks, by a
hash); the view is a stereo partner 6 cm to the right plus a small rotation, so that occlusions, disocclusions and both image borders occur.
  (fused)     rdm_depth_warp through warp.render: the pose upload and the workspace and output allocations of the wrapper included, as a caller
              pays them;
  (composed)  torch operators on the same inputs: the float64 unprojection, pose and projection in the header's order, the footprint's first cell,
              the range mask, int64 keys (float bits << 32 | source index), one `scatter_reduce_("amin")` per footprint cell into a full-frame int64
              plane, the decode, the gathers of depth, index and colour, and a vectorised row-wise hole fill (nearest keyed column to the left and to
              the right by `cummax` / `cummin` of column numbers, the farther one taken).
Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is what a
caller pays), taken in `rounds` rounds that alternate the candidates after `warmup` untimed calls each; reported: median, minimum and maximum
over the rounds.  Before timing, the four planes of both paths are compared on the timed input (equal).  `atomic_bytes` is 8 bytes per atomic the
splat issues (the number of in-range footprint cells of all kept points, counted by the composed path); `atomic_gbps` sets them against the
WHOLE call's median time, a lower bound of the rate the splat launch itself sustains.
One JSON line per figure.  `python tools/warp_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import filler, warp  # noqa: E402

EMPTY = torch.iinfo(torch.int64).max


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


def surface(B, H, W):
    """(B,H,W) float32 and (B,H,W,3) uint8: see the module docstring"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 2.0 + 0.4 * np.sin(xx / 90.0) + 0.3 * np.cos(yy / 70.0) + 0.8 * ((xx // 64) % 2)
    d = (z[None] * (1.0 + 0.002 * filler.unit("warp_bench.noise/%d" % H, B * H * W).reshape(B, H, W))).astype(np.float32)
    bh, bw = -(-H // 16), -(-W // 16)
    keep = filler.unit("warp_bench.blocks/%d" % H, B * bh * bw).reshape(B, bh, bw) >= 1.0 / 16.0
    d[~np.repeat(np.repeat(keep, 16, 1), 16, 2)[:, :H, :W]] = 0.0
    rgb = (filler.unit("warp_bench.rgb/%d" % H, B * H * W * 3) * 256.0).astype(np.uint8).reshape(B, H, W, 3)
    return d, rgb


def composed(d, rgb, intr, pose, splat, fill, count=None):
    """-> the four planes; `count`: a list that receives the number of atomics the fused splat issues for this input"""
    B, H, W = d.shape
    fx, fy, cx, cy = intr
    T = [float(v) for v in pose.reshape(-1)]
    ys = torch.arange(H, device=d.device, dtype=torch.float64).view(1, H, 1)
    xs = torch.arange(W, device=d.device, dtype=torch.float64).view(1, 1, W)
    ok = torch.isfinite(d) & (d > 0)
    Z = d.double()
    X = ((xs - cx) * Z) / fx
    Y = ((ys - cy) * Z) / fy
    Qx = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3]
    Qy = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7]
    Qz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11]
    zf = Qz.float()
    u = (fx * Qx) / Qz + cx
    v = (fy * Qy) / Qz + cy
    c0 = torch.floor((u - (splat - 1) * 0.5) + 0.5)
    r0 = torch.floor((v - (splat - 1) * 0.5) + 0.5)
    ok = ok & torch.isfinite(Qz) & torch.isfinite(zf) & (zf > 0) & torch.isfinite(u) & torch.isfinite(v)
    ok = ok & (c0 >= 1 - splat) & (c0 <= W - 1) & (r0 >= 1 - splat) & (r0 <= H - 1)
    src = torch.arange(H * W, device=d.device, dtype=torch.int64).view(1, H, W)
    key = (zf.view(torch.int32).to(torch.int64) << 32) | src
    c0 = torch.where(ok, c0, torch.zeros_like(c0)).long()
    r0 = torch.where(ok, r0, torch.zeros_like(r0)).long()
    keys = torch.full((B, H * W), EMPTY, dtype=torch.int64, device=d.device)
    n = 0
    for dr in range(splat):
        for dc in range(splat):
            r, c = r0 + dr, c0 + dc
            inside = ok & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            if count is not None:
                n += int(inside.sum())
            cell = torch.where(inside, r * W + c, torch.zeros_like(r)).view(B, -1)
            keys.scatter_reduce_(1, cell, torch.where(inside, key, torch.full_like(key, EMPTY)).view(B, -1), "amin", include_self=True)
    if count is not None:
        count.append(n)
    keys = keys.view(B, H, W)
    has = keys != EMPTY
    mask = has.to(torch.uint8)
    if fill > 0:
        col = torch.arange(W, device=d.device, dtype=torch.int64).view(1, 1, W).expand(B, H, W)
        left = torch.cummax(torch.where(has, col, torch.full_like(col, -1)), dim=2).values                       # the nearest keyed column at or left of each cell
        right = torch.flip(torch.cummin(torch.flip(torch.where(has, col, torch.full_like(col, 2 * W)), (2,)), dim=2).values, (2,))
        hl, hr = (left >= 0) & (col - left <= fill), (right < W) & (right - col <= fill)
        kl = torch.gather(keys, 2, left.clamp(min=0))
        kr = torch.gather(keys, 2, right.clamp(max=W - 1))
        pick = torch.where(hl & hr, torch.where((kr >> 32) > (kl >> 32), kr, kl), torch.where(hl, kl, kr))
        filled = ~has & (hl | hr)
        keys = torch.where(filled, pick, keys)
        mask = torch.where(filled, torch.full_like(mask, 2), mask)
    got = mask > 0
    index = torch.where(got, keys & 0xFFFFFFFF, torch.full_like(keys, -1))
    depth = torch.where(got, (keys >> 32).to(torch.int32).view(torch.float32), torch.zeros((), dtype=torch.float32, device=d.device))
    colour = torch.gather(rgb.view(B, H * W, 3), 1, index.clamp(min=0).view(B, -1, 1).expand(B, H * W, 3)).view(B, H, W, 3) * got.unsqueeze(-1).to(torch.uint8)
    return {"depth": depth, "rgb": colour, "index": index.to(torch.int32), "mask": mask}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    pose = warp.pose_from_rt((0.0, 0.02, 0.0), (-0.06, 0.0, 0.0))
    for B, H, W, splat, fill in ((8, 480, 640, 1, 0), (1, 480, 640, 1, 0), (8, 226, 226, 1, 0), (8, 480, 640, 2, 16)):
        dn, cn = surface(8, H, W)
        d, rgb = torch.from_numpy(dn[:B]).to(dev).contiguous(), torch.from_numpy(cn[:B]).to(dev).contiguous()
        intr = (518.8579 * W / 640.0, 519.4696 * W / 640.0, (W - 1) / 2.0, (H - 1) / 2.0)
        fused = lambda: warp.render(d, intr, pose, rgb=rgb, splat=splat, fill=fill)
        other = lambda: composed(d, rgb, intr, pose, splat, fill)
        count = []
        a, b = fused(), composed(d, rgb, intr, pose, splat, fill, count)
        torch.cuda.synchronize()
        for k in warp.PLANES:
            same = torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) if k == "depth" else torch.equal(a[k], b[k])
            assert same, "plane %s of the fused call differs from the composed path at B = %d, %dx%d, splat %d, fill %d" % (k, B, H, W, splat, fill)
        base = {"batch": B, "frame": [H, W], "splat": splat, "fill": fill, "kept_cells": int((a["mask"] == 1).sum()), "filled_cells": int((a["mask"] == 2).sum()),
                "cells": B * H * W}
        t = alternate({"fused": fused, "composed": other}, args.reps, args.rounds)
        f = summary(t["fused"])
        emit({"figure": "rdm_depth_warp (warp.render)", **base, "atomics": count[0], "atomic_bytes": 8 * count[0], "atomic_gbps": round(8 * count[0] / f["us"] / 1e3, 1), **f})
        emit({"figure": "composed torch path", **base, **summary(t["composed"])})
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
