"""The mesh-face call (rdm_depth_mesh, include/rdm_mesh.h: two launches) against the composed torch path it replaces, at the native 480x640 frame
and at 226x226, B = 8 and B = 1, for the 12-byte (int32 triples) and the 13-byte (PLY face record) layouts, one process.  The frame is a smooth
surface (neighbouring depths within 1 %) with a depth step every 64 columns that the default edge_ratio cuts, and half the pixels valid: 16x16
blocks, each valid or not by a hash - a surface with holes, so that about one face per cell is written (pixels dropped one by one at random would
leave almost no cell with three valid corners, and nothing to write).
  (fused)     rdm_depth_mesh through mesh.faces: the workspace, output and count allocations of the wrapper included, as a caller pays them;
  (composed)  torch operators: the exclusive scan of the validity mask (cumsum), four shifted views of depth, validity and index, the float64
              diagonal rule, the two candidates' masks and index triples, the `.sum()` that sizes the output AND its transfer to the host (a caller
              cannot allocate without it), one boolean index over the stacked (cell, candidate) axis - which keeps the row-major face order without
              a separate interleave, cheaper than an index per triangle kind - the int32 cast and, for the 13-byte record, the byte views behind a
              column of 3s.  Its faces are packed over the batch (no per-sample stride), which is less than the contract asks.
There is no launch-shape argument to sweep: the first launch is one workgroup per sampled row, the second one per cell row, both fixed by the
frame.  Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is
what a caller pays), taken in `rounds` rounds that alternate the candidates; reported: median, minimum and maximum over the rounds.  Before timing,
the fused faces and both counts are compared with the composed ones on the timed input (equal).  `bytes` is what the fused call must move through
memory by its shapes: the depth plane read once, the faces and the two tables written; the second launch's re-read of the plane and of the tables
is cache traffic and not in it.
One JSON line per figure.  `python tools/mesh_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import filler, mesh  # noqa: E402

RATIO = mesh.EDGE_RATIO


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
    """(B,H,W) float32: see the module docstring"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 2.0 + 0.4 * np.sin(xx / 90.0) + 0.3 * np.cos(yy / 70.0) + 0.8 * ((xx // 64) % 2)
    d = (z[None] * (1.0 + 0.002 * filler.unit("mesh_bench.noise/%d" % H, B * H * W).reshape(B, H, W))).astype(np.float32)
    bh, bw = -(-H // 16), -(-W // 16)
    keep = filler.unit("mesh_bench.blocks/%d" % H, B * bh * bw).reshape(B, bh, bw) < 0.5
    d[~np.repeat(np.repeat(keep, 16, 1), 16, 2)[:, :H, :W]] = 0.0
    return d


def composed_faces(d, layout):
    """-> (faces packed over the batch (n, rec) uint8, face counts (B,) int32, vertex counts (B,) int32)"""
    B, H, W = d.shape
    valid = torch.isfinite(d) & (d > 0)
    flat = valid.view(B, -1)
    index = (torch.cumsum(flat, 1, dtype=torch.int32) - flat.int()).view(B, H, W)             # the exclusive scan
    corner = lambda a: (a[:, :-1, :-1], a[:, :-1, 1:], a[:, 1:, :-1], a[:, 1:, 1:])
    dA, dB, dC, dD = corner(d)
    vA, vB, vC, vD = corner(valid)
    iA, iB, iC, iD = corner(index)
    ad = vA & vD & (~(vB & vC) | ((dA.double() - dD.double()).abs() <= (dB.double() - dC.double()).abs()))

    def passes(a, b, c):
        return torch.maximum(torch.maximum(a, b), c).double() <= torch.minimum(torch.minimum(a, b), c).double() * RATIO
    m = torch.stack([torch.where(ad, vA & vC & vD & passes(dA, dC, dD), vA & vC & vB & passes(dA, dC, dB)),
                     torch.where(ad, vA & vD & vB & passes(dA, dD, dB), vB & vC & vD & passes(dB, dC, dD))], dim=-1)
    tri = torch.stack([torch.stack([iA, iC, torch.where(ad, iD, iB)], dim=-1),
                       torch.stack([torch.where(ad, iA, iB), torch.where(ad, iD, iC), torch.where(ad, iB, iD)], dim=-1)], dim=-2)      # (B, H-1, W-1, 2, 3)
    counts = m.sum(dim=(1, 2, 3), dtype=torch.int32)
    n = int(counts.sum())                                                                     # sizes the output: a host synchronisation
    picked = tri[m].view(torch.uint8).view(n, 12)
    if layout == "i32":
        return picked, counts, flat.sum(1, dtype=torch.int32)
    out = torch.empty(n, 13, dtype=torch.uint8, device=d.device)
    out[:, 0] = 3
    out[:, 1:] = picked
    return out, counts, flat.sum(1, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for H, W in ((480, 640), (226, 226)):
        full = torch.from_numpy(surface(8, H, W)).to(dev)
        for B in (8, 1):
            d = full[:B].contiguous()
            for layout in ("i32", "ply"):
                rec = mesh.face_bytes(layout)
                fused = lambda: mesh.faces(d, edge_ratio=RATIO, layout=layout)
                composed = lambda: composed_faces(d, layout)
                (tri, fc, vc), (ctri, cfc, cvc) = fused(), composed()
                torch.cuda.synchronize()
                assert torch.equal(fc, cfc), "the fused face counts differ from the composed ones"
                assert torch.equal(vc, cvc), "the fused vertex counts differ from the composed ones"
                at, n = 0, fc.cpu().tolist()
                for b in range(B):
                    assert torch.equal(tri[b, :n[b] * rec].view(n[b], rec), ctri[at:at + n[b]]), "the fused faces of sample %d differ from the composed ones" % b
                    at += n[b]
                base = {"batch": B, "frame": [H, W], "layout": layout, "record_bytes": rec, "faces": sum(n), "cells": B * (H - 1) * (W - 1), "vertices": int(vc.sum()),
                        "edge_ratio": RATIO}
                t = alternate({"fused": fused, "composed": composed}, args.reps, args.rounds)
                emit({"figure": "rdm_depth_mesh (mesh.faces)", **base, "bytes": B * H * W * 4 + sum(n) * rec + B * (2 * H * 4 + 8), **summary(t["fused"])})
                emit({"figure": "composed torch path", **base, **summary(t["composed"])})
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
