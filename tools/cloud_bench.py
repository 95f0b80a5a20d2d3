"""The point-cloud launch (rdm_depth_cloud, include/rdm_cloud.h) against the composed torch path it replaces, B = 8 at the native 480x640 frame
and at 226x226, for the 12-byte (position) and 27-byte (position, normal, colour) records, about half the pixels valid, one process:
  (fused)     one launch: validity, unprojection, normals, colour, in-order compaction into packed records, the counts;
  (composed)  torch operators: meshgrid, the float64 unprojection and its casts, the mask, its per-sample sums, a boolean index per plane and a
              cat of their byte views.  For the 27-byte record the composed normals are central differences by torch.roll (wrapping at the frame's
              edges, no one-sided differences next to holes): LESS than the contract asks, so its time is a lower bound for a faithful one.
Then the fused launch at split = 0 (the library's default) against fixed splits: every workgroup counts the valid pixels ahead of its run itself,
so more workgroups per sample trade parallelism against re-read L2 traffic.  Every figure is the time per call of `reps` back-to-back calls on
one stream between two device events (host enqueue included: that is what a caller pays), taken in `rounds` rounds that alternate the
candidates; reported: median, minimum and maximum over the rounds.  Before timing, the fused positions and counts are compared with the composed
ones on the timed input (equal).  `bytes` is what the fused launch must move through memory by its shapes: the depth (and colour) planes read
once, the records written; the re-reads of the count ahead are L2 traffic and not in it.
One JSON line per figure.  `python tools/cloud_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import cloud, filler  # noqa: E402

INTR = cloud.INTRINSICS["nyu"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--splits", type=int, nargs="*", default=[1, 4, 8, 16, 32, 64, 128, 256])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    B = 8
    fx, fy, cx, cy = INTR
    for H, W in ((480, 640), (226, 226)):
        d = filler.uniform("cloud_bench.depth/%d" % H, (B, H, W), 0.5, 8.0)
        d[filler.unit("cloud_bench.mask/%d" % H, B * H * W).reshape(B, H, W) < 0.5] = 0.0
        d = torch.from_numpy(d).to(dev)
        rgb = torch.from_numpy((filler.unit("cloud_bench.rgb/%d" % H, B * H * W * 3) * 256.0).astype("uint8").reshape(B, H, W, 3)).to(dev)
        ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
        div = {k: torch.full((1,), v, dtype=torch.float64, device=dev) for k, v in (("fx", fx), ("fy", fy))}      # a divisor on the device: a host scalar goes through its reciprocal

        def points():
            Z = d.double()
            return torch.stack([((xs - cx) * Z) / div["fx"], ((ys - cy) * Z) / div["fy"], Z], dim=-1), torch.isfinite(d) & (d > 0)

        def composed12():
            P, m = points()
            return P.float()[m].view(torch.uint8), m.sum(dim=(1, 2), dtype=torch.int32)

        def composed27():
            P, m = points()
            a = torch.roll(P, -1, 2) - torch.roll(P, 1, 2)
            b = torch.roll(P, -1, 1) - torch.roll(P, 1, 1)
            n = torch.cross(b, a, dim=-1)
            n = torch.where(((n * P).sum(-1, keepdim=True) > 0), -n, n)
            n = n / n.norm(dim=-1, keepdim=True)
            rec = torch.cat([P.float()[m].view(torch.uint8), n.float()[m].view(torch.uint8), rgb[m]], dim=1)
            return rec, m.sum(dim=(1, 2), dtype=torch.int32)

        for rec, fused, composed in ((12, lambda split=0: cloud.point_cloud(d, INTR, split=split), composed12),
                                     (27, lambda split=0: cloud.point_cloud(d, INTR, rgb=rgb, normals=True, split=split), composed27)):
            (records, counts), (crec, ccnt) = fused(), composed()
            torch.cuda.synchronize()
            assert torch.equal(counts, ccnt), "the fused counts differ from the composed ones"
            at, n = 0, counts.cpu().tolist()
            for b in range(B):                                # positions: the first 12 bytes of every record
                got = records[b, :n[b] * rec].view(n[b], rec)[:, :12]
                assert torch.equal(got, crec.view(-1, rec)[at:at + n[b], :12]), "the fused positions of sample %d differ from the composed ones" % b
                at += n[b]
            base = {"batch": B, "frame": [H, W], "record_bytes": rec, "valid": sum(n)}
            t = alternate({"fused": fused, "composed": composed}, args.reps, args.rounds)
            emit({"figure": "rdm_depth_cloud", **base, "bytes": B * H * W * (4 + (3 if rec == 27 else 0)) + sum(n) * rec + 4 * B, **summary(t["fused"])})
            emit({"figure": "composed torch path" + (" (central differences only)" if rec == 27 else ""), **base, **summary(t["composed"])})
            cands = {"split 0": fused}
            for s in args.splits:
                cands["split %d" % s] = (lambda s_: lambda: fused(s_))(s)
            t = alternate(cands, args.reps, args.rounds)
            for k, v in t.items():
                emit({"figure": "rdm_depth_cloud, " + k, **base, **summary(v)})
    if args.out:
        with open(args.out, "w") as fh:
            for d_ in lines:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
