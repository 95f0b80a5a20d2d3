"""The standard-protocol scoring launch at B = 8, at the loader's 226x226 depth and at the native 480x640 frame, one process:
  (a) rdm_eval_standard_f64 (the map stretched over the whole frame);
  (b) rdm_eval_standard_view_f64 with the full view (the same bytes as (a)) and with the test transform's view of the frame;
each under median alignment (the radix select runs) and without alignment, with the Eigen crop at 480x640.  The kernel runs ONE workgroup per
sample, so a native frame (307 200 pixels against 51 076) is six times the work of the same eight workgroups: this tool is how that cost is read.
Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is what a
caller pays), taken in `rounds` rounds that alternate the candidates; reported: median, minimum and maximum over the rounds.  Before timing,
(a) and (b, full view) are compared on the timed input (equal bytes).
One JSON line per figure.  `python tools/evalstd_bench.py [--out FILE]`"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, filler  # noqa: E402
from md_rdm_amd.dataloaders import nyu  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    B = 8
    m = torch.from_numpy(filler.uniform("evalstd_bench.map", (B, 1, 128, 128), -1.0, 2.0).astype("float64")).to(dev)
    for H, W, crop in ((226, 226, None), (480, 640, (45, 41, 471, 601))):
        d = filler.log_uniform("evalstd_bench.d/%dx%d" % (H, W), (B, 1, H, W), 0.3, 12.0)
        d[filler.unit("evalstd_bench.hole/%dx%d" % (H, W), B * H * W).reshape(B, 1, H, W) < 0.1] = 0.0
        d = torch.from_numpy(d).to(dev)
        ws = torch.empty(L.rdm_eval_standard_workspace_bytes(B, H, W) // 8, dtype=torch.float64, device=dev)
        c = (C.c_int32 * 4)(*crop) if crop else None
        # the rectangle the network input covers: the test transform's view of a 480x640 frame; at the loader's size, the same fractions of it
        tv = nyu.test_view((480, 640))
        part = (C.c_double * 4)(tv[0] * H / 480, tv[1] * W / 640, tv[2] * H / 480, tv[3] * W / 640)
        full = (C.c_double * 4)(0.0, 0.0, float(H), float(W))

        def old(align, rows):
            _lib.check(L.rdm_eval_standard_f64(_lib.ptr(m), _lib.ptr(d), 0, B, H, W, align, 1e-3, 10.0, c, _lib.ptr(rows), None, _lib.ptr(ws), ws.numel() * 8, _lib.stream()))

        def new(align, rows, view):
            _lib.check(L.rdm_eval_standard_view_f64(_lib.ptr(m), _lib.ptr(d), 0, B, H, W, align, 1e-3, 10.0, c, view, _lib.ptr(rows), None, _lib.ptr(ws), ws.numel() * 8,
                                                    _lib.stream()))

        for name, align in (("median", 1), ("none", 0)):
            r0, r1, r2 = (torch.empty(B, 16, dtype=torch.float64, device=dev) for _ in range(3))
            old(align, r0)
            new(align, r1, full)
            torch.cuda.synchronize()
            assert torch.equal(r0.view(torch.int64), r1.view(torch.int64)), "the full view does not give rdm_eval_standard_f64's bytes"
            t = alternate({"old": lambda: old(align, r0), "full": lambda: new(align, r1, full), "part": lambda: new(align, r2, part)}, args.reps, args.rounds)
            base = {"batch": B, "depth": [H, W], "align": name, "crop": list(crop) if crop else None}
            emit({"figure": "rdm_eval_standard_f64", **base, **summary(t["old"])})
            emit({"figure": "rdm_eval_standard_view_f64, full view", **base, **summary(t["full"])})
            emit({"figure": "rdm_eval_standard_view_f64, the test transform's view", **base, "view": [round(v, 3) for v in part], **summary(t["part"])})
    if args.out:
        with open(args.out, "w") as fh:
            for d_ in lines:
                fh.write(json.dumps(d_) + "\n")


if __name__ == "__main__":
    main()
