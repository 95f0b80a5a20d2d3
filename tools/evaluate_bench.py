"""Batched evaluation (harness.evaluate, rdm_eval_target_metrics_f64) at B = 1, 8, 16 with 226x226 depth planes, one process:
  (a) the composed target and metric chain PER SAMPLE, as the batch-1 validation loop runs it: harness.prepare_target (rdm_resize_bicubic_f64
      + four ATen mask ops), harness.normalize (rdm_gm_normalize_f64) and MetricComputation.compute (a memset, rdm_depth_metrics_f64 and the
      blocking copy of the ten sums) - the baseline; B samples take B such chains;
  (b) the fused launch MetricComputation.compute_rows on the whole batch - as harness.evaluate enqueues it (no copy), and followed by a
      blocking copy of the rows per call (the like-for-like of (a)'s synchronisation);
  (c) a whole harness.evaluate pass of 64 samples at batch size 1, 8 and 16 against the batch-1 validation_step + log_val loop over the same
      samples (host clock around a pass that ends in a device synchronise).
  (d) the standard protocol (metrics.StandardMetrics, rdm_eval_standard_f64; --legs standard runs it alone): the fused launch
      StandardMetrics.compute_rows at B = 8 on 226x226 and 480x640 depth, median alignment, against the composed torch path on the same
      device - F.interpolate(bicubic) of the map, exp, and per sample a sort of the masked depth and of the masked prediction for the two
      medians (boolean indexing: a host synchronisation per sample), the clamp and the eleven sums.  Compared first: counts equal, sums at 1e-9 (torch's bicubic and exp are
      not the library's bit for bit).
(a), (b) and (d) are the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is what
a caller pays), taken in `rounds` rounds that alternate the candidates; reported: median, minimum and maximum over the rounds.  Before
timing, (a) and (b) are compared on the timed input (counts equal, sums at 1e-11).
One JSON line per figure.  `python tools/evaluate_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, evaluate, filler, harness  # noqa: E402
from md_rdm_amd.metrics import MetricComputation, MetricLogger, StandardMetrics  # noqa: E402
from md_rdm_amd.network.RDM_Net import DepthEstimationNet  # noqa: E402

METRICS = ["delta1", "delta2", "delta3", "mse", "mae", "log10", "rmse"]


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                   # us per call


def host_window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6                 # us per pass


def alternate(cands, measure, rounds, warmup=3):
    """{name: [us, one per round]}: the candidates take turns inside every round."""
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


def composed_standard(log_map, depth, lo=1e-3, hi=10.0):
    """the standard protocol from torch operators: (B,16) rows like rdm_eval_standard_f64's under median alignment (column 14 left 0)"""
    B, _, H, W = depth.shape
    p = torch.nn.functional.interpolate(log_map, size=(H, W), mode="bicubic", align_corners=False).exp()
    d = depth.double()
    rows = torch.zeros(B, 16, dtype=torch.float64, device=depth.device)
    for b in range(B):
        v = torch.isfinite(d[b]) & (d[b] > lo) & (d[b] < hi)
        dv, pv = d[b][v], p[b][v]
        n = dv.numel()
        if n == 0:
            continue
        ds, ps = dv.sort().values, pv.sort().values
        sd = ds[(n - 1) // 2] if n % 2 else (ds[n // 2 - 1] + ds[n // 2]) / 2
        sp = ps[(n - 1) // 2] if n % 2 else (ps[n // 2 - 1] + ps[n // 2]) / 2
        s = sd / sp
        q = (s * pv).clamp(lo, hi)
        r, e, g = torch.maximum(q / dv, dv / q), q - dv, q.log() - dv.log()
        rows[b, :14] = torch.stack([torch.tensor(float(n), dtype=torch.float64, device=d.device), (r < 1.25).sum().double(), (r < 1.25 ** 2).sum().double(),
                                    (r < 1.25 ** 3).sum().double(), (e.abs() / dv).sum(), (e * e / dv).sum(), (e * e).sum(), (g * g).sum(), g.sum(),
                                    (q.log10() - dv.log10()).abs().sum(), e.abs().sum(), s, sd, sp])
    return rows


def standard_leg(dev, emit, rounds):
    sm = StandardMetrics()
    for (B, H, W) in ((8, 226, 226), (8, 480, 640)):
        y = torch.from_numpy(filler.synthetic_batch(B, H, W, seed=3)[1]).to(dev)
        pred = torch.from_numpy(filler.uniform("evaluate-bench-pred/std/%d" % B, (B, 1, 128, 128), -1.0, 2.0, dtype="float64")).to(dev)
        rows, ref = sm.compute_rows(pred, y).cpu(), composed_standard(pred, y).cpu()
        rel = float(((rows[:, 4:14] - ref[:, 4:14]).abs() / ref[:, 4:14].abs()).max())
        counts = int((rows[:, :4] != ref[:, :4]).sum())
        assert torch.equal(rows[:, 0], ref[:, 0]) and rel <= 1e-9, rel
        emit({"figure": "(d) fused vs composed standard rows on the timed input", "batch": B, "depth": [H, W], "max_rel_diff_sums": rel, "delta_counts_differing": counts})
        t = alternate({"composed": lambda: composed_standard(pred, y), "fused": lambda: sm.compute_rows(pred, y), "fused+copy": lambda: sm.compute_rows(pred, y).cpu()},
                      lambda fn: window(fn, 20), rounds)
        a, f, fc = summary(t["composed"]), summary(t["fused"]), summary(t["fused+copy"])
        emit({"figure": "(d) composed torch path: interpolate + exp + per-sample sort of the masked values for the medians + sums", "batch": B, "depth": [H, W], **a})
        emit({"figure": "(d) fused launch rdm_eval_standard_f64, enqueue only (as harness.evaluate)", "batch": B, "depth": [H, W], **f, "speedup_vs_composed": round(a["us"] / f["us"], 1)})
        emit({"figure": "(d) fused launch + one blocking copy of the rows per call", "batch": B, "depth": [H, W], **fc, "speedup_vs_composed": round(a["us"] / fc["us"], 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="all", choices=["all", "reference", "standard"], help="reference: (a)-(c); standard: (d)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--samples", type=int, default=64, help="samples of the whole-pass figure (c)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    with torch.no_grad():
        if args.legs in ("all", "standard"):
            standard_leg(dev, emit, args.rounds)
        if args.legs in ("all", "reference"):
            reference_legs(dev, L, emit, args)
    if args.out:
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


def reference_legs(dev, L, emit, args):
    """(a)-(c); called under no_grad"""
    mc = MetricComputation(METRICS)
    for B in (1, 8, 16):
        y = torch.from_numpy(filler.synthetic_batch(B, 226, 226, seed=3)[1]).to(dev)
        pred = torch.from_numpy(filler.uniform("evaluate-bench-pred/%d" % B, (B, 1, 128, 128), -1.0, 2.0, dtype="float64")).to(dev)

        def composed():
            out = []
            for b in range(B):
                tn = harness.normalize(harness.prepare_target(y[b:b + 1]))
                out.append(mc.compute(pred[b:b + 1], tn))
            return out

        def fused():
            return mc.compute_rows(pred, y)

        def fused_copy():
            return mc.compute_rows(pred, y).cpu()

        ref = torch.empty(B, 10, dtype=torch.float64, device=dev)
        for b in range(B):
            tn = harness.normalize(harness.prepare_target(y[b:b + 1]))
            _lib.check(L.rdm_depth_metrics_f64(_lib.ptr(pred[b].contiguous()), _lib.ptr(tn.contiguous()), 128 * 128, _lib.ptr(ref[b]), _lib.stream()))
        rows = fused_copy()
        ref = ref.cpu()
        rel = float(((rows[:, 4:] - ref[:, 4:]).abs() / ref[:, 4:].abs()).max())
        assert torch.equal(rows[:, :4], ref[:, :4]) and rel <= 1e-11, rel
        emit({"figure": "fused vs composed rows on the timed input", "batch": B, "max_rel_diff_sums": rel, "counts_equal": True})

        t = alternate({"composed": composed, "fused": fused, "fused+copy": fused_copy}, lambda fn: window(fn, 100), args.rounds)
        a, f, fc = summary(t["composed"]), summary(t["fused"]), summary(t["fused+copy"])
        emit({"figure": "(a) composed target + metric chain, B per-sample chains with their blocking copies", "batch": B, **a})
        emit({"figure": "(b) fused launch rdm_eval_target_metrics_f64, enqueue only (as harness.evaluate)", "batch": B, **f, "speedup_vs_a": round(a["us"] / f["us"], 1)})
        emit({"figure": "(b) fused launch + one blocking copy of the rows per call", "batch": B, **fc, "speedup_vs_a": round(a["us"] / fc["us"], 1)})

    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    xs, ys = evaluate.synthetic_samples(args.samples, 226, 226)
    xs, ys = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)

    def batches(bs):
        return [(xs[i:i + bs], ys[i:i + bs]) for i in range(0, args.samples, bs)]

    def loop():
        logger = MetricLogger(METRICS)
        for x, yy in batches(1):
            y_hat, y_n = harness.validation_step(m, x, yy)
            logger.log_val(y_hat, y_n)
        return {k: logger.computer.avg(k) for k in METRICS}

    want, got = loop(), harness.evaluate(m, batches(8), METRICS)
    rel = max(abs(got[k] / want[k] - 1) for k in METRICS)
    assert rel <= 1e-11, rel
    emit({"figure": "evaluate (batch 8) vs the batch-1 validation loop on the timed samples", "samples": args.samples, "max_rel_diff": rel})
    cands = {"loop": loop}
    cands.update({"evaluate_b%d" % bs: (lambda bs=bs: harness.evaluate(m, batches(bs), METRICS)) for bs in (1, 8, 16)})
    t = alternate(cands, host_window, args.rounds, warmup=1)
    base = summary(t["loop"])
    emit({"figure": "(c) batch-1 validation_step + log_val loop, whole pass", "samples": args.samples, **base, "images_per_s": round(args.samples / (base["us"] * 1e-6), 1)})
    for bs in (1, 8, 16):
        s = summary(t["evaluate_b%d" % bs])
        emit({"figure": "(c) harness.evaluate, whole pass", "samples": args.samples, "batch": bs, **s, "images_per_s": round(args.samples / (s["us"] * 1e-6), 1),
              "speedup_vs_loop": round(base["us"] / s["us"], 2)})


if __name__ == "__main__":
    main()
