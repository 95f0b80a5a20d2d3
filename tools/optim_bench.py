#!/usr/bin/env python3
"""Times of the optimiser-side gradient kernels (include/rdm_optim.h) at the model's flat size, in the manner of bench_ops.py: one JSON line each.

  * rdm_grad_accumulate_f32 (both modes), rdm_grad_sumsq_f64, rdm_adamw_fused_clip and, beside them, rdm_adamw_fused: achieved GB/s of the
    compulsory bytes against the HBM3E peak;
  * the clipped step as the optimiser issues it (one sum of squares + one clipped AdamW launch) against the composed torch path on the same
    device: torch.nn.utils.clip_grad_norm_ on the flat gradient view, then the plain fused step;
  * with --train: md_rdm_amd.train's step with and without --gradient_clip_val, `--rounds` alternating runs of each, the median step time of every
    run and the spread over the runs (a difference inside that spread is no difference).

  python tools/optim_bench.py [--n 90529720] [--reps 20] [--train --rounds 3 --batch_size 16 --steps 12]
No speed is asserted anywhere; DESIGN.md 4.9 records what this prints."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib  # noqa: E402

PEAK = 8000.0


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def report(name, seconds, nbytes, note):
    gbs = nbytes / seconds / 1e9
    print(json.dumps({"kernel": name, "ms": round(seconds * 1e3, 4), "algorithmic_MB": round(nbytes / 1e6, 2), "achieved_GBps": round(gbs, 1),
                      "hbm_peak_GBps": PEAK, "frac": round(gbs / PEAK, 4), "note": note}), flush=True)


def kernels(n, reps):
    dev = torch.device("cuda:0")
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream
    p, m, v, acc = (torch.zeros(n, device=dev) for _ in range(4))
    g = torch.randn(n, device=dev) * 1e-3
    slots = torch.zeros(8, dtype=torch.float64, device=dev)
    coef = torch.zeros(1, device=dev)
    need = int(L.rdm_grad_sumsq_workspace_bytes(n))
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    hp = (1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 1.0)
    t = timeit(lambda: _lib.check(L.rdm_grad_accumulate_f32(P(acc), P(g), n, _lib.GRAD_ACC_COPY, S())), reps)
    report(f"grad_accumulate copy n={n}", t, n * 8, "8 B/element: read g, write acc")
    t = timeit(lambda: _lib.check(L.rdm_grad_accumulate_f32(P(acc), P(g), n, _lib.GRAD_ACC_ADD, S())), reps)
    report(f"grad_accumulate add n={n}", t, n * 12, "12 B/element: read acc, g, write acc")
    t = timeit(lambda: _lib.check(L.rdm_grad_sumsq_f64(P(g), n, P(slots), P(ws), need, S())), reps)
    report(f"grad_sumsq n={n}", t, n * 4, "4 B/element: read g (two launches: partials, then their sum)")
    t_plain = timeit(lambda: _lib.check(L.rdm_adamw_fused(P(p), P(g), P(m), P(v), n, *hp, S())), reps)
    report(f"adamw_fused n={n}", t_plain, n * 28, "28 B/element: read p,g,m,v, write p,m,v")
    t = timeit(lambda: _lib.check(L.rdm_adamw_fused_clip(P(p), P(g), P(m), P(v), n, *hp, P(slots), 1, 1.0, P(coef), S())), reps)
    report(f"adamw_fused_clip n={n}", t, n * 28, "28 B/element + the slots, read by every thread")

    def fused():
        _lib.check(L.rdm_grad_sumsq_f64(P(g), n, P(slots), P(ws), need, S()))
        _lib.check(L.rdm_adamw_fused_clip(P(p), P(g), P(m), P(v), n, *hp, P(slots), 1, 1.0, P(coef), S()))
    scratch = g.clone()
    q = torch.nn.Parameter(torch.zeros(n, device=dev))           # stands for the flat parameter view whose .grad is the flat gradient view
    q.grad = scratch

    def composed():
        scratch.copy_(g)                                         # clip_grad_norm_ scales in place: a fresh gradient per step, as backward leaves one
        torch.nn.utils.clip_grad_norm_([q], 1.0)
        _lib.check(L.rdm_adamw_fused(P(p), P(scratch), P(m), P(v), n, *hp, S()))
    t_copy = timeit(lambda: scratch.copy_(g), reps)
    t_f, t_c = timeit(fused, reps), timeit(composed, reps)
    print(json.dumps({"path": "clipped step", "n": n, "fused_ms": round(t_f * 1e3, 4), "torch_composed_ms": round((t_c - t_copy) * 1e3, 4),
                      "plain_step_ms": round(t_plain * 1e3, 4), "note": "fused: grad_sumsq + adamw_fused_clip (32 B/element); composed: clip_grad_norm_ (norm pass, a host decision "
                      "in some torch versions, a scaling pass) + adamw_fused, the gradient refresh copy subtracted"}), flush=True)


def train_steps(clip, args):
    """median optimiser-step time of one md_rdm_amd.train epoch in this process (the first `skip` steps dropped)"""
    import contextlib
    import io

    from md_rdm_amd import harness, train
    stamps = []
    plain = harness.FusedAdamW.step

    def timed(self, *a, **kw):
        r = plain(self, *a, **kw)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return r
    harness.FusedAdamW.step = timed
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            train.main(["--synthetic", "--batch_size", str(args.batch_size), "--size", "228", "304", "--max_steps", str(args.steps), "--seed", "1"] +
                       (["--gradient_clip_val", str(clip)] if clip else []))
    finally:
        harness.FusedAdamW.step = plain
    d = [b - a for a, b in zip(stamps, stamps[1:])][args.skip:]
    return statistics.median(d) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=90_529_720, help="elements (default: the model's flat parameter count)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="also time md_rdm_amd.train's step with and without --gradient_clip_val")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--skip", type=int, default=3)
    args = ap.parse_args()
    kernels(args.n, args.reps)
    if args.train:
        runs = {"off": [], "on": []}
        for _ in range(args.rounds):                             # alternating, so that drift lands on both
            runs["off"].append(train_steps(0.0, args))
            runs["on"].append(train_steps(1.0, args))
        print(json.dumps({"path": "train step", "batch_size": args.batch_size, "size": [228, 304],
                          "clip_off_ms": [round(x, 3) for x in runs["off"]], "clip_on_ms": [round(x, 3) for x in runs["on"]],
                          "spread_off_ms": round(max(runs["off"]) - min(runs["off"]), 3), "spread_on_ms": round(max(runs["on"]) - min(runs["on"]), 3),
                          "note": "median step time per run (loss printing and its synchronisation included, as train.py runs); runs alternate"}), flush=True)


if __name__ == "__main__":
    main()
