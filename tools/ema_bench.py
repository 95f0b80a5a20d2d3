#!/usr/bin/env python3
"""Times of the weight-average kernels (include/rdm_ema.h) at the model's flat size, in the manner of tools/optim_bench.py: one JSON line each.

Three ways to take one optimiser step, timed in alternating rounds so that drift lands on all of them:
  (a) plain     rdm_adamw_fused                                   7 streams of 4 B per element: read p, g, m, v, write p, m, v
  (b) fused     rdm_adamw_fused_ema                               9 streams: (a)'s and read + write of the average
  (c) composed  rdm_adamw_fused, then ema.lerp_(p, 1 - decay)     7 + 3 streams: (a)'s, then read p, read + write of the average, in a second launch
and rdm_ema_swap_f32 (4 streams: read and write both buffers).  Each round times `--reps` calls between two synchronisations with a host clock, after
one warm-up call of the same shape; reported are the median over the rounds, the spread (max - min) over the rounds, and the achieved GB/s of the
compulsory bytes against the HBM3E peak.  A difference inside the spread is no difference.  Before timing, (b)'s parameter and moment bytes are
compared with (a)'s on the same inputs.

  python tools/ema_bench.py [--n 90529720] [--reps 200] [--rounds 5] [--out profiles/ema_bench.json]
No speed is asserted anywhere; DESIGN.md 4.9b records what this prints."""
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
DECAY = 0.999


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=90_529_720, help="elements (default: the model's flat parameter count)")
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window (about 0.1 s of work at the default n)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", type=str, default=None, help="also write the lines, as a JSON list, to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ema_bench.py: no GPU is visible to this process; nothing here can be timed without one")
    n, dev = args.n, torch.device("cuda:0")
    L, P, S = _lib.lib(), _lib.ptr, _lib.stream
    g = torch.randn(n, device=dev) * 1e-3
    p0 = torch.randn(n, device=dev) * 1e-2
    hp = (1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 1.0)

    def fresh():
        return p0.clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev), p0.clone()

    # results first: the fused step's parameter and moment bytes are the plain step's
    pa, ma, va, _ = fresh()
    pb, mb, vb, eb = fresh()
    _lib.check(L.rdm_adamw_fused(P(pa), P(g), P(ma), P(va), n, *hp, S()))
    _lib.check(L.rdm_adamw_fused_ema(P(pb), P(g), P(mb), P(vb), P(eb), n, *hp, None, 0, 0.0, None, DECAY, S()))
    identical = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in ((pa, pb), (ma, mb), (va, vb)))
    ec = p0.clone().lerp_(pa, 1.0 - DECAY)
    lerp_gap = float((eb - ec).abs().max())
    del pa, ma, va, pb, mb, vb, eb, ec

    p, m, v, e = fresh()
    other = torch.zeros(n, device=dev)
    paths = {
        "plain": (lambda: _lib.check(L.rdm_adamw_fused(P(p), P(g), P(m), P(v), n, *hp, S())), 28, "28 B/element: read p,g,m,v, write p,m,v"),
        "fused": (lambda: _lib.check(L.rdm_adamw_fused_ema(P(p), P(g), P(m), P(v), P(e), n, *hp, None, 0, 0.0, None, DECAY, S())), 36,
                  "36 B/element: the plain step's and read + write of the average, one launch"),
        "composed": (lambda: (_lib.check(L.rdm_adamw_fused(P(p), P(g), P(m), P(v), n, *hp, S())), e.lerp_(p, 1.0 - DECAY)), 40,
                     "40 B/element: the plain step, then torch lerp_ (read p, read + write the average), two launches"),
        "swap": (lambda: _lib.check(L.rdm_ema_swap_f32(P(p), P(other), n, S())), 16, "16 B/element: read and write both buffers"),
    }
    times = {k: [] for k in paths}
    for _ in range(args.rounds):                                 # alternating, so that drift lands on all of them
        for k, (fn, _, _) in paths.items():
            times[k].append(timeit(fn, args.reps))
    lines = []
    for k, (_, bpe, note) in paths.items():
        med = statistics.median(times[k])
        gbs = n * bpe / med / 1e9
        lines.append({"path": k, "n": n, "ms": round(med * 1e3, 4), "spread_ms": round((max(times[k]) - min(times[k])) * 1e3, 4), "rounds": args.rounds, "reps": args.reps,
                      "algorithmic_MB": round(n * bpe / 1e6, 2), "achieved_GBps": round(gbs, 1), "hbm_peak_GBps": PEAK, "frac": round(gbs / PEAK, 4), "note": note})
    ta, tb, tc = (statistics.median(times[k]) for k in ("plain", "fused", "composed"))
    lines.append({"path": "summary", "n": n, "plain_ms": round(ta * 1e3, 4), "fused_ms": round(tb * 1e3, 4), "composed_ms": round(tc * 1e3, 4),
                  "fused_over_plain": round(tb / ta, 4), "streams_ratio_9_over_7": round(9 / 7, 4), "fused_over_composed": round(tb / tc, 4),
                  "fused_bytes_identical_to_plain": identical, "fused_vs_lerp_max_abs_difference": lerp_gap,
                  "note": "medians of the rounds; host clock around reps calls ending in a synchronise; the expectation is fused below composed and near 9/7 of plain"})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
