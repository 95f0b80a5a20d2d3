"""The predict path (DepthEstimationNet.predict, rdm_predict_tail_f32) at B = 1, 8, 16 with the 8x8 head (226x226 inputs), one process:
  (a) the composed tail as forward + recombination run it, from the logits tensor to the log map (rdm_dorn_fwd, the float64 cast,
      rdm_gm_normalize_f64, the float32 cast, rdm_decompose_f64, rdm_fine_detail_pred_f32, rdm_recombine_f64 and the torch glue between them);
  (b) the fused launch rdm_predict_tail_f32 at the library's default row split, and the sweep over the split S;
  (c) predict end to end at both precisions beside the bare forward, and forward + composed tail (what predict replaced).
Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is what a
caller pays), taken in `rounds` rounds that alternate the candidates; reported: median, minimum and maximum over the rounds.  Before timing,
(a) and (b) are compared on the timed input (counts equal, maps at 1e-4 of the maximum).
One JSON line per figure.  `python tools/predict_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, filler  # noqa: E402
from md_rdm_amd.network import computations as cp  # noqa: E402
from md_rdm_amd.network.RDM_Net import DepthEstimationNet  # noqa: E402


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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    wl = m.weight_layer
    wv = torch.cat([wl.get(k).detach().reshape(-1)[:1].float() for k in range(4)]).contiguous()

    with torch.no_grad():
        for B in (1, 8, 16):
            x = torch.from_numpy(filler.synthetic_batch(B, 226, 226, seed=filler.MARGIN_SEEDS["eval226"])[0]).to(dev)
            logits = m._native_forward(x).clone()
            out = torch.empty(B, 1, 128, 128, dtype=torch.float64, device=dev)

            def composed():
                dec, _ = cp.dorn_ordinal_regression(logits)
                norm = cp.gm_normalize(dec, 1.0 / 64).float()
                y = wl(cp.relative_fine_detail_matrix([cp.decompose_depth_map([], norm, 3)[::-1]], True))
                return cp.recombination(list(y)), dec

            def fused(split=0, decode=None):
                _lib.check(L.rdm_predict_tail_f32(_lib.ptr(logits), _lib.ptr(wv), _lib.ptr(out), _lib.ptr(decode), None, B, 90, 8, 8, 7, split, _lib.stream()))

            ref, ref_dec = composed()
            dec = torch.empty(B, 1, 8, 8, dtype=torch.int64, device=dev)
            fused(0, dec)
            torch.cuda.synchronize()
            diff = float((out - ref).abs().max())
            assert torch.equal(dec, ref_dec) and diff <= 1e-4 * float(ref.abs().max()), diff
            emit({"figure": "fused vs composed tail on the timed input", "batch": B, "max_abs_diff": diff, "max_abs_ref": float(ref.abs().max()), "counts_equal": True})

            t = alternate({"composed": composed, "fused": fused}, reps=200, rounds=args.rounds)
            a, b = summary(t["composed"]), summary(t["fused"])
            emit({"figure": "(a) composed tail, logits -> log map", "batch": B, **a})
            emit({"figure": "(b) fused tail rdm_predict_tail_f32, default split", "batch": B, **b, "speedup_vs_a": round(a["us"] / b["us"], 1)})
            sweep = alternate({str(s): (lambda s=s: fused(s)) for s in (1, 2, 4, 8, 16, 32, 64, 128)}, reps=500, rounds=args.rounds)
            emit({"figure": "(b) fused tail, sweep over the row split S (us per call: median [min, max])", "batch": B,
                  "S": {k: [summary(v)["us"], summary(v)["min_us"], summary(v)["max_us"]] for k, v in sweep.items()}})

            for prec in ("f32", "bf16"):
                m.set_precision(prec)
                fwd = (lambda: m._native_forward_bf16(x)) if prec == "bf16" else (lambda: m._native_forward(x))

                def old():
                    return cp.recombination(list(m(x)[0]))

                t = alternate({"forward": fwd, "predict": lambda: m.predict(x), "forward+composed": old}, reps=20, rounds=args.rounds)
                f, p, o = summary(t["forward"]), summary(t["predict"]), summary(t["forward+composed"])
                emit({"figure": "(c) predict end to end", "batch": B, "precision": prec, "forward_us": f["us"], "forward_min_max": [f["min_us"], f["max_us"]],
                      "predict_us": p["us"], "predict_min_max": [p["min_us"], p["max_us"]], "forward_plus_composed_tail_us": o["us"],
                      "forward_plus_composed_min_max": [o["min_us"], o["max_us"]], "images_per_s": round(B / (p["us"] * 1e-6), 1)})
            m.set_precision("f32")
    if args.out:
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
