"""The TRAINING-mode forward of the relative decoders (RDM_Net.py:57-61,106-125) in f32 and bf16 (set_relative_train_precision), one process:
  * the train-mode feature maps of d_6..d_10 at B=8 228x228 on the f32 plan's encoder output (the bf16 figure includes the one shared
    conversion of that output to bf16 and its column statistics);
  * a whole training step (forward, backward, fused AdamW) of DepthEstimationNet(relative_decoders=(6,7,8,9)) - the authors' best
    configuration, decoders 1, 6, 7, 8, 9 - at B=16 228x228.
One JSON line per figure.  `python tools/relative_bf16_train_bench.py [--out FILE]`"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, filler, harness  # noqa: E402
from md_rdm_amd.network.RDM_Net import DepthEstimationNet  # noqa: E402


def timeit(fn, reps=10, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    B, rel = 8, (6, 7, 8, 9, 10)
    m = DepthEstimationNet(relative_decoders=rel)
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).train()
    x = torch.from_numpy(filler.synthetic_batch(B, 228, 228, seed=3)[0]).to(dev)
    decs = [getattr(m, "d_%d" % d) for d in rel]
    with torch.no_grad():
        m._native_forward(x)
        enc32 = m.encoder_output()
        enc16 = torch.empty(B * 64, 1056, dtype=torch.bfloat16, device=dev)
        stats = torch.empty(2 * 1056, dtype=torch.float64, device=dev)

        def shared():
            _lib.check(L.rdm_rel_bf16_input_nchw(_lib.ptr(enc32), B, _lib.ptr(enc16), 1056, _lib.stream()))
            _lib.check(L.rdm_colstats_bf16(_lib.ptr(enc16), 1056, B * 64, 1056, _lib.ptr(stats[:1056]), _lib.ptr(stats[1056:]), _lib.stream()))

        shared()
        t_in = timeit(shared, reps=20)
        t32 = {d.id: timeit(lambda d=d: d.features(enc32), reps=3, warmup=1) for d in decs}
        t16 = {d.id: timeit(lambda d=d: d.features_bf16_train(enc16, 1056, B, stats)) for d in decs}
        for d in decs:
            emit({"figure": "train-mode feature map d_%d" % d.id, "batch": B, "f32_ms": round(t32[d.id], 3), "bf16_ms": round(t16[d.id], 3),
                  "speedup": round(t32[d.id] / t16[d.id], 2)})
        s32, s16 = sum(t32.values()), sum(t16.values()) + t_in
        emit({"figure": "train-mode feature maps d_6..d_10 (bf16: + shared input conversion and statistics %.3f ms)" % t_in, "batch": B,
              "f32_ms": round(s32, 3), "bf16_ms": round(s16, 3), "speedup": round(s32 / s16, 2), "bf16_over_f32": round(s16 / s32, 3)})
    del m, decs
    torch.cuda.empty_cache()

    B, rel = 16, (6, 7, 8, 9)
    xs, ys = filler.synthetic_batch(B, 228, 228, seed=filler.MARGIN_SEEDS["train228"])
    xs, ys = torch.from_numpy(xs).to(dev), torch.from_numpy(ys).to(dev)
    step_ms = {}
    for mode in ("f32", "bf16"):
        m = DepthEstimationNet(relative_decoders=rel)
        filler.fill_state_dict(m.state_dict())
        m = m.to(dev).train().set_relative_train_precision(mode)
        m.flatten_parameters()
        opt = harness.FusedAdamW(m, lr=1e-4)

        def step():
            opt.zero_grad()
            loss, _ = harness.training_step(m, xs, ys)
            loss.backward()
            opt.step()

        step_ms[mode] = timeit(step, reps=5, warmup=2)
        del m, opt
        torch.cuda.empty_cache()
    emit({"figure": "training step relative_decoders=(6,7,8,9) 228x228", "batch": B, "f32_ms": round(step_ms["f32"], 2), "bf16_ms": round(step_ms["bf16"], 2),
          "saved_ms": round(step_ms["f32"] - step_ms["bf16"], 2), "speedup": round(step_ms["f32"] / step_ms["bf16"], 2)})
    if args.out:
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
