"""The relative decoders d_6..d_10 (RDM_Net.py:57-61,106-125) in f32 and bf16, one process, one input (B=8 228x228 unless given):
  * the five decoders' feature maps (dense block -> WSM chain -> conv1) on the encoder output of each path;
  * the whole eval forward of DepthEstimationNet(relative_decoders=(6,7,8,9,10)) in both precisions;
  * the WSM bf16 conv kernel (csrc/wsm_bf16.hip) at the WSM_4 and WSM_1 5x5 shapes, fraction of the ~2.5 PF dense bf16 MFMA peak.
One JSON line per figure.  `python tools/relative_bf16_bench.py [--batch 8] [--out FILE]`"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import _lib, filler  # noqa: E402
from md_rdm_amd.network.RDM_Net import DepthEstimationNet  # noqa: E402

BF16_PEAK_TF = 2500.0
REL = (6, 7, 8, 9, 10)


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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B = args.batch
    dev = torch.device("cuda:0")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    m = DepthEstimationNet(relative_decoders=REL)
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    x = torch.from_numpy(filler.synthetic_batch(B, 228, 228, seed=3)[0]).to(dev)
    decs = [getattr(m, "d_%d" % d) for d in REL]
    with torch.no_grad():
        m._native_forward(x)
        enc32 = m.encoder_output()
        m.set_precision("bf16")
        m._native_forward_bf16(x)
        enc16 = m.encoder_output_bf16()
        t32 = {d.id: timeit(lambda d=d: d.features(enc32), reps=3, warmup=1) for d in decs}
        t16 = {d.id: timeit(lambda d=d: d.features_bf16(enc16, 1056, B)) for d in decs}
        for d in decs:
            emit({"figure": "feature map d_%d" % d.id, "batch": B, "f32_ms": round(t32[d.id], 3), "bf16_ms": round(t16[d.id], 3),
                  "speedup": round(t32[d.id] / t16[d.id], 2)})
        s32, s16 = sum(t32.values()), sum(t16.values())
        emit({"figure": "feature maps d_6..d_10", "batch": B, "f32_ms": round(s32, 3), "bf16_ms": round(s16, 3), "speedup": round(s32 / s16, 2)})
        m.set_precision("f32")
        f32 = timeit(lambda: m(x), reps=3, warmup=1)
        m.set_precision("bf16")
        b16 = timeit(lambda: m(x), reps=5, warmup=1)
        emit({"figure": "eval forward relative_decoders=(6,7,8,9,10) 228x228", "batch": B, "f32_ms": round(f32, 3), "bf16_ms": round(b16, 3),
              "speedup": round(f32 / b16, 2)})
    L = _lib.lib()
    for name, S, cin, n in (("WSM_4 conv2_2 5x5 52->52 @128x128", 128, 64, 52), ("WSM_1 conv2_2 5x5 416->416 @16x16", 16, 416, 416)):
        xb = torch.randn(B * S * S, cin, device=dev).to(torch.bfloat16)
        w = (torch.randn((n + 63) // 64 * 64, 25 * cin, device=dev) * 0.02).to(torch.bfloat16)
        bias = torch.zeros(n, device=dev)
        out = torch.empty(B * S * S, n, dtype=torch.bfloat16, device=dev)
        t = timeit(lambda: _lib.check(L.rdm_wsm_conv_bf16(_lib.ptr(xb), cin, 0, cin, _lib.ptr(w), _lib.ptr(bias), n, _lib.ptr(out), n, 0, B, S, S, 5,
                                                          _lib.stream())), reps=20)
        real_cin = 52 if cin == 64 else cin
        fl = 2.0 * B * S * S * n * real_cin * 25
        emit({"kernel": name + " B=%d" % B, "ms": round(t, 4), "algorithmic_GFLOP": round(fl / 1e9, 2), "achieved_TFLOPs": round(fl / t / 1e9, 1),
              "bf16_peak_TFLOPs": BF16_PEAK_TF, "frac": round(fl / t / 1e9 / BF16_PEAK_TF, 4)})
    if args.out:
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
