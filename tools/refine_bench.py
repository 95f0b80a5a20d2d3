"""The guided-refinement launch (rdm_depth_refine, include/rdm_refine.h) against the composed torch path it replaces, B = 1 and 8 at the native
480x640 frame and at 226x226, for the default parameters (radius 3, step 4: 49 taps) and for radius 8, step 3 (289 taps), a quarter of the
pixels without a measurement, filling on, both planes, one process:
  (fused)     one launch: the tile and its halo staged in LDS, the tap loop, the divide, the float32 plane and the quantised 16-bit plane;
  (composed)  torch operators: F.unfold with dilation of the depth and of the guide to (B, taps, h w) intermediates, the colour and spatial
              weights (one float64 exp per tap, where the kernel multiplies table entries), the validity mask, the two sums over the taps,
              the divide, the cast and the quantisation.
Every figure is the time per call of `reps` back-to-back calls on one stream between two device events (host enqueue included: that is what a
caller pays), taken in `rounds` rounds that alternate the two candidates; reported: median, minimum and maximum over the rounds.  The composed
path gets fewer calls per window (it is slower by orders of magnitude; its windows are still tens of milliseconds).  Before timing, the fused
float32 plane is compared with the composed one on the timed input (relative 1e-6: the composed weights are not the contract's roundings).
`bytes` is what the fused launch must move through memory by its shapes: depth and guide read once (the halo re-reads of neighbouring tiles are
cache traffic and not in it), the two planes written; `composed_bytes` is the size of the composed path's two unfold results alone.
One JSON line per figure.  `python tools/refine_bench.py [--out FILE]`"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from md_rdm_amd import filler, refine  # noqa: E402


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                   # us per call


def alternate(cands, rounds, warmup=2):
    """{name: (fn, reps)} -> {name: [us per call, one per round]}: the candidates take turns inside every round."""
    for fn, _ in cands.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in cands}
    for _ in range(rounds):
        for k, (fn, reps) in cands.items():
            out[k].append(window(fn, reps))
    return out


def summary(v):
    return {"us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def composed_path(d, g, radius, step, sigma_space, sigma_color, fill, unit):
    B, h, w = d.shape
    K, halo, T = 2 * radius + 1, radius * step, (2 * radius + 1) ** 2
    gf = g.permute(0, 3, 1, 2).float().contiguous()
    off = torch.arange(-radius, radius + 1, dtype=torch.float64, device=d.device) * step
    wsp = torch.exp(-(off * off) / (2.0 * sigma_space * sigma_space))
    wsp = (wsp[:, None] * wsp[None, :]).reshape(1, T, 1)

    def run():
        valid = torch.isfinite(d) & (d > 0)
        dv = torch.where(valid, d, torch.zeros_like(d))
        D = F.unfold(dv[:, None], K, dilation=step, padding=halo)                                 # (B, T, h w); outside the frame: 0, not valid
        Gq = F.unfold(gf, K, dilation=step, padding=halo).view(B, 3, T, h * w)
        diff = Gq - gf.view(B, 3, 1, h * w)
        wgt = torch.exp(-(diff * diff).sum(1).double() / (2.0 * sigma_color * sigma_color)) * wsp * (D > 0)
        num, den = (wgt * D).sum(1).view(B, h, w), wgt.sum(1).view(B, h, w)
        ok = valid | (den > 0) if fill else valid
        Dd = num / den
        zero = torch.zeros_like(Dd)
        f32 = torch.where(ok, Dd, zero).float()
        u16 = torch.where(ok, torch.clamp(torch.round(Dd / unit), max=65535.0), zero).to(torch.int32)
        return f32, u16
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--composed_reps", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    for H, W in ((480, 640), (226, 226)):
        for B in (1, 8):
            d = filler.uniform("refine_bench.depth/%d/%d" % (H, B), (B, H, W), 0.5, 9.5).astype("float32")
            d[filler.unit("refine_bench.mask/%d/%d" % (H, B), B * H * W).reshape(B, H, W) < 0.25] = 0.0
            d = torch.from_numpy(d).to(dev)
            g = (filler.unit("refine_bench.rgb/%d/%d" % (H, B), B * (H // 8 + 1) * (W // 8 + 1) * 3) * 256.0).astype("uint8").reshape(B, H // 8 + 1, W // 8 + 1, 3)
            g = torch.from_numpy(g).to(dev).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()      # 8x8 blocks: equal colours occur
            for radius, step in ((3, 4), (8, 3)):
                sigma_space, sigma_color = radius * step / 2.0, 12.0
                fused = lambda: refine.joint_bilateral(d, g, radius=radius, step=step, sigma_color=sigma_color, fill=True, want=("f32", "u16"))
                composed = composed_path(d, g, radius, step, sigma_space, sigma_color, True, 1e-3)
                got, want = fused()["f32"], composed()[0]
                torch.cuda.synchronize()
                assert torch.equal(got == 0, want == 0), "the fused plane's invalid pixels differ from the composed ones"
                rel = float(((got - want).abs() / want.clamp(min=1e-3)).max())
                assert rel <= 1e-6, "the fused plane differs from the composed one by a relative %g" % rel
                del got, want
                taps = (2 * radius + 1) ** 2
                base = {"batch": B, "frame": [H, W], "radius": radius, "step": step, "taps": taps}
                t = alternate({"fused": (fused, args.reps), "composed": (composed, args.composed_reps)}, args.rounds)
                emit({"figure": "rdm_depth_refine", **base, "bytes": B * H * W * (4 + 3 + 4 + 2), **summary(t["fused"])})
                emit({"figure": "composed torch path", **base, "composed_bytes": B * H * W * taps * 4 * 4, **summary(t["composed"])})
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
