#!/usr/bin/env python3
"""Generate tests/golden/viz_goldens.npz by RUNNING THE REFERENCE's rendering functions (utils.py:71-91: colored_depthmap, merge_into_row)
with the matplotlib they import (3.10.8 when the committed fixture was written), followed by save_image's ``astype('uint8')`` (utils.py:116).

Runs only where the reference checkout exists (see make_golden.py); here ``utils.py`` imports as it is, no stand-ins.  Inputs come from
``md_rdm_amd.filler`` (re-derivable), only OUTPUTS are stored:
  lut8            (256,3)  colored_depthmap on the exact ramp (i + 0.5) / 256 over [0, 1]: the jet table, truncated to uint8
  cd_37x53        (2,37,53,3)   colored_depthmap of LU("viz.m128", (2,1,128,128), 0.5, 9.5), resized to 37x53, each image over its own range
  cd_16x16        (2,16,16,3)   ... of LU("viz.m8", (2,1,8,8), 0.5, 2.0), resized to 16x16
  rows_23x31      (2,23,93,3)   merge_into_row(x, target, pred): x = every k / 255 as float32, target LU("viz.t", (2,1,57,76), 0.5, 9.5) and pred
                                LU("viz.p", (2,1,16,16), 0.2, 4.0), both resized to 23x31
  rows_pred_23x31 (2,23,31,3)   colored_depthmap of that resized pred alone (the right panel of a two-panel row)
Resizing is the reference's ``resize`` (computations.py:308-311): float64 bicubic F.interpolate, align_corners=False.

Usage:  python tests/golden/make_viz_golden.py        (regenerates the file bit for bit)
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

import numpy as np
import torch
import torch.nn.functional as F

from md_rdm_amd import filler  # noqa: E402

LU = filler.log_uniform


def ref_resize(a, size):
    return F.interpolate(torch.from_numpy(a).double(), size=size, mode="bicubic", align_corners=False)


def rows_input():
    """(2,3,23,31) float32 holding every k / 255"""
    n = 2 * 3 * 23 * 31
    return ((np.arange(n) * 7 % 256).astype(np.float64) / 255.0).astype(np.float32).reshape(2, 3, 23, 31)


def main():
    sys.path.insert(0, REF)
    import utils as u
    u8 = lambda a: np.ascontiguousarray(a.astype("uint8"))
    out = {}
    ramp = ((np.arange(256) + 0.5) / 256.0).reshape(1, 256)
    out["lut8"] = u8(u.colored_depthmap(ramp, 0.0, 1.0))[0]
    for name, key, shape, lo, hi, size in (("cd_37x53", "viz.m128", (2, 1, 128, 128), 0.5, 9.5, (37, 53)), ("cd_16x16", "viz.m8", (2, 1, 8, 8), 0.5, 2.0, (16, 16))):
        r = ref_resize(LU(key, shape, lo, hi), size).numpy()
        out[name] = np.stack([u8(u.colored_depthmap(r[i, 0])) for i in range(shape[0])])
    x = torch.from_numpy(rows_input())
    t = ref_resize(LU("viz.t", (2, 1, 57, 76), 0.5, 9.5), (23, 31))
    p = ref_resize(LU("viz.p", (2, 1, 16, 16), 0.2, 4.0), (23, 31))
    out["rows_23x31"] = np.stack([u8(u.merge_into_row(x[i:i + 1], t[i:i + 1], p[i:i + 1])) for i in range(2)])
    out["rows_pred_23x31"] = np.stack([u8(u.colored_depthmap(p[i, 0].numpy())) for i in range(2)])
    path = os.path.join(HERE, "viz_goldens.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
