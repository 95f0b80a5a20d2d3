"""numpy restatement of the rendering semantics of include/rdm_viz.h (the reference's colored_depthmap / merge_into_row + astype('uint8'),
utils.py:71-91,116), for the tests: the jet table comes from the fixture (tests/golden/viz_goldens.npz, written by the reference's own
functions), resizing is the oracle's bit-exact bicubic."""
import os

import numpy as np

from conftest import GOLDEN

_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLDEN, "viz_goldens.npz"), allow_pickle=False) as z:
            _gold = {k: z[k] for k in z.files}
    return _gold


def resized(m, size):
    """(B,1,h,w) -> float64 (B,1,H,W); a map that already has the size is taken as it is"""
    m = np.asarray(m)
    if tuple(m.shape[2:]) == tuple(size):
        return m.astype(np.float64)
    from oracle import computations_cpu as ocp
    return ocp.resize(m, tuple(size))


def colour(v, lo, hi):
    """float64 array -> (..., 3) uint8: matplotlib's Colormap.__call__ on floats, then trunc(255 * rgb)"""
    with np.errstate(all="ignore"):
        xa = (np.asarray(v, dtype=np.float64) - lo) / (hi - lo) * 256.0
        inside = (xa >= 0) & (xa < 256.0)
    idx = np.zeros(xa.shape, dtype=np.int64)                 # xa < 0 (and NaN, blackened below)
    idx[inside] = xa[inside].astype(np.int64)                # truncation
    idx[xa >= 256.0] = 255                                   # xa == 256 and everything above
    out = gold()["lut8"][idx]
    out[np.isnan(xa)] = 0
    return out


def rows(x, target, pred, size, d_min=None, d_max=None):
    """[x | target | pred] -> (B,H,P*W,3) uint8; x (B,3,H,W) float32 or None, target (B,1,h,w) or None; range per image over its depth panels"""
    maps = [resized(m, size) for m in (target, pred) if m is not None]
    B = maps[0].shape[0]
    imgs = []
    for i in range(B):
        lo = min(np.min(m[i]) for m in maps) if d_min is None else d_min          # np.min propagates NaN
        hi = max(np.max(m[i]) for m in maps) if d_max is None else d_max
        if d_min is None and any(np.isnan(m[i]).any() for m in maps):
            lo = np.nan
        if d_max is None and any(np.isnan(m[i]).any() for m in maps):
            hi = np.nan
        panels = [colour(m[i, 0], lo, hi) for m in maps]
        if x is not None:
            xi = np.asarray(x[i])
            assert xi.dtype == np.float32
            panels.insert(0, np.transpose(np.float32(255.0) * xi, (1, 2, 0)).astype(np.uint8))
        imgs.append(np.hstack(panels))
    return np.stack(imgs)


def colorize(maps, size=None, d_min=None, d_max=None):
    maps = np.asarray(maps)
    return rows(None, None, maps, tuple(maps.shape[2:]) if size is None else size, d_min, d_max)
