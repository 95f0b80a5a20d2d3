"""Float64 numpy statement of rdm_depth_frames (include/rdm_depth.h) for tests/test_depthframe_cpu.py and tests/test_gpu_depthframe.py: the
per-sample log scale in the header's order of operations (A and Bc from Python's ``math.log``, the C library's), the resampling of
tests/evalview_ref.py (``resize_view``: bit-exact with the device arithmetic), ``exp``, the float32 plane, the quantised plane, and the mask
of ROUNDING-CRITICAL pixels - those whose quotient D / unit lies within 1e-9 * max(q, 1) of a half-integer, where the device's exponential
(some float64 ulps from numpy's) may round the other way."""
import math

import numpy as np

import evalview_ref as vref

SIDE = vref.SIDE
SID = {"nyu": (0.02, 10.0, 90.0), "kitti": (0.001, 80.0, 71.0), "floorplan3d": (0.0552, 10.0, 68.0), "Structured3D": (0.02, 10.0, 68.0)}


def log_scale(batch, counts=None, log_scale=None, sid="nyu", offset=0.0):
    """ls_b (batch,) float64: S_b + (log_scale ? log_scale[b] : 0); S_b = A + Bc * ((double)sum_b / count_n + offset) / K with counts, else 0"""
    S = np.zeros(batch, dtype=np.float64)
    if counts is not None:
        alpha, beta, K = SID[sid] if isinstance(sid, str) else sid
        A, Bc = np.float64(math.log(alpha)), np.float64(math.log(beta / alpha))
        c = np.asarray(counts, dtype=np.int64).reshape(batch, -1)
        x = c.sum(axis=1).astype(np.float64) / np.float64(c.shape[1])
        x = x + np.float64(offset)
        x = Bc * x
        x = x / np.float64(K)
        S = A + x
    return S + (np.asarray(log_scale, dtype=np.float64).reshape(batch) if log_scale is not None else np.float64(0.0))


def inside_mask(h, w, view=None):
    """(h, w) bool: the pixel's centre (y + 0.5, x + 0.5) lies in [vy0, vy0 + vh) x [vx0, vx0 + vw), the sums formed in float64"""
    vy0, vx0, vh, vw = (np.float64(v) for v in (vref.full_view(h, w) if view is None else view))
    cy, cx = np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5
    return ((cy >= vy0) & (cy < vy0 + vh))[:, None] & ((cx >= vx0) & (cx < vx0 + vw))[None, :]


def quantise(D, unit):
    """(u16 plane, q): NaN -> 0, q >= 65535 -> 65535, else rint (ties to even)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = D / np.float64(unit)
    u = np.zeros(q.shape, dtype=np.uint16)
    big = q >= 65535.0
    u[big] = 65535
    mid = ~big & ~np.isnan(q)
    u[mid] = np.rint(q[mid]).astype(np.uint16)
    return u, q


def reference(log_map, h, w, view=None, counts=None, log_scale_in=None, sid="nyu", offset=0.0, unit=1e-3, outside="zero"):
    """dict: ls (B,), D (B,h,w) float64, f32, u16, inside (h,w) bool, critical (B,h,w) bool"""
    m = np.asarray(log_map, dtype=np.float64).reshape(-1, 1, SIDE, SIDE)
    B = m.shape[0]
    ls = log_scale(B, counts, log_scale_in, sid, offset)
    with np.errstate(over="ignore", invalid="ignore"):
        D = np.exp(vref.resize_view(m, h, w, view)[:, 0] + ls[:, None, None])
        f32 = D.astype(np.float32)
    u16, q = quantise(D, unit)
    with np.errstate(invalid="ignore"):
        critical = np.abs(q - (np.floor(q) + 0.5)) <= 1e-9 * np.maximum(q, 1.0)
    critical &= np.isfinite(q) & (q < 65535.5)
    inside = inside_mask(h, w, view)
    if outside == "zero":
        D = np.where(inside[None], D, 0.0)
        f32 = np.where(inside[None], f32, np.float32(0.0))
        u16 = np.where(inside[None], u16, np.uint16(0))
        critical = critical & inside[None]
    else:
        assert outside == "edge", outside
    return dict(ls=ls, D=D, f32=f32, u16=u16, inside=inside, critical=critical)
