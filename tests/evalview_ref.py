"""Float64 numpy restatement of rdm_eval_standard_view_f64 (include/rdm_eval_view.h) for tests/test_evalview_cpu.py and tests/test_gpu_evalview.py:
step 1 with a view - a bicubic sampler of its own, every fused step an explicit fma in the kernel's order (csrc/postproc_dev.h) - and steps 2 to 5
from tests/evalstd_ref.py.

numpy has no fused multiply-add, so ``fma`` forms one from error-free transformations: the product exactly as a pair (Veltkamp / Dekker), two
exact additions, and the sum of the two small parts rounded to ODD, after which one ordinary addition rounds correctly (Boldo and Melquiond,
"Emulation of a FMA and correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 2008).  Valid without overflow or underflow,
which map values and cubic coefficients of order one are far from; tests/test_evalview_cpu.py holds it against the C library's fma."""
import numpy as np

import evalstd_ref as ref

SIDE = 128


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                   # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_odd(x, y):
    s, e = _two_sum(x, y)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where((e != 0) & even, np.nextafter(s, toward), s)


def fma(a, b, c):
    """round(a * b + c), one rounding, elementwise in float64"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, ul)
    vh, vl = _two_sum(uh, th)
    return vh + _add_round_odd(tl, vl)


def full_view(h, w):
    return (0.0, 0.0, float(h), float(w))


def cubic_index_view(n_out, v0, vn, n_in=SIDE):
    """index (int64) and t of the n_out depth samples along one axis: real = fma(n_in / vn, (i + 0.5) - v0, -0.5), the float floor"""
    scale = np.float64(n_in) / np.float64(vn)
    pos = (np.arange(n_out, dtype=np.float64) + 0.5) - np.float64(v0)
    real = fma(scale, pos, -0.5)
    fl = np.clip(np.floor(real.astype(np.float32)), np.float32(-2.0 ** 62), np.float32(2.0 ** 62))
    idx = np.minimum(fl.astype(np.int64), n_in - 1)
    t = np.minimum(np.maximum(real - idx.astype(np.float64), 0.0), 1.0)
    return idx, t


def cubic_coeffs(t):
    A = -0.75
    x2 = 1.0 - t
    xa, xb = t + 1.0, x2 + 1.0
    return [fma(fma(A, xa, -5.0 * A), xa, 8.0 * A) * xa - 4.0 * A, fma(A + 2.0, t, -(A + 3.0)) * t * t + 1.0,
            fma(A + 2.0, x2, -(A + 3.0)) * x2 * x2 + 1.0, fma(fma(A, xb, -5.0 * A), xb, 8.0 * A) * xb - 4.0 * A]


def dot4(v, w):
    acc = v[1] * w[1]
    acc = fma(v[0], w[0], acc)
    acc = fma(v[2], w[2], acc)
    return fma(v[3], w[3], acc)


def resize_view(m, h, w, view=None):
    """the (B,1,128,128) map sampled at the (h, w) depth pixels under ``view`` = (vy0, vx0, vh, vw); None: the full frame.  Taps clamped to
    [0, 127]: outside the view the map's edge is replicated."""
    m = np.asarray(m, dtype=np.float64)
    vy0, vx0, vh, vw = full_view(h, w) if view is None else view
    iy, ty = cubic_index_view(h, vy0, vh)
    ix, tx = cubic_index_view(w, vx0, vw)
    cy = [c[:, None] for c in cubic_coeffs(ty)]
    cx = [c[None, :] for c in cubic_coeffs(tx)]
    ys = [np.clip(iy - 1 + i, 0, SIDE - 1) for i in range(4)]
    xs = [np.clip(ix - 1 + j, 0, SIDE - 1) for j in range(4)]
    out = np.empty(m.shape[:2] + (h, w))
    for b in range(m.shape[0]):
        for c in range(m.shape[1]):
            rows = [dot4([m[b, c][ys[i][:, None], xs[j][None, :]] for j in range(4)], cx) for i in range(4)]
            out[b, c] = dot4(rows, cy)
    return out


def prediction(log_map, h, w, view=None):
    """step 1 of include/rdm_eval_view.h: a 128x128 frame under the full view reads the map as it is"""
    m = np.asarray(log_map, dtype=np.float64)
    whole = view is None or tuple(float(v) for v in view) == full_view(h, w)
    r = m if (h, w) == (SIDE, SIDE) and whole else resize_view(m, h, w, view)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(r)


def reference(log_map, depth, align="median", min_depth=1e-3, max_depth=10.0, crop=None, view=None):
    """evalstd_ref.reference with the view's prediction as step 1: the same dict (rows, q, p, valid, margin, abs_rel, g_abs, sp_low, sp_high)"""
    whole = ref.prediction
    ref.prediction = lambda m, h, w: prediction(m, h, w, view)
    try:
        return ref.reference(log_map, depth, align, min_depth, max_depth, crop)
    finally:
        ref.prediction = whole
