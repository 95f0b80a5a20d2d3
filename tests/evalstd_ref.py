"""Float64 numpy restatement of the standard evaluation protocol (include/rdm_eval.h, steps 1-5) and of StandardMetrics.values_from_rows,
for tests/test_evalstd_cpu.py and tests/test_gpu_evalstd.py.  The bicubic resize is the oracle's (oracle/computations_cpu.py, bit-exact with the
reference's torch CPU path); every sum is math.fsum, so the restatement's own error is one rounding per column."""
import math

import numpy as np

from oracle import computations_cpu as ocp

COLS = 16
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
NAMES = ("delta1", "delta2", "delta3", "abs_rel", "sq_rel", "rmse", "rmse_log", "silog", "log10", "mae", "scale")


def median(a):
    """numpy's median, restated: the middle order statistic for odd n, (a + b) / 2 of the two middle ones for even n"""
    s = np.sort(np.asarray(a, dtype=np.float64).ravel())
    n = s.size
    return float(s[(n - 1) // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def prediction(log_map, h, w):
    """step 1: exp of the map resized bicubically to (h, w); a 128x128 frame reads the map as it is"""
    m = np.asarray(log_map, dtype=np.float64)
    r = m if (h, w) == (128, 128) else ocp.resize(m, (h, w))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(r)


def valid_mask(depth, min_depth, max_depth, crop=None):
    d = np.asarray(depth, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v = np.isfinite(d) & (d > min_depth) & (d < max_depth)
    if crop is not None:
        y0, x0, y1, x1 = crop
        inside = np.zeros(d.shape, dtype=bool)
        inside[..., y0:y1, x0:x1] = True
        v &= inside
    return v


def reference(log_map, depth, align="median", min_depth=1e-3, max_depth=10.0, crop=None):
    """-> dict: rows (B,16), q (B,1,h,w) the aligned clamped prediction at every pixel (s = 1 where the row is zeros or NaN), sp_low / sp_high
    (B,) valid pixels clamped at each end, margin (B,) the smallest |maxratio / 1.25^k - 1| over the valid pixels (inf without one),
    abs_rel (B,) the mean of |q-d|/d (nan without a valid pixel), g_abs (B,) sum |ln q - ln d| (what column 8, the one signed sum, cancels from)."""
    d = np.asarray(depth, dtype=np.float64)
    B, _, h, w = d.shape
    p = prediction(log_map, h, w)
    valid = valid_mask(d, min_depth, max_depth, crop)
    rows, q = np.zeros((B, COLS)), np.empty_like(p)
    margin, abs_rel, g_abs = np.full(B, np.inf), np.full(B, np.nan), np.zeros(B)
    low, high = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b in range(B):
        v = valid[b, 0]
        dv, pv = d[b, 0][v], p[b, 0][v]
        n = dv.size
        ok = n > 0 and bool(np.isfinite(pv).all())
        s, sd, sp_ = 1.0, 0.0, 0.0
        with np.errstate(all="ignore"):
            if ok and align == "median":
                sd, sp_ = median(dv), median(pv)
                s = np.float64(sd) / np.float64(sp_)
            elif ok and align == "logmean":
                sd, sp_ = math.fsum(np.log(dv)) / n, math.fsum(np.log(pv)) / n
                s = math.exp(sd - sp_)
            elif align not in ("none", "median", "logmean"):
                raise ValueError(align)
            raw = s * p[b, 0]
            q[b, 0] = np.where(raw < min_depth, min_depth, np.where(raw > max_depth, max_depth, raw))
            if n == 0:
                continue
            if not ok:
                rows[b] = [n] + [np.nan] * 13 + [0.0, 0.0]
                continue
            qv, rv = q[b, 0][v], raw[v]
            ratio = np.maximum(qv / dv, dv / qv)
            e, g = qv - dv, np.log(qv) - np.log(dv)
            low[b], high[b] = int((rv < min_depth).sum()), int((rv > max_depth).sum())
            rows[b] = [n] + [float((ratio < t).sum()) for t in THRESHOLDS] + [
                math.fsum(np.abs(e) / dv), math.fsum(e * e / dv), math.fsum(e * e), math.fsum(g * g), math.fsum(g), math.fsum(np.abs(np.log10(qv) - np.log10(dv))),
                math.fsum(np.abs(e)), float(s), sd, sp_, float(low[b] + high[b]), 0.0]
            margin[b] = min(float(np.abs(ratio / t - 1.0).min()) for t in THRESHOLDS)
            abs_rel[b], g_abs[b] = rows[b, 4] / n, math.fsum(np.abs(g))
    return dict(rows=rows, q=q, p=p, valid=valid, margin=margin, abs_rel=abs_rel, g_abs=g_abs, sp_low=low, sp_high=high)


def values_from_rows(rows, names=NAMES):
    """the table of metrics.StandardMetrics: one list per row, None for n = 0"""
    out = []
    for r in np.asarray(rows, dtype=np.float64).reshape(-1, COLS):
        n = r[0]
        if not n > 0:
            out.append(None)
            continue
        with np.errstate(invalid="ignore"):
            g2, g1 = r[7] / n, r[8] / n
            v = dict(delta1=r[1] / n, delta2=r[2] / n, delta3=r[3] / n, abs_rel=r[4] / n, sq_rel=r[5] / n, rmse=np.sqrt(r[6] / n), rmse_log=np.sqrt(g2),
                     silog=100.0 * np.sqrt(np.maximum(g2 - g1 * g1, 0.0)), log10=r[9] / n, mae=r[10] / n, scale=r[11])
        out.append([float(v[m]) for m in names])
    return out
