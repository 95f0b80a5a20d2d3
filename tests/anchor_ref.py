"""Float64 numpy statement of include/rdm_anchor.h for tests/test_anchor_cpu.py and tests/test_gpu_anchor.py: the cell sums in the header's
order (a lane's pixels in sequence, then the lane tree), the fit, the re-centring, the separable normalised convolution with the host-made tap
table (Python's ``math.exp``: the C library's, as the launcher's), the field, and the corrected frames.  ``R_view`` is
tests/evalview_ref.py's ``resize_view`` (bit-exact with the device arithmetic), the frame arithmetic tests/depthframe_ref.py's.  The one step
that is not bit-exact against the device is ``ln`` (``log=`` lets a test replace it, to measure what a perturbed logarithm does)."""
import math

import numpy as np

import depthframe_ref as dref
import evalview_ref as vref

FIT_NONE, FIT_LOGMEAN = 0, 1
MAX_CELLS, MAX_RADIUS = 5120, 96


def cdiv(a, b):
    return (a + b - 1) // b


def residuals(log_map, anchors, view=None, prior=None, min_depth=0.0, max_depth=math.inf, reject=math.inf, log=np.log):
    """(r (B,h,w) float64, keep (B,h,w) bool, v (B,h,w)): the residual of every pixel and whether it is an anchor that passes the gate"""
    a = np.asarray(anchors, dtype=np.float32)
    B, h, w = a.shape
    v = vref.resize_view(np.asarray(log_map, dtype=np.float64).reshape(B, 1, vref.SIDE, vref.SIDE), h, w, view)[:, 0]
    a64 = a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(a) & (a > 0) & (a64 >= np.float64(min_depth)) & (a64 <= np.float64(max_depth)) & dref.inside_mask(h, w, view)[None]
    p = np.zeros(B) if prior is None else np.asarray(prior, dtype=np.float64).reshape(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = log(np.where(valid, a64, 1.0)) - v
        r = r - p[:, None, None]
        keep = valid & ~(np.abs(r) > np.float64(reject))
    return r, keep, v


def lane_tree_sum(vals):
    """the header's order for the values of one cell in pixel order p: lane l adds p = l, l + 64, ... to 0.0 in sequence, then the fold 32 .. 1"""
    vals = np.asarray(vals, dtype=np.float64)
    pad = (-len(vals)) % 64
    t = np.zeros(64)
    for row in np.concatenate([vals, np.zeros(pad)]).reshape(-1, 64):
        t = t + row
    o = 32
    while o:
        t = t[:o] + t[o:2 * o]
        o >>= 1
    return t[0]


def cells(log_map, anchors, cell, view=None, prior=None, min_depth=0.0, max_depth=math.inf, reject=math.inf, log=np.log):
    """launch 1: (n (B,gy,gx) int32, s (B,gy,gx) float64).  A pixel that is not kept adds 0.0, which leaves every partial sum's bits alone."""
    r, keep, _ = residuals(log_map, anchors, view, prior, min_depth, max_depth, reject, log)
    B, h, w = keep.shape
    gy, gx = cdiv(h, cell), cdiv(w, cell)
    n, s = np.zeros((B, gy, gx), dtype=np.int32), np.zeros((B, gy, gx))
    rz = np.where(keep, r, 0.0)
    for b in range(B):
        for cy in range(gy):
            for cx in range(gx):
                sl = (b, slice(cy * cell, min((cy + 1) * cell, h)), slice(cx * cell, min((cx + 1) * cell, w)))
                n[b, cy, cx] = int(keep[sl].sum())
                s[b, cy, cx] = lane_tree_sum(rz[sl].reshape(-1))
    return n, s


def taps(sigma):
    """g[0 .. Rg], Rg = ceil(3 * sigma): g[0] = 1.0 set, the rest exp(-(k * k) / (2 * (sigma * sigma))) with the C library's exp"""
    rg = int(math.ceil(3.0 * float(sigma)))
    two_s2 = 2.0 * (float(sigma) * float(sigma))
    return np.array([1.0] + [math.exp(-(float(k) * float(k)) / two_s2) for k in range(1, rg + 1)])


def smooth_axis(P, g, axis):
    """acc from 0.0, k ascending from -Rg to Rg, taps beyond the border skipped: acc = acc + g[|k|] * P(.. + k ..); a skipped tap adds nothing,
    so the cells it would have reached are left out of that step (not given a zero, which a NaN or an infinity in P would turn into a NaN)"""
    P = np.moveaxis(np.asarray(P, dtype=np.float64), axis, -1)
    n = P.shape[-1]
    acc = np.zeros_like(P)
    rg = len(g) - 1
    for k in range(-min(rg, n - 1), min(rg, n - 1) + 1):
        lo, hi = max(0, -k), min(n, n - k)                                   # the cells i with 0 <= i + k < n
        acc[..., lo:hi] = acc[..., lo:hi] + g[abs(k)] * P[..., lo + k:hi + k]
    return np.moveaxis(acc, -1, axis)


def field(n, s, prior=None, fit=FIT_LOGMEAN, sigma=2.0, lam=1.0, want_field=True):
    """launch 2: (ls (B,), count (B,) int32, field (B,gy,gx) | None)"""
    n, s = np.asarray(n, dtype=np.int32), np.asarray(s, dtype=np.float64)
    B = n.shape[0]
    count = n.reshape(B, -1).astype(np.int64).sum(axis=1)
    delta = np.zeros(B)
    if fit == FIT_LOGMEAN:
        for b in range(B):
            if count[b] > 0:
                acc = np.float64(0.0)
                for x in s[b].reshape(-1):                                  # row-major, one by one
                    acc = acc + x
                delta[b] = acc / np.float64(count[b])
    else:
        assert fit == FIT_NONE, fit
    p = np.zeros(B) if prior is None else np.asarray(prior, dtype=np.float64).reshape(B)
    ls = p + delta
    if not want_field:
        return ls, count.astype(np.int32), None
    nd = n.astype(np.float64)
    sc = s - nd * delta[:, None, None]
    g = taps(sigma)
    with np.errstate(invalid="ignore", over="ignore"):
        N = smooth_axis(smooth_axis(sc, g, 2), g, 1)
        W = smooth_axis(smooth_axis(nd, g, 2), g, 1)
        den = W + np.float64(lam)
        F = np.where(den == 0.0, 0.0, N / np.where(den == 0.0, 1.0, den))
    return ls, count.astype(np.int32), F


def lerp_axis(n_out, cell, n_cells):
    """(i0, i1, t) of the n_out output coordinates along one axis: u = (i + 0.5) / cell; u = u - 0.5; f = floor(u); t = u - f; clamped indices"""
    u = (np.arange(n_out, dtype=np.float64) + 0.5) / np.float64(cell)
    u = u - 0.5
    f = np.floor(u)
    i = f.astype(np.int64)
    return np.clip(i, 0, n_cells - 1), np.clip(i + 1, 0, n_cells - 1), u - f


def field_at_pixels(F, h, w, cell):
    """c (B,h,w): top = fma(tx, F(i0,j1) - F(i0,j0), F(i0,j0)); bot likewise on row i1; c = fma(ty, bot - top, top)"""
    F = np.asarray(F, dtype=np.float64)
    B, gy, gx = F.shape
    assert (gy, gx) == (cdiv(h, cell), cdiv(w, cell))
    i0, i1, ty = lerp_axis(h, cell, gy)
    j0, j1, tx = lerp_axis(w, cell, gx)
    tx, ty = np.broadcast_to(tx[None, None, :], (B, h, w)), np.broadcast_to(ty[None, :, None], (B, h, w))
    a0, a1 = F[:, i0][:, :, j0], F[:, i1][:, :, j0]
    top = vref.fma(tx, F[:, i0][:, :, j1] - a0, a0)
    bot = vref.fma(tx, F[:, i1][:, :, j1] - a1, a1)
    return vref.fma(ty, bot - top, top)


def frames(log_map, h, w, ls, F=None, cell=1, view=None, unit=1e-3, outside="zero"):
    """launch 3 with counts NULL: depthframe_ref.reference's dict for D = exp((v + ls_b) + c(y, x)); F None: no field (rdm_depth_frames)"""
    m = np.asarray(log_map, dtype=np.float64).reshape(-1, 1, vref.SIDE, vref.SIDE)
    B = m.shape[0]
    lsb = dref.log_scale(B, None, ls)
    e = vref.resize_view(m, h, w, view)[:, 0] + lsb[:, None, None]
    if F is not None:
        e = e + field_at_pixels(F, h, w, cell)
    with np.errstate(over="ignore", invalid="ignore"):
        D = np.exp(e)
        f32 = D.astype(np.float32)
    u16, q = dref.quantise(D, unit)
    with np.errstate(invalid="ignore"):
        critical = np.abs(q - (np.floor(q) + 0.5)) <= 1e-9 * np.maximum(q, 1.0)
    critical &= np.isfinite(q) & (q < 65535.5)
    inside = dref.inside_mask(h, w, view)
    if outside == "zero":
        D, f32, u16 = np.where(inside[None], D, 0.0), np.where(inside[None], f32, np.float32(0.0)), np.where(inside[None], u16, np.uint16(0))
        critical = critical & inside[None]
    else:
        assert outside == "edge", outside
    return dict(ls=lsb, D=D, f32=f32, u16=u16, inside=inside, critical=critical)


def median_log_scale(log_map, anchors, view=None, prior=None, min_depth=0.0, max_depth=math.inf):
    """fit="median": ln(median(a_valid) / median(exp(v)_valid)) per sample, valid by rdm_eval_standard_view_f64's rule (finite,
    min_depth < a < max_depth) among the pixels whose centre is inside the view; a sample without one keeps its prior (or 0)"""
    a = np.asarray(anchors, dtype=np.float32)
    B, h, w = a.shape
    v = vref.resize_view(np.asarray(log_map, dtype=np.float64).reshape(B, 1, vref.SIDE, vref.SIDE), h, w, view)[:, 0]
    a64 = a.astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(a) & (a64 > np.float64(min_depth)) & (a64 < np.float64(max_depth)) & dref.inside_mask(h, w, view)[None]
    out = np.zeros(B) if prior is None else np.asarray(prior, dtype=np.float64).reshape(B).copy()
    for b in range(B):
        if valid[b].any():
            out[b] = np.log(np.median(a64[b][valid[b]]) / np.median(np.exp(v[b][valid[b]])))
    return out


def fit(log_map, anchors, view=None, prior=None, fit="logmean", cell=16, sigma=2.0, lam=1.0, reject=None, min_depth=0.0, max_depth=math.inf, want_field=True,
        log=np.log):
    """md_rdm_amd.anchor.fit: dict(log_scale, count, field, cell, n, s)"""
    if fit == "median":
        prior = median_log_scale(log_map, anchors, view, prior, min_depth, max_depth)
    n, s = cells(log_map, anchors, cell, view, prior, min_depth, max_depth, math.inf if reject is None else reject, log)
    ls, count, F = field(n, s, prior, FIT_LOGMEAN if fit == "logmean" else FIT_NONE, sigma, lam, want_field)
    return dict(log_scale=ls, count=count, field=F, cell=cell, n=n, s=s)


def ln_bounds(log_map, anchors, cell, view=None, prior=None, fit=FIT_LOGMEAN, sigma=2.0, lam=1.0, reject=math.inf, min_depth=0.0, max_depth=math.inf, ulps=2.0):
    """How far the outputs of launches 1 and 2 of two implementations of the header may lie apart when their float64 logarithms differ by up
    to ``ulps`` units in the last place in all (1 ulp each for the device's and for the C library's documented error) and every other step is
    the same IEEE operation in the same order: dict(s, ls, field), arrays like the outputs.  With u = 2^-53 and ulp(x) numpy's spacing:
      e_r    = ulps * ulp(max |ln a|) + ulp(max |ln a - v|) + ulp(max |r|): the logarithm, then the two subtractions, each of which may round
               the other way on a perturbed operand;
      E_s    = n_c * e_r + 2 (n_c + 6) u (sum |r| + n_c * e_r): the perturbations add up, and each of the at most n_c + 6 additions on a path of
               the lane-then-tree order may round the other way (relative 2u of the partial sums, which sum |r| bounds);
      E_S    = sum E_s + 2 cells u (sum |s_c| + sum E_s);  E_delta = E_S / n_b + ulp(delta);  E_ls = E_delta + ulp(ls);
      E_s'   = E_s + n_c * E_delta + 2 ulp(|s_c| + n_c |delta|): the product and the subtraction of the re-centring;
      E_N    = G(E_s') + 4 T u (G(|s'|) + G(E_s')), G the two smoothing passes (positive weights) and T = 2 Rg + 1 their taps;  W is exact;
      E_C    = E_N / (W + lambda) + ulp(C): a normalised weighted mean carries the bound through, the division rounds once more.
    The gate and the validity tests must decide alike on both sides: the caller asserts n_c equal."""
    r, keep, v = residuals(log_map, anchors, view, prior, min_depth, max_depth, reject)
    B, h, w = keep.shape
    a64 = np.asarray(anchors, dtype=np.float32).astype(np.float64)
    L = np.log(np.where(keep, a64, 1.0))
    u = 2.0 ** -53
    mx = lambda x: float(np.abs(np.where(keep, x, 0.0)).max())
    e_r = ulps * np.spacing(mx(L)) + np.spacing(mx(L - v)) + np.spacing(mx(r))
    n, s = cells(log_map, anchors, cell, view, prior, min_depth, max_depth, reject)
    gy, gx = n.shape[1:]
    A = np.zeros_like(s)
    ra = np.where(keep, np.abs(r), 0.0)
    for cy in range(gy):
        for cx in range(gx):
            A[:, cy, cx] = ra[:, cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell].sum(axis=(1, 2))
    nd = n.astype(np.float64)
    E_s = nd * e_r + 2.0 * (nd + 6.0) * u * (A + nd * e_r)
    ls, count, F = field(n, s, prior, fit, sigma, lam)
    p = np.zeros(B) if prior is None else np.asarray(prior, dtype=np.float64).reshape(B)
    delta = ls - p
    E_delta = np.zeros(B)
    if fit == FIT_LOGMEAN:
        tot = E_s.reshape(B, -1).sum(axis=1)
        E_S = tot + 2.0 * gy * gx * u * (np.abs(s).reshape(B, -1).sum(axis=1) + tot)
        E_delta = np.where(count > 0, E_S / np.maximum(count, 1) + np.spacing(np.abs(delta)), 0.0)
    E_ls = E_delta + np.spacing(np.abs(ls))
    E_sp = E_s + nd * E_delta[:, None, None] + 2.0 * np.spacing(np.abs(s) + nd * np.abs(delta)[:, None, None])
    g = taps(sigma)
    G = lambda P: smooth_axis(smooth_axis(P, g, 2), g, 1)
    sp = s - nd * delta[:, None, None]
    T = 2 * (len(g) - 1) + 1
    E_N = G(E_sp) + 4.0 * T * u * (G(np.abs(sp)) + G(E_sp))
    den = G(nd) + lam
    E_C = np.where(den > 0, E_N / np.where(den > 0, den, 1.0) + np.spacing(np.abs(F)), 0.0)
    return dict(s=E_s, ls=E_ls, field=E_C)
