"""include/rdm_refine.h restated in numpy float64: the planes rdm_depth_refine must write.  Plain loops over the taps (j outer, i inner, ascending),
whole planes per tap; every float64 step is one numpy operation on arrays (numpy contracts nothing), in the header's order.  A tap that the
header skips adds an exact 0.0 here, which leaves both sums as they are (they are never -0.0)."""
import numpy as np


def valid_mask(depth):
    """finite and > 0"""
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0)


def tables(radius, step, sigma_space, sigma_color):
    """(ws (radius + 1,), E (256,)) float64; entry 0 of each is set to 1.0, not computed"""
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        sk = np.arange(radius + 1, dtype=np.int64) * int(step)
        sk = sk.astype(np.float64)
        ws = np.exp(-(sk * sk) / (2.0 * (np.float64(sigma_space) * np.float64(sigma_space))))
        dk = np.arange(256, dtype=np.float64)
        E = np.exp(-(dk * dk) / (2.0 * (np.float64(sigma_color) * np.float64(sigma_color))))
    ws[0] = 1.0
    E[0] = 1.0
    return ws, E


def quantise(D, unit, ok):
    """the header's uint16 rule on the float64 D -> (u16, q); pixels that are not ok are 0"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        q = D / np.float64(unit)
        r = np.where(np.isnan(q), 0.0, np.where(q >= 65535.0, 65535.0, np.rint(np.where(q >= 65535.0, 0.0, q))))
    r = np.where(ok, r, 0.0)
    return r.astype(np.uint16), q


def sample(depth, guide, radius, step, sigma_space, sigma_color, fill, unit):
    """one (h,w) float32 depth and (h,w,3) uint8 guide -> dict: "f32" (h,w) float32, "u16" (h,w) uint16, "ok" (h,w) bool (the pixel is not
    invalid), "D" (h,w) float64 (only meaningful where ok), "q" (h,w) float64 D / unit, "den" (h,w) float64"""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    guide = np.ascontiguousarray(guide, dtype=np.uint8)
    h, w = depth.shape
    assert guide.shape == (h, w, 3)
    ws, E = tables(radius, step, sigma_space, sigma_color)
    halo = radius * step
    v = valid_mask(depth)
    dp = np.zeros((h + 2 * halo, w + 2 * halo), dtype=np.float64)          # outside the frame: not valid
    vp = np.zeros((h + 2 * halo, w + 2 * halo), dtype=bool)
    gp = np.zeros((h + 2 * halo, w + 2 * halo, 3), dtype=np.int64)
    dp[halo:halo + h, halo:halo + w] = np.where(v, depth, np.float32(0)).astype(np.float64)
    vp[halo:halo + h, halo:halo + w] = v
    gp[halo:halo + h, halo:halo + w] = guide
    gc = guide.astype(np.int64)
    num = np.zeros((h, w), dtype=np.float64)
    den = np.zeros((h, w), dtype=np.float64)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            ys, xs = slice(halo + j * step, halo + j * step + h), slice(halo + i * step, halo + i * step + w)
            dq, vq, gq = dp[ys, xs], vp[ys, xs], gp[ys, xs]
            dc = np.abs(gq - gc)
            wgt = (ws[abs(j)] * ws[abs(i)]) * ((E[dc[..., 0]] * E[dc[..., 1]]) * E[dc[..., 2]])
            num = num + np.where(vq, wgt * dq, 0.0)
            den = den + np.where(vq, wgt, 0.0)
    ok = v | ((den > 0) if fill else np.zeros_like(v))
    with np.errstate(invalid="ignore", divide="ignore"):
        D = num / den
    u16, q = quantise(D, unit, ok)
    with np.errstate(invalid="ignore", over="ignore"):
        f32 = np.where(ok, D, 0.0).astype(np.float32)
    return {"f32": f32, "u16": u16, "ok": ok, "D": D, "q": q, "den": den}


def reference(depth, guide, radius=3, step=4, sigma_space=None, sigma_color=12.0, fill=False, unit=1e-3):
    """(B,h,w) float32, (B,h,w,3) uint8 -> the dict of ``sample`` with a leading batch axis"""
    depth = np.asarray(depth, dtype=np.float32)
    if sigma_space is None:
        sigma_space = radius * step / 2.0
    outs = [sample(depth[b], guide[b], radius, step, sigma_space, sigma_color, fill, unit) for b in range(depth.shape[0])]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}
