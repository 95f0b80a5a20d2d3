"""Plain float64 references of the elementwise kernels of csrc/elementwise.hip (BatchNorm statistics / finalisation / backward, the deferred
norm1 backward, the 3x3/s2 max-pool, the padded transition pooling, fused AdamW) and the planted inputs they are tested on, for
tests/test_normpool_ref_cpu.py and tests/test_gpu_norm_pool_edges.py.  numpy only, no library BatchNorm / pooling / optimiser.  Where a
tolerance needs it a reference also returns S_abs, the float64 sum of the absolute values of the terms of each reduction, or T, the sum of
the absolute values of the terms of an element.  Rows are pixels, columns are channels ((M, C) or NHWC) everywhere."""
import math

import numpy as np

from md_rdm_amd import filler

EPS32 = float(np.float32(1e-5))                     # the eps the kernels are launched with (1e-5f)
MOMENTUM32 = float(np.float32(0.1))


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------
# BatchNorm
# ----------------------------------------------------------------------------------
def colsums(x):
    """-> (sum x, sum x^2, S_abs of the first, S_abs of the second) over the rows of (M, C).  math.fsum: each sum is the correctly rounded
    exact one (the square of a float32 value is exact in float64), because the variance formula of bn_finalize magnifies what is left"""
    x = f64(x)
    q = x * x
    fs = lambda a: np.array([math.fsum(col) for col in a.T])
    return fs(x), fs(q), np.abs(x).sum(0), q.sum(0)


def bn_finalize(s, sq, count, gamma, beta, rm, rv, training, eps=1e-5, momentum=0.1):
    """nn.BatchNorm2d's bookkeeping from the channel sums -> (scale, shift, mean, rstd, running_mean', running_var'): biased variance in the
    normalisation, unbiased in the running estimate (count == 1 keeps the biased value), eval mode reads the running statistics"""
    gamma, beta, rm, rv = f64(gamma), f64(beta), f64(rm), f64(rv)
    if training:
        mean = f64(s) / count
        var = np.maximum(f64(sq) / count - mean * mean, 0.0)
        unbiased = var * count / (count - 1) if count > 1 else var
        rm2, rv2 = (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * unbiased
    else:
        mean, var, rm2, rv2 = rm, rv, rm, rv
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    return scale, beta - mean * scale, mean, rstd, rm2, rv2


def gate(x, sc, sh):
    """relu'(x * sc + sh) for float32 operands: the product of two float32 values is exact in float64 and a rounded sum keeps the sign of the
    exact one (zero stays zero), so this is the sign of the exact value - the sign of the kernel's float32 fmaf, exact zero included"""
    assert np.asarray(x).dtype == np.float32 and np.asarray(sc).dtype == np.float32 and np.asarray(sh).dtype == np.float32
    return f64(x) * f64(sc) + f64(sh) > 0


def bn_bwd_sums(dz, x, sc, sh, mask=None):
    """-> (dz masked by the gate (float32, exact), sum dz, sum dz x, S_abs of both); mask replaces gate(x, sc, sh) when given"""
    dzm = np.where(gate(x, sc, sh) if mask is None else mask, dz, np.float32(0)).astype(np.float32)
    d, t = f64(dzm), f64(dzm) * f64(x)
    return dzm, d.sum(0), t.sum(0), np.abs(d).sum(0), np.abs(t).sum(0)


def bn_bwd_coeffs(s0, s1, count, gamma, mean, rstd, training):
    """dx = A dz + B x + C -> (A, B, C, dgamma, dbeta)"""
    s0, s1, g, mu, rs = f64(s0), f64(s1), f64(gamma), f64(mean), f64(rstd)
    dgamma = rs * (s1 - mu * s0)
    A = g * rs
    if training:
        B = -A * rs * dgamma / count
        Cc = -A * s0 / count - B * mu
    else:
        B, Cc = np.zeros_like(A), np.zeros_like(A)
    return A, B, Cc, dgamma, s0.copy()


def bn_bwd_apply(dzm, x, s0, s1, count, gamma, mean, rstd, training, old=None):
    """-> (dx, dgamma, dbeta, T) with T = |A dz| + |B x| + |C| (+ |old| when dx accumulates onto old)"""
    A, B, Cc, dgamma, dbeta = bn_bwd_coeffs(s0, s1, count, gamma, mean, rstd, training)
    dzm, x = f64(dzm), f64(x)
    dx = A * dzm + B * x + Cc
    T = np.abs(A * dzm) + np.abs(B * x) + np.abs(Cc)
    if old is not None:
        dx, T = dx + f64(old), T + np.abs(f64(old))
    return dx, dgamma, dbeta, T


def bn_bwd_sens(x, count, gamma, mean, rstd, training):
    """(|d dx / d s0|, |d dx / d s1|) of bn_bwd_apply per element: how an error of the sums reaches dx"""
    A, rs, mu, x = f64(gamma) * f64(rstd), f64(rstd), f64(mean), f64(x)
    if not training:
        return np.zeros_like(x), np.zeros_like(x)
    d1 = -A * rs * rs * (x - mu) / count
    return np.abs(-A / count - d1 * mu), np.abs(d1)


def bn_bwd_defer(G, x, s0, s1, count, gamma, mean, rstd, b_in, c_in, slice_c0, slice_n, training):
    """one call of the deferred norm1 backward: the layer's (B, C) join the running sums (b_out = b_in + B, c_out = c_in + C over the layer's
    channels) and the slice [slice_c0, +slice_n) of the block gradient takes  G += b_out x + c_out
    -> (G', dgamma, dbeta, b_out, c_out, T) with T = |b_out x| + |c_out| + |G| on the slice (zero elsewhere: G is untouched there)"""
    _, B, Cc, dgamma, dbeta = bn_bwd_coeffs(s0, s1, count, gamma, mean, rstd, training)
    C = B.shape[0]
    b_out, c_out = f64(b_in)[:C] + B, f64(c_in)[:C] + Cc
    G2, T = f64(G).copy(), np.zeros(np.shape(G))
    sl = slice(slice_c0, slice_c0 + slice_n)
    xs = f64(x)[:, sl]
    T[:, sl] = np.abs(b_out[sl] * xs) + np.abs(c_out[sl]) + np.abs(G2[:, sl])
    G2[:, sl] += b_out[sl] * xs + c_out[sl]
    return G2, dgamma, dbeta, b_out, c_out, T


# ----------------------------------------------------------------------------------
# 3x3 / stride 2 / pad 1 max-pool (NHWC)
# ----------------------------------------------------------------------------------
def _taps(H, W):
    """(tap code r*3+q, output rows, input rows, output columns, input columns) of the in-image part of every tap, row-major"""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for r in range(3):
        oy = np.array([o for o in range(Ho) if 0 <= 2 * o - 1 + r < H], dtype=np.int64)
        for q in range(3):
            ox = np.array([o for o in range(Wo) if 0 <= 2 * o - 1 + q < W], dtype=np.int64)
            if len(oy) and len(ox):                           # both runs are contiguous: plain slices (views, no gather)
                iy, ix = 2 * oy - 1 + r, 2 * ox - 1 + q
                yield (r * 3 + q, slice(oy[0], oy[-1] + 1), slice(iy[0], iy[-1] + 1, 2), slice(ox[0], ox[-1] + 1), slice(ix[0], ix[-1] + 1, 2))


def maxpool3s2(x):
    """-> (y, argmax uint8 in the tap code r*3+q): the FIRST maximum in row-major tap order, out-of-image taps skipped"""
    x = np.asarray(x)
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = np.full((B, Ho, Wo, C), -np.inf, dtype=x.dtype)
    arg = np.zeros((B, Ho, Wo, C), dtype=np.uint8)
    for t, oy, iy, ox, ix in _taps(H, W):
        o = (slice(None), oy, ox)
        v = x[:, iy, ix]
        better = v > y[o]                                       # strictly: a later equal tap never replaces an earlier one
        y[o] = np.where(better, v, y[o])
        arg[o] = np.where(better, np.uint8(t), arg[o])
    return y, arg


def maxpool3s2_bwd(gy, arg, H, W):
    """-> (dx, S_abs): every window routes its gradient to its argmax tap; S_abs = sum |g| over the windows that route to an element"""
    gy = f64(gy)
    B, Ho, Wo, C = gy.shape
    dx, sa = np.zeros((B, H, W, C)), np.zeros((B, H, W, C))
    for t, oy, iy, ox, ix in _taps(H, W):
        o, i = (slice(None), oy, ox), (slice(None), iy, ix)
        g = np.where(arg[o] == t, gy[o], 0.0)                    # within one tap distinct windows reach distinct pixels
        dx[i] += g
        sa[i] += np.abs(g)
    return dx, sa


def tie_fraction(x):
    """share of the pooling windows in which two or more in-image taps equal the maximum"""
    x = np.asarray(x)
    B, H, W, C = x.shape
    y, _ = maxpool3s2(x)
    n = np.zeros(y.shape, dtype=np.int32)
    for t, oy, iy, ox, ix in _taps(H, W):
        o = (slice(None), oy, ox)
        n[o] += x[:, iy, ix] == y[o]
    return float((n >= 2).mean())


# ----------------------------------------------------------------------------------
# transition front end: ZeroPad2d((0,1,0,1)) -> BN affine -> ReLU -> AvgPool2d(2)
# ----------------------------------------------------------------------------------
def _pad(x):
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 1, W + 1, C), dtype=x.dtype)
    xp[:, :H, :W] = x
    return xp


def padavgpool2(x, sc, sh):
    """-> (pooled, S_abs = 0.25 * sum of the four relu terms, which are their own absolute values)"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    z = np.maximum(f64(_pad(np.asarray(x))) * f64(sc) + f64(sh), 0.0)[:, :2 * Ho, :2 * Wo]
    p = 0.25 * z.reshape(B, Ho, 2, Wo, 2, C).sum(axis=(2, 4))
    return p, p.copy()


def padavgpool2_bwd(gp, x, sc, sh, gamma, mean, rstd, training, mask=None):
    """backward over the PADDED extent (pad pixels are BatchNorm inputs and count): dz = 0.25 gp on the pixels a window covers, gated
    -> dict(dx, dgamma, dbeta, T, s0, s1, S0abs, S1abs, d0, d1, count, dz); dx / T / d0 / d1 on the real H x W extent, dz (masked) on the
    padded one; mask (padded extent) replaces the gate when given"""
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = _pad(np.asarray(x))
    dz = np.zeros(xp.shape, dtype=np.float32)
    up = np.repeat(np.repeat(np.float32(0.25) * np.asarray(gp, dtype=np.float32), 2, axis=1), 2, axis=2)
    hh, ww = min(H + 1, 2 * Ho), min(W + 1, 2 * Wo)
    dz[:, :hh, :ww] = up[:, :hh, :ww]
    count = float(B * (H + 1) * (W + 1))
    dzm, s0, s1, a0, a1 = bn_bwd_sums(dz.reshape(-1, C), xp.reshape(-1, C), sc, sh, None if mask is None else np.asarray(mask).reshape(-1, C))
    dx, dgamma, dbeta, T = bn_bwd_apply(dzm, xp.reshape(-1, C), s0, s1, count, gamma, mean, rstd, training)
    d0, d1 = bn_bwd_sens(xp.reshape(-1, C), count, gamma, mean, rstd, training)
    real = lambda a: a.reshape(xp.shape)[:, :H, :W]
    return dict(dx=real(dx), dgamma=dgamma, dbeta=dbeta, T=real(T), s0=s0, s1=s1, S0abs=a0, S1abs=a1, d0=real(d0), d1=real(d1), count=count,
                dz=dzm.reshape(xp.shape))


# ----------------------------------------------------------------------------------
# AdamW (torch.optim.AdamW, decoupled weight decay, no amsgrad)
# ----------------------------------------------------------------------------------
def adamw(p, g, m, v, step, lr, b1, b2, eps, wd, gscale):
    """-> dict(p, m, v, update, Tm, Tv, denom): Tm / Tv the absolute terms of the moments, update the step subtracted from the decayed p"""
    p, g, m, v = f64(p), f64(g) * gscale, f64(m), f64(v)
    m2, v2 = b1 * m + (1.0 - b1) * g, b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v2) / np.sqrt(bc2) + eps
    update = (lr / bc1) * m2 / denom
    return dict(p=p * (1.0 - lr * wd) - update, m=m2, v=v2, update=update, Tm=np.abs(b1 * m) + np.abs((1.0 - b1) * g),
                Tv=np.abs(b2 * v) + np.abs((1.0 - b2) * g * g), denom=denom, step_scale=lr / bc1)


# ----------------------------------------------------------------------------------
# planted inputs
# ----------------------------------------------------------------------------------
RATIOS = (0.0, 3.0, 30.0, 300.0)                    # |mean| / std of channel c is RATIOS[c % 4]
BN_SHAPES = [(1, 4), (3, 48), (17, 48), (35, 260), (570, 100), (24593, 8)]


def bn_case(M, C, key="np"):
    """The channel recipe: x[:, c] = mean_c + std_c u, |mean_c| / std_c cycling through RATIOS with the sign of the mean alternating every four
    channels, gamma ~ U(-1.5, 1.5), beta ~ U(-0.5, 0.5), and the special channels (as many as C holds):
      zero_x   x = 0 on every row, beta = 0: mean = 0 and shift = 0, so every gate value is exactly 0
      const_x  x = 0.75 on every row: var = 0 (and the float32 sums of 0.75 and 0.5625 are exact)
      g0neg    gamma = 0, beta < 0: scale = 0, gate closed everywhere      g0pos  gamma = 0, beta > 0: gate open everywhere
      tiny     gamma = 1e-6
      tie_pos / tie_neg (every 16 channels when C >= 16)  x in multiples of 0.25, half of them the value at which the planted affine
               (scale 2, shift -1 / scale -4, shift 1: bn_planted) is exactly 0
    -> dict(x (M, C) float32, gamma, beta, rm, rv, ratio (C,), special {name: [channels]})"""
    k = f"{key}.{M}x{C}"
    c = np.arange(C)
    ratio = np.array(RATIOS)[c % 4]
    sign = np.where((c // 4) % 2 == 0, 1.0, -1.0)
    std = filler.uniform(k + ".std", (C,), 0.5, 2.0, np.float64)
    u = filler.uniform(k + ".u", (M, C), -np.sqrt(3.0), np.sqrt(3.0), np.float64)          # unit variance
    x = (sign * ratio * std + std * u).astype(np.float32)
    gamma = filler.uniform(k + ".gamma", (C,), -1.5, 1.5)
    beta = filler.uniform(k + ".beta", (C,), -0.5, 0.5)
    rm = filler.uniform(k + ".rm", (C,), -0.2, 0.2)
    rv = filler.uniform(k + ".rv", (C,), 0.5, 1.5)
    sp = {n: [] for n in ("zero_x", "const_x", "g0neg", "g0pos", "tiny", "tie_pos", "tie_neg")}
    if C >= 16:
        sp.update(zero_x=[C - 1], const_x=[C - 2], g0neg=[C - 3], g0pos=[C - 4], tiny=[C - 5])
        sp["tie_pos"] = [i for i in range(9, C - 5, 16)]
        sp["tie_neg"] = [i for i in range(10, C - 5, 16)]
    elif C >= 8:
        sp.update(zero_x=[C - 1], const_x=[C - 2], g0neg=[C - 3], g0pos=[C - 4], tiny=[1])
    else:
        sp.update(zero_x=[C - 1], g0neg=[C - 2])
    q = np.floor(filler.uniform(k + ".q", (M, C), 0.0, 5.0, np.float64)) * 0.25                # 0, 0.25, .., 1
    coin = filler.uniform(k + ".coin", (M, C), 0.0, 1.0, np.float64) < 0.5
    for ch in sp["tie_pos"]:
        x[:, ch] = np.where(coin[:, ch], 0.5, q[:, ch])
        ratio[ch] = np.nan
    for ch in sp["tie_neg"]:
        x[:, ch] = np.where(coin[:, ch], 0.25, q[:, ch])
        ratio[ch] = np.nan
    for ch in sp["zero_x"]:
        x[:, ch] = 0.0; beta[ch] = 0.0; ratio[ch] = np.nan
    for ch in sp["const_x"]:
        x[:, ch] = 0.75; ratio[ch] = np.nan
    for ch in sp["g0neg"]:
        gamma[ch] = 0.0; beta[ch] = -abs(beta[ch]) - np.float32(0.125)
    for ch in sp["g0pos"]:
        gamma[ch] = 0.0; beta[ch] = abs(beta[ch]) + np.float32(0.125)
    for ch in sp["tiny"]:
        gamma[ch] = 1e-6
    return dict(x=x, gamma=gamma, beta=beta, rm=rm, rv=rv, ratio=ratio, special=sp)


def bn_planted(case, count=None):
    """What a BatchNorm backward is handed for bn_case's data, as float32: mean / rstd (the float64 two-pass statistics over `count` rows - the
    rows beyond x's count as zeros, the transition's padding - rounded once), scale = gamma rstd, shift = beta - mean scale.  The tie channels
    get the power-of-two affine whose gate value is exactly 0 on half their rows: (gamma 1, mean 0.5, rstd 2) -> scale 2, shift -1 and
    (gamma -2, mean 0.25, rstd 2) -> scale -4, shift 1, beta = 0.  -> dict(gamma, beta, mean, rstd, sc, sh), all float32"""
    x = f64(case["x"])
    M = x.shape[0]
    count = float(count or M)
    mu = x.sum(0) / count
    var = (((x - mu) ** 2).sum(0) + (count - M) * mu * mu) / count
    gamma, beta = case["gamma"].copy(), case["beta"].copy()
    mean, rstd = mu.astype(np.float32), (1.0 / np.sqrt(var + EPS32)).astype(np.float32)
    for ch in case["special"]["tie_pos"]:
        gamma[ch], beta[ch], mean[ch], rstd[ch] = 1.0, 0.0, 0.5, 2.0
    for ch in case["special"]["tie_neg"]:
        gamma[ch], beta[ch], mean[ch], rstd[ch] = -2.0, 0.0, 0.25, 2.0
    sc = (gamma * rstd).astype(np.float32)
    sh = (beta - mean * sc).astype(np.float32)
    return dict(gamma=gamma, beta=beta, mean=mean, rstd=rstd, sc=sc, sh=sh)


def gate_zero_fraction(x, sc, sh):
    """share of the elements whose gate value x * sc + sh is exactly 0"""
    return float((f64(x) * f64(sc) + f64(sh) == 0).mean())


def pool_input(B, H, W, C, key="np.mp", rng=None):
    """relu of data quantised to multiples of 0.25, about half zeros (what the stem's pool reads: relu(bn(conv0)) is full of exact ties);
    rng (numpy Generator) instead of the keyed filler for the large grid-stride cases"""
    if rng is not None:
        return np.maximum(rng.integers(-8, 7, size=(B, H, W, C)).astype(np.float32) * np.float32(0.25), np.float32(0))
    v = filler.uniform(f"{key}.{B}x{H}x{W}x{C}", (B, H, W, C), -2.0, 2.0, np.float64)
    return np.maximum(np.round(v * 4.0) * 0.25, 0.0).astype(np.float32)


def adamw_inputs(n, key="np.adamw"):
    """p ~ U(-1e-3, 1e-3) (the update dominates the value), g ~ U(-1, 1) with a block of exact zeros (v = 0, denom = eps at step 1),
    planted moments for a late step (m0 ~ U(-0.5, 0.5), v0 ~ U(0, 0.5))"""
    k = f"{key}.{n}"
    g = filler.uniform(k + ".g", (n,), -1.0, 1.0)
    g2 = filler.uniform(k + ".g2", (n,), -1.0, 1.0)
    zero = np.zeros(n, dtype=bool)
    if n >= 3:
        zero[1:1 + max(1, n // 8)] = True
    g[zero] = 0.0
    g2[zero] = 0.0
    return dict(p=filler.uniform(k + ".p", (n,), -1e-3, 1e-3), g=g, g2=g2, zero=zero, m0=filler.uniform(k + ".m", (n,), -0.5, 0.5),
                v0=filler.uniform(k + ".v", (n,), 0.0, 0.5))
