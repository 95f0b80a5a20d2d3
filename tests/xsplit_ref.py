"""Planted inputs, float64 references and exactness conditions for the split-precision kernels of csrc/xsplit.hip.  No GPU, no torch.cuda.

The kernels multiply bf16 PLANES of their f32 operands on v_mfma_f32_16x16x32_bf16 and accumulate in f32 (csrc/xsplit_dev.h):
    two-way   x -> (hi, lo):        hi = bf16(x), lo = bf16(x - hi);                 products  a0 b0 + a0 b1 + a1 b0          ("x3")
    three-way x -> (x0, x1, x2):    one more step on the residual;                   products  + a0 b2 + a2 b0 + a1 b1        ("x6", the 1x1 forward)
    one-product mode:               bf16(x) alone;                                   product   a0 b0                          ("x1")
The references here are float64 sums of exactly those RETAINED products of the planes - not a @ b.  On the planted operands
    x = H + m 2^-9 (+ t 2^-18),   H a small integer or zero, |m 2^-9| below half a bf16 ulp of H (no rounding tie),
every retained product is an integer multiple of one quantum q and sum |product| < 2^24 q per output (exact_ok), so every f32 summation order -
tile shape, slab order, K split, atomics, operand form - gives the float64 value bit for bit.  The prologue (scale a power of two, shift a
quarter-integer) is one exact fma whose RESULT is the planted value (preimage); the gate compares scale * y + shift with 0 strictly, scale a power of two and y zero or a signed power of two,
with planted exact ties; the statistics are sums of exactly representable values under the same 2^24 q condition (stats_ok).

The x6 forward has q = 2^-18 against hi x hi products of order 1: its operands are sparse.  Its sum of SQUARES cannot be exact on such outputs
(an output with bits from 2^0 down to 2^-18 has no f32 square), so the statistics cases mirror every fine column k as (x[:, k], -w[:, k]) in a
second column K0 + k: the fine products cancel ACROSS k-steps, the outputs are quarter-integers, and any plane misplaced in one k-step leaves a
residue.  The general (unmirrored) planting runs through the same statistics instantiation with its outputs compared exactly.

tests/test_xsplit_ref_cpu.py asserts the conditions and the teeth on every case below; tests/test_gpu_xsplit_exact.py runs them on the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

import bf16_ref as B

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
X3 = ((0, 0), (0, 1), (1, 0))
X6 = X3 + ((0, 2), (2, 0), (1, 1))          # the six products of xs_fwd1x1_kernel
X1 = ((0, 0),)
PAIRS = {3: X3, 6: X6, 1: X1}
DY_ROWS, X_ROWS, DY_FRAME, ACC_SCALED = 0x10, 0x20, 0x40, 0x80


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def cdiv(a, b):
    return -(-a // b)


# ---- the split, restated with torch casts -----------------------------------------------------------------------------------------------------
def is_f32(x64):
    x64 = np.asarray(x64, dtype=np.float64)
    return bool(np.array_equal(x64.astype(np.float32).astype(np.float64), x64))


def planes(x64, n):
    """the n bf16 planes (float64 arrays) of f32-representable values: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1); residuals formed in f32"""
    assert is_f32(x64)
    r = T(np.asarray(x64, dtype=np.float64)).to(f32)
    out = []
    for _ in range(n):
        p = r.to(bf16)
        out.append(p.to(f64).numpy())
        r = r - p.to(f32)
    return out


def split_rows_bits(v32):
    """(M, C) f32 tensor -> int16 (M, C / 4, 8): the bytes of a split row, [hi x4 | lo x4] per four values (xsplit_dev.h)"""
    hi = v32.to(bf16)
    lo = (v32 - hi.to(f32)).to(bf16)
    M, C = v32.shape
    return torch.cat([hi.view(M, C // 4, 4), lo.view(M, C // 4, 4)], dim=2).contiguous().view(torch.int16)


def no_ties(x64):
    """no element of x64 sits on a bf16 rounding tie"""
    return not B._round_bits(x64)[1].any()


# ---- planted values -----------------------------------------------------------------------------------------------------------------------------
def plant(key, shape, hmax, dh, dm, dt=0.0):
    """H + m 2^-9 + t 2^-18: H integer in [-hmax, hmax] on a share dh of the elements (else the element is 0), m on a share dm of those with
    |m| <= 1 / 3 / 7 for |H| = 1 / 2-3 / >= 4 (strictly inside half a bf16 ulp of H), t in {-1, 1} on a share dt of the elements with m != 0.
    The planes are then p0 = H, p1 = m 2^-9, p2 = t 2^-18: every retained product is a multiple of 2^-9 (x3) or 2^-18 (x6).  An element with
    p0 = 0 is 0 (a non-zero value has a non-zero first plane), so the zero-hi elements are the zeros; zero-lo elements are the bare integers."""
    u = lambda k: B.filler.uniform(key + k, shape, 0.0, 1.0, np.float64)
    H = np.where(u(".dh") < dh, B.ints(key + ".h", shape, 1, hmax) * B.choice(key + ".hs", shape, (-1.0, 1.0)), 0.0)
    mmax = np.select([np.abs(H) == 1, (np.abs(H) == 2) | (np.abs(H) == 3)], [1.0, 3.0], 7.0)
    msign = np.where(np.isin(np.abs(H), (1.0, 2.0, 4.0)), np.sign(H), B.choice(key + ".ms", shape, (-1.0, 1.0)))      # |H| a power of two: m away from zero, or
    m = np.where((u(".dm") < dm) & (H != 0), np.ceil(mmax * u(".m")) * msign, 0.0)                                     # the value would fall into the binade below
    t = np.where((u(".dt") < dt) & (m != 0), B.choice(key + ".t", shape, (-1.0, 1.0)), 0.0)
    return H + m * 2.0 ** -9 + t * 2.0 ** -18


def pow2(key, shape, values=(0.5, 1.0, 2.0)):
    return B.choice(key, shape, values)


def quarters(key, shape, lo=-6, hi=6):
    return B.ints(key, shape, lo, hi) / 4.0


def preimage(pre, sc, sh):
    """x with fma(x, scale, shift) == pre exactly: the ACTIVATION is what is planted (its planes must be H, m 2^-9, t 2^-18), the input follows"""
    if sc is None:
        return pre
    x = (pre - sh) / sc
    assert is_f32(x) and np.array_equal(x * sc + sh, pre)
    return x


def activate(x64, sc, sh):
    """the prologue, ONE fma then ReLU; exact on the planted values (asserted), so float64 arithmetic is the f32 result"""
    if sc is None:
        return x64
    a = np.maximum(x64 * sc + sh, 0.0)
    assert is_f32(x64 * sc + sh)
    return a


# ---- contractions (float64) ---------------------------------------------------------------------------------------------------------------------
def mm_wgrad1(g, a):                        # g (M, N), a (M, C) -> (N, C)
    return (T(g).t() @ T(a)).numpy()


def mm_rows(g, w):                          # g (M, K), w (K, C) -> (M, C)
    return (T(g) @ T(w)).numpy()


def mm_fwd(a, w):                           # a (M, K), w (N, K) -> (M, N)
    return (T(a) @ T(w).t()).numpy()


def mm_dgrad3(gy, w9):                      # gy (B, H, W, N), w9 (9, N, C) -> (B H W, C): shifted slices, zero padding 1
    Bn, H, W, N = gy.shape
    gp = F.pad(T(gy), (0, 0, 1, 1, 1, 1))
    out = torch.zeros(Bn * H * W, w9.shape[2], dtype=f64)
    for r in range(3):
        for q in range(3):
            out += gp[:, 2 - r:2 - r + H, 2 - q:2 - q + W, :].reshape(-1, N) @ T(w9[r * 3 + q])
    return out.numpy()


def mm_wgrad3(gy, a):                       # gy (B, H, W, N), a (B, H, W, C) -> (9, N, C)
    Bn, H, W, N = gy.shape
    ap = F.pad(T(a), (0, 0, 1, 1, 1, 1))
    g2 = T(gy).reshape(-1, N).t().contiguous()
    return torch.stack([g2 @ ap[:, r:r + H, q:q + W, :].reshape(-1, a.shape[3]) for r in range(3) for q in range(3)]).numpy()


def retained(mm, ap, bp, pairs):
    """float64 sum of the retained plane products and the sum of their absolute values"""
    ref = sum(mm(ap[i], bp[j]) for i, j in pairs)
    mag = sum(mm(np.abs(ap[i]), np.abs(bp[j])) for i, j in pairs)
    return ref, mag


# ---- exactness conditions -----------------------------------------------------------------------------------------------------------------------
def lowbit(a):
    """exponent e of the largest 2^e dividing every element of a (None for an all-zero array)"""
    v = np.abs(np.asarray(a, dtype=np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return None
    m, e = np.frexp(v)
    i = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((i & -i).astype(np.float64)).astype(np.int64)
    return int((e - 53 + tz).min())


def quantum(ap, bp, pairs):
    es = [lowbit(ap[i]) + lowbit(bp[j]) for i, j in pairs if lowbit(ap[i]) is not None and lowbit(bp[j]) is not None]
    return 2.0 ** min(es)


def exact_ok(ap, bp, pairs, mag):
    """every retained product is a multiple of q (by construction of q) and sum |product| < 2^24 q for every output: boolean per output"""
    return mag < 2.0 ** 24 * quantum(ap, bp, pairs)


def stats_ok(values, q):
    """per column: the values are multiples of q and sum |value| < 2^24 q, so every order of f32 / f64 partial sums is exact"""
    v = np.asarray(values, dtype=np.float64)
    return (np.array_equal(np.round(v / q), v / q)) & (np.abs(v).sum(0) < 2.0 ** 24 * q)


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------------
def plant_gate(key, M, C, share=0.25):
    """mask operand y (M, C) of zeros and signed powers of two, per channel scale (a power of two) and shift such that a share of the elements gives
    scale * y + shift == 0 EXACTLY (channels of kind 0: strict comparison, gated off) or one ulp of the shift above / below zero (kinds 1 / 2: the
    tie value gated on / off); the other elements fall on either side.  Returns y, scale, shift, gate (bool), ties (bool)."""
    y = B.choice(key + ".y", (M, C), (0.0, 0.5, 1.0, 2.0, -0.5, -1.0, -2.0))
    y0 = B.choice(key + ".y0", (C,), (0.5, 1.0, 2.0, -0.5, -1.0, -2.0))
    y = np.where(B.filler.uniform(key + ".tie", (M, C), 0.0, 1.0, np.float64) < share, y0, y)
    scale = pow2(key + ".sc", (C,)) * B.choice(key + ".ss", (C,), (1.0, 1.0, 1.0, -1.0))
    kind = B.ints(key + ".kind", (C,), 0, 2)
    kind[:3] = (0, 1, 2)
    base = -scale * y0                                        # a signed power of two; its neighbours two f32 steps away are base (1 +- 2^-23)
    shift = base + np.select([kind == 1, kind == 2], [1.0, -1.0], 0.0) * np.abs(base) * 2.0 ** -23
    pre = scale * y + shift                                   # exact in float64 (scale * y is exact in f32 too): its sign is the sign of the f32 fma
    assert is_f32(shift) and is_f32(scale * y)
    return y, scale, shift, pre > 0, pre == 0


# ---- case tables ----------------------------------------------------------------------------------------------------------------------------------
# rdm_conv2d_wgrad_x3, 1x1.  name: (B, H, W, C, N, bn).  C = 96 / 144 / 192: one column tile of each width; 240 = 144 + 96; 336 = 192 + 144 (launch_xs_wgrad1x1).
# N = 200: below one 256-row tile; 260: a ragged second one.  77 pixels = 3 slabs (the last of 13 rows); 1037 pixels = 33 slabs (the last of 13 rows): the
# launcher's own K split is 2 there, so split_k = 0 / 1 / 3 are three different partitions.
WGRAD1_CASES = {}
for _c in (96, 144, 192, 240, 336):
    for _bn in (False, True):
        WGRAD1_CASES["c%d_small_bn%d" % (_c, _bn)] = (1, 7, 11, _c, 200, _bn)
        WGRAD1_CASES["c%d_split_bn%d" % (_c, _bn)] = (1, 17, 61, _c, 260, _bn)


def wgrad1_auto_split(M, C, N):
    """split_k the launcher picks (launch_xs_wgrad1x1)"""
    nct = cdiv(C // 48, 4)
    tiles, tiles128, kslabs = nct * cdiv(N, 256), nct * cdiv(N, 128), cdiv(M, 32)
    assert tiles128 <= 512 and tiles <= 256
    split128 = max(1, min(512 // tiles128, kslabs // 16))
    split = max(2, min(256 // tiles, kslabs // 16)) if split128 > 1 else 1
    return min(split, kslabs)


def build_wgrad1(name):
    Bn, H, W, C, N, bn = WGRAD1_CASES[name]
    M, ld, ldg = Bn * H * W, C + 8, N + 8
    x = np.full((M, ld), np.nan)
    sc, sh = (pow2(name + ".sc", (C,)), quarters(name + ".sh", (C,))) if bn else (None, None)
    x[:, :C] = preimage(plant(name + ".x", (M, C), 3, 0.6, 0.5), sc, sh)
    g = np.full((M, ldg), np.nan)
    g[:, :N] = plant(name + ".g", (M, N), 2, 0.6, 0.5)
    return dict(B=Bn, H=H, W=W, M=M, C=C, N=N, ld=ld, ldg=ldg, x=x, g=g, sc=sc, sh=sh, A=g[:, :N], Bop=activate(x[:, :C], sc, sh), mm=mm_wgrad1, kaxis=0)


# rdm_conv1x1_dgrad_x3.  name: (B, H, W, K, N, dg, dw): K = contracted channels, N = outputs; dg, dw = shares of non-zero integer parts.
# px128 is M <= 8192, px320 the smallest M above it (8193 = 3 x 2731, no multiple of 16); the ABI needs K >= 32, so the shortest K is ONE k-step (32), not less.
# N = 192: one column tile of 12; 224: 7 + 7; 208: 7 + 6 (N / 16 = 13).  K = 72 and 40: a ragged last k-step of 8.
DGRAD1_CASES = {
    "one_tile": (2, 9, 11, 72, 192, 0.5, 0.5),
    "even_tiles_k32": (3, 7, 9, 32, 224, 0.5, 0.5),
    "uneven_tiles": (3, 7, 9, 104, 208, 0.4, 0.5),
    "px320": (1, 3, 2731, 40, 32, 0.02, 0.5),
}


def build_dgrad1(name):
    Bn, H, W, K, N, dg, dw = DGRAD1_CASES[name]
    M, ldg, ldx, ldo = Bn * H * W, K + 8, N + 16, N + 12
    g = np.full((M, ldg), np.nan)
    g[:, :K] = plant(name + ".g", (M, K), 2, dg, 0.5)
    w = plant(name + ".w", (K, N), 2, dw, 0.5)
    y, sc, sh, gate, ties = plant_gate(name + ".gate", M, N)
    yb = np.full((M, ldx), np.nan)
    yb[:, :N] = y
    G0 = B.ints(name + ".G0", (M, N), -50, 50)
    return dict(B=Bn, H=H, W=W, M=M, K=K, N=N, ldg=ldg, ldx=ldx, ldo=ldo, g=g, w=w, y=yb, sc=sc, sh=sh, gate=gate, ties=ties, G0=G0,
                A=g[:, :K], Bop=w, mm=mm_rows, kaxis=1)


# rdm_conv3x3_dgrad_x3.  name: (B, H, W, Cb, ldg).  48: the 48-wide tile alone; 96; 144 = 96 + 48 inside one 128-channel item + a second item.
# wide: W = 318, the widest row whose two LDS images fit (xs_dgrad3_lds_bytes).  walk: W = 120 makes the images larger than 80 KB -> 256 resident
# workgroups; 4 pixel tiles x 65 column tiles = 260 items, so four workgroups walk two items (launch_xs_dgrad3x3).
DGRAD3_CASES = {
    "cb48_tiny": (3, 9, 7, 48, 64),
    "cb96_tiny": (3, 9, 7, 96, 48),
    "cb144_tiny": (3, 9, 7, 144, 96),
    "wide": (1, 2, 318, 48, 64),
    "walk": (1, 5, 120, 8320, 48),
}


def dgrad3_grid(Bn, H, W, Cb):
    nslots = 1 + 192 + 2 * (W + 1)
    lds = 2 * ((nslots * 96 + 1023) & ~1023)
    items, slots = cdiv(Bn * H * W, 192) * cdiv(Cb, 128), 256 * (2 if lds <= 80 * 1024 else 1)
    return items, slots, lds


def build_dgrad3(name):
    Bn, H, W, Cb, ldg = DGRAD3_CASES[name]
    M = Bn * H * W
    g = np.full((Bn, H, W, ldg), np.nan)
    g[..., ldg - 48:] = plant(name + ".g", (Bn, H, W, 48), 2, 0.5, 0.5)
    w9 = plant(name + ".w", (9, 48, Cb), 2, 0.4, 0.5)
    y, sc, sh, gate, ties = plant_gate(name + ".gate", M, Cb)
    yb = np.full((M, Cb + 8), np.nan)
    yb[:, :Cb] = y
    return dict(B=Bn, H=H, W=W, M=M, Cb=Cb, ldg=ldg, ldx=Cb + 8, ldo=Cb + 12, g=g, w=w9, y=yb, sc=sc, sh=sh, gate=gate, ties=ties,
                A=g[..., ldg - 48:], Bop=w9, mm=mm_dgrad3, kaxis=1)


# rdm_conv2d_wgrad_x3, 3x3.  name: (B, H, W, C, ld, N, ldg, bn).  C = 80: one full 64-channel block + 16; 48: less than a block.  N = 48 and 40.  An explicit
# split_k is honoured only up to nslab / 8 (launch_xs_wgrad3x3): 8 frames of 11 x 9 are 25 slabs, 2 frames of 5 x 95 are 30 - split_k = 3 is a real split.
WGRAD3_CASES = {
    "frame9x7": (8, 9, 7, 80, 96, 48, 64, True),
    "frame9x7_n40": (8, 9, 7, 48, 56, 40, 48, False),
    "w93": (2, 3, 93, 80, 88, 40, 48, True),
}


def build_wgrad3(name):
    Bn, H, W, C, ld, N, ldg, bn = WGRAD3_CASES[name]
    x = np.full((Bn, H, W, ld), np.nan)
    sc, sh = (pow2(name + ".sc", (C,)), quarters(name + ".sh", (C,))) if bn else (None, None)
    x[..., :C] = preimage(plant(name + ".x", (Bn, H, W, C), 3, 0.6, 0.5), sc, sh)
    g = np.full((Bn, H, W, ldg), np.nan)
    g[..., :N] = plant(name + ".g", (Bn, H, W, N), 2, 0.6, 0.5)
    return dict(B=Bn, H=H, W=W, M=Bn * H * W, C=C, ld=ld, N=N, ldg=ldg, x=x, g=g, sc=sc, sh=sh, A=g[..., :N], Bop=activate(x[..., :C], sc, sh),
                mm=mm_wgrad3, kaxis=0)


def frame_image(g, N):
    """(B, H, W, >= N) -> f32 tensor (U rounded up to 32, 48): the padded-frame ordering of rdm_frame_split_rows_f32 before the split; zero borders / tail / channels >= N"""
    fr = F.pad(T(np.ascontiguousarray(g[..., :N])), (0, 48 - N, 1, 1, 1, 1)).reshape(-1, 48)
    return F.pad(fr, (0, 0, 0, cdiv(fr.shape[0], 32) * 32 - fr.shape[0])).to(f32)


# rdm_conv1x1_fwd_x6.  name: (B, H, W, K, ld, N, bn, mirror).  N = 208: one full column tile (192) + 16; N = 16.  K = 40 / 72: a ragged last k-step.
# mirror: the statistics planting (module docstring): K = 2 K0, columns K0 + k mirror the fine columns k.
FWD_CASES = {}
for _n, _k in ((208, 40), (16, 72)):
    for _bn in (False, True):
        for _mir in (False, True):
            FWD_CASES["n%d_k%d_bn%d%s" % (_n, _k, _bn, "_mirror" if _mir else "")] = (3, 9, 11, _k, _k + 8, _n, _bn, _mir)


def build_fwd(name):
    Bn, H, W, K, ld, N, bn, mirror = FWD_CASES[name]
    M = Bn * H * W
    K0 = K // 2 if mirror else K
    xs = plant(name + ".x", (M, K0), 2, 0.3, 0.3, 0.3)
    ws = plant(name + ".w", (N, K0), 2, 0.3, 0.3, 0.3)
    sc, sh = (pow2(name + ".sc", (K0,)), quarters(name + ".sh", (K0,))) if bn else (None, None)
    if mirror:
        coarse = np.arange(K0) % 3 == 0                                  # integer-only columns: they carry the outputs
        xs[:, coarse], ws[:, coarse] = np.round(xs[:, coarse]), np.round(ws[:, coarse])
        xm, wm = xs.copy(), -ws
        wm[:, coarse] = 0.0
        xs, ws = np.concatenate([xs, xm], 1), np.concatenate([ws, wm], 1)
        if bn:
            sc, sh = np.concatenate([sc, sc]), np.concatenate([sh, sh])
    x = np.full((M, ld), np.nan)
    x[:, :K] = preimage(xs, sc, sh)
    return dict(B=Bn, H=H, W=W, M=M, K=K, ld=ld, N=N, x=x, w=ws, sc=sc, sh=sh, mirror=mirror, A=activate(x[:, :K], sc, sh), Bop=ws, mm=mm_fwd, kaxis=1)


BUILDERS = {"wgrad1": (WGRAD1_CASES, build_wgrad1, 3), "dgrad1": (DGRAD1_CASES, build_dgrad1, 3), "dgrad3": (DGRAD3_CASES, build_dgrad3, 3),
            "wgrad3": (WGRAD3_CASES, build_wgrad3, 3), "fwd": (FWD_CASES, build_fwd, 6)}


def reference(c, np_):
    """(reference, sum |product|, planes of A, planes of B) of a built case in the np_-product arithmetic (3, 6 or 1)"""
    n = {3: 2, 6: 3, 1: 1}[np_]
    ap, bp = planes(c["A"], n), planes(c["Bop"], n)
    ref, mag = retained(c["mm"], ap, bp, PAIRS[np_])
    return ref, mag, ap, bp


# ---- real-valued leg ------------------------------------------------------------------------------------------------------------------------------
def real(key, shape, lo, hi):
    return B.filler.uniform(key, shape, lo, hi, np.float32).astype(np.float64)


def bound(mag, k_terms):
    """|f32 accumulation of k_terms exactly formed products - their exact sum| <= (k_terms + 2) 2^-24 sum |product| (+ 2 ulp of slack for the epilogue's
    adds), to first order in 2^-24: every addition rounds once, by at most 2^-24 of a partial sum that is at most sum |product|."""
    return (k_terms + 2) * 2.0 ** -24 * mag
