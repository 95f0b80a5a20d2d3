"""Float64 references, planted inputs and input-condition checkers for the bf16 forward kernels (csrc/bf16.hip).  No GPU, no torch.cuda.

The idea (tests/test_gpu_bf16_exact.py): every bf16 kernel multiplies bf16 operands on v_mfma_f32_16x16x32_bf16 and accumulates in f32.  With
small-integer activations and weights, power-of-two prologue scales, quarter-integer shifts / biases and +-power-of-two output scales every
product, partial sum and fmaf is exactly representable in f32 in ANY summation order, so the f32 result must equal the float64 reference bit for
bit and the bf16 result its round-to-nearest-even rounding.  tests/test_bf16_ref_cpu.py holds the references against independent formulations
and the planted inputs of every GPU case against the conditions (a)-(d) below.

Each reference follows the header comment of its entry point in include/rdm_hip.h.  Arrays are float64 numpy; NHWC for activations."""
import numpy as np
import torch
import torch.nn.functional as F

from md_rdm_amd import filler

BIG = 2.0 ** 100          # a large finite bf16 value for columns a kernel must not read into a sum


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bf16 rounding
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _round_bits(x64):
    f = np.ascontiguousarray(np.asarray(x64, dtype=np.float64).astype(np.float32))
    b = f.view(np.uint32).astype(np.uint64)
    low, odd = b & 0xFFFF, (b >> 16) & 1
    r = ((b + 0x7FFF + odd) & 0xFFFF0000).astype(np.uint32)
    nan = np.isnan(f)
    r = np.where(nan, (b.astype(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x00400000), r).astype(np.uint32)
    finite = np.isfinite(f)
    return r, finite & (low == 0x8000), finite & (low != 0), odd.astype(bool)


def round_bf16(x64):
    """x64 rounded to the nearest bf16 (ties to even) through an explicit float32 step -> (float64 array, mask of the elements that were exact ties).
    The kernels round an f32 accumulator, so this is meant ONLY for values that are exact in float32 (the float64 -> float32 step is then the
    identity); for other values it is a double rounding."""
    r, tie, _, _ = _round_bits(x64)
    return r.view(np.float32).astype(np.float64), tie


def bf16_bits(x64):
    """the 16 stored bits (int16) of round_bf16(x64); -0.0 is returned as +0.0"""
    r, _, _, _ = _round_bits(x64)
    h = (r >> 16).astype(np.uint16)
    h[h == 0x8000] = 0
    return h.view(np.int16)


def canon_bits(t):
    """int16 bits of a bf16 torch tensor with -0.0 folded onto +0.0 (numpy)"""
    h = t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).copy()
    h[h == 0x8000] = 0
    return h.view(np.int16)


def rounding_census(exact64):
    """conditions (b) and (c): share of values that are not bf16 numbers, ties that round down (towards zero) and up (away from zero)"""
    _, tie, inexact, odd = _round_bits(exact64)
    return float(inexact.mean()), int((tie & ~odd).sum()), int((tie & odd).sum())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b)).t()).numpy()


def activate(x, scale, shift):
    """the prologue: relu(x * scale + shift) rounded to bf16 ONCE (scale None: x is already activated)"""
    if scale is None:
        return x
    return round_bf16(np.maximum(x * scale + shift, 0.0))[0]


def gemm(x, w, K, scale=None, shift=None, bias=None, oscale=None, oshift=None):
    """rdm_gemm_bf16 / rdm_gemm_bf16_act before the output rounding: bias[n] + sum_{k<K} f(x[m][k]) * w[n][k], then relu(. * oscale + oshift).
    Also returns sum |a||w| + |bias| per output (condition (a), the real-valued leg's bound)."""
    a = activate(x[:, :K], scale, shift)
    acc, mag = _mm(a, w[:, :K]), _mm(np.abs(a), np.abs(w[:, :K]))
    if bias is not None:
        acc, mag = acc + bias, mag + np.abs(bias)
    if oscale is not None:
        acc = np.maximum(acc * oscale + oshift, 0.0)
    return acc, mag


def stored_stats(exact64):
    """the statistics forms: the raw bf16 output and the float64 sum / sum of squares of the STORED values per column"""
    v = round_bf16(exact64)[0]
    return v, v.sum(0), (v * v).sum(0)


def _conv(a_nhwc, w_oihw):
    y = F.conv2d(torch.from_numpy(np.ascontiguousarray(a_nhwc)).permute(0, 3, 1, 2), torch.from_numpy(np.ascontiguousarray(w_oihw)), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w_oihw.shape[0]).numpy()


def conv3x3(y, w9, C, scale=None, shift=None, drop_tap=None, drop_channel=None, activate_pad=False):
    """rdm_conv3x3_bf16 before the output rounding: y (B,H,W,ldy), prologue over the C real channels, ZERO padding of the activated tensor,
    w9 [9][48][C] -> (B*H*W, 48), and sum |a||w|.  drop_tap / drop_channel / activate_pad build the deliberately wrong references of the teeth
    tests (one tap or channel removed; the zero pad sent through the prologue)."""
    a = activate(y[..., :C], scale, shift)
    w = np.array(w9[:, :, :C], dtype=np.float64)
    if drop_tap is not None:
        w[drop_tap] = 0.0
    if drop_channel is not None:
        w[:, :, drop_channel] = 0.0
    wo = w.reshape(3, 3, 48, C).transpose(2, 3, 0, 1)
    out, mag = _conv(a, wo), _conv(np.abs(a), np.abs(wo))
    if activate_pad and scale is not None:             # what a padded pixel that went through the prologue would add: relu(shift) at every pad tap
        B, H, W = y.shape[:3]
        pad = np.zeros((B, H + 2, W + 2, C))
        pad[:] = np.maximum(shift, 0.0)
        pad[:, 1:-1, 1:-1] = 0.0
        out = out + F.conv2d(torch.from_numpy(pad).permute(0, 3, 1, 2), torch.from_numpy(np.ascontiguousarray(wo))).permute(0, 2, 3, 1).reshape(-1, 48).numpy()
    return out, mag


def conv3x3_act(y, w_oihw, C):
    """rdm_conv3x3_act_bf16: y (B,H,W,ldy) already activated, OIHW f32 weights (48, C, 3, 3) that rdm_conv3x3_act_bf16_pack rounds to bf16"""
    wo = round_bf16(w_oihw)[0]
    return _conv(y[..., :C], wo), _conv(np.abs(y[..., :C]), np.abs(wo))


def colstats(x, C):
    """rdm_colstats_bf16: float64 sum and sum of squares over the rows of the first C columns"""
    return x[:, :C].sum(0), (x[:, :C] ** 2).sum(0)


def stem_patches(x):
    """x (B,3,H,W) -> bf16 patches (B*Ho*Wo, 160) of the 7x7 / stride 2 / pad 3 stem: k = c*49 + r*7 + s, zeros from column 147"""
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.zeros((B, 3, H + 6, W + 6))
    xp[:, :, 3:3 + H, 3:3 + W] = x
    out = np.zeros((B, Ho, Wo, 160))
    for c in range(3):
        for r in range(7):
            for s in range(7):
                out[..., c * 49 + r * 7 + s] = xp[:, c, r:r + 2 * Ho:2, s:s + 2 * Wo:2]
    return round_bf16(out.reshape(-1, 160))[0]


def maxpool3s2(x, drop_tap=None):
    """nn.MaxPool2d(3, 2, 1) on NHWC (B,H,W,C) -> (B*Ho*Wo, C); the padding never wins"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = np.full((B, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.full((B, Ho, Wo, C), -np.inf)
    for r in range(3):
        for s in range(3):
            if (r, s) != drop_tap:
                out = np.maximum(out, xp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2])
    return out.reshape(-1, C)


def padavgpool2(x, C, scale, shift, pad_is_input=True):
    """pad bottom / right to even sizes with ZEROS -> x * scale + shift -> ReLU -> 2x2 average, before the one bf16 rounding.  The zero pad is a
    BatchNorm INPUT: a pad pixel contributes relu(shift) (pad_is_input=False builds the wrong reference in which it contributes 0)."""
    B, H, W = x.shape[:3]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = np.zeros((B, 2 * Ho, 2 * Wo, C))
    xp[:, :H, :W] = x[..., :C]
    a = np.maximum(xp * scale + shift, 0.0)
    if not pad_is_input:
        a[:, H:] = 0.0
        a[:, :, W:] = 0.0
    return (0.25 * (a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2])).reshape(-1, C)


def rows_to_bf16(src, cols, cols_pad):
    """rdm_f32_to_bf16_rows: src (rows, ld_src) -> (rows, cols_pad) bf16, zeros from column `cols`"""
    out = np.zeros((src.shape[0], cols_pad))
    out[:, :cols] = src[:, :cols]
    return round_bf16(out)[0]


def pack_weight(w_oit):
    """[O][I][T] -> [T][O][I] bf16"""
    return round_bf16(np.transpose(w_oit, (2, 0, 1)))[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# launcher selection rules, restated (launch_gemm_bf16, launch_conv3x3_bf16, plan_conv3_act of csrc/bf16.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def gemm_variant(M, K, N, ws_floats=0, bias=False, out_f32=False, stats=False):
    split = 1
    small, nk64 = cdiv(M, 32) * cdiv(N, 96), cdiv(K, 64)
    if ws_floats and not out_f32 and not bias and M <= 1024 and small < 256 and nk64 >= 8:
        split = max(1, min(nk64 // 4, cdiv(512, small), ws_floats // (M * N)))
        split = cdiv(nk64, cdiv(nk64, split))
    t96, t112 = cdiv(M, 128) * cdiv(N, 96), cdiv(M, 128) * cdiv(N, 112)
    n96 = cdiv(N, 96) * 96 <= 1.04 * N
    wide112 = cdiv(t112, 512) * 112 < cdiv(t96, 512) * 96 and t96 <= 4096
    if not stats and not out_f32 and not bias and split == 1 and K <= 352 and M >= 8192 and N >= 1024 and cdiv(M, 256) * cdiv(N, 96) >= 1024:
        return "gemm_panel_bf16_kernel/nkk%d" % cdiv(K, 32)
    if t96 >= 512 and wide112:
        tile = "128x112"
    elif t96 >= 512 and n96:
        tile = "128x96"
    elif cdiv(M, 128) * cdiv(N, 48) >= 512:
        tile = "128x48"
    else:
        tile = "64x96" if M > 1024 else "32x96"
    return "gemm_bf16_kernel/%s%s" % (tile, "/splitK" if split > 1 else "")


def conv3_slots(B, H, W, bm):
    return ((bm // W + 4 + 2 * (bm // (H * W) + 1)) * (W + 2) + 7) & ~7


def conv3_plan(B, H, W, C, ws_floats=0):
    """(bm, HL, split) of launch_conv3x3_bf16; HL None: the geometry is refused"""
    M = B * H * W
    bm = 256 if M >= 8192 else 128 if M >= 4096 else 64
    if bm == 256 and cdiv(conv3_slots(B, H, W, 256) * 4, 256) > 12:
        bm = 128
    tiles, slabs, split = cdiv(M, bm), cdiv(C, 32), 1
    hl = cdiv(conv3_slots(B, H, W, bm) * 4, 256)
    if ws_floats and tiles < 1024:
        slots = 256 * (2 if bm == 256 or hl > 6 else 3)
        t_slab = 2.5e-6 if bm == 256 else 1.5e-6 if bm == 128 else 1.0e-6
        red = M * 384.0 / 3e12 / t_slab
        best = -1.0
        for sp in range(1, min(max(slabs // 2, 1), ws_floats // (M * 48)) + 1):
            per = cdiv(slabs, sp)
            spe = cdiv(slabs, per)
            cost = float(cdiv(tiles * spe, slots)) * (per + 2) + (spe * red if spe > 1 else 0.0)
            if best < 0 or cost < best * 0.97:
                best, split = cost, spe
    HL = next((c for c in (4, 6, 9, 12, 20) if hl <= c), None)
    return bm, HL, split


def conv3_tile_slots(B, H, W, bm):
    """the largest zero-padded LDS image a tile of conv3x3_bf16_kernel addresses (must fit conv3_slots: checked on the CPU before a GPU runs it)"""
    M, worst = B * H * W, 0
    prow = lambda m: (m // (H * W)) * (H + 2) + (m % (H * W)) // W + 1
    for m0 in range(0, M, bm):
        worst = max(worst, (prow(min(M, m0 + bm) - 1) + 1 - (prow(m0) - 1) + 1) * (W + 2))
    return worst


def act_plan(C, B, H, W, ws_floats=0, n_counters=0):
    """(nc, split, rect) of plan_conv3_act; None: nothing fits"""
    HW, slabs, best = H * W, C // 32, None
    for pas in (0, 1):
        if best is not None:
            break
        nc = 1
        while nc <= 4:
            bm = nc * 128
            tpi = cdiv(H, bm // 64) * cdiv(W, 64) if pas else cdiv(HW, bm)
            rows = max((min(HW, (t + 1) * bm) - 1) // W - (t * bm) // W + 3 for t in range(cdiv(HW, bm)))
            if pas or rows * (W + 2) <= 832:
                tiles = B * tpi
                for sp in range(1, min(slabs, 32) + 1):
                    per = cdiv(slabs, sp)
                    if cdiv(slabs, per) != sp:
                        continue
                    if sp > 1 and (tiles * sp * bm * 48 > ws_floats or tiles > n_counters):
                        break
                    cost = cdiv(tiles * sp, 256) * (per * 1.8 + 3.0) + (1.0 + 2 * cdiv(sp, 6) * 1.7 if sp > 1 else 0.0)
                    if best is None or cost < best[3] * 0.98:
                        best = (nc, sp, pas, cost)
            nc += nc if pas else 1
    return None if best is None else best[:3]


def act_census(C, B, H, W, ws_bytes=0):
    nc, sp, rect = act_plan(C, B, H, W, max(ws_bytes - 16384, 0) // 4 if ws_bytes > 16384 else 0, 4096 if ws_bytes > 16384 else 0)
    return "conv3x3_act_bf16_kernel/nc%d/%s%s" % (nc, "splitK" if sp > 1 else "direct", "/rect" if rect else "")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ints(key, shape, lo, hi):
    """integers uniform in [lo, hi] as float64, seeded through md_rdm_amd.filler"""
    u = filler.uniform(key, shape, 0.0, 1.0, dtype=np.float64)
    return np.minimum(np.floor(lo + (hi - lo + 1) * u), hi)


def choice(key, shape, values):
    return np.asarray(values, dtype=np.float64)[ints(key, shape, 0, len(values) - 1).astype(np.int64)]


def amplitudes(k_total, prologue, target=700.0):
    """integer ranges (x in [-xa, xa], w in [-wa, wa]) at which the exact outputs have a standard deviation of about `target` output units
    (1, or 0.25 behind a prologue with quarter-integer shifts): then about half of them are no bf16 numbers and a fifth are exact ties.  Small K
    gets large integers, large K small ones; the CPU test asserts the conditions on the reference itself."""
    for r in range(2, 8):
        xa, wa = 2 ** r, 2 ** r - 1
        ea2 = xa * (xa + 1) / 3.0 * (14.0 if prologue else 1.0)        # prologue: units of 0.25 (x16), half the values cut by the ReLU, E[scale^2] = 1.75
        if k_total * ea2 * wa * (wa + 1) / 3.0 >= target * target:
            break
    return xa, wa


def prologue_coeffs(key, K):
    """power-of-two scales and quarter-integer shifts in [-2, 2]; every 5th channel has a positive shift >= 1"""
    sc = choice(key + ".sc", (K,), (0.5, 1.0, 2.0))
    sh = ints(key + ".sh", (K,), -8, 8) / 4.0
    sh[::5] = np.abs(sh[::5]) + 1.0
    return sc, sh


def out_coeffs(key, N):
    """+- power-of-two output scales (half of them negative) and quarter-integer output shifts"""
    return choice(key + ".os", (N,), (0.5, 1.0, 2.0, -0.5, -1.0, -2.0)), ints(key + ".oh", (N,), -64, 64) / 4.0


def gemm_operands(name, M, K, N, ldx, ldw, prologue, k_amp=None):
    xa, wa = amplitudes(k_amp or K, prologue)
    x = np.full((M, ldx), BIG)
    x[:, :K] = ints(name + ".x", (M, K), -xa, xa)
    w = np.full((N, ldw), BIG)
    w[:, :K] = ints(name + ".w", (N, K), -wa, wa)
    return x, w


def sparse_signs(key, rows, k_total, nnz=5):
    """[rows][k_total] weights with `nnz` entries of +-1 per row at positions >= 1 that walk over the whole K range from row to row"""
    w = np.zeros((rows, k_total))
    sg = choice(key, (rows, nnz), (-1.0, 1.0))
    step = max((k_total - 1) // nnz, 1)
    for j in range(nnz):
        pos = 1 + (np.arange(rows) * 7 + j * step + j) % (k_total - 1)
        w[np.arange(rows), pos] += sg[:, j]
    return w


def stats_gemm_operands(name, M, K, N, ldx):
    """the statistics forms need stored values that are integers below 256 (condition (d)) AND exact values that need rounding: column 0 is
    activated to exactly 1 and carries a weight of 192, five weights of +-1 per output row spread over the other columns add a zero-mean
    quarter-integer of at most 5 * 10.75 = 53.75: every exact value lies in [138, 246], where bf16 numbers are the integers."""
    x = np.full((M, ldx), BIG)
    x[:, :K] = ints(name + ".x", (M, K), -4, 4)
    x[:, 0] = 1.0
    sc, sh = prologue_coeffs(name, K)
    sc[0], sh[0] = 1.0, 0.0
    w = sparse_signs(name + ".w", N, K)
    w[:, 0] = 192.0
    return x, w, sc, sh


def stats_conv_operands(name, B, H, W, C, ldy):
    y = np.full((B, H, W, ldy), BIG)
    y[..., :C] = ints(name + ".y", (B, H, W, C), -4, 4)
    y[..., 0] = 1.0
    sc, sh = prologue_coeffs(name, C)
    sc[0], sh[0] = 1.0, 0.0
    wn = sparse_signs(name + ".w", 48, 9 * C).reshape(48, 9, C)
    wn[:, :, 0] = 0.0
    wn[:, 4, 0] = 192.0                                    # the centre tap exists at every pixel, borders included
    return y, np.ascontiguousarray(wn.transpose(1, 0, 2)), sc, sh


def conv_operands(name, B, H, W, C, ldy, prologue):
    xa, wa = amplitudes(9 * C, prologue)
    y = np.full((B, H, W, ldy), BIG)
    y[..., :C] = ints(name + ".y", (B, H, W, C), -xa, xa) if prologue else ints(name + ".y", (B, H, W, C), 0, 2 * xa)
    return y, ints(name + ".w", (9, 48, C), -wa, wa)


def condition_a(mag, unit, oscale=None, oshift=None):
    """condition (a): max over the outputs of (sum |a||w| + |bias|) / unit, which must stay below 2^23; with an output affine additionally the
    largest |value| it can form, in ITS unit (unit * min |oscale|, at most 0.25), which must stay below 2^24"""
    a = float(mag.max()) / unit
    if oscale is None:
        return a, 0.0
    u2 = min(unit * float(np.abs(oscale).min()), 0.25)
    return a, float((mag * np.abs(oscale) + np.abs(oshift)).max()) / u2


def condition_d(stored):
    """condition (d): 256 * max(v*v) (must stay below 2^24) and whether any stored value is fractional"""
    return 256.0 * float((stored * stored).max()), bool((stored != np.floor(stored)).any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the case lists of tests/test_gpu_bf16_exact.py (shapes: the smallest at which launch_gemm_bf16 / launch_conv3x3_bf16 / plan_conv3_act select
# the variant, every M and N just past the threshold and no multiple of the tile)
# ---------------------------------------------------------------------------------------------------------------------------------------------
# option sets of a tiled GEMM case: (prologue, bias, out_f32, output activation)
OPTS = ((True, False, False, False), (False, True, True, False), (True, False, False, True), (False, True, False, False), (True, False, True, False))
OPTS_SPLIT = ((True, False, False, False), (False, False, False, False), (True, False, False, True))

GEMM_CASES = {
    # name: (M, K, N, ldx - K, ldw - K, census tile)
    "t128x112": (8201, 72, 680, 8, 0, "128x112"),
    "t128x96": (13061, 88, 476, 0, 8, "128x96"),
    "t128x48": (21765, 104, 104, 16, 16, "128x48"),
    "t64x96": (1031, 120, 100, 8, 0, "64x96"),
    "t32x96_m33": (33, 8, 308, 24, 8, "32x96"),
    "t32x96_m1": (1, 8, 1204, 0, 0, "32x96"),
}
SPLIT_CASE = (70, 1048, 212, 8, 8)                       # cdiv(K, 64) = 17: the heuristic's scratch (8 M N floats) splits 4 ways, 2 M N floats 2 ways
PANEL_MN = (8201, 2980)                                   # 33 row panels x 32 column tiles = 1056 items; the last column tile holds 4 columns
PANEL_K = {8: 1, 40: 2, 120: 4, 184: 6, 200: 7, 312: 10, 352: 11}
STATS_GEMM_CASES = {"s64x96": (1031, 72, 100, 8), "s32x96": (77, 1048, 212, 8)}        # (M, K, N, ldx - K); the second runs unsplit and split

CONV_CASES = {
    # name: (B, H, W, C, prologue, (bm, HL))
    "img1x1": (200, 1, 1, 8, True, (64, 12)),
    "img2x3": (37, 2, 3, 24, True, (64, 4)),
    "img1x40": (7, 1, 40, 40, False, (64, 6)),
    "img40x1": (7, 40, 1, 24, True, (64, 4)),
    "w76": (2, 5, 76, 72, True, (64, 9)),
    "w150": (1, 3, 150, 8, False, (64, 20)),
    "c104": (3, 9, 13, 104, True, (64, 4)),
    "c136": (3, 9, 13, 136, False, (64, 4)),          # 5 slabs: the scratch permits a split of 2 over an odd slab count
    "bm128": (2, 47, 45, 40, True, (128, 6)),
    "bm256": (2, 64, 65, 24, False, (256, 12)),
    "bm256to128": (2, 28, 150, 8, True, (128, 20)),
}
STATS_CONV_CASES = {"sc64": (3, 9, 13, 104), "sc128": (2, 47, 45, 40), "sc256": (2, 64, 65, 24)}

ACT_CASES = {
    # name: (B, H, W, real channels, scratch, census)
    "nc1": (5, 9, 13, 8, False, "nc1/direct"),
    "nc2": (3, 182, 60, 40, False, "nc2/direct"),
    "nc3": (3, 367, 60, 72, False, "nc3/direct"),
    "nc4": (3, 550, 60, 8, False, "nc4/direct"),
    "nc1s": (2, 9, 13, 136, True, "nc1/splitK"),
    "nc2s": (12, 30, 19, 136, True, "nc2/splitK"),
    "nc3s": (20, 30, 19, 136, True, "nc3/splitK"),
    "nc4s": (30, 17, 23, 136, True, "nc4/splitK"),
    "rect": (1, 9, 260, 8, False, "nc1/direct/rect"),
}
COLSTATS_CASES = [(M, C) for M in (1, 255, 256, 257, 1000) for C in (8, 24)]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case builders shared by tests/test_bf16_ref_cpu.py (conditions) and tests/test_gpu_bf16_exact.py (the runs)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def build_gemm(name, M, K, N, px, pw, opt):
    """operands and exact float64 result of one planted GEMM run; opt = (prologue, bias, out_f32, output activation)"""
    pro, bias, _, act = opt
    x, w = gemm_operands(name, M, K, N, K + px, K + pw, pro)
    sc, sh = prologue_coeffs(name, K) if pro else (None, None)
    b = ints(name + ".b", (N,), -64, 64) / 4.0 if bias else None
    osc, osh = out_coeffs(name, N) if act else (None, None)
    exact, mag = gemm(x, w, K, sc, sh, b, osc, osh)
    return dict(x=x, w=w, sc=sc, sh=sh, bias=b, osc=osc, osh=osh, exact=exact, mag=mag, unit=0.25 if pro or bias else 1.0)


def panel_opt(K):
    """the panel kernel takes no bias and bf16 output: K alternates between prologue + output activation and the bare product"""
    return (True, False, False, True) if PANEL_K[K] % 2 == 0 or K == 352 else (False, False, False, False)


def build_conv(name, B, H, W, C, pro):
    ldy = C + 8
    y, w9 = conv_operands(name, B, H, W, C, ldy, pro)
    sc, sh = prologue_coeffs(name, C) if pro else (None, None)
    exact, mag = conv3x3(y, w9, C, sc, sh)
    return dict(y=y, w9=w9, sc=sc, sh=sh, ldy=ldy, exact=exact, mag=mag, unit=0.25 if pro else 1.0)


def build_act(name, B, H, W, C):
    Cp = (C + 31) // 32 * 32
    xa, wa = amplitudes(9 * C, False)
    y = np.full((B, H, W, Cp + 8), BIG)
    y[..., :C] = ints(name + ".y", (B, H, W, C), 0, 2 * xa)
    y[..., C:Cp] = 2.0 ** 60                                  # pad channels: large and finite, their weights are zero
    w = ints(name + ".w", (48, C, 3, 3), -wa, wa)
    exact, mag = conv3x3_act(y, w, C)
    return dict(y=y, w=w, Cp=Cp, exact=exact, mag=mag, unit=1.0)
