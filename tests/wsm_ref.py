"""Float64 references, planted inputs, case tables and exactness predicates for the WSM decoder bf16 kernels (csrc/wsm_bf16.hip).  No GPU.

The idea is that of tests/bf16_ref.py: wsm_conv_bf16_kernel multiplies bf16 operands on v_mfma_f32_16x16x32_bf16 and accumulates in f32.  With
activations and weights that are integers in [-4, 4] and biases that are multiples of 1/4 every product, every partial sum and the bias add are
exact in f32 in ANY order as long as sum |x||w| + |b| < 2^22 per output, so the f32 result equals the float64 reference and a bf16 output its
round-to-nearest-even rounding, on bits.  tests/test_wsm_ref_cpu.py asserts those conditions on every case below;
tests/test_gpu_wsm_exact.py runs the cases.

Layouts follow include/rdm_hip.h: activations NHWC (pixels, ld) with the operator's channels at [xoff, xoff + cin); weights [pad64(rows)][K]
with k = tap * pad32(cin) + ci.  Arrays are float64 numpy.

TILE RULE.  launch_wsm_conv_bf16 records no census entry, so `tile()` below is a restatement of the code, not a recording: the launcher
picks wsm_conv_bf16_kernel<4,2> (128 x 64 tiles) iff ceil(M / 128) * ceil(N / 64) >= 512 and <2,2> (64 x 64) otherwise, with N the GEMM's
row count (4 * pad32(c) for the deconv)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bf16_ref import BIG, bf16_bits, canon_bits, cdiv, choice, ints, round_bf16      # noqa: F401  (re-exported to the two test modules)
from md_rdm_amd import filler
from test_rel_restatement_cpu import WSM_GEOM, decoder_state, wsm_layer

PAD = 2.0 ** 60            # activation pad channels [cin, pad32(cin)): finite, their weights are zero (the packer's contract)
LIMIT = 2.0 ** 22          # exact accumulation: sum |x||w| + |b| per output stays below this


def p32(c):
    return (c + 31) // 32 * 32


def p64(c):
    return (c + 63) // 64 * 64


def tile(M, N):
    """the tile launch_wsm_conv_bf16 picks (restated from the code, see the module docstring)"""
    return "<4,2>" if cdiv(M, 128) * cdiv(N, 64) >= 512 else "<2,2>"


def k_steps(K):
    """nk of wsm_conv_bf16_kernel: 64-deep K steps (the pipeline prologue branches on nk > 1, nk > 2 and k + 3 < nk)"""
    return cdiv(K, 64)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exactness predicates
# ---------------------------------------------------------------------------------------------------------------------------------------------
def is_bf16(v):
    """every value is a bf16 number"""
    v = np.asarray(v, dtype=np.float64)
    return bool(np.array_equal(round_bf16(v)[0], v))


def rounding_counts(exact64):
    """how the exact values meet the bf16 grid, by VALUE (above = towards +inf): inexact values that are no ties and round up / down, exact ties
    whose even neighbour lies above / below"""
    v = np.asarray(exact64, dtype=np.float64)
    r, tie = round_bf16(v)
    return dict(up=int(((r > v) & ~tie).sum()), down=int(((r < v) & ~tie).sum()), tie_above=int(((r > v) & tie).sum()), tie_below=int(((r < v) & tie).sum()))


def exact_sum(mag):
    """the largest sum |x||w| + |b| of a case: below LIMIT every f32 summation order is exact for integer operands and quarter-integer biases"""
    return float(np.max(mag))


def operands_ok(c):
    """the planted operands are what the issue's conditions name: integers in [-4, 4], biases multiples of 1/4 with |b| <= 8"""
    ok = all(np.array_equal(a, np.floor(a)) and np.abs(a).max() <= 4 for a in (c["xin"], c["w"]))
    b = c.get("b")
    return ok and (b is None or (np.array_equal(4 * b, np.floor(4 * b)) and np.abs(b).max() <= 8))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# float64 references (torch CPU); each also returns sum |x||w| + |b| per output
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _nchw(x, B, H, W):
    return T(x).reshape(B, H, W, -1).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def conv_ref(xin, w, b, B, H, W):
    """rdm_wsm_conv_bf16: xin (B*H*W, cin), w (n, cin, k, k), stride 1, zero padding k // 2 -> (B*H*W, n)"""
    k = w.shape[2]
    out = _nhwc(F.conv2d(_nchw(xin, B, H, W), T(w), padding=k // 2))
    mag = _nhwc(F.conv2d(_nchw(np.abs(xin), B, H, W), T(np.abs(w)), padding=k // 2))
    return (out, mag) if b is None else (out + b, mag + np.abs(b))


def deconv_ref(xin, w, b, B, h, wd):
    """rdm_wsm_deconv_bf16: ConvTranspose2d(k 2, s 2), w (cin, c, 2, 2) -> (B*2h*2w, c), pixel (2y + r, 2x + s) from phase (r, s)"""
    out = _nhwc(F.conv_transpose2d(_nchw(xin, B, h, wd), T(w), stride=2))
    mag = _nhwc(F.conv_transpose2d(_nchw(np.abs(xin), B, h, wd), T(np.abs(w)), stride=2))
    return (out, mag) if b is None else (out + b, mag + np.abs(b))


def strip_values(xin, w, b, B, S, columns):
    """the strip conv's ONE value per row (columns = 0: w (n, ci, 3, S) after ZeroPad2d((0,0,1,1))) or per column (columns = 1: w (n, ci, S, 3) after
    ZeroPad2d((1,1,0,0))) of a (B,S,S) map: (B, S, n), and its sum |x||w| + |b|"""
    def run(x, wt):
        x = _nchw(x, B, S, S)
        if columns:
            return F.conv2d(F.pad(x, (1, 1, 0, 0)), T(wt), stride=(S, 1))[:, :, 0, :].permute(0, 2, 1).numpy()
        return F.conv2d(F.pad(x, (0, 0, 1, 1)), T(wt), stride=(1, S))[:, :, :, 0].permute(0, 2, 1).numpy()
    out, mag = run(xin, w), run(np.abs(xin), np.abs(w))
    return (out, mag) if b is None else (out + b, mag + np.abs(b))


def strip_broadcast(v, columns):
    """(B, S, n) values -> the (B*S*S, n) map: row values repeated along W, column values repeated along H"""
    B, S, n = v.shape
    full = np.broadcast_to(v[:, None, :, :] if columns else v[:, :, None, :], (B, S, S, n))
    return np.ascontiguousarray(full).reshape(-1, n)


def nchw_to_nhwc(x, ld):
    """rdm_rel_bf16_input_nchw: (B,1056,8,8) f32 -> (B*64, ld) rounded to bf16; columns from 1056 on are not written (NaN here)"""
    B, C = x.shape[:2]
    out = np.full((B * 64, ld), np.nan)
    out[:, :C] = round_bf16(x.reshape(B, C, 64).transpose(0, 2, 1).reshape(B * 64, C))[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted operands in the kernels' layouts
# ---------------------------------------------------------------------------------------------------------------------------------------------
def place_x(xin, ldx, xoff, cin):
    """the activation buffer as ONE flat array: 2^100 outside [xoff, xoff + pad32(cin)), 2^60 in the pad channels, and 64 NaNs directly behind the
    last element (a read past x_bytes would fold one into a sum).  Where xoff + pad32(cin) > ldx the kernel's pad channels are the first channels
    of the next pixel: finite, whatever they are."""
    M = xin.shape[0]
    x = np.full((M, ldx), BIG)
    x[:, xoff + cin:min(xoff + p32(cin), ldx)] = PAD
    x[:, xoff:xoff + cin] = xin
    return np.concatenate([x.reshape(-1), np.full(64, np.nan)])


def pack_rows(wt, cin):
    """(rows, taps, cin) -> [pad64(rows)][taps * pad32(cin)]: zero weight columns ci in [cin, pad32(cin)) of every tap, 2^100 in the rows from `rows` on"""
    rows, taps, _ = wt.shape
    wp = np.full((p64(rows), taps, p32(cin)), BIG)
    wp[:rows] = 0.0
    wp[:rows, :, :cin] = wt
    return wp.reshape(p64(rows), -1)


def _operands(name, M, cin, wshape, bias, real, nb=None):
    if real:                                                    # the real-valued leg: uniform reals rounded to bf16, f32 bias
        xin = round_bf16(filler.uniform(name + ".rx", (M, cin), -2.0, 2.0, np.float32).astype(np.float64))[0]
        fan = float(np.prod(wshape[1:])) if len(wshape) == 4 else float(wshape[0])
        w = round_bf16(filler.uniform(name + ".rw", wshape, -1.0, 1.0, np.float32).astype(np.float64) / np.sqrt(fan))[0]
        b = filler.uniform(name + ".rb", (nb,), -0.5, 0.5, np.float32).astype(np.float64) if bias else None
    else:
        xin, w = ints(name + ".x", (M, cin), -4, 4), ints(name + ".w", wshape, -4, 4)
        b = ints(name + ".b", (nb,), -32, 32) / 4.0 if bias else None
    return xin, w, b


@functools.lru_cache(maxsize=None)
def build_conv(name, real=False):
    """one rdm_wsm_conv_bf16 case of CONV_CASES: operands in the kernel's layouts and the exact float64 result"""
    B, H, W, cin, n, k, ldx, xoff, bias = CONV_CASES[name]
    M = B * H * W
    xin, w, b = _operands(name, M, cin, (n, cin, k, k), bias, real, n)
    exact, mag = conv_ref(xin, w, b, B, H, W)
    wp = pack_rows(w.transpose(0, 2, 3, 1).reshape(n, k * k, cin), cin)
    return dict(x=place_x(xin, ldx, xoff, cin), wp=wp, b=b, xin=xin, w=w, exact=exact, mag=mag, M=M, N=n, K=k * k * p32(cin), geom=(B, H, W), k=k,
                cin=cin, n=n, ldx=ldx, xoff=xoff)


@functools.lru_cache(maxsize=None)
def build_conv1x1_f32(cin, M, real=False):
    """rdm_wsm_conv1x1_f32: ldx = cin (for cin % 32 != 0 the pad channels of a pixel are the next pixel's first channels), one output channel + bias"""
    name = "c1f.%d.%d" % (cin, M)
    xin, w, b = _operands(name, M, cin, (1, cin, 1, 1), True, real, 1)
    exact, mag = conv_ref(xin, w, b, 1, 1, M)
    return dict(x=place_x(xin, cin, 0, cin), wp=pack_rows(w.reshape(1, 1, cin), cin), b=b, xin=xin, w=w, exact=exact, mag=mag, M=M, N=1, K=p32(cin), cin=cin)


@functools.lru_cache(maxsize=None)
def build_deconv(cin, c, B, h, wd, real=False):
    """rdm_wsm_deconv_bf16: weight rows (2 r + s) * pad32(c) + co with the bias in the same row order (zeros in the pad rows, as
    tests/test_gpu_relative_bf16.py::run_deconv lays it out); the pad rows [c, pad32(c)) of every phase hold 2^100: the kernel computes them and
    must not store them"""
    name = "dc.%d.%d.%d.%d.%d" % (cin, c, B, h, wd)
    M, cp = B * h * wd, p32(c)
    xin, w, b = _operands(name, M, cin, (cin, c, 2, 2), True, real, c)
    exact, mag = deconv_ref(xin, w, b, B, h, wd)
    wt = np.full((4 * cp, 1, cin), BIG)
    br = np.zeros(4 * cp)
    for r in range(2):
        for s in range(2):
            ph = 2 * r + s
            wt[ph * cp:ph * cp + c, 0] = w[:, :, r, s].T
            br[ph * cp:ph * cp + c] = b
    return dict(x=place_x(xin, p32(cin) + 8, 0, cin), wp=pack_rows(wt, cin), b=br, xin=xin, w=w, exact=exact, mag=mag, M=M, N=4 * cp, K=p32(cin), ldx=p32(cin) + 8,
                ldc=c + 8, cin=cin, c=c)


@functools.lru_cache(maxsize=None)
def build_strip(name, columns, real=False):
    """one rdm_wsm_strip_bf16 case of STRIP_CASES: cw - 6 real input channels in a slot of cw, k = (tap * S + position) * cw + ci"""
    S, cw, n, B, xoff, coff = STRIP_CASES[name]
    cr, M = cw - 6, B * S * S
    key = "%s.%d" % (name, columns)
    xin, w, b = _operands(key, M, cr, (n, cr, S, 3) if columns else (n, cr, 3, S), True, real, n)
    values, mag = strip_values(xin, w, b, B, S, columns)
    wt = (w.transpose(0, 3, 2, 1) if columns else w.transpose(0, 2, 3, 1)).reshape(n, 3 * S, cr)        # (n, tap, position, ci)
    ldx = xoff + cw + 8
    return dict(x=place_x(xin, ldx, xoff, cr), wp=pack_rows(wt, cr), b=b, xin=xin, w=w, values=values, exact=strip_broadcast(values, columns), mag=mag, M=B * S, N=n,
                K=3 * S * cw, S=S, cw=cw, n=n, B=B, ldx=ldx, xoff=xoff, coff=coff, ldc=coff + n + 6)


def with_ties(key, shape, lo, hi):
    """f32-representable reals: a quarter exact bf16 ties (bf16 value + half an ulp, the even neighbour above for some and below for others), a
    quarter each just below / above a tie, the rest uniform"""
    u = filler.uniform(key, shape, lo, hi, np.float32).astype(np.float64)
    b = round_bf16(u)[0]
    half = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(b), 2.0 ** -100))) - 8)
    kind = ints(key + ".k", shape, 0, 7)
    t = b + half * np.select([kind == 0, kind == 1, kind == 2], [1.0, 1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10], 0.0)
    v = np.where(kind <= 2, t, u)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v


# ---------------------------------------------------------------------------------------------------------------------------------------------
# operator case tables: the smallest shapes past each branch of wsm_conv_bf16_kernel and its launcher
# ---------------------------------------------------------------------------------------------------------------------------------------------
CONV_CASES = {}          # name: (B, H, W, cin, n, k, ldx, xoff, bias)
STORES = {}              # name: the (coff, ldc) pairs a case is stored through (one launch each, one reference)
TILES = {}               # name: the tile the launcher picks (recomputed by the CPU test)


def _case(name, B, H, W, cin, n, k, ldx=None, xoff=0, bias=True, stores=None, tile_="<2,2>"):
    CONV_CASES[name] = (B, H, W, cin, n, k, p32(cin) + 8 if ldx is None else ldx, xoff, bias)
    STORES[name] = tuple(stores) if stores else ((4, n + 12),)
    TILES[name] = tile_


# k = 1, K steps and tails: pad32(cin) = 32, 64, 96, 160, 192, 224, 288 -> nk = 1, 1, 2, 3, 3, 4, 5 and K % 64 in {32, 0}; M = 105, N = 130: 2 x 3 blocks
K_AXIS = {32: (32, 1), 64: (64, 1), 72: (96, 2), 136: (160, 3), 192: (192, 3), 200: (224, 4), 264: (288, 5)}      # cin: (pad32(cin), nk)
for _cin in K_AXIS:
    _case("k1_K%d" % _cin, 3, 5, 7, _cin, 130, 1)
_case("k1_c40_ld40", 1, 5, 13, 40, 26, 1, ldx=40)                # kc = 64 > ldx = 40: the pad channels are the next pixel's, and NaN behind the buffer
_case("k1_c208_ld208", 1, 5, 13, 208, 52, 1, ldx=208)            # d_10's conv1 geometry
# N and store paths: (0, n+12) / (4, n+12) can take the 8-byte store, (2, n+10) / (3, n+9) give an odd ldc and 2-byte stores throughout
N_AXIS = (1, 10, 26, 52, 64, 65, 130)
for _n in N_AXIS:
    _case("k1_n%d" % _n, 1, 5, 13, 32, _n, 1, stores=[(0, _n + 12), (4, _n + 12), (2, _n + 10), (3, _n + 9)] + ([(156, 208), (182, 208)] if _n == 26 else []))
# M = 1, 33, 64, 65, 105 with bias and with NULL
M_AXIS = {1: (1, 1, 1), 33: (1, 3, 11), 64: (1, 8, 8), 65: (1, 5, 13), 105: (3, 5, 7)}
for _m, _g in M_AXIS.items():
    _case("k1_M%d" % _m, *_g, 64, 26, 1)
    _case("k1_M%d_nobias" % _m, *_g, 64, 26, 1, bias=False)
# xoff = 0, 8, 40 with ldx > xoff + cin: once narrower than xoff + pad32(cin) (the pad channels wrap into the next pixel), once wider
for _xo in (0, 8, 40):
    _case("k1_xoff%d" % _xo, 1, 5, 13, 40, 26, 1, ldx=_xo + 48, xoff=_xo)
    _case("k1_xoff%d_wide" % _xo, 1, 5, 13, 40, 26, 1, ldx=_xo + 72, xoff=_xo)
# k = 3 and k = 5: all four borders, the corners and the batch boundaries are distinct terms; maps smaller than the kernel (64 of them: enough outputs
# for the rounding counts although only 2 taps of 9 / 25 ever meet the image)
for _k in (3, 5):
    _case("k%d_b3" % _k, 3, 5, 7, 32, 26, _k)
    _case("k%d_1x2" % _k, 64, 1, 2, 32, 26, _k)
    _case("k%d_2x9" % _k, 3, 2, 9, 32, 26, _k)
_case("k5_c40", 3, 5, 7, 40, 26, 5, ldx=48)                      # pad32 = 64 per tap, K = 1600
# the <4,2> tile and the shape just below its threshold
_case("t42_k1", 1, 65, 125, 32, 450, 1, tile_="<4,2>")           # M = 8125: 64 x 8 = 512 tiles
_case("t22_k1", 1, 63, 128, 32, 450, 1, tile_="<2,2>")           # M = 8064: 63 x 8 = 504 tiles
_case("t42_k3", 2, 64, 65, 32, 450, 3, tile_="<4,2>")            # M = 8320: 65 x 8 = 520 tiles
DECONV_TILE_CASE = (32, 104, 1, 65, 125)                         # N = 4 * 128 = 512: 64 x 8 = 512 tiles -> <4,2>

DECONV_CC = ((32, 26), (64, 40), (96, 104))                      # (cin, c): c % 4 != 0 and c % 32 != 0
DECONV_GEOMS = tuple((B, h, w) for B in (1, 2) for (h, w) in ((1, 1), (3, 5), (5, 3)))

STRIP_CASES = {
    # name: (S, cw, n, B, xoff, coff); K = 3 * S * cw.  The cases with K >= 256 have enough outputs (B * S * n) for the rounding counts
    "S1_a": (1, 32, 5, 1, 0, 0),
    "S1_b": (1, 64, 26, 3, 32, 6),
    "S2_a": (2, 32, 5, 1, 0, 6),
    "S2_b": (2, 32, 32, 3, 32, 0),
    "S2_c": (2, 64, 32, 3, 0, 6),
    "S4_a": (4, 32, 32, 3, 32, 0),
    "S4_b": (4, 64, 26, 3, 0, 6),
    "S8_a": (8, 32, 26, 3, 32, 6),
    "S8_b": (8, 64, 32, 1, 0, 0),
}
CONV1X1_CASES = tuple((cin, M) for cin in (32, 40, 208) for M in (1, 65))
NCHW_CASES = tuple((B, ld) for B in (1, 2) for ld in (1056, 1064))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the chain: a planted Decoder whose WSM chain + conv1 is exact in bf16 / f32
# ---------------------------------------------------------------------------------------------------------------------------------------------
def sparse_rows(key, rows, length):
    """(rows, length): two entries of +-1 per row at filler-hashed positions over the whole row (they may meet: the row's L1 norm is at most 2)"""
    pos = ints(key + ".p", (rows, 2), 0, length - 1).astype(np.int64)
    sg = choice(key + ".s", (rows, 2), (-1.0, 1.0))
    w = np.zeros((rows, length))
    np.add.at(w, (np.arange(rows)[:, None], pos), sg)
    return w


@functools.lru_cache(maxsize=None)
def planted_state(did):
    """float64 state of decoder d_`did`: the dense block from the filler with every conv2.weight zero (the block the chain reads is [enc | 0]);
    WSM weights sparse +-1 (two per GEMM output row: every stage at most doubles max |v|), WSM biases zero except WSM_1 of d_7 ({-1, 0, 1});
    conv1 dense integers in [-4, 4], bias 2.0"""
    sd = dict(decoder_state(did))
    for key in list(sd):
        shape = tuple(sd[key].shape)
        if key.startswith("dense_layer.") and key.endswith("conv2.weight"):
            sd[key] = torch.zeros_like(sd[key])
        elif key.startswith("wsm_block."):
            if key.endswith(".bias"):
                sd[key] = T(ints(key, shape, -1, 1)) if did == 7 else torch.zeros_like(sd[key])
            elif ".deconv1." in key:                             # (Cin, Cout, 2, 2): a GEMM row is (co, r, s) over ci
                sd[key] = T(sparse_rows(key, shape[1] * 4, shape[0]).reshape(shape[1], 2, 2, shape[0]).transpose(3, 0, 1, 2))
            else:                                                # (out, in, kh, kw): a GEMM row is `out` over (in, kh, kw)
                sd[key] = T(sparse_rows(key, shape[0], int(np.prod(shape[1:]))).reshape(shape))
    sd["conv1.weight"] = T(ints("d_%d.conv1.dense" % did, tuple(sd["conv1.weight"].shape), -4, 4))
    sd["conv1.bias"] = torch.full_like(sd["conv1.bias"], 2.0)
    return sd


@functools.lru_cache(maxsize=None)
def planted_enc(did):
    """(2 * 64, 1056) integers in {-1, 0, 1}: the B = 2 encoder output; the B = 1 runs take its two images"""
    return ints("d_%d.enc.planted" % did, (128, 1056), -1, 1)


def enc_buffer(enc, ld):
    """enc in a (rows, ld) buffer with 2^100 in the columns from 1056 on"""
    out = np.full((enc.shape[0], ld), BIG)
    out[:, :1056] = enc
    return out


def chain_input(enc):
    """(B*64, 1056) NHWC -> the (B, 2208, 8, 8) block [enc | 0] the WSM chain reads"""
    B = enc.shape[0] // 64
    x = torch.zeros(B, 2208, 8, 8, dtype=torch.float64)
    x[:, :1056] = T(enc).reshape(B, 8, 8, 1056).permute(0, 3, 1, 2)
    return x


def wsm_stages(x, sd, pre, S):
    """every tensor the bf16 chain STORES for one WSM layer (t, out1, the five conv1_k outputs) and the five slots, as WSMLayer.forward forms them;
    chain_f64 holds the assembled slots against the imported wsm_layer"""
    w = lambda n: sd[pre + n + ".weight"]                                     # noqa: E731
    b = lambda n: sd[pre + n + ".bias"]                                       # noqa: E731
    t = F.conv2d(x, w("input_adjustment_layer"), b("input_adjustment_layer"))
    out1 = F.conv_transpose2d(t, w("deconv1.0"), b("deconv1.0"), stride=2)
    o = [F.conv2d(out1, w("conv1_%d" % k), b("conv1_%d" % k)) for k in range(1, 6)]
    wx3 = F.conv2d(F.pad(o[3], (0, 0, 1, 1)), w("wsm_wx3.1"), b("wsm_wx3.1"), stride=(1, S))
    h3 = F.conv2d(F.pad(o[4], (1, 1, 0, 0)), w("wsm_3xh.1"), b("wsm_3xh.1"), stride=(S, 1))
    slots = [o[0], F.conv2d(o[1], w("conv2_1"), b("conv2_1"), padding=1), F.conv2d(o[2], w("conv2_2"), b("conv2_2"), padding=2),
             h3.repeat(1, 1, h3.shape[3], 1), wx3.repeat(1, 1, 1, wx3.shape[2])]
    return dict(t=t, out1=out1, conv1_1=o[0], conv1_2=o[1], conv1_3=o[2], conv1_4=o[3], conv1_5=o[4], slot0=slots[0], slot1=slots[1], slot2=slots[2],
                slot3=slots[3], slot4=slots[4])


def chain_f64(did, sd, enc, stages=None, slot_order=(0, 1, 2, 3, 4)):
    """the expected map: WSM_1..WSM_(did-6) (tests/test_rel_restatement_cpu.py::wsm_layer, imported) on [enc | 0], then conv1, in float64.
    `stages` (a list) collects wsm_stages of every layer plus conv1's sum |x||w|; `slot_order` permutes the cat order of the LAST layer's slots
    (a mutation of the reference's structure)."""
    with torch.no_grad():
        h = chain_input(enc)
        for l in range(did - 6):
            pre, S = "wsm_block.WSM_%d." % (l + 1), WSM_GEOM[l][1]
            nxt = wsm_layer(h, sd, pre, S)
            if stages is not None:
                st = wsm_stages(h, sd, pre, S)
                assert torch.equal(torch.cat([st["slot%d" % i] for i in range(5)], 1), nxt)
                stages.append(st)
            if l == did - 7 and tuple(slot_order) != (0, 1, 2, 3, 4):
                C = nxt.shape[1]
                edges = [0, C // 4, C // 2, 3 * C // 4, 7 * C // 8, C]
                nxt = torch.cat([nxt[:, edges[i]:edges[i + 1]] for i in slot_order], 1)
            h = nxt
        if stages is not None:
            stages.append(dict(conv1_mag=F.conv2d(h.abs(), sd["conv1.weight"].abs()) + sd["conv1.bias"].abs()))
        return F.conv2d(h, sd["conv1.weight"], sd["conv1.bias"]).numpy()


@functools.lru_cache(maxsize=None)
def expected_map(did):
    """the float64 map (2, 1, S, S) of the planted decoder on the planted B = 2 input, computed once and shared"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m = chain_f64(did, planted_state(did), planted_enc(did))
    m.setflags(write=False)
    return m


WSM_CONVS = ("input_adjustment_layer", "deconv1.0", "conv1_1", "conv1_2", "conv1_3", "conv1_4", "conv1_5", "conv2_1", "conv2_2", "wsm_wx3.1", "wsm_3xh.1")


def _swap(sd, a, b, fa=lambda t: t, fb=lambda t: t):
    sd[a], sd[b] = fb(sd[b]).contiguous(), fa(sd[a]).contiguous()


def mutations(pre="wsm_block.WSM_1."):
    """name -> (state transform, slot order): the packing / routing errors the planted chain must be able to see.  Each is applied to a COPY of
    the planted state (or to the reference's cat order) and must change the expected map."""
    xy = lambda t: t.permute(0, 1, 3, 2)                                      # noqa: E731

    def on(key, f):
        def apply(sd):
            sd[pre + key] = f(sd[pre + key]).contiguous()
        return apply

    def strips_swapped(sd):
        _swap(sd, pre + "wsm_wx3.1.weight", pre + "wsm_3xh.1.weight", xy, xy)

    def strips_rolled(sd):
        sd[pre + "wsm_wx3.1.weight"] = sd[pre + "wsm_wx3.1.weight"].roll(1, 3)
        sd[pre + "wsm_3xh.1.weight"] = sd[pre + "wsm_3xh.1.weight"].roll(1, 2)

    def conv1_k_exchanged(sd):
        _swap(sd, pre + "conv1_2.weight", pre + "conv1_3.weight")
        _swap(sd, pre + "conv1_2.bias", pre + "conv1_3.bias")

    keep = (0, 1, 2, 3, 4)
    return {
        "conv2_2 spatial axes transposed": (on("conv2_2.weight", xy), keep),
        "conv2_1 tap order reversed": (on("conv2_1.weight", lambda t: t.flip(2, 3)), keep),
        "wsm_wx3 and wsm_3xh swapped": (strips_swapped, keep),
        "strip positions rolled by one": (strips_rolled, keep),
        "deconv phases (r, s) swapped": (on("deconv1.0.weight", xy), keep),
        "conv1_2 exchanged with conv1_3": (conv1_k_exchanged, keep),
        "slots 1 and 2 exchanged in the cat": (lambda sd: None, (0, 2, 1, 3, 4)),
        "slots 3 and 4 exchanged in the cat": (lambda sd: None, (0, 1, 2, 4, 3)),
        "input_adjustment_layer input channels rolled by one": (on("input_adjustment_layer.weight", lambda t: t.roll(1, 1)), keep),
        **{"%s bias dropped" % k: (on(k + ".bias", torch.zeros_like), keep) for k in WSM_CONVS},
    }
