"""-m gpu: the bf16 forward kernels (csrc/bf16.hip) BIT FOR BIT against float64 on inputs whose f32 arithmetic is exact.

Planted inputs (tests/bf16_ref.py): small-integer activations and weights, power-of-two prologue scales, quarter-integer shifts / biases, +-power-
of-two output scales.  Every product, partial sum and fmaf is then exact in f32 in any summation order (tests/test_bf16_ref_cpu.py asserts the
conditions (a)-(d) on every case below), so the tile shape, the K split, the panel kernel and the reduction order cannot change a bit: the f32
result must EQUAL the float64 reference, the bf16 result its round-to-nearest-even rounding, the statistics their float64 sums.  The tolerance of
these legs is zero - derived, not measured; a dropped, duplicated or misplaced term anywhere is a nonzero difference.  -0.0 and +0.0 compare equal.

Every output buffer is NaN-filled and wider than its slot (the columns outside the slot must still be NaN), every reference is computed on the CPU
in float64, every case asserts through the census that the kernel variant it was shaped for ran (shapes: the smallest past each threshold of
launch_gemm_bf16 / launch_conv3x3_bf16 / plan_conv3_act, ragged in M and N).  The helper kernels, which round and move but do not sum, run on
real-valued inputs with planted ties.  A last leg runs uniform real inputs against the bound (K+2) 2^-24 sum|a||w| (+ half a bf16 ulp)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_ref as R

pytestmark = pytest.mark.gpu
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def lib():
    from md_rdm_amd import _lib
    return _lib


def D(a, dtype, dev):
    """float64 numpy -> device tensor of `dtype` (None stays None); the planted values are exact in every dtype they are sent in"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    assert dtype == bf16 or torch.equal(t.double(), torch.from_numpy(np.ascontiguousarray(a)))
    return t.to(dev)


def nans(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def ran(call):
    """census entries added by `call`"""
    L = lib()
    before = L.census()
    call()
    torch.cuda.synchronize()
    after = L.census()
    return {k for k, v in after.items() if v > before.get(k, 0)}


def same(out, n0, n1, exact):
    """the slot [n0, n1) of `out` holds `exact` (f32: equal; bf16: equal to its rounding, on bits), everything outside is still NaN"""
    assert torch.isnan(out[:, :n0].float()).all() and torch.isnan(out[:, n1:].float()).all(), "columns outside the slot were written"
    got = out[:, n0:n1]
    if out.dtype == f32:
        bad = got.cpu().double().numpy() != exact
    else:
        bad = R.canon_bits(got) != R.bf16_bits(exact)
    assert not bad.any(), "%d of %d differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
def call_gemm(dev, c, M, K, N, px, pw, opt, ws_floats=0, exact=None, check=same):
    L, P = lib().lib(), lib().ptr
    pro, bias, out_f32, act = opt
    x, w = D(c["x"], bf16, dev), D(c["w"], bf16, dev)
    sc, sh, b, osc, osh = (D(c[k], f32, dev) for k in ("sc", "sh", "bias", "osc", "osh"))
    ws = torch.empty(max(ws_floats, 64), dtype=f32, device=dev)
    ldc = N + 12
    out = nans((M, ldc), f32 if out_f32 else bf16, dev)
    wsp, wsb = (P(ws), ws_floats * 4) if ws_floats else (None, 0)
    if act:
        fn = lambda: lib().check(L.rdm_gemm_bf16_act(P(x), K + px, K, P(sc), P(sh), P(w), K + pw, P(osc), P(osh), P(out), ldc, M, N, wsp, wsb, lib().stream()))
    else:
        fn = lambda: lib().check(L.rdm_gemm_bf16(P(x), K + px, K, P(sc), P(sh), P(w), K + pw, P(b), P(out), ldc, M, N, int(out_f32), wsp, wsb, lib().stream()))
    names = ran(fn)
    check(out, 0, N, c["exact"] if exact is None else exact)
    return names


@pytest.mark.parametrize("name", sorted(R.GEMM_CASES))
def test_gemm_tiles_exact(dev, op_census, name):
    """rdm_gemm_bf16 / rdm_gemm_bf16_act, one case per tile of launch_gemm_bf16; each runs prologue on / off, bias on / off, f32 and bf16 output and the
    output affine + ReLU with negative scales.  K = 8 alone and tails of 8, 24, 40, 56 past a 64-deep step; N % 16 in {4, 8, 12}; ldx > K and ldw > K
    with 2^100 in the extra columns; M = 1 and M = 33."""
    M, K, N, px, pw, tile = R.GEMM_CASES[name]
    for opt in R.OPTS:
        assert call_gemm(dev, R.build_gemm(name, M, K, N, px, pw, opt), M, K, N, px, pw, opt) == {"gemm_bf16_kernel/" + tile}, opt


def test_gemm_split_k_exact(dev, op_census):
    """the K-split over grid.z + k_reduce_partials_bf16: the heuristic's scratch (4 splits of 17 steps) and one that allows 2; K % 64 = 24"""
    M, K, N, px, pw = R.SPLIT_CASE
    for opt in R.OPTS_SPLIT:
        c = R.build_gemm("split", M, K, N, px, pw, opt)
        for ws in (8 * M * N, 2 * M * N):
            assert call_gemm(dev, c, M, K, N, px, pw, opt, ws) == {"gemm_bf16_kernel/32x96/splitK"}, (opt, ws)
        assert call_gemm(dev, c, M, K, N, px, pw, opt, 0) == {"gemm_bf16_kernel/32x96"}


@pytest.mark.parametrize("K", sorted(R.PANEL_K))
def test_gemm_panel_exact(dev, op_census, K):
    """gemm_panel_bf16_kernel/nkk{1,2,4,6,7,10,11}: K % 32 in {8, 24, 0}; 33 ragged row panels x 32 column tiles, the last 4 columns wide"""
    M, N = R.PANEL_MN
    opt = R.panel_opt(K)
    assert call_gemm(dev, R.build_gemm("panel%d" % K, M, K, N, 8, 0, opt), M, K, N, 8, 0, opt) == {"gemm_panel_bf16_kernel/nkk%d" % R.PANEL_K[K]}


def check_stats(s, q, stored):
    assert np.array_equal(s.cpu().numpy(), stored.sum(0)) and np.array_equal(q.cpu().numpy(), (stored * stored).sum(0))


@pytest.mark.parametrize("name", sorted(R.STATS_GEMM_CASES))
def test_gemm_stats_exact(dev, op_census, name):
    """rdm_gemm_bf16_stats: stored output bit-exact, sum / sumsq bit-equal to float64 (condition (d)); unsplit and split, M no multiple of 8 or of the tile"""
    L, P = lib().lib(), lib().ptr
    M, K, N, px = R.STATS_GEMM_CASES[name]
    xh, wh, sch, shh = R.stats_gemm_operands(name, M, K, N, K + px)
    exact = R.gemm(xh, wh, K, sch, shh)[0]
    stored = R.stored_stats(exact)[0]
    x, w, sc, sh = D(xh, bf16, dev), D(wh, bf16, dev), D(sch, f32, dev), D(shh, f32, dev)
    sb = int(L.rdm_bf16_stats_workspace_bytes(M, N))
    for extra in (0, 8 * M * N * 4):
        ws = torch.empty(sb + extra, dtype=torch.uint8, device=dev)
        out, s, q = nans((M, N + 8), bf16, dev), nans((N,), f64, dev), nans((N,), f64, dev)
        names = ran(lambda: lib().check(L.rdm_gemm_bf16_stats(P(x), K + px, K, P(sc), P(sh), P(w), K, P(out), N + 8, M, N, P(s), P(q), P(ws), sb + extra, lib().stream())))
        assert names == {R.gemm_variant(M, K, N, extra // 4, stats=True)}
        same(out, 0, N, exact)
        check_stats(s, q, stored)
    assert (name == "s32x96") == ("gemm_bf16_kernel/32x96/splitK" in names)


# ---- 3x3 ----------------------------------------------------------------------------------------------------------------------------------
def conv_scratches(L, B, H, W, C):
    M = B * H * W
    return (0, int(L.rdm_conv3x3_bf16_workspace_bytes(C, B, H, W)), 2 * M * 48 * 4)      # absent, the heuristic's, one that permits a split of 2


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_conv3x3_exact(dev, name):
    """rdm_conv3x3_bf16 with and without prologue: bm = 64 / 128 / 256 (and 256 -> 128 for wide rows), every HL class, C % 32 in {8, 24}, images
    smaller than a tile (1x1, 2x3, 1x40, 40x1: a 64-pixel tile spans up to 64 images), H*W no divisor of bm, ragged last tiles; positive shifts:
    a zero-padded pixel sent through the prologue would add relu(shift).  The eval form records no census: the expected (bm, HL) is computed
    from the rules of launch_conv3x3_bf16 (bf16_ref.conv3_plan) and held against the case list on the CPU."""
    L, P = lib().lib(), lib().ptr
    B, H, W, Cc, pro, _ = R.CONV_CASES[name]
    c = R.build_conv(name, B, H, W, Cc, pro)
    M, ldy = B * H * W, c["ldy"]
    y, wp, sc, sh = D(c["y"], bf16, dev), D(c["w9"], bf16, dev), D(c["sc"], f32, dev), D(c["sh"], f32, dev)
    for wsb in conv_scratches(L, B, H, W, Cc):
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        out = nans((M, 96), bf16, dev)
        lib().check(L.rdm_conv3x3_bf16(P(y), ldy, Cc, P(sc), P(sh), P(wp), C.c_void_p(out.data_ptr() + 32), 96, B, H, W, P(ws) if wsb else None, wsb, lib().stream()))
        same(out, 16, 64, c["exact"])
    if name == "c136":
        assert R.conv3_plan(B, H, W, Cc, 2 * M * 48)[2] == 2 and R.cdiv(Cc, 32) % 2 == 1


@pytest.mark.parametrize("name", sorted(R.STATS_CONV_CASES))
def test_conv3x3_stats_exact(dev, op_census, name):
    """rdm_conv3x3_bf16_stats at bm = 64 (split and unsplit), 128, 256: stored output, sum and sumsq"""
    L, P = lib().lib(), lib().ptr
    B, H, W, Cc = R.STATS_CONV_CASES[name]
    M = B * H * W
    yh, w9, sch, shh = R.stats_conv_operands(name, B, H, W, Cc, Cc + 8)
    exact = R.conv3x3(yh, w9, Cc, sch, shh)[0]
    stored = R.stored_stats(exact)[0]
    y, wp, sc, sh = D(yh, bf16, dev), D(w9, bf16, dev), D(sch, f32, dev), D(shh, f32, dev)
    sb = int(L.rdm_bf16_stats_workspace_bytes(M, 48))
    for extra in (0, 2 * M * 48 * 4):
        ws = torch.empty(sb + extra, dtype=torch.uint8, device=dev)
        out, s, q = nans((M, 96), bf16, dev), nans((48,), f64, dev), nans((48,), f64, dev)
        names = ran(lambda: lib().check(L.rdm_conv3x3_bf16_stats(P(y), Cc + 8, Cc, P(sc), P(sh), P(wp), C.c_void_p(out.data_ptr() + 32), 96, B, H, W, P(s), P(q), P(ws),
                                                                 sb + extra, lib().stream())))
        bm, _, split = R.conv3_plan(B, H, W, Cc, extra // 4)
        assert names == {"conv3x3_bf16_kernel/%d/stats%s" % (bm, "/splitK" if split > 1 else "")}
        same(out, 16, 64, exact)
        check_stats(s, q, stored)


@pytest.mark.parametrize("name", sorted(R.ACT_CASES))
def test_conv3x3_act_exact(dev, op_census, name):
    """rdm_conv3x3_act_bf16 behind rdm_conv3x3_act_bf16_pack: nc = 1..4, direct and K-split (the planner splits from 5 slabs on: 136 real channels
    padded to 160), 64-column rectangles for W > 250; real channel counts 8 / 40 / 72 padded to 32 / 64 / 96 with 2^60 in the pad channels of the
    activation (their weights are zero).  After a split launch the tile counters at the front of the workspace are zero."""
    L, P = lib().lib(), lib().ptr
    B, H, W, Cc, use_ws, census = R.ACT_CASES[name]
    c = R.build_act(name, B, H, W, Cc)
    M, Cp = B * H * W, c["Cp"]
    y, w = D(c["y"], bf16, dev), D(c["w"], f32, dev)
    img = torch.empty(int(L.rdm_conv3x3_act_bf16_weight_bytes(Cc)), dtype=torch.uint8, device=dev)
    lib().check(L.rdm_conv3x3_act_bf16_pack(P(w), Cc, P(img), lib().stream()))
    wsb = int(L.rdm_conv3x3_act_bf16_workspace_bytes(Cp, B, H, W)) if use_ws else 0
    ws = torch.full((max(wsb, 256),), 0xEE, dtype=torch.uint8, device=dev)
    out = nans((M, 96), bf16, dev)
    names = ran(lambda: lib().check(L.rdm_conv3x3_act_bf16(P(y), Cp + 8, Cp, P(img), C.c_void_p(out.data_ptr() + 32), 96, B, H, W, P(ws) if wsb else None, wsb, lib().stream())))
    assert names == {"conv3x3_act_bf16_kernel/" + census} == {R.act_census(Cp, B, H, W, wsb)}
    same(out, 16, 64, c["exact"])
    if wsb:
        assert int(ws[:16384].view(torch.int32).abs().sum().item()) == 0


@pytest.mark.parametrize("M,Cc", R.COLSTATS_CASES)
def test_colstats_exact(dev, M, Cc):
    L, P = lib().lib(), lib().ptr
    xh = R.ints("cs%d.%d" % (M, Cc), (M, Cc + 8), -255, 255)
    x, s, q = D(xh, bf16, dev), nans((Cc + 2,), f64, dev), nans((Cc + 2,), f64, dev)
    lib().check(L.rdm_colstats_bf16(P(x), Cc + 8, M, Cc, P(s), P(q), lib().stream()))
    rs, rq = R.colstats(xh, Cc)
    assert np.array_equal(s[:Cc].cpu().numpy(), rs) and np.array_equal(q[:Cc].cpu().numpy(), rq) and torch.isnan(s[Cc:]).all() and torch.isnan(q[Cc:]).all()


# ---- the helper kernels: real-valued inputs ---------------------------------------------------------------------------------------------------
def with_ties(key, shape, lo, hi):
    """f32-representable reals: a quarter exact bf16 ties (bf16 value + half an ulp), a quarter each just below / above a tie, the rest uniform"""
    u = R.filler.uniform(key, shape, lo, hi, np.float32).astype(np.float64)
    b = R.round_bf16(u)[0]
    half = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(b), 2.0 ** -100))) - 8)
    kind = R.ints(key + ".k", shape, 0, 7)
    t = b + half * np.select([kind == 0, kind == 1, kind == 2], [1.0, 1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10], 0.0)
    v = np.where(kind <= 2, t, u)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v) and R.round_bf16(v)[1].mean() > 0.1
    return v


@pytest.mark.parametrize("H,W", [(7, 7), (8, 9), (15, 14)])
def test_stem_patches_exact(dev, H, W):
    L, P = lib().lib(), lib().ptr
    B = 2
    xh = with_ties("sp%d" % H, (B, 3, H, W), -3.0, 3.0)
    want = R.stem_patches(xh)
    x, out = D(xh, f32, dev), nans((want.shape[0] + 1, 160), bf16, dev)
    lib().check(L.rdm_stem_patches_bf16(P(x), P(out), B, H, W, lib().stream()))
    assert np.array_equal(R.canon_bits(out[:-1]), R.bf16_bits(want)) and torch.isnan(out[-1].float()).all()


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (5, 4), (7, 8)])
@pytest.mark.parametrize("Cc", [8, 24])
def test_maxpool_bf16_exact(dev, H, W, Cc):
    """signed input with a -inf and equal maxima, and an all-negative input: a border tap that contributed 0 would win every border window"""
    L, P = lib().lib(), lib().ptr
    B = 2
    base = R.round_bf16(R.filler.uniform("mp%d.%d" % (H, Cc), (B, H, W, Cc), -3.0, 3.0, np.float64))[0]
    base[0, 0, 0, 0] = -np.inf
    base[1, H - 1, W - 1, :] = base.max()
    base[1, 0, 0, :] = base.max()
    for xh in (base, -1.0 - np.abs(base)):
        want = R.maxpool3s2(xh)
        x, out = D(xh, bf16, dev), nans((want.shape[0], Cc + 8), bf16, dev)
        lib().check(L.rdm_maxpool3s2_bf16(P(x), P(out), Cc + 8, B, H, W, Cc, lib().stream()))
        same(out, 0, Cc, want)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 6), (5, 1), (4, 6), (5, 7), (6, 5)])
def test_padavgpool_bf16_exact(dev, H, W):
    """multiples of 1/16, power-of-two scales and POSITIVE quarter-integer shifts: exact before the one rounding; a pad pixel contributing 0 instead
    of relu(shift) changes every output of an odd border"""
    L, P = lib().lib(), lib().ptr
    B, Cc, ldx = 2, 24, 40
    xh = np.full((B, H, W, ldx), R.BIG)
    xh[..., :Cc] = R.ints("tp%d.%d" % (H, W), (B, H, W, Cc), -64, 64) / 16.0
    sch, shh = R.choice("tp.s", (Cc,), (0.5, 1.0, 2.0)), R.ints("tp.t", (Cc,), 1, 11) / 4.0
    want = R.padavgpool2(xh, Cc, sch, shh)
    if H % 2 or W % 2:
        assert (R.bf16_bits(want) != R.bf16_bits(R.padavgpool2(xh, Cc, sch, shh, pad_is_input=False))).any()
    x, sc, sh, out = D(xh, bf16, dev), D(sch, f32, dev), D(shh, f32, dev), nans((want.shape[0] + 1, Cc), bf16, dev)
    lib().check(L.rdm_padavgpool2_bf16(P(x), ldx, P(sc), P(sh), P(out), B, H, W, Cc, lib().stream()))
    assert np.array_equal(R.canon_bits(out[:-1]), R.bf16_bits(want)) and torch.isnan(out[-1].float()).all()


def test_f32_to_bf16_rows_exact(dev):
    """147 -> 160 columns, source stride 152, destination stride 168; ties, +-0, denormals, +-inf and values that round to inf"""
    L, P = lib().lib(), lib().ptr
    rows, cols, pad, lds, ldd = 37, 147, 160, 152, 168
    src = with_ties("rows", (rows, lds), -100.0, 100.0)
    big = float(torch.finfo(bf16).max)
    src[0, :10] = [0.0, -0.0, np.inf, -np.inf, big, big * (1 + 2.0 ** -8), -big * (1 + 2.0 ** -8), 2.0 ** -130, -2.0 ** -140, 2.0 ** -149]
    src[:, cols:] = np.nan                                     # the source's stride padding must not be read into dst
    want = R.rows_to_bf16(src, cols, pad)
    x, out = D(np.nan_to_num(src, nan=7.0, posinf=np.inf, neginf=-np.inf), f32, dev), nans((rows, ldd), bf16, dev)
    lib().check(L.rdm_f32_to_bf16_rows(P(x), lds, P(out), ldd, rows, cols, pad, lib().stream()))
    same(out, 0, pad, want)


@pytest.mark.parametrize("T", [9, 1])
def test_pack_conv_weight_bf16_exact(dev, T):
    L, P = lib().lib(), lib().ptr
    O, I, ld = 48, 40, 56
    wh = with_ties("pw%d" % T, (O, I, T), -1.0, 1.0)
    w, out = D(wh, f32, dev), nans((T * O, ld), bf16, dev)
    lib().check(L.rdm_pack_conv_weight_bf16(P(w), P(out), O, I, ld, T, lib().stream()))
    same(out, 0, I, R.pack_weight(wh).reshape(T * O, I))


# ---- argument errors: an error code, nothing launched -------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    L, P = lib().lib(), lib().ptr
    st = lib().stream()
    x, w, out = torch.zeros(64, 64, dtype=bf16, device=dev), torch.zeros(64, 64, dtype=bf16, device=dev), nans((64, 64), bf16, dev)
    v, xf = torch.ones(64, device=dev), torch.zeros(3 * 64 * 64, device=dev)
    s, q, ws = nans((64,), f64, dev), nans((64,), f64, dev), torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    o1 = lambda t: C.c_void_p(t.data_ptr() + 2)                # misaligned by one bf16
    sb = int(L.rdm_bf16_stats_workspace_bytes(32, 16))
    img = torch.zeros(int(L.rdm_conv3x3_act_bf16_weight_bytes(32)), dtype=torch.uint8, device=dev)
    calls = {
        "gemm misaligned": lambda: L.rdm_gemm_bf16(o1(x), 64, 16, None, None, P(w), 64, None, P(out), 64, 32, 16, 0, None, 0, st),
        "gemm K % 8": lambda: L.rdm_gemm_bf16(P(x), 64, 12, None, None, P(w), 64, None, P(out), 64, 32, 16, 0, None, 0, st),
        "gemm N % 4": lambda: L.rdm_gemm_bf16(P(x), 64, 16, None, None, P(w), 64, None, P(out), 64, 32, 6, 0, None, 0, st),
        "gemm_act misaligned": lambda: L.rdm_gemm_bf16_act(P(x), 64, 16, None, None, o1(w), 64, P(v), P(v), P(out), 64, 32, 16, None, 0, st),
        "gemm_act K % 8": lambda: L.rdm_gemm_bf16_act(P(x), 64, 12, None, None, P(w), 64, P(v), P(v), P(out), 64, 32, 16, None, 0, st),
        "gemm_act N % 4": lambda: L.rdm_gemm_bf16_act(P(x), 64, 16, None, None, P(w), 64, P(v), P(v), P(out), 64, 32, 6, None, 0, st),
        "gemm_stats misaligned": lambda: L.rdm_gemm_bf16_stats(o1(x), 64, 16, None, None, P(w), 64, P(out), 64, 32, 16, P(s), P(q), P(ws), sb, st),
        "gemm_stats K % 8": lambda: L.rdm_gemm_bf16_stats(P(x), 64, 12, None, None, P(w), 64, P(out), 64, 32, 16, P(s), P(q), P(ws), sb, st),
        "gemm_stats N % 4": lambda: L.rdm_gemm_bf16_stats(P(x), 64, 16, None, None, P(w), 64, P(out), 64, 32, 6, P(s), P(q), P(ws), sb, st),
        "gemm_stats scratch": lambda: L.rdm_gemm_bf16_stats(P(x), 64, 16, None, None, P(w), 64, P(out), 64, 32, 16, P(s), P(q), P(ws), sb - 256, st),
        "conv misaligned": lambda: L.rdm_conv3x3_bf16(o1(x), 16, 16, None, None, P(w), P(out), 64, 1, 4, 4, None, 0, st),
        "conv C % 8": lambda: L.rdm_conv3x3_bf16(P(x), 16, 12, None, None, P(w), P(out), 64, 1, 4, 4, None, 0, st),
        "conv_stats misaligned": lambda: L.rdm_conv3x3_bf16_stats(o1(x), 16, 16, None, None, P(w), P(out), 64, 1, 4, 4, P(s), P(q), P(ws), 1 << 20, st),
        "conv_stats C % 8": lambda: L.rdm_conv3x3_bf16_stats(P(x), 16, 12, None, None, P(w), P(out), 64, 1, 4, 4, P(s), P(q), P(ws), 1 << 20, st),
        "conv_stats scratch": lambda: L.rdm_conv3x3_bf16_stats(P(x), 16, 16, None, None, P(w), P(out), 64, 1, 4, 4, P(s), P(q), P(ws),
                                                               int(L.rdm_bf16_stats_workspace_bytes(16, 48)) - 256, st),
        "act misaligned": lambda: L.rdm_conv3x3_act_bf16(o1(x), 40, 32, P(img), P(out), 64, 1, 4, 4, None, 0, st),
        "act C % 32": lambda: L.rdm_conv3x3_act_bf16(P(x), 40, 24, P(img), P(out), 64, 1, 4, 4, None, 0, st),
        "act_pack misaligned": lambda: L.rdm_conv3x3_act_bf16_pack(P(xf), 32, o1(out), st),
        "colstats misaligned": lambda: L.rdm_colstats_bf16(o1(x), 64, 32, 16, P(s), P(q), st),
        "colstats C % 8": lambda: L.rdm_colstats_bf16(P(x), 64, 32, 12, P(s), P(q), st),
        "stem misaligned": lambda: L.rdm_stem_patches_bf16(P(xf), o1(out), 1, 8, 8, st),
        "stem NULL": lambda: L.rdm_stem_patches_bf16(None, P(out), 1, 8, 8, st),
        "maxpool misaligned": lambda: L.rdm_maxpool3s2_bf16(o1(x), P(out), 16, 1, 4, 4, 16, st),
        "maxpool C % 8": lambda: L.rdm_maxpool3s2_bf16(P(x), P(out), 16, 1, 4, 4, 12, st),
        "maxpool ld < C": lambda: L.rdm_maxpool3s2_bf16(P(x), P(out), 8, 1, 4, 4, 16, st),
        "maxpool ld % 8": lambda: L.rdm_maxpool3s2_bf16(P(x), P(out), 20, 1, 4, 4, 16, st),
        "padavgpool misaligned": lambda: L.rdm_padavgpool2_bf16(P(x), 16, P(v), P(v), o1(out), 1, 4, 4, 16, st),
        "padavgpool C % 8": lambda: L.rdm_padavgpool2_bf16(P(x), 16, P(v), P(v), P(out), 1, 4, 4, 12, st),
        "padavgpool ld < C": lambda: L.rdm_padavgpool2_bf16(P(x), 8, P(v), P(v), P(out), 1, 4, 4, 16, st),
        "padavgpool NULL scale": lambda: L.rdm_padavgpool2_bf16(P(x), 16, None, P(v), P(out), 1, 4, 4, 16, st),
        "rows misaligned": lambda: L.rdm_f32_to_bf16_rows(P(xf), 16, o1(out), 16, 4, 12, 16, st),
        "rows ld < cols_pad": lambda: L.rdm_f32_to_bf16_rows(P(xf), 16, P(out), 8, 4, 12, 16, st),
        "rows ld % 8": lambda: L.rdm_f32_to_bf16_rows(P(xf), 16, P(out), 20, 4, 12, 16, st),
        "pack misaligned": lambda: L.rdm_pack_conv_weight_bf16(P(xf), o1(out), 4, 12, 16, 9, st),
        "pack ld < I": lambda: L.rdm_pack_conv_weight_bf16(P(xf), P(out), 4, 12, 8, 9, st),
        "pack ld % 8": lambda: L.rdm_pack_conv_weight_bf16(P(xf), P(out), 4, 12, 20, 9, st),
    }
    before = int(L.rdm_launch_count())
    for what, call in calls.items():
        assert call() != 0, what
    torch.cuda.synchronize()
    assert int(L.rdm_launch_count()) == before
    assert torch.isnan(out.float()).all() and torch.isnan(s).all() and torch.isnan(q).all()


# ---- real-valued leg: uniform inputs, derived bound ------------------------------------------------------------------------------------------
FRACTIONS = {}


def within(op):
    """f32: |got - want| <= e + 2^-24 |want|; bf16: <= e + half a bf16 ulp at (|want| + e); e = (K_total + 2) 2^-24 sum |a||w| per output"""
    def check(out, n0, n1, ref):
        want, mag, kt = ref
        assert torch.isnan(out[:, :n0].float()).all() and torch.isnan(out[:, n1:].float()).all()
        got = out[:, n0:n1].cpu().double().numpy()
        e = (kt + 2) * 2.0 ** -24 * mag
        if out.dtype == f32:
            bound = e + 2.0 ** -24 * np.abs(want)
        else:
            bound = e + 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want) + e, 2.0 ** -120))) - 8)
        frac = float((np.abs(got - want) / bound).max())
        FRACTIONS[op] = max(FRACTIONS.get(op, 0.0), frac)
        print("real-valued leg %s: largest error / bound = %.3f" % (op, frac))
        assert frac <= 1.0
    return check


def real(key, shape, lo, hi, to_bf16=True):
    v = R.filler.uniform(key, shape, lo, hi, np.float32).astype(np.float64)
    return R.round_bf16(v)[0] if to_bf16 else v


@pytest.mark.parametrize("name", ["t64x96", "split", "panel"])
def test_gemm_real_valued(dev, op_census, name):
    """uniform real operands (as tests/test_gpu_bf16.py) against float64 on the same bf16-rounded operands at the derived bound; f32 and bf16 output"""
    M, K, N, px, pw = {"t64x96": R.GEMM_CASES["t64x96"][:5], "split": R.SPLIT_CASE, "panel": R.PANEL_MN[:1] + (120, R.PANEL_MN[1], 8, 0)}[name]
    c = dict(x=real(name + ".rx", (M, K + px), -2, 2), w=real(name + ".rw", (N, K + pw), -0.1, 0.1), sc=real(name + ".rs", (K,), 0.5, 1.5, False),
             sh=real(name + ".rt", (K,), -0.3, 0.3, False), bias=None, osc=None, osh=None)
    want, mag = R.gemm(c["x"], c["w"], K, c["sc"], c["sh"])
    for out_f32 in (False,) if name != "t64x96" else (False, True):
        call_gemm(dev, c, M, K, N, px, pw, (True, False, out_f32, False), 8 * M * N if name == "split" else 0, exact=(want, mag, K), check=within("gemm"))


@pytest.mark.parametrize("name", ["c104", "bm128", "nc2s"])
def test_conv_real_valued(dev, op_census, name):
    L, P = lib().lib(), lib().ptr
    act = name in R.ACT_CASES
    B, H, W, Cc = (R.ACT_CASES if act else R.CONV_CASES)[name][:4]
    M, Cp = B * H * W, (Cc + 31) // 32 * 32 if act else Cc
    yh = real(name + ".ry", (B, H, W, Cp + 8), 0 if act else -2, 2)
    y, out = D(yh, bf16, dev), nans((M, 96), bf16, dev)
    if act:
        wh = real(name + ".rw", (48, Cc, 3, 3), -0.05, 0.05, False)
        img = torch.empty(int(L.rdm_conv3x3_act_bf16_weight_bytes(Cc)), dtype=torch.uint8, device=dev)
        w = D(wh, f32, dev)
        lib().check(L.rdm_conv3x3_act_bf16_pack(P(w), Cc, P(img), lib().stream()))
        wsb = int(L.rdm_conv3x3_act_bf16_workspace_bytes(Cp, B, H, W))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        lib().check(L.rdm_conv3x3_act_bf16(P(y), Cp + 8, Cp, P(img), C.c_void_p(out.data_ptr() + 32), 96, B, H, W, P(ws), wsb, lib().stream()))
        want, mag = R.conv3x3_act(yh, wh, Cc)
    else:
        w9, sch, shh = real(name + ".rw", (9, 48, Cc), -0.05, 0.05), real(name + ".rs", (Cc,), 0.5, 1.5, False), real(name + ".rt", (Cc,), -0.3, 0.3, False)
        wsb = int(L.rdm_conv3x3_bf16_workspace_bytes(Cc, B, H, W))
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
        wp, sc, sh = D(w9, bf16, dev), D(sch, f32, dev), D(shh, f32, dev)
        lib().check(L.rdm_conv3x3_bf16(P(y), Cc + 8, Cc, P(sc), P(sh), P(wp), C.c_void_p(out.data_ptr() + 32), 96, B, H, W, P(ws) if wsb else None, wsb, lib().stream()))
        want, mag = R.conv3x3(yh, w9, Cc, sch, shh)
    torch.cuda.synchronize()
    within("conv3x3_act" if act else "conv3x3")(out, 16, 64, (want, mag, 9 * Cc))
