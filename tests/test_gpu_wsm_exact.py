"""-m gpu: the WSM decoder bf16 kernels (csrc/wsm_bf16.hip: wsm_conv_bf16_kernel<MT,NT>, k_wsm_pack_bf16, k_nchw_f32_to_nhwc_bf16) BIT FOR BIT
against float64 on inputs whose f32 arithmetic is exact, at the operator entries and through the whole chain of a planted Decoder.

Every tolerance in this file is DERIVED; nothing in it is measured.
  * Planted legs (tests/wsm_ref.py): activations and weights are integers in [-4, 4], biases multiples of 1/4 with |b| <= 8 and
    sum |x||w| + |b| < 2^22 per output, so every product, every f32 partial sum in any order and the bias add are exact
    (tests/test_wsm_ref_cpu.py asserts this on every case below).  The tolerance is ZERO: an f32 output must EQUAL the float64 reference, a bf16
    output its round-to-nearest-even rounding on bits (-0.0 and +0.0 compare equal).  A dropped, duplicated or misplaced term - at a border, in a
    K tail, in a pipeline stage, in a low-magnitude channel - is a nonzero difference; the assert message names the first differing (pixel, channel).
  * Chain legs: a Decoder planted so that every tensor the chain stores is a bf16 integer and conv1's sums stay below 2^24
    (tests/test_wsm_ref_cpu.py, condition (e)); the f32 map of features_bf16 / features_bf16_train must EQUAL the float64 restatement
    (tests/test_rel_restatement_cpu.py::wsm_layer).  The CPU module shows that each packing / routing error of rdm_rel_bf16_prepare and
    rel_wsm_chain it lists changes that map.
  * Real-valued leg: uniform real operands rounded to bf16; |got - want| <= (K + 2) 2^-24 sum |x||w| per output (K f32 accumulations of exact
    products plus the bias add, each within 2^-24 relative of a partial sum that sum |x||w| + |b| bounds), plus half a bf16 ulp for bf16 outputs.

Poison: every output buffer is NaN-filled, wider than its slot and one pixel longer than the map (everything outside the slot must still be NaN);
the columns of X outside [xoff, xoff + pad32(cin)) hold 2^100, its pad channels 2^60; weight rows from n on hold 2^100; NaN sits directly behind the
last element of X, so a read past x_bytes (ldx no multiple of 32: the last pixel's pad channels) would reach a sum.  The tile each case runs on is
named in wsm_ref.TILES by the launcher's rule restated (launch_wsm_conv_bf16 records no census entry); the CPU module recomputes it."""
import numpy as np
import pytest
import torch

import wsm_ref as R

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def lib():
    from md_rdm_amd import _lib
    return _lib


def D(a, dtype, dev):
    """float64 numpy -> device tensor of `dtype` (None stays None)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(dev)


def nans(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def same(out, n0, n1, exact):
    """rows [0, len(exact)) x columns [n0, n1) of `out` hold `exact` (f32: equal; bf16: equal to its rounding, on bits); everything else is still NaN"""
    M = exact.shape[0]
    assert torch.isnan(out[:M, :n0].float()).all() and torch.isnan(out[:M, n1:].float()).all(), "columns outside the slot were written"
    assert torch.isnan(out[M:].float()).all(), "pixels behind the map were written"
    got = out[:M, n0:n1]
    bad = (got.cpu().double().numpy() != exact) if out.dtype == f32 else (R.canon_bits(got) != R.bf16_bits(exact))
    if bad.any():
        m, c = np.argwhere(bad)[0]
        raise AssertionError("%d of %d differ, first at (pixel %d, channel %d): got %r, exact %r" % (bad.sum(), bad.size, m, c, float(got[m, c]), float(exact[m, c])))


FRACTIONS = {}


def within(op, K):
    """|got - want| <= e (+ half a bf16 ulp at |want| + e for bf16 outputs), e = (K + 2) 2^-24 (sum |x||w| + |b|) per output"""
    def check(out, n0, n1, ref):
        want, mag = ref
        M = want.shape[0]
        assert torch.isnan(out[:M, :n0].float()).all() and torch.isnan(out[:M, n1:].float()).all() and torch.isnan(out[M:].float()).all()
        got = out[:M, n0:n1].cpu().double().numpy()
        bound = (K + 2) * 2.0 ** -24 * mag
        if out.dtype != f32:
            bound = bound + 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want) + bound, 2.0 ** -120))) - 8)
        frac = float((np.abs(got - want) / bound).max())
        FRACTIONS[op] = frac
        print("real-valued leg %s: largest error / bound = %.3f" % (op, frac))
        assert frac <= 1.0, (op, frac)
    return check


# ---- rdm_wsm_conv_bf16 -----------------------------------------------------------------------------------------------------------------------
def run_conv(dev, name, real=False):
    L, P = lib().lib(), lib().ptr
    c = R.build_conv(name, real)
    B, H, W = c["geom"]
    x, wp, b = D(c["x"], bf16, dev), D(c["wp"], bf16, dev), D(c["b"], f32, dev)
    for coff, ldc in R.STORES[name]:
        out = nans((c["M"] + 1, ldc), bf16, dev)
        lib().check(L.rdm_wsm_conv_bf16(P(x), c["ldx"], c["xoff"], c["cin"], P(wp), P(b), c["n"], P(out), ldc, coff, B, H, W, c["k"], lib().stream()))
        if real:
            within("conv", c["K"])(out, coff, coff + c["n"], (c["exact"], c["mag"]))
        else:
            try:
                same(out, coff, coff + c["n"], c["exact"])
            except AssertionError as e:
                raise AssertionError("%s (coff %d, ldc %d, tile %s): %s" % (name, coff, ldc, R.TILES[name], e)) from None


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_conv_exact(dev, name):
    """k = 1: nk = 1..5 with K % 64 in {32, 0}, ldx = 40 / 208 with the pad channels in the next pixel (behind the buffer for the last one), n = 1..130
    through aligned, odd and real-slot (coff, ldc), M = 1..105 with and without bias, xoff = 0 / 8 / 40; k = 3 / 5: every tap its own weights, maps
    smaller than the kernel, cin = 40 at K = 1600; the <4,2> tile at k = 1 and k = 3 and the <2,2> tile just below its threshold"""
    run_conv(dev, name)


# ---- rdm_wsm_deconv_bf16 -----------------------------------------------------------------------------------------------------------------------
def run_deconv(dev, cin, c, B, h, w, real=False):
    L, P = lib().lib(), lib().ptr
    d = R.build_deconv(cin, c, B, h, w, real)
    x, wp, b = D(d["x"], bf16, dev), D(d["wp"], bf16, dev), D(d["b"], f32, dev)
    out = nans((4 * d["M"] + 1, d["ldc"]), bf16, dev)
    lib().check(L.rdm_wsm_deconv_bf16(P(x), d["ldx"], cin, P(wp), P(b), c, P(out), d["ldc"], B, h, w, lib().stream()))
    if real:
        return within("deconv", d["K"])(out, 0, c, (d["exact"], d["mag"]))
    try:
        same(out, 0, c, d["exact"])
    except AssertionError as e:
        raise AssertionError("deconv cin %d c %d B %d h %d w %d (output pixels are (b, 2h, 2w) row-major): %s" % (cin, c, B, h, w, e)) from None


@pytest.mark.parametrize("cc", R.DECONV_CC, ids=lambda cc: "cin%d_c%d" % cc)
def test_deconv_exact(dev, cc):
    """c % 4 != 0 and c % 32 != 0, h != w both ways (the pixel shuffle indexes with H and W), a 1x1 map, B = 1 and 2, ldc = c + 8; the pad rows of
    every phase hold 2^100 and must not be stored"""
    for B, h, w in R.DECONV_GEOMS:
        run_deconv(dev, cc[0], cc[1], B, h, w)


def test_deconv_exact_tile42(dev):
    run_deconv(dev, *R.DECONV_TILE_CASE)


# ---- rdm_wsm_strip_bf16 ------------------------------------------------------------------------------------------------------------------------
def run_strip(dev, name, columns, real=False):
    L, P = lib().lib(), lib().ptr
    c = R.build_strip(name, columns, real)
    x, wp, b = D(c["x"], bf16, dev), D(c["wp"], bf16, dev), D(c["b"], f32, dev)
    out = nans((c["B"] * c["S"] * c["S"] + 1, c["ldc"]), bf16, dev)
    lib().check(L.rdm_wsm_strip_bf16(P(x), c["ldx"], c["xoff"], c["cw"], P(wp), P(b), c["n"], P(out), c["ldc"], c["coff"], c["B"], c["S"], columns, lib().stream()))
    if real:
        return within("strip", c["K"])(out, c["coff"], c["coff"] + c["n"], (c["exact"], strip_mag(c, columns)))
    try:
        same(out, c["coff"], c["coff"] + c["n"], c["exact"])
    except AssertionError as e:
        raise AssertionError("strip %s columns %d: %s" % (name, columns, e)) from None


def strip_mag(c, columns):
    return R.strip_broadcast(c["mag"], columns)


@pytest.mark.parametrize("columns", [0, 1])
@pytest.mark.parametrize("name", sorted(R.STRIP_CASES))
def test_strip_exact(dev, name, columns):
    """S = 1, 2, 4, 8 over rows and over columns, cw = 32 / 64, n = 5 / 26 / 32, xoff = 0 / 32 inside a wider ldx, coff = 0 / 6: every one of the S
    broadcast positions holds the row's (column's) value and nothing else is written; with B = 3 the taps at t = 0 and t = S - 1 see zeros, not the
    neighbouring image"""
    run_strip(dev, name, columns)


# ---- rdm_wsm_conv1x1_f32 -----------------------------------------------------------------------------------------------------------------------
def run_conv1x1(dev, cin, M, real=False):
    L, P = lib().lib(), lib().ptr
    c = R.build_conv1x1_f32(cin, M, real)
    x, wp, b = D(c["x"], bf16, dev), D(c["wp"], bf16, dev), D(c["b"], f32, dev)
    out = nans((M + 4, 1), f32, dev)
    lib().check(L.rdm_wsm_conv1x1_f32(P(x), cin, cin, P(wp), P(b), P(out), 1, 1, M, lib().stream()))
    if real:
        return within("conv1x1_f32", c["K"])(out, 0, 1, (c["exact"], c["mag"]))
    same(out, 0, 1, c["exact"])


@pytest.mark.parametrize("cin,M", R.CONV1X1_CASES)
def test_conv1x1_f32_exact(dev, cin, M):
    """ldx = cin = 32 / 40 / 208: the f32 output EQUALS the float64 reference; the three f32 columns of the 4-wide segment that are not stored stay NaN"""
    run_conv1x1(dev, cin, M)


# ---- rdm_rel_bf16_input_nchw -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ld", R.NCHW_CASES)
def test_input_nchw_exact(dev, B, ld):
    """real-valued input with planted ties in both directions: RNE on bits, the guard columns from 1056 on and the row behind the map still NaN"""
    L, P = lib().lib(), lib().ptr
    xh = R.with_ties("nchw%d" % B, (B, 1056, 8, 8), -3.0, 3.0)
    counts = R.rounding_counts(xh)
    assert min(counts.values()) > 100, counts
    want = R.nchw_to_nhwc(xh, ld)
    x, enc = D(xh, f32, dev), nans((B * 64 + 1, ld), bf16, dev)
    lib().check(L.rdm_rel_bf16_input_nchw(P(x), B, P(enc), ld, lib().stream()))
    same(enc, 0, 1056, want[:, :1056])


# ---- real-valued leg ---------------------------------------------------------------------------------------------------------------------------
def test_real_valued(dev):
    """one case per entry on uniform real operands against the derived bound (module docstring), not a measured one"""
    run_conv(dev, "k3_b3", real=True)
    run_deconv(dev, 64, 40, 2, 3, 5, real=True)
    run_strip(dev, "S4_b", 0, real=True)
    run_strip(dev, "S4_b", 1, real=True)
    run_conv1x1(dev, 208, 65, real=True)


# ---- the chain through Decoder.features_bf16 / features_bf16_train -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(dev):
    made = {}

    def get(did):
        if did not in made:
            from md_rdm_amd.network import RDM_Net
            dec = RDM_Net.Decoder(in_channels=1056, num_wsm_layers=did - 6, DORN=False, id=did, quant=RDM_Net.Quantization())
            sd = R.planted_state(did)
            with torch.no_grad():
                for key, t in dec.state_dict().items():
                    if key in sd:
                        t.copy_(sd[key].float())
                        assert torch.equal(t.double(), sd[key])
            made[did] = dec.to(dev).eval()
        return made[did]
    return get


def equal_map(got, want, what):
    assert got.dtype == f32 and tuple(got.shape) == want.shape, what
    g = got.cpu().double().numpy()
    bad = g != want
    if bad.any():
        b, _, y, x = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d map entries differ, first at (image %d, y %d, x %d): got %r, exact %r" % (what, bad.sum(), bad.size, b, y, x, g[b, 0, y, x], want[b, 0, y, x]))


@pytest.mark.parametrize("did", [7, 8])
def test_chain_exact(dev, planted, did):
    """d_7 (one WSM layer, S = 16) and d_8 (two, S = 32) through the public entry: rdm_rel_bf16_prepare's packing of the 22 tensors per layer, the
    two-segment epilogue of the fused conv1_1..conv1_5 GEMM and rel_wsm_chain's slot offsets, held to EQUALITY with the float64 restatement; B = 2
    and both B = 1 images, ld_enc = 1056 and 1064 (2^100 in the extra columns), twice the same bits; d_7 also in train() mode through
    features_bf16_train (the chain is shared code; the zero conv2 weights keep the block [enc | 0] whatever the batch statistics are)"""
    dec, enc, want = planted(did), R.planted_enc(did), R.expected_map(did)
    runs = {}
    for B, rows, ld in ((2, slice(0, 128), 1056), (2, slice(0, 128), 1064), (1, slice(0, 64), 1056), (1, slice(64, 128), 1064)):
        e = D(R.enc_buffer(enc[rows], ld), bf16, dev)
        got = dec.features_bf16(e, ld, B)
        equal_map(got, want[rows.start // 64:rows.stop // 64], "d_%d B %d ld %d" % (did, B, ld))
        assert torch.equal(dec.features_bf16(e, ld, B), got)
        runs[(B, rows.start)] = got
    assert torch.equal(torch.cat((runs[(1, 0)], runs[(1, 64)])), runs[(2, 0)])
    if did == 7:
        dec.train()
        try:
            for B, rows in ((2, slice(0, 128)), (1, slice(64, 128))):
                e = D(R.enc_buffer(enc[rows], 1064), bf16, dev)
                got = dec.features_bf16_train(e, 1064, B)
                equal_map(got, want[rows.start // 64:rows.stop // 64], "d_7 train() B %d" % B)
                assert torch.equal(got, runs[(B, rows.start)]) and torch.equal(dec.features_bf16_train(e, 1064, B), got)
        finally:
            dec.eval()
        e = D(R.enc_buffer(enc, 1056), bf16, dev)                                        # the running statistics moved: the eval map does not
        assert torch.equal(dec.features_bf16(e, 1056, 2), runs[(2, 0)])
