"""-m gpu: the split-precision kernels of csrc/xsplit.hip BIT FOR BIT against float64 on inputs whose f32 arithmetic is exact.

Planted inputs and references: tests/xsplit_ref.py (operands H + m 2^-9 (+ t 2^-18), power-of-two scales, quarter-integer shifts, gate operands of
signed powers of two with exact ties).  The reference is the float64 sum of the RETAINED plane products (a0 b0 + a0 b1 + a1 b0; six products for
the x6 forward; a0 b0 in the one-product mode), every one of which is a multiple of one quantum q with sum |product| < 2^24 q per output
(tests/test_xsplit_ref_cpu.py asserts it for every case), so tile shape, slab order, split_k, atomics and operand form cannot change a bit: f32
outputs must EQUAL the reference, f64 statistics their float64 sums.  Tolerance zero - derived, not measured.  -0.0 == +0.0.

Every output is NaN-filled with a row stride wider than its slot where the ABI has a stride (the weight gradients have none: they get NaN guard
rows in front and behind), statistics are zeroed between NaN guards, input rows carry NaN behind their contracted prefix, and every launch is held
to the census entry of the variant the case was shaped for.  Split rows / frame images are produced by rdm_split_rows_f32 /
rdm_frame_split_rows_f32 and their bits checked against the restatement first.

A last leg runs real-valued inputs against  |got - retained-terms reference| <= (K_terms + 2) 2^-24 sum |product|  per ELEMENT: the products of
bf16 planes are exact in f32, every one of the K_terms additions rounds once by at most 2^-24 of a partial sum that never exceeds sum |product|
(first order in 2^-24), + 2 for the epilogue.  It measures accumulation rounding only: the dropped lo x lo terms are not in the reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import xsplit_ref as X

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def lib():
    from md_rdm_amd import _lib
    return _lib


def D(a, dev, dtype=f32):
    """float64 numpy (NaN allowed) -> device tensor; the finite values are exact in f32"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    assert dtype != f32 or X.is_f32(np.nan_to_num(a, nan=0.0))
    return torch.from_numpy(a).to(dtype).to(dev)


def nans(shape, dev, dtype=f32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def guarded(n, dev, dtype, lead):
    """n zeros between `lead` NaN elements in front and behind -> (buffer, pointer to the zeros, view of the zeros)"""
    buf = nans((n + 2 * lead,), dev, dtype)
    buf[lead:lead + n] = 0
    return buf, C.c_void_p(buf.data_ptr() + lead * buf.element_size()), buf[lead:lead + n]


def guards_intact(buf, n, lead):
    return bool(torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + n:]).all())


def ran(call):
    """census entries of the split-precision kernels added by `call`"""
    L = lib()
    before = L.census()
    call()
    torch.cuda.synchronize()
    return {k for k, v in L.census().items() if v > before.get(k, 0) and k.startswith("xs_")}


def same(out, n, exact):
    """columns [0, n) of `out` equal `exact`, everything behind is still NaN"""
    assert torch.isnan(out[:, n:]).all(), "columns outside the slot were written"
    bad = out[:, :n].cpu().double().numpy() != exact
    assert not bad.any(), "%d of %d differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])


def equal(t, exact):
    bad = t.cpu().double().numpy().reshape(exact.shape) != exact
    assert not bad.any(), "%d of %d differ, first at %s" % (bad.sum(), bad.size, np.argwhere(bad)[0])


def split_rows(dev, src, ld, sc, sh, rows, ch, want64):
    """rdm_split_rows_f32 into a NaN-filled buffer of the same stride; bits == the restatement on want64 (rows, ch), nothing behind ch touched"""
    L, P = lib().lib(), lib().ptr
    dst = nans((rows, ld), dev)
    lib().check(L.rdm_split_rows_f32(P(src), ld, P(sc) if sc is not None else None, P(sh) if sh is not None else None, P(dst), ld, rows, ch, lib().stream()))
    got = dst[:, :ch].contiguous().cpu().view(torch.int16).view(rows, ch // 4, 8)
    assert torch.equal(got, X.split_rows_bits(X.T(want64).to(f32))) and torch.isnan(dst[:, ch:]).all()
    return dst


# ---- 1x1 weight gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.WGRAD1_CASES))
def test_wgrad1x1_exact(dev, op_census, name):
    """xs_wgrad1x1_kernel: column tiles 96 / 144 / 192 / 144 + 96 / 192 + 144, one and two (ragged) row tiles, ragged last slab, with / without
    prologue; float operands, dY as split rows, dY and the activated input as split rows; split_k 0 / 1 / 3 equal to the reference and so to each
    other; the one-product mode on float operands."""
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    c = X.build_wgrad1(name)
    M, Cc, N, ld, ldg, bn = c["M"], c["C"], c["N"], c["ld"], c["ldg"], c["sc"] is not None
    ref3, ref1 = X.reference(c, 3)[0], X.reference(c, 1)[0]
    xg, gg, sc, sh = D(c["x"], dev), D(c["g"], dev), D(c["sc"], dev), D(c["sh"], dev)
    g_rows = split_rows(dev, gg, ldg, None, None, M, N, c["A"])
    x_rows = split_rows(dev, xg, ld, sc, sh, M, Cc, c["Bop"])
    d = ConvDesc(c["B"], c["H"], c["W"], Cc, ld, N, ldg, 1, 1, 1, 1, 0, 0)
    auto, kslabs = X.wgrad1_auto_split(M, Cc, N), X.cdiv(M, 32)

    def launch(gop, xop, bnp, split, flags, x1=False):
        buf, p, view = guarded(N * Cc, dev, f32, Cc)
        names = ran(lambda: lib().check(L.rdm_conv2d_wgrad_x3(C.byref(d), P(gop), P(xop), P(sc) if bnp else None, P(sh) if bnp else None, p, split, flags | int(x1), lib().stream())))
        eff = min(split or auto, kslabs)
        sfx = {0: "", 0x10: "/rowsG", 0x30: "/rowsGX"}[flags]
        assert names == {"xs_wgrad1x1_kernel/x%d/bn%d/%s%s" % (1 if x1 else 3, bnp, "splitK" if eff > 1 else "split1", sfx)}, names
        assert guards_intact(buf, N * Cc, Cc)
        return view

    for flags, gop, xop, bnp in ((0, gg, xg, bn), (X.DY_ROWS, g_rows, xg, bn), (X.DY_ROWS | X.X_ROWS, g_rows, x_rows, False)):
        for split in (0, 1, 3):
            equal(launch(gop, xop, bnp, split, flags), ref3)
    for split in (0, 3):
        equal(launch(gg, xg, bn, split, 0, x1=True), ref1)


# ---- 1x1 input gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.DGRAD1_CASES))
def test_dgrad1x1_exact(dev, op_census, name):
    """xs_dgrad1x1_kernel, both instantiations (px128, px320): one / two even / two uneven column tiles, K of one k-step and with a ragged last one,
    M no multiple of 16; plain store, gate + statistics (exact ties gated off), the accumulating epilogue into an integer block gradient; each on
    float dY and on split rows; mask_ld > N, dx_ld > N; the one-product mode."""
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    c = X.build_dgrad1(name)
    M, K, N, ldg, ldx, ldo = c["M"], c["K"], c["N"], c["ldg"], c["ldx"], c["ldo"]
    ref3, ref1 = X.reference(c, 3)[0], X.reference(c, 1)[0]
    y, gate = np.nan_to_num(c["y"][:, :N], nan=0.0), c["gate"]
    gg, wg, yg, sc, sh = D(c["g"], dev), D(c["w"], dev), D(c["y"], dev), D(c["sc"], dev), D(c["sh"], dev)
    g_rows = split_rows(dev, gg, ldg, None, None, M, K, c["A"])
    d = ConvDesc(c["B"], c["H"], c["W"], N, N, K, ldg, 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_dgrad_x3_workspace_bytes(K, N))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    px = "px128" if M <= 8192 else "px320"

    def launch(gop, flags, mask, ref, init=None, x1=False):
        out = nans((M, ldo), dev)
        if init is not None:
            out[:, :N] = D(init, dev)
        sb0, p0, s0 = guarded(N, dev, f64, 2)
        sb1, p1, s1 = guarded(N, dev, f64, 2)
        m = (P(yg), ldx, P(sc), P(sh), p0, p1) if mask else (None, 0, None, None, None, None)
        names = ran(lambda: lib().check(L.rdm_conv1x1_dgrad_x3(C.byref(d), P(gop), P(wg), P(out), ldo, *m, P(ws), wsb, flags | int(x1), lib().stream())))
        assert names == {"xs_dgrad1x1_kernel/x%d/%s/%s%s" % (1 if x1 else 3, px, "MASK_STATS" if mask else "STORE", "/rowsG" if flags & X.DY_ROWS else "")}, names
        dz = ref * gate if mask else ref
        same(out, N, c["G0"] + c["sc"] * dz if init is not None else dz)
        assert guards_intact(sb0, N, 2) and guards_intact(sb1, N, 2)
        if mask:
            assert np.array_equal(s0.cpu().numpy(), dz.sum(0)) and np.array_equal(s1.cpu().numpy(), (dz * y).sum(0))

    for gop, flags in ((gg, 0), (g_rows, X.DY_ROWS)):
        launch(gop, flags, False, ref3)
        launch(gop, flags, True, ref3)
        launch(gop, flags | X.ACC_SCALED, True, ref3, init=c["G0"])
    launch(gg, 0, False, ref1, x1=True)
    launch(gg, 0, True, ref1, x1=True)


# ---- 3x3 input gradient -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.DGRAD3_CASES))
def test_dgrad3x3_exact(dev, op_census, name):
    """xs_dgrad3x3_kernel: Cb = 48 / 96 / 144, the gradient's 48 channels the last of a wider row, 3 x 9 x 7 (three images inside one pixel tile), the
    widest row, and more work items than resident workgroups (a workgroup walks two); plain and gate + statistics; the one-product mode."""
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    c = X.build_dgrad3(name)
    M, Cb, ldg, ldx, ldo = c["M"], c["Cb"], c["ldg"], c["ldx"], c["ldo"]
    ref3, ref1 = X.reference(c, 3)[0], X.reference(c, 1)[0]
    y, gate = np.nan_to_num(c["y"][:, :Cb], nan=0.0), c["gate"]
    gg, wg, yg, sc, sh = D(c["g"], dev), D(c["w"], dev), D(c["y"], dev), D(c["sc"], dev), D(c["sh"], dev)
    gptr = C.c_void_p(gg.data_ptr() + (ldg - 48) * 4)
    d = ConvDesc(c["B"], c["H"], c["W"], Cb, Cb, 48, ldg, 3, 3, 1, 1, 1, 1)
    wsb = int(L.rdm_conv3x3_dgrad_x3_workspace_bytes(Cb))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def launch(mask, ref, x1=False):
        out = nans((M, ldo), dev)
        sb0, p0, s0 = guarded(Cb, dev, f64, 2)
        sb1, p1, s1 = guarded(Cb, dev, f64, 2)
        m = (P(yg), ldx, P(sc), P(sh), p0, p1) if mask else (None, 0, None, None, None, None)
        names = ran(lambda: lib().check(L.rdm_conv3x3_dgrad_x3(C.byref(d), gptr, P(wg), P(out), ldo, *m, P(ws), wsb, int(x1), lib().stream())))
        assert names == {"xs_dgrad3x3_kernel/x%d/%s" % (1 if x1 else 3, "MASK_STATS" if mask else "STORE")}, names
        dz = ref * gate if mask else ref
        same(out, Cb, dz)
        assert guards_intact(sb0, Cb, 2) and guards_intact(sb1, Cb, 2)
        if mask:
            assert np.array_equal(s0.cpu().numpy(), dz.sum(0)) and np.array_equal(s1.cpu().numpy(), (dz * y).sum(0))

    for ref, x1 in ((ref3, False), (ref1, True)):
        launch(False, ref, x1)
        launch(True, ref, x1)


# ---- 3x3 weight gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.WGRAD3_CASES))
def test_wgrad3x3_exact(dev, op_census, name):
    """xs_wgrad3x3_kernel: N = 48 / 40, C = 64 + 16 / 48, ld > C, ldg > N, 9 x 7 frames and the widest row (93), split_k 0 / 1 / 3 equal to the
    reference; the frame image (bits == the restatement, borders zero) bit-identical to the float-operand launch; the one-product mode."""
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    c = X.build_wgrad3(name)
    Bn, H, W, Cc, ld, N, ldg, bn = c["B"], c["H"], c["W"], c["C"], c["ld"], c["N"], c["ldg"], c["sc"] is not None
    ref3, ref1 = X.reference(c, 3)[0], X.reference(c, 1)[0]
    xg, gg, sc, sh = D(c["x"], dev), D(c["g"], dev), D(c["sc"], dev), D(c["sh"], dev)
    d = ConvDesc(Bn, H, W, Cc, ld, N, ldg, 3, 3, 1, 1, 1, 1)
    fb = int(L.rdm_frame_split_rows_bytes(Bn, H, W))
    frame = nans((fb // 4,), dev)
    lib().check(L.rdm_frame_split_rows_f32(P(gg), ldg, N, Bn, H, W, P(frame), lib().stream()))
    assert torch.equal(frame.view(torch.int16).view(-1, 12, 8).cpu(), X.split_rows_bits(X.frame_image(c["g"], N)))

    def launch(gop, split, flags, x1=False):
        buf, p, view = guarded(9 * N * Cc, dev, f32, Cc)
        names = ran(lambda: lib().check(L.rdm_conv2d_wgrad_x3(C.byref(d), P(gop), P(xg), P(sc) if bn else None, P(sh) if bn else None, p, split, flags | int(x1), lib().stream())))
        assert names == {"xs_wgrad3x3_kernel/x%d/bn%d%s" % (1 if x1 else 3, bn, "/frameG" if flags else "")}, names
        assert guards_intact(buf, 9 * N * Cc, Cc)
        return view

    for split in (0, 1, 3):
        a, b = launch(gg, split, 0), launch(frame, split, X.DY_FRAME)
        equal(a, ref3)
        assert torch.equal(a, b)
    equal(launch(gg, 0, 0, x1=True), ref1)
    equal(launch(gg, 3, 0, x1=True), ref1)


# ---- 1x1 forward, three-way split -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.FWD_CASES))
def test_fwd1x1_x6_exact(dev, op_census, name):
    """xs_fwd1x1_kernel: N = 192 + 16 and 16, ragged K, ld > K, with / without prologue and statistics epilogue; the one-product mode.  The sums of
    the statistics epilogue are compared (== float64) on the mirrored planting, whose outputs are quarter-integers (xsplit_ref); on the general
    planting an output has no exact f32 square, so there the statistics instantiation is held to its stored output alone."""
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    c = X.build_fwd(name)
    M, K, ld, N, bn = c["M"], c["K"], c["ld"], c["N"], c["sc"] is not None
    ldo = N + 12
    ref6, ref1 = X.reference(c, 6)[0], X.reference(c, 1)[0]
    xg, wg, sc, sh = D(c["x"], dev), D(c["w"], dev), D(c["sc"], dev), D(c["sh"], dev)
    d = ConvDesc(c["B"], c["H"], c["W"], K, ld, N, ldo, 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_fwd_x6_workspace_bytes(K, N))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    for ref, x1 in ((ref6, False), (ref1, True)):
        for stats in (False, True):
            out = nans((M, ldo), dev)
            sb0, p0, s0 = guarded(N, dev, f64, 2)
            sb1, p1, s1 = guarded(N, dev, f64, 2)
            names = ran(lambda: lib().check(L.rdm_conv1x1_fwd_x6(C.byref(d), P(xg), P(wg), P(sc) if bn else None, P(sh) if bn else None, P(out), p0 if stats else None,
                                                                 p1 if stats else None, P(ws), wsb, int(x1), lib().stream())))
            assert names == {"xs_fwd1x1_kernel/x%d/bn%d/%s" % (1 if x1 else 6, bn, "STORE_STATS" if stats else "STORE")}, names
            same(out, N, ref)
            assert guards_intact(sb0, N, 2) and guards_intact(sb1, N, 2)
            if stats and c["mirror"]:
                assert np.array_equal(s0.cpu().numpy(), ref.sum(0)) and np.array_equal(s1.cpu().numpy(), (ref * ref).sum(0))
            elif stats:
                assert torch.isfinite(s0).all() and torch.isfinite(s1).all()
            else:
                assert not s0.any() and not s1.any()


# ---- real-valued leg: derived bound per element -------------------------------------------------------------------------------------------------
def within(op, got, ref, mag, k_terms):
    frac = float((np.abs(got.cpu().double().numpy().reshape(ref.shape) - ref) / np.maximum(X.bound(mag, k_terms), 1e-300)).max())
    print("real-valued leg %s: largest error / bound = %.4f" % (op, frac))
    assert frac <= 1.0, frac


def real_case(build, name, keys):
    """the planted case `name` with its operands replaced by uniform reals (the prologue's activation: one f32 rounding of the float64 fma)"""
    c = build(name)
    for k, (lo, hi) in keys.items():
        fin = ~np.isnan(c[k])
        c[k] = np.where(fin, X.real(name + ".real." + k, c[k].shape, lo, hi), np.nan)
    return c


def f32_act(x, sc, sh):
    return np.maximum((x * sc + sh).astype(np.float32).astype(np.float64), 0.0)


def test_real_valued(dev, op_census):
    L, P, ConvDesc = lib().lib(), lib().ptr, lib().ConvDesc
    st, keep = lib().stream(), []

    def DP(a):
        """device copy of `a`, kept alive until the test ends, as a pointer"""
        keep.append(D(a, dev))
        return P(keep[-1])

    # 1x1 weight gradient, split_k = 1: 3 M products per output
    c = real_case(X.build_wgrad1, "c240_split_bn1", dict(x=(-2, 2), g=(-1, 1), sc=(0.5, 1.5), sh=(-0.3, 0.3)))
    c["A"], c["Bop"] = c["g"][:, :c["N"]], f32_act(c["x"][:, :c["C"]], c["sc"], c["sh"])
    ref, mag = X.reference(c, 3)[:2]
    d = ConvDesc(c["B"], c["H"], c["W"], c["C"], c["ld"], c["N"], c["ldg"], 1, 1, 1, 1, 0, 0)
    dw = torch.zeros(c["N"], c["C"], device=dev)
    lib().check(L.rdm_conv2d_wgrad_x3(C.byref(d), DP(c["g"]), DP(c["x"]), DP(c["sc"]), DP(c["sh"]), P(dw), 1, 0, st))
    within("wgrad1x1", dw, ref, mag, 3 * c["M"])
    # 3x3 weight gradient, split_k = 1: 3 products per padded position
    c = real_case(X.build_wgrad3, "frame9x7", dict(x=(-2, 2), g=(-1, 1), sc=(0.5, 1.5), sh=(-0.3, 0.3)))
    c["A"], c["Bop"] = c["g"][..., :c["N"]], f32_act(c["x"][..., :c["C"]], c["sc"], c["sh"])
    ref, mag = X.reference(c, 3)[:2]
    d = ConvDesc(c["B"], c["H"], c["W"], c["C"], c["ld"], c["N"], c["ldg"], 3, 3, 1, 1, 1, 1)
    dw = torch.zeros(9, c["N"], c["C"], device=dev)
    lib().check(L.rdm_conv2d_wgrad_x3(C.byref(d), DP(c["g"]), DP(c["x"]), DP(c["sc"]), DP(c["sh"]), P(dw), 1, 0, st))
    within("wgrad3x3", dw, ref, mag, 3 * c["B"] * (c["H"] + 2) * (c["W"] + 2))
    # 1x1 input gradient: 3 K products per output
    c = real_case(X.build_dgrad1, "uneven_tiles", dict(g=(-1, 1), w=(-0.2, 0.2)))
    c["A"], c["Bop"] = c["g"][:, :c["K"]], c["w"]
    ref, mag = X.reference(c, 3)[:2]
    d = ConvDesc(c["B"], c["H"], c["W"], c["N"], c["N"], c["K"], c["ldg"], 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_dgrad_x3_workspace_bytes(c["K"], c["N"]))
    ws, out = torch.empty(wsb, dtype=torch.uint8, device=dev), nans((c["M"], c["N"]), dev)
    lib().check(L.rdm_conv1x1_dgrad_x3(C.byref(d), DP(c["g"]), DP(c["w"]), P(out), c["N"], None, 0, None, None, None, None, P(ws), wsb, 0, st))
    within("dgrad1x1", out, ref, mag, 3 * c["K"])
    # 3x3 input gradient: 3 x 9 x 48 products per output
    c = real_case(X.build_dgrad3, "cb144_tiny", dict(g=(-1, 1), w=(-0.1, 0.1)))
    c["A"], c["Bop"] = c["g"][..., c["ldg"] - 48:], c["w"]
    ref, mag = X.reference(c, 3)[:2]
    gg = D(c["g"], dev)
    d = ConvDesc(c["B"], c["H"], c["W"], c["Cb"], c["Cb"], 48, c["ldg"], 3, 3, 1, 1, 1, 1)
    wsb = int(L.rdm_conv3x3_dgrad_x3_workspace_bytes(c["Cb"]))
    ws, out = torch.empty(wsb, dtype=torch.uint8, device=dev), nans((c["M"], c["Cb"]), dev)
    lib().check(L.rdm_conv3x3_dgrad_x3(C.byref(d), C.c_void_p(gg.data_ptr() + (c["ldg"] - 48) * 4), DP(c["w"]), P(out), c["Cb"], None, 0, None, None, None, None, P(ws), wsb, 0, st))
    within("dgrad3x3", out, ref, mag, 3 * 9 * 48)
    # 1x1 forward: 6 K products per output
    c = real_case(X.build_fwd, "n208_k40_bn1", dict(x=(-2, 2), w=(-0.2, 0.2), sc=(0.5, 1.5), sh=(-0.3, 0.3)))
    c["A"], c["Bop"] = f32_act(c["x"][:, :c["K"]], c["sc"], c["sh"]), c["w"]
    ref, mag = X.reference(c, 6)[:2]
    d = ConvDesc(c["B"], c["H"], c["W"], c["K"], c["ld"], c["N"], c["N"], 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_fwd_x6_workspace_bytes(c["K"], c["N"]))
    ws, out = torch.empty(wsb, dtype=torch.uint8, device=dev), nans((c["M"], c["N"]), dev)
    lib().check(L.rdm_conv1x1_fwd_x6(C.byref(d), DP(c["x"]), DP(c["w"]), DP(c["sc"]), DP(c["sh"]), P(out), None, None, P(ws), wsb, 0, st))
    torch.cuda.synchronize()
    within("fwd1x1_x6", out, ref, mag, 6 * c["K"])
