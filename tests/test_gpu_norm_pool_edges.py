"""-m gpu: the elementwise kernels of csrc/elementwise.hip through the C ABI (rdm_bn_*, rdm_maxpool3s2_*, rdm_padavgpool2_*, rdm_adamw_fused)
against the float64 references of tests/normpool_ref.py (themselves checked in tests/test_normpool_ref_cpu.py), at the edges the older operator
tests do not reach: channels with |mean| / std up to 300, negative / zero / tiny gamma, gate values that are exactly 0, tied pooling taps,
row counts below the lane count and at the 512-row reduction chunk, grids past their block cap.  Every output buffer starts as NaN, every buffer
with a pixel stride gets ld > C with NaN behind the prefix, and the NaN must still be there afterwards.  Tolerances are per element (or per
channel), in terms of the reference's S_abs / T (sum of the absolute values of the terms), with the rounding count at each assert; `within`
prints the largest observed fraction of each bound.

Measured on one MI355X (float32 partial sums of up to 128 terms, float64 across workgroups).  Relative error of  var = sq / count - mu^2  from
the device's sums against the two-pass float64 variance of the data, largest over the channels of a case:
    |mean| / std = 30:   1.7e-6 at M = 24 593, 2.9e-5 at M = 570, 1.8e-4 at M = 35, 6.8e-4 at M = 3
    |mean| / std = 300:  1.2e-3 at M = 24 593, 3.4e-3 at M = 570, 1.2e-2 at M = 35, 4.5e-2 at M = 3
all below 0.006 of the propagated bound 2^-16 (S_abs(x^2) + 2 |mu| S_abs(x)) / count, which is all that is asserted.  It is the float32 rounding
of each square (2^-24 x^2 = 2^-24 x 9e4 var at 300 sigma) that shows, not the summation.  It is inside the bound, so nothing is changed for it.
Largest observed fraction of each bound: sums 0.0074, variance 0.0057, finalisation 0.47 (shift), constant-channel rstd 0.43, masked sums
0.0034, bn_bwd dx 0.26, dgamma / dbeta 0.25, deferred G 0.36 and running sums 0.62, max-pool dx 0.65, pooled 0.47, transition dx 0.21 and
dgamma / dbeta 0.0026, AdamW m 0.46, v 0.50, p 0.41 (zero-gradient block 0.61)."""
import ctypes as C

import numpy as np
import pytest
import torch

import normpool_ref as nr
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
E24, E16 = 2.0 ** -24, 2.0 ** -16
NAN = float("nan")
F32 = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


def L():
    from md_rdm_amd import _lib
    return _lib


def P(t):
    return L().ptr(t)


def dbuf(a, ld, dev, dtype=torch.float32):
    """(rows.., C) host array -> device buffer with pixel stride ld, NaN behind the first C columns"""
    a = np.asarray(a)
    buf = torch.full(a.shape[:-1] + (ld,), NAN, dtype=dtype)
    buf[..., :a.shape[-1]] = torch.from_numpy(np.ascontiguousarray(a))
    return buf.to(dev)


def dvec(a, dev, pad=4):
    """per-channel vector with `pad` NaN elements behind it"""
    return dbuf(np.asarray(a)[None], np.asarray(a).shape[0] + pad, dev)[0]


def nans(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def host(t):
    return t.detach().cpu().numpy()


def tail_is_nan(t, Cc):
    return bool(torch.isnan(t[..., Cc:]).all())


def within(got, want, tol, what):
    """|got - want| <= tol element-wise, NaN never passes; prints the largest fraction of the bound before asserting"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), want.shape)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bad = ~(err <= tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))
    print(f"BOUND {what}: {np.nanmax(frac) if frac.size else 0.0:.3g} of its bound")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside, first at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r} want {want[bad][0]!r} tol {tol[bad][0]!r}"


def ulps(v, k):
    """k float32 ulps of |v|"""
    return k * np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(F32)).astype(np.float64)


# ------------------------------------------------------------------------------------------
# (a) statistics and finalisation
# ------------------------------------------------------------------------------------------
# k_colreduce: 256 threads = 64 channel quads x 4 row lanes, rows_per_block = clamp(roundup16(ceil(M / 48)), 16, 512):
#   (1, 4), (3, 48)   fewer rows than the 4 row lanes (lanes 1..3 / lane 3 idle), one 16-row chunk
#   (17, 48)          two chunks, the second with one row; (35, 260): 3 chunks and a second column block with ONE live lane (quad 64 of 65)
#   (570, 100)        ceil(570 / 48) = 12 -> 16 rows: 36 chunks (also the 36 row blocks of k_bn_bwd_apply: gx = 1, cdiv(570, 2048) = 1 -> 16 rows)
#   (24 593, 8)       ceil(24 593 / 48) = 513 -> 528 -> capped at 512 (the cap is reached from ceil = 497, M = 23 809, on): 48 full chunks of
#                     512 rows = 128 terms per thread, the regime the 2^-16 bound is derived for, and a 49th chunk of 17 rows
@pytest.mark.parametrize("M,Cc", nr.BN_SHAPES)
def test_bn_statistics_and_finalisation(dev, M, Cc):
    lib, st = L().lib(), L().stream()
    case = nr.bn_case(M, Cc)
    x = case["x"]
    ld = Cc + 4
    xd = dbuf(x, ld, dev)
    sums = torch.zeros(2, Cc + 4, dtype=torch.float64, device=dev)
    sums[:, Cc:] = NAN
    L().check(lib.rdm_bn_stats(P(xd), ld, M, Cc, P(sums[0]), P(sums[1]), st))
    assert tail_is_nan(sums, Cc)
    s, q = host(sums[0, :Cc]), host(sums[1, :Cc])
    s64, q64, sa, qa = nr.colsums(x)
    # 128 sequential float32 adds + one rounding of the square + 3 adds through LDS = 132 x 2^-24; 2^-16 is twice that (f64 atomics negligible)
    within(s, s64, E16 * sa, f"bn_stats sum x M={M}")
    within(q, q64, E16 * qa, f"bn_stats sum x^2 M={M}")
    # ---- finalisation on the device's own sums
    for training in (1, 0):
        g = {k: dvec(case[k], dev) for k in ("gamma", "beta", "rm", "rv")}
        nbt = torch.full((1,), 7, dtype=torch.int64, device=dev)
        out = nans((4, Cc + 4), dev)
        L().check(lib.rdm_bn_finalize(P(sums[0]), P(sums[1]), float(M), P(g["gamma"]), P(g["beta"]), P(g["rm"]), P(g["rv"]), P(nbt),
                                      P(out[0]), P(out[1]), P(out[2]), P(out[3]), Cc, training, st))
        assert tail_is_nan(out, Cc) and all(tail_is_nan(g[k], Cc) for k in g)
        assert int(nbt) == (8 if training else 7)
        sc, sh, mean, rstd, rm2, rv2 = nr.bn_finalize(s, q, float(M), case["gamma"], case["beta"], case["rm"], case["rv"], training,
                                                      eps=nr.EPS32, momentum=nr.MOMENTUM32)
        o = host(out[:, :Cc])
        assert np.isfinite(o).all()
        # 4 float32 ulps: one rounding each for mean and rstd, then at most three dependent float32 operations.  shift = beta - mean * scale and
        # running_mean' = 0.9 rm + 0.1 mean END in an add of two terms of either sign, and a rounding is relative to the operand it rounds, so
        # their 4 ulps are ulps of the larger of the value and its two terms (equal to ulps of the value unless the terms cancel)
        tag = f"M={M} training={training}"
        within(o[2], mean, ulps(mean, 4), "bn_finalize mean " + tag)
        within(o[3], rstd, ulps(rstd, 4), "bn_finalize rstd " + tag)
        within(o[0], sc, ulps(sc, 4), "bn_finalize scale " + tag)
        within(o[1], sh, ulps(np.maximum(np.abs(sh), np.maximum(np.abs(case["beta"]), np.abs(mean * sc))), 4), "bn_finalize shift " + tag)
        within(host(g["rm"][:Cc]), rm2, ulps(np.maximum(np.abs(rm2), np.maximum(0.9 * np.abs(case["rm"]), 0.1 * np.abs(mean))), 4) if training else 0,
               "bn_finalize running_mean " + tag)
        within(host(g["rv"][:Cc]), rv2, ulps(rv2, 4) if training else 0, "bn_finalize running_var " + tag)
        ch = case["special"]["const_x"]
        if training and ch:
            within(o[3][ch], np.full(len(ch), nr.EPS32 ** -0.5), ulps(nr.EPS32 ** -0.5, 1), "rstd of a constant channel = 1 / sqrt(eps) " + tag)
    # ---- end to end: the variance the sums give against the two-pass float64 variance of the data; only the propagated bound is asserted
    if M > 1:
        x64 = x.astype(np.float64)
        mu64, var64 = x64.mean(0), x64.var(0)
        var = np.maximum(q / M - (s / M) ** 2, 0.0)
        within(var, var64, E16 * (qa / M + 2 * np.abs(mu64) * sa / M), f"variance from the device sums M={M}")
        for ratio in (30.0, 300.0):
            ch = np.flatnonzero(case["ratio"] == ratio)
            if not len(ch):
                continue
            rel = np.abs(var[ch] - var64[ch]) / var64[ch]
            print(f"VARERR M={M} |mean|/std={ratio:g}: relative variance error max {rel.max():.3g} median {np.median(rel):.3g}")


# ------------------------------------------------------------------------------------------
# (b) BatchNorm backward
# ------------------------------------------------------------------------------------------
# k_bn_bwd_apply: 64 quads x 4 row lanes, rows_per_block = max(16, roundup16(cdiv(M, 2048 / gx))) = 16 at all of these:
#   M = 1, 3: only the guarded tail, lanes past M masked by the -1 offset;  M = 17, 35: the 16-row main loop, then a tail of 1 / 3 rows
#   C = 260: gx = 2, the second column block has one live lane;  (570, 100): 36 row blocks;  (24 593, 8): 1 538 row blocks
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("M,Cc", nr.BN_SHAPES)
def test_bn_backward(dev, M, Cc, training):
    lib, st = L().lib(), L().stream()
    case = nr.bn_case(M, Cc)
    pl = nr.bn_planted(case)
    x = case["x"]
    gz = filler.uniform(f"npe.gz.{M}x{Cc}", (M, Cc), -1.0, 1.0)
    ldz, ldx, ldd = Cc + 4, Cc + 8, Cc + 12
    xd, dz = dbuf(x, ldx, dev), dbuf(gz, ldz, dev)
    v = {k: dvec(pl[k], dev) for k in ("sc", "sh", "gamma", "mean", "rstd")}
    r = torch.zeros(2, Cc + 4, dtype=torch.float64, device=dev)
    r[:, Cc:] = NAN
    L().check(lib.rdm_bn_bwd_reduce(P(dz), ldz, P(xd), ldx, P(v["sc"]), P(v["sh"]), M, Cc, P(r[0]), P(r[1]), st))
    dzm, s0_64, s1_64, a0, a1 = nr.bn_bwd_sums(gz, x, pl["sc"], pl["sh"])
    assert tail_is_nan(dz, Cc) and tail_is_nan(r, Cc)
    np.testing.assert_array_equal(host(dz[:, :Cc]), dzm)                            # the gate is exact: sign of the exact x * sc + sh, 0 closed
    s0, s1 = host(r[0, :Cc]), host(r[1, :Cc])
    within(s0, s0_64, E16 * a0, f"bn_bwd_reduce sum dz M={M}")                        # 132 x 2^-24 as in (a), the product dz * x for the square
    within(s1, s1_64, E16 * a1, f"bn_bwd_reduce sum dz x M={M}")
    # ---- apply, fed the device's own sums
    base = filler.uniform(f"npe.base.{M}x{Cc}", (M, Cc), -1.0, 1.0)
    for acc in (0, 1):
        dx = dbuf(base, ldd, dev) if acc else nans((M, ldd), dev)
        dgam, dbet = nans((Cc + 4,), dev), nans((Cc + 4,), dev)
        L().check(lib.rdm_bn_bwd(P(dx), ldd, P(dz), ldz, P(xd), ldx, P(r[0]), P(r[1]), float(M), P(v["gamma"]), P(v["mean"]), P(v["rstd"]),
                                 None if acc else P(dgam), None if acc else P(dbet), M, Cc, acc, training, st))
        want, dg, db, T = nr.bn_bwd_apply(dzm, x, s0, s1, float(M), pl["gamma"], pl["mean"], pl["rstd"], training, old=base if acc else None)
        assert tail_is_nan(dx, Cc)
        # per element: three coefficient roundings, two fmas, one add (accumulate) <= 8 x 2^-24 of the terms
        tag = f"M={M} C={Cc} training={training} accumulate={acc}"
        within(host(dx[:, :Cc]), want, 8 * E24 * T, "bn_bwd dx " + tag)
        if acc:
            assert torch.isnan(dgam).all() and torch.isnan(dbet).all()               # NULL dgamma / dbeta: nothing written
            continue
        assert tail_is_nan(dgam, Cc) and tail_is_nan(dbet, Cc)
        within(host(dgam[:Cc]), dg, ulps(dg, 2), "bn_bwd dgamma " + tag)             # float64 arithmetic on the same sums, rounded once
        within(host(dbet[:Cc]), db, ulps(db, 2), "bn_bwd dbeta " + tag)
        ch = case["special"]["g0neg"]
        if ch:                                                                       # gamma = 0 and a closed gate: exact zeros
            assert not host(dx[:, ch]).any() and not host(dgam[ch]).any() and not host(dbet[ch]).any()


def test_bn_backward_deferred_block(dev):
    """rdm_bn_bwd_defer over one three-layer block (C0 = 48, growth 48, M = 35), last layer first, ping-pong running sums carried on the device,
    with the channel recipe (offset channels, negative / zero gammas).  Each call is held to normpool_ref.bn_bwd_defer fed the SAME inputs the
    device had (its running sums and block gradient read back before the call)."""
    lib, st = L().lib(), L().stream()
    M, C0, GR, layers = 35, 48, 48, 3
    ctot = C0 + layers * GR                                                          # 192
    ld = ctot + 8
    x = nr.bn_case(M, ctot, "np.defer")["x"]
    xd = dbuf(x, ld, dev)
    G = dbuf(filler.uniform("npe.defer.G", (M, ctot), -1.0, 1.0), ld, dev)
    bc = torch.zeros(2, 2, ctot + 4, device=dev)                                      # [parity][b | c][channel]
    bc[..., ctot:] = NAN
    for i in reversed(range(layers)):
        cin = C0 + i * GR
        case = nr.bn_case(M, cin, f"np.defer.l{i}")
        pl = nr.bn_planted(dict(case, x=x[:, :cin]))
        gz = filler.uniform(f"npe.defer.gz.{i}", (M, cin), -1.0, 1.0)
        _, s0, s1, _, _ = nr.bn_bwd_sums(gz, x[:, :cin], pl["sc"], pl["sh"])
        sd = torch.from_numpy(np.stack([s0, s1])).to(dev)
        v = {k: dvec(pl[k], dev) for k in ("gamma", "mean", "rstd")}
        dgam, dbet = nans((cin + 4,), dev), nans((cin + 4,), dev)
        b_in, b_out = bc[(i + 1) & 1], bc[i & 1]
        c0, n = (cin - GR, GR) if i > 0 else (0, cin)
        G_before, b_before = host(G), host(b_in)
        out_before = host(b_out).copy()
        L().check(lib.rdm_bn_bwd_defer(P(G), ld, P(xd), ld, P(sd[0]), P(sd[1]), float(M), P(v["gamma"]), P(v["mean"]), P(v["rstd"]), P(dgam), P(dbet),
                                       P(b_in[0]), P(b_in[1]), P(b_out[0]), P(b_out[1]), M, cin, c0, n, 1, st))
        want, dg, db, b2, c2, T = nr.bn_bwd_defer(G_before[:, :cin], x[:, :cin], s0, s1, float(M), pl["gamma"], pl["mean"], pl["rstd"],
                                                  b_before[0], b_before[1], c0, n, 1)
        Gh, bo = host(G), host(b_out)
        assert tail_is_nan(G, ctot) and tail_is_nan(dgam, cin) and tail_is_nan(dbet, cin) and tail_is_nan(bc, ctot)
        # per element: rounding of the layer's B and C, their float32 adds onto the running sums, one fma, one add onto G <= 8 x 2^-24
        within(Gh[:, :cin], want, 8 * E24 * T, f"bn_bwd_defer G layer {i}")
        np.testing.assert_array_equal(Gh[:, cin:ctot], G_before[:, cin:ctot])        # outside the layer's channels: untouched
        np.testing.assert_array_equal(bo[:, cin:], out_before[:, cin:])
        _, B, Cc_, _, _ = nr.bn_bwd_coeffs(s0, s1, float(M), pl["gamma"], pl["mean"], pl["rstd"], 1)
        within(bo[0, :cin], b2, 2 * E24 * (np.abs(b_before[0, :cin]) + np.abs(B)), f"bn_bwd_defer running b layer {i}")      # round B, round the add
        within(bo[1, :cin], c2, 2 * E24 * (np.abs(b_before[1, :cin]) + np.abs(Cc_)), f"bn_bwd_defer running c layer {i}")
        within(host(dgam[:cin]), dg, ulps(dg, 2), f"bn_bwd_defer dgamma layer {i}")
        within(host(dbet[:cin]), db, ulps(db, 2), f"bn_bwd_defer dbeta layer {i}")


# ------------------------------------------------------------------------------------------
# (c) max-pool
# ------------------------------------------------------------------------------------------
# the small shapes put every out-of-image tap pattern in both directions (H or W of 1, 2, odd, even).  The last: k_maxpool3s2 launches
# min(cdiv(quads, 256), 8192) blocks; forward quads = B Ho Wo C/4 = 3 x 2 x 349 526 = 2 097 156 > 8192 x 256 = 2 097 152 (4 quads take a second
# trip), backward quads = B H W C/4 = 3 x 3 x 699 051 = 6 291 459 (three trips); 100 MB of input, the pool cannot shrink it below 3/2 x 2 per output
POOL_SHAPES = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 8), (2, 3, 3, 20), (3, 5, 4, 8), (2, 16, 16, 20), (3, 3, 699051, 4)]


@pytest.mark.parametrize("B,H,W,Cc", POOL_SHAPES)
def test_maxpool_ties_forward_backward(dev, B, H, W, Cc):
    lib, st = L().lib(), L().stream()
    big = W > 1000
    x = nr.pool_input(B, H, W, Cc, rng=np.random.default_rng(5) if big else None)
    y, arg = nr.maxpool3s2(x)
    Ho, Wo = y.shape[1:3]
    if H * W >= 9:
        assert nr.tie_fraction(x[:, :, :4096]) >= 0.20
    ld = Cc + 4
    xd = torch.from_numpy(x).to(dev)
    yd, argd = nans((B, Ho, Wo, ld), dev), torch.full((B, Ho, Wo, Cc), 255, dtype=torch.uint8, device=dev)
    L().check(lib.rdm_maxpool3s2_fwd(P(xd), P(yd), ld, P(argd), B, H, W, Cc, st))
    assert tail_is_nan(yd, Cc)
    np.testing.assert_array_equal(host(yd[..., :Cc]), y)                            # a max is exact
    np.testing.assert_array_equal(host(argd), arg)                                  # the FIRST maximum in row-major tap order
    gy = (np.random.default_rng(6).random(y.shape, dtype=F32) * 2 - 1) if big else filler.uniform(f"npe.mp.g.{B}x{H}x{W}x{Cc}", y.shape, -1.0, 1.0)
    gd = dbuf(gy, ld, dev)
    dx = nans((B, H, W, Cc), dev)
    L().check(lib.rdm_maxpool3s2_bwd(P(gd), ld, P(argd), P(dx), B, H, W, Cc, st))
    want, sa = nr.maxpool3s2_bwd(gy, arg, H, W)
    within(host(dx), want, 3 * E24 * sa, f"maxpool dx {B}x{H}x{W}x{Cc}")             # up to four addends in fixed order: three roundings


# ------------------------------------------------------------------------------------------
# (d) transition front end
# ------------------------------------------------------------------------------------------
# the last: k_trans_pool launches min(cdiv(quads, 256), 4096) blocks; forward quads = B Ho Wo C/4 = 2 x 2 x 65 537 x 4 = 1 048 592 > 4096 x 256 =
# 1 048 576 (16 quads take a second trip); k_trans_pool_bwd_apply: B H W C/4 = 2 x 3 x 131 073 x 4 = 3 145 752 (three trips); the padded row
# count 2 x 4 x 131 074 = 1 048 592 puts k_trans_pool_bwd_reduce at its 512-row chunk too
TRANS_SHAPES = [(1, 1, 1, 4), (2, 1, 6, 8), (2, 6, 1, 8), (2, 7, 9, 48), (2, 8, 10, 48), (2, 3, 131073, 16)]


# (the grid-stride shape runs in training mode only: eval mode is the same kernels with B = C = 0)
@pytest.mark.parametrize("B,H,W,Cc,training", [s + (t,) for s in TRANS_SHAPES for t in (1, 0) if t or s[2] < 1000])
def test_transition_pool_forward_backward(dev, B, H, W, Cc, training):
    lib, st = L().lib(), L().stream()
    big = W > 1000
    M = B * H * W
    case = nr.bn_case(M, Cc, "np.tp")
    pl = nr.bn_planted(case, count=B * (H + 1) * (W + 1))
    x = case["x"].reshape(B, H, W, Cc)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    ldx, ldd = Cc + 4, Cc + 8
    xd = dbuf(x, ldx, dev)
    v = {k: dvec(pl[k], dev) for k in ("sc", "sh", "gamma", "mean", "rstd")}
    pooled = nans((B * Ho * Wo * Cc + 4,), dev)
    L().check(lib.rdm_padavgpool2_fwd(P(xd), ldx, P(v["sc"]), P(v["sh"]), P(pooled), B, H, W, Cc, st))
    want_p, sabs = nr.padavgpool2(x, pl["sc"], pl["sh"])
    assert torch.isnan(pooled[-4:]).all()
    # four float32 fmas (one rounding each, relative to the relu term), three adds, x 0.25 exact <= 6 x 2^-24 of 0.25 x the sum of the terms
    tag = f"{B}x{H}x{W}x{Cc} training={training}"
    within(host(pooled[:-4]).reshape(want_p.shape), want_p, 6 * E24 * sabs, "padavgpool2 pooled " + tag)
    gp = (np.random.default_rng(7).random(want_p.shape, dtype=F32) * 2 - 1) if big else filler.uniform(f"npe.tp.g.{B}x{H}x{W}x{Cc}", want_p.shape, -1.0, 1.0)
    gpd = torch.from_numpy(gp).to(dev)
    wsb = int(lib.rdm_padavgpool2_bwd_workspace_bytes(Cc))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    dx, dgam, dbet = nans((B, H, W, ldd), dev), nans((Cc + 4,), dev), nans((Cc + 4,), dev)
    L().check(lib.rdm_padavgpool2_bwd(P(gpd), P(xd), ldx, P(v["sc"]), P(v["sh"]), P(v["gamma"]), P(v["mean"]), P(v["rstd"]), P(dx), ldd, P(dgam), P(dbet),
                                      B, H, W, Cc, training, P(ws), wsb, st))
    r = nr.padavgpool2_bwd(gp, x, pl["sc"], pl["sh"], pl["gamma"], pl["mean"], pl["rstd"], training)
    assert tail_is_nan(dx, Cc) and tail_is_nan(dgam, Cc) and tail_is_nan(dbet, Cc)
    e0, e1 = E16 * r["S0abs"], E16 * r["S1abs"]                                        # the sums as in (b), over the padded extent
    mu, rs = pl["mean"].astype(np.float64), pl["rstd"].astype(np.float64)
    within(host(dbet[:Cc]), r["dbeta"], e0 + ulps(r["dbeta"], 2), "padavgpool2 dbeta " + tag)
    within(host(dgam[:Cc]), r["dgamma"], rs * (e1 + np.abs(mu) * e0) + ulps(r["dgamma"], 2), "padavgpool2 dgamma " + tag)
    # the entry point fuses the passes, so the sum bound is propagated through A, B, C: 8 x 2^-24 T + |d dx / d s0| e0 + |d dx / d s1| e1
    within(host(dx[..., :Cc]), r["dx"], 8 * E24 * r["T"] + r["d0"] * e0 + r["d1"] * e1, "padavgpool2 dx " + tag)
    ch = case["special"]["g0neg"]
    if ch and training:
        assert not host(dx[..., ch]).any() and not host(dgam[ch]).any() and not host(dbet[ch]).any()


# ------------------------------------------------------------------------------------------
# (e) AdamW
# ------------------------------------------------------------------------------------------
# k_adamw: min(max(cdiv(n / 4, 256), 1), 2048) blocks of 256 quads, the n % 4 tail on block 0.  n = 1, 2, 3: tail only; 4: one quad; 5, 7: quad + tail;
# 1027: 2 blocks + tail of 3; 2 097 159 = 4 x (2048 x 256 + 1) + 3: ONE quad takes the second trip of the grid-stride loop, and a tail of 3
ADAMW_N = [1, 2, 3, 4, 5, 7, 1027, 4 * (2048 * 256 + 1) + 3]
HP = dict(lr=F32(1e-2), b1=F32(0.9), b2=F32(0.999), eps=F32(1e-8))


def adamw_check(got, ref, p0, tag):
    """per element against the float64 reference fed the same float32 state
    m: b1 * m, (1 - b1) * g, their add: 3 roundings of the terms <= 4 x 2^-24 (|b1 m0| + |(1 - b1) g|)
    v: b2 * v, (1 - b2) * g, * g, the add: 4 roundings <= 4 x 2^-24 (the terms are non-negative)
    p: the issue's 2 x 2^-24 |p0| + 16 x 2^-24 |update| counts the update's roundings on |update|; the honest count differs in two places:
       |p0| takes 3, not 2: 1 - lr * wd rounds to 2^-25, the product p0 * (..) to 2^-24, and the final subtraction to 2^-24 of |p|
       the moment's error is 4 x 2^-24 of its TERMS (above), not of m: where b1 * m0 and (1 - b1) * g cancel it exceeds any multiple of |update|,
       so it enters as 4 x 2^-24 Tm x lr / bc1 / denom (= 4 x 2^-24 |update| when they do not cancel)
       the rest on |update|: bc1 to float32 and lr / bc1 (2), v's 4 halved by the root (2), sqrtf, rsqrt_bc2 to float32, their product, + eps (4),
       m / denom, the product with lr / bc1, the subtraction (3) = 11 -> 12;  12 + 4 is the issue's 16"""
    within(got["m"], ref["m"], 4 * E24 * ref["Tm"], "adamw m " + tag)
    within(got["v"], ref["v"], 4 * E24 * ref["Tv"], "adamw v " + tag)
    within(got["p"], ref["p"], 3 * E24 * np.abs(p0) + 12 * E24 * np.abs(ref["update"]) + 4 * E24 * ref["Tm"] * ref["step_scale"] / ref["denom"], "adamw p " + tag)


@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_fused(dev, n):
    lib, st = L().lib(), L().stream()
    inp = nr.adamw_inputs(n)
    pad = 5
    hp = {k: float(v) for k, v in HP.items()}

    def buf(a):
        t = nans((n + pad,), dev)
        t[:n] = torch.from_numpy(np.asarray(a, dtype=F32))
        return t

    def call(p, g, m, v, step, wd, gs):
        L().check(lib.rdm_adamw_fused(P(p), P(g), P(m), P(v), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"], float(F32(wd)), step, gs, st))
        assert all(torch.isnan(t[n:]).all() for t in (p, m, v))                      # elements past n in a padded allocation stay NaN
        return dict(p=host(p[:n]), m=host(m[:n]), v=host(v[:n]))

    for wd in (0.0, 0.1):
        for gs in (1.0, 0.5, 0.125):
            wd32 = float(F32(wd))
            tag = f"n={n} wd={wd} grad_scale={gs}"
            # steps 1 and 2, the moments carried on the device; the reference of step 2 starts from the device's state after step 1
            p, m, v = buf(inp["p"]), buf(np.zeros(n)), buf(np.zeros(n))
            cur = dict(p=inp["p"], m=np.zeros(n, F32), v=np.zeros(n, F32))
            for step, g in ((1, inp["g"]), (2, inp["g2"])):
                ref = nr.adamw(cur["p"], g, cur["m"], cur["v"], step, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd32, gs)
                got = call(p, buf(g), m, v, step, wd, gs)
                adamw_check(got, ref, cur["p"], f"step {step} " + tag)
                if step == 1 and inp["zero"].any():                                  # zero gradients: v = 0, denom = eps, nothing but the decay moves p
                    z = inp["zero"]
                    assert not got["v"][z].any() and not got["m"][z].any()
                    within(got["p"][z], cur["p"][z].astype(np.float64) * (1.0 - hp["lr"] * wd32), 2 * E24 * np.abs(cur["p"][z]), "adamw zero-gradient block " + tag)
                cur = got
            # step 1000: one call on planted moments
            p, m, v = buf(inp["p"]), buf(inp["m0"]), buf(inp["v0"])
            ref = nr.adamw(inp["p"], inp["g"], inp["m0"], inp["v0"], 1000, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd32, gs)
            adamw_check(call(p, buf(inp["g"]), m, v, 1000, wd, gs), ref, inp["p"], "step 1000 " + tag)
