"""tests/bf16_ref.py without a GPU: each float64 reference against an independent torch float64 formulation (1e-12 relative), round_bf16
against tensor.to(torch.bfloat16), and the PLANTED INPUTS of every case of tests/test_gpu_bf16_exact.py against the conditions under which the
kernels' f32 arithmetic is exact:
  (a) sum |a||w| + |bias| per output < 2^23 in the operands' unit (1 or 0.25): every f32 summation order is exact;
  (b) at least 25 % of the bf16 outputs are no bf16 numbers;  (c) at least 10 exact ties rounding down and 10 rounding up;
  (d) statistics forms: the stored values are integers with 256 * max(v*v) < 2^24, so f32 sums over up to 256 rows are exact.
These are conditions on the inputs (the reference alone), not measurements of a kernel.  Teeth: a reference with one tap, one channel or the pad
contribution removed differs from the intact one on the planted inputs of every case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bf16_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- round_bf16 -----------------------------------------------------------------------------------------------------------------------------
def test_round_bf16_matches_torch_and_flags_ties():
    big = float(torch.finfo(torch.bfloat16).max)
    x = np.concatenate([R.filler.uniform("rb.a", (50000,), -1000.0, 1000.0), R.filler.log_uniform("rb.b", (50000,), 1e-30, 1e30) * R.choice("rb.s", (50000,), (-1.0, 1.0)),
                        [257.0, 259.0, 1027.0, 1029.0, -257.0, -259.0, 0.0, -0.0, np.inf, -np.inf, big, -big, big * (1 + 2.0 ** -9), big * (1 + 2.0 ** -8), -big * (1 + 2.0 ** -8),
                         2.0 ** -130, -2.0 ** -140, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20]]).astype(np.float32).astype(np.float64)
    got, tie = R.round_bf16(x)
    want = T(x).float().to(torch.bfloat16).double().numpy()
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
    n = 100000
    assert got[n:n + 6].tolist() == [256.0, 260.0, 1024.0, 1032.0, -256.0, -260.0] and tie[n:n + 6].tolist() == [True, True, False, False, True, True]
    assert not tie[n + 6:n + 12].any() and got[n + 10] == big and np.isinf(got[n + 13]) and np.isinf(got[n + 14]) and got[n + 14] < 0
    assert tie[n + 17] and not tie[n + 18] and not tie[n + 19]
    assert got[n + 17] == 1.0 and got[n + 18] == 1.0 + 2.0 ** -7 and got[n + 19] == 1.0
    assert np.array_equal(R.bf16_bits(x), R.canon_bits(T(x).float().to(torch.bfloat16)))
    assert np.isnan(R.round_bf16(np.array([np.nan]))[0][0])
    assert R.rounding_census(np.array([257.0, 259.0, 3.0, 1027.0, 1028.0])) == (0.8, 2, 1)


# ---- the references against independent formulations ----------------------------------------------------------------------------------------
def test_gemm_reference():
    M, K, N = 37, 40, 28
    x, w = R.filler.uniform("rg.x", (M, K + 8), -2, 2, np.float64), R.filler.uniform("rg.w", (N, K), -1, 1, np.float64)
    sc, sh = R.filler.uniform("rg.s", (K,), 0.5, 1.5, np.float64), R.filler.uniform("rg.t", (K,), -0.5, 0.5, np.float64)
    b, osc, osh = (R.filler.uniform("rg." + k, (N,), -1, 1, np.float64) for k in "bcd")
    a = torch.relu(T(x[:, :K]) * T(sc) + T(sh)).float().to(torch.bfloat16).double()
    close(R.gemm(x, w, K, sc, sh)[0], torch.einsum("mk,nk->mn", a, T(w)).numpy())
    close(R.gemm(x, w, K, sc, sh, b)[0], (torch.einsum("mk,nk->mn", a, T(w)) + T(b)).numpy())
    close(R.gemm(x, w, K, sc, sh, None, osc, osh)[0], torch.relu(torch.einsum("mk,nk->mn", a, T(w)) * T(osc) + T(osh)).numpy())
    close(R.gemm(x, w, K)[0], torch.einsum("mk,nk->mn", T(x[:, :K]), T(w)).numpy())
    close(R.gemm(x, w, K, sc, sh, b)[1], (torch.einsum("mk,nk->mn", a.abs(), T(w).abs()) + T(b).abs()).numpy())
    v, s, q = R.stored_stats(R.gemm(x, w, K)[0])
    close(v, T(R.gemm(x, w, K)[0]).float().to(torch.bfloat16).double().numpy())
    close(s, v.sum(0))
    close(q, np.einsum("mn,mn->n", v, v))


def test_conv_references():
    B, H, W, C = 2, 5, 4, 16
    y = R.filler.uniform("rc.y", (B, H, W, C + 8), -2, 2, np.float64)
    w9 = R.filler.uniform("rc.w", (9, 48, C), -1, 1, np.float64)
    sc, sh = R.filler.uniform("rc.s", (C,), 0.5, 1.5, np.float64), R.filler.uniform("rc.t", (C,), -0.5, 0.5, np.float64)
    a = torch.relu(T(y[..., :C]) * T(sc) + T(sh)).float().to(torch.bfloat16).double()
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))                     # zero padding of the ACTIVATED tensor
    want = sum(torch.einsum("bhwc,nc->bhwn", ap[:, r:r + H, s:s + W], T(w9[r * 3 + s])) for r in range(3) for s in range(3)).reshape(-1, 48).numpy()
    close(R.conv3x3(y, w9, C, sc, sh)[0], want)
    w_oihw = np.ascontiguousarray(w9.reshape(3, 3, 48, C).transpose(2, 3, 0, 1))
    wr = T(w_oihw).float().to(torch.bfloat16).double()
    yp = F.pad(T(y[..., :C]), (0, 0, 1, 1, 1, 1))
    want = sum(torch.einsum("bhwc,nc->bhwn", yp[:, r:r + H, s:s + W], wr[:, :, r, s]) for r in range(3) for s in range(3)).reshape(-1, 48).numpy()
    close(R.conv3x3_act(y, w_oihw, C)[0], want)
    s, q = R.colstats(y.reshape(-1, C + 8), C)
    close(s, T(y.reshape(-1, C + 8))[:, :C].sum(0).numpy())
    close(q, torch.einsum("mc,mc->c", T(y.reshape(-1, C + 8))[:, :C], T(y.reshape(-1, C + 8))[:, :C]).numpy())


@pytest.mark.parametrize("H,W", [(7, 7), (8, 9), (15, 14), (1, 1)])
def test_helper_references(H, W):
    B, C = 2, 16
    x = R.filler.uniform("rh.x%d" % H, (B, 3, H, W), -3, 3, np.float64)
    u = F.unfold(T(x), 7, padding=3, stride=2).permute(0, 2, 1).reshape(-1, 147).float().to(torch.bfloat16).double().numpy()
    got = R.stem_patches(x)
    assert got.shape == (u.shape[0], 160) and np.array_equal(got[:, :147], u) and not got[:, 147:].any()
    y = R.filler.uniform("rh.y%d" % H, (B, H, W, C), -3, 3, np.float64)
    close(R.maxpool3s2(y), F.max_pool2d(T(y).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, C).numpy())
    sc, sh = R.filler.uniform("rh.s", (C,), 0.5, 1.5, np.float64), R.filler.uniform("rh.t", (C,), -0.5, 0.5, np.float64)
    yp = F.pad(T(y).permute(0, 3, 1, 2), (0, W % 2, 0, H % 2))
    want = F.avg_pool2d(torch.relu(yp * T(sc).view(1, C, 1, 1) + T(sh).view(1, C, 1, 1)), 2).permute(0, 2, 3, 1).reshape(-1, C).numpy()
    close(R.padavgpool2(np.concatenate([y, y], -1), C, sc, sh), want)
    src = R.filler.uniform("rh.r", (5, 12), -3, 3, np.float64)
    got = R.rows_to_bf16(src, 9, 16)
    assert np.array_equal(got[:, :9], T(src[:, :9]).float().to(torch.bfloat16).double().numpy()) and not got[:, 9:].any() and got.shape == (5, 16)
    w = R.filler.uniform("rh.w", (6, 5, 9), -1, 1, np.float64)
    assert np.array_equal(R.pack_weight(w), T(w).permute(2, 0, 1).float().to(torch.bfloat16).double().numpy())


# ---- the planted inputs of every GPU case -------------------------------------------------------------------------------------------------
def hold(c, bf16_out=True, what=""):
    a, a_out = R.condition_a(c["mag"], c["unit"], c.get("osc"), c.get("osh"))
    assert a < 2 ** 23 and a_out < 2 ** 24, (what, a, a_out)
    if bf16_out:
        share, down, up = R.rounding_census(c["exact"])
        assert share >= 0.25 and down >= 10 and up >= 10, (what, share, down, up)


@pytest.mark.parametrize("name", sorted(R.GEMM_CASES))
def test_conditions_gemm_tiles(name):
    M, K, N, px, pw, tile = R.GEMM_CASES[name]
    for opt in R.OPTS:
        assert R.gemm_variant(M, K, N, 0, opt[1], opt[2]) == "gemm_bf16_kernel/" + tile
        c = R.build_gemm(name, M, K, N, px, pw, opt)
        hold(c, not opt[2], (name, opt))
        if opt == R.OPTS[0]:                               # teeth: the last 8-column chunk of K removed
            wd = c["w"].copy()
            wd[:, K - 8:K] = 0.0
            assert (R.gemm(c["x"], wd, K, c["sc"], c["sh"])[0] != c["exact"]).mean() > 0.5


def test_conditions_gemm_split():
    M, K, N, px, pw = R.SPLIT_CASE
    assert R.gemm_variant(M, K, N, 8 * M * N) == R.gemm_variant(M, K, N, 2 * M * N) == "gemm_bf16_kernel/32x96/splitK"
    for opt in R.OPTS_SPLIT:
        hold(R.build_gemm("split", M, K, N, px, pw, opt), True, opt)


@pytest.mark.parametrize("K", sorted(R.PANEL_K))
def test_conditions_gemm_panel(K):
    M, N = R.PANEL_MN
    assert R.gemm_variant(M, K, N) == "gemm_panel_bf16_kernel/nkk%d" % R.PANEL_K[K]
    hold(R.build_gemm("panel%d" % K, M, K, N, 8, 0, R.panel_opt(K)), True, K)


@pytest.mark.parametrize("name", sorted(R.STATS_GEMM_CASES))
def test_conditions_gemm_stats(name):
    M, K, N, px = R.STATS_GEMM_CASES[name]
    x, w, sc, sh = R.stats_gemm_operands(name, M, K, N, K + px)
    exact, mag = R.gemm(x, w, K, sc, sh)
    hold(dict(exact=exact, mag=mag, unit=0.25), True, name)
    d, frac = R.condition_d(R.stored_stats(exact)[0])
    assert d < 2 ** 24 and not frac


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_conditions_conv3x3(name):
    B, H, W, C, pro, (bm, HL) = R.CONV_CASES[name]
    assert R.conv3_plan(B, H, W, C)[:2] == (bm, HL)
    assert R.conv3_tile_slots(B, H, W, bm) <= R.conv3_slots(B, H, W, bm) <= 1280          # the LDS image the launcher sizes holds every tile
    c = R.build_conv(name, B, H, W, C, pro)
    hold(c, True, name)
    for kw in (dict(drop_tap=4), dict(drop_tap=0), dict(drop_channel=C - 1)) + ((dict(activate_pad=True),) if pro else ()):
        if "drop_tap" in kw and kw["drop_tap"] == 0 and min(H, W) == 1:
            continue                                       # one row or one column: the corner tap only ever meets the padding
        if "activate_pad" in kw and not (c["sh"] > 0).any():
            continue
        assert (R.conv3x3(c["y"], c["w9"], C, c["sc"], c["sh"], **kw)[0] != c["exact"]).any(), (name, kw)
    if pro:
        assert (c["sh"] > 0).any()


@pytest.mark.parametrize("name", sorted(R.STATS_CONV_CASES))
def test_conditions_conv3x3_stats(name):
    B, H, W, C = R.STATS_CONV_CASES[name]
    y, w9, sc, sh = R.stats_conv_operands(name, B, H, W, C, C + 8)
    exact, mag = R.conv3x3(y, w9, C, sc, sh)
    hold(dict(exact=exact, mag=mag, unit=0.25), True, name)
    d, frac = R.condition_d(R.stored_stats(exact)[0])
    assert d < 2 ** 24 and not frac
    assert (R.conv3x3(y, w9, C, sc, sh, activate_pad=True)[0] != exact).any()


@pytest.mark.parametrize("name", sorted(R.ACT_CASES))
def test_conditions_conv3x3_act(name):
    B, H, W, C, ws, census = R.ACT_CASES[name]
    c = R.build_act(name, B, H, W, C)
    hold(c, True, name)
    wd = c["w"].copy()
    wd[:, :, 0, 0] = 0.0
    assert (R.conv3x3_act(c["y"], wd, C)[0] != c["exact"]).any()


def test_conditions_colstats_and_pools():
    for M, C in R.COLSTATS_CASES:
        x = R.ints("cs%d.%d" % (M, C), (M, C + 8), -255, 255)
        d, frac = R.condition_d(x)
        assert d < 2 ** 24 and not frac and np.array_equal(R.round_bf16(x)[0], x)
    # teeth of the pooling references on planted inputs: a pad that contributes 0 instead of relu(shift); a missing border tap
    x = R.ints("tp.x", (2, 3, 5, 8), -64, 64) / 16.0
    sc, sh = R.choice("tp.s", (8,), (0.5, 1.0, 2.0)), R.ints("tp.t", (8,), 1, 8) / 4.0
    assert (R.padavgpool2(x, 8, sc, sh) != R.padavgpool2(x, 8, sc, sh, pad_is_input=False)).any()
    y = -1.0 - np.abs(R.ints("mp.x", (2, 5, 4, 8), -64, 64) / 16.0)
    for tap in ((0, 0), (2, 2), (1, 1)):
        assert (R.maxpool3s2(y) != R.maxpool3s2(y, drop_tap=tap)).any()
