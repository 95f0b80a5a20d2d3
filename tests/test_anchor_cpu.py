"""Anchored metric depth without a GPU: properties of the numpy statement of include/rdm_anchor.h (tests/anchor_ref.py), so that the GPU tests
compare against something that is itself checked; the wrapper's parameter rules, the rules of the command-line flags, the 16-bit PNG reader,
and the C-ABI boundary of include/rdm_anchor.h (declared == bound == exported)."""
import math
import os
import re
import struct
import zlib

import numpy as np
import pytest

import anchor_ref as aref
import depthframe_ref as dref
import evalview_ref as vref
from conftest import ROOT
from md_rdm_amd import filler

HEADER = os.path.join(ROOT, "include", "rdm_anchor.h")
H, W, CELL = 96, 128, 8


def log_map(key, B=1):
    return filler.uniform("anchor.cpu.map/" + key, (B, 1, 128, 128), -1.0, 1.0, dtype=np.float64)


def resampled(m, h=H, w=W, view=None):
    return vref.resize_view(m, h, w, view)[:, 0]


def planted(h=H, w=W):
    y, x = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    return 0.1 * np.sin(2.0 * np.pi * y / h) * np.cos(2.0 * np.pi * x / w)


def test_planted_field_is_recovered():
    """Dense anchors exp(v + ls0 + P), P = 0.1 sin(2 pi y / h) cos(2 pi x / w) on a 96x128 frame (one period of 12 x 16 cells at cell 8), sigma 1,
    lambda 0, fit logmean without a prior.  What the fit cannot return: the Gaussian of sigma 1 cell attenuates a sinusoid of period L cells by
    1 - exp(-2 pi^2 / L^2): 12.8 % along y (L = 12) and 7.4 % along x, at most 19 % of the amplitude together = 0.019; the cell mean and the
    bilinear interpolation between cell centres lose (pi / L)^2 / 6 and (pi / L)^2 / 2 of it, under 0.005 more; the border, where the indices
    are clamped and the kernel is one-sided, adds the field's change over half a cell, 0.1 * 2 pi / 12 / 2 = 0.026 at the steepest place.
    Bound: 0.03 inside (more than one cell from the border), 0.06 at the border; the reference run gives 0.0245 and 0.0390.  The scale: P has zero mean over
    the frame, so delta = ls0 to the rounding of float32 anchors."""
    m = log_map("planted")
    v, P, ls0 = resampled(m), planted(), 0.83
    a = np.exp(v + ls0 + P[None]).astype(np.float32)
    f = aref.fit(m, a, fit="logmean", cell=CELL, sigma=1.0, lam=0.0)
    assert f["count"][0] == H * W and abs(f["log_scale"][0] - ls0) < 1e-6
    got = f["log_scale"][:, None, None] + aref.field_at_pixels(f["field"], H, W, CELL)
    err = np.abs(got - (ls0 + P[None]))[0]
    inner = err[CELL:-CELL, CELL:-CELL].max()
    print("planted field: max error inside %.4f, at the border %.4f" % (inner, err.max()))
    assert inner < 0.03 and err.max() < 0.06
    frames = aref.frames(m, H, W, f["log_scale"], f["field"], CELL)
    assert np.abs(np.log(frames["D"][0]) - np.log(a[0].astype(np.float64))).max() < 0.06


def test_constant_offset_is_all_scale():
    m = log_map("offset", 2)
    a = np.exp(resampled(m) + 0.37).astype(np.float32)
    f = aref.fit(m, a, fit="logmean", cell=CELL, sigma=2.0, lam=1.0)
    assert np.abs(f["log_scale"] - 0.37).max() < 1e-7                      # float32 anchors: relative 6e-8 each, and they average
    assert np.abs(f["field"]).max() < 2e-7
    with_prior = aref.fit(m, a, prior=np.array([0.3, 0.5]), fit="logmean", cell=CELL)
    assert np.abs(with_prior["log_scale"] - 0.37).max() < 1e-7             # the prior moves the residuals, not the result
    kept = aref.fit(m, a, prior=np.array([0.3, 0.5]), fit="none", cell=CELL, sigma=0.0, lam=0.0)
    np.testing.assert_array_equal(kept["log_scale"], [0.3, 0.5])
    assert np.abs(kept["field"][0] - 0.07).max() < 1e-6 and np.abs(kept["field"][1] + 0.13).max() < 1e-6      # sigma 0, lambda 0: the cell means


def test_no_anchors_is_exactly_nothing():
    m = log_map("none", 2)
    a = np.zeros((2, 37, 53), dtype=np.float32)
    a[1, 3, 4] = np.nan
    a[1, 5, 6] = -1.0
    a[1, 7, 8] = np.inf
    for fit in ("logmean", "none", "median"):
        f = aref.fit(m, a, prior=np.array([0.25, -1.5]), fit=fit, cell=8)
        np.testing.assert_array_equal(f["log_scale"], [0.25, -1.5])
        assert (f["count"] == 0).all() and (f["field"] == 0).all() and not np.signbit(f["field"]).any()
    f = aref.fit(m, a, fit="logmean", cell=8, lam=0.0)
    assert (f["log_scale"] == 0).all() and (f["field"] == 0).all()
    # anchors outside the view or outside the depth range are no anchors either
    a = np.full((2, 37, 53), 2.0, dtype=np.float32)
    assert (aref.fit(m, a, view=(40.0, 0.0, 20.0, 53.0), cell=8)["count"] == 0).all()
    assert (aref.fit(m, a, cell=8, min_depth=3.0)["count"] == 0).all() and (aref.fit(m, a, cell=8, max_depth=1.0)["count"] == 0).all()
    assert (aref.fit(m, a, cell=8, min_depth=2.0, max_depth=2.0)["count"] == 37 * 53).all()                  # the limits themselves are valid


def test_reject_with_a_median_prior_removes_outliers():
    m = log_map("outliers")
    v = resampled(m)
    a = np.exp(v + 0.6).astype(np.float32)
    bad = filler.unit("anchor.cpu.outliers", H * W).reshape(1, H, W) < 0.10
    assert 0.08 < bad.mean() < 0.12
    a[bad] *= np.float32(3.0)
    plain = aref.fit(m, a, fit="logmean", cell=CELL)
    assert abs(plain["log_scale"][0] - (0.6 + bad.mean() * math.log(3.0))) < 1e-6 and plain["count"][0] == H * W      # the mean takes the outliers in
    med = aref.fit(m, a, fit="median", cell=CELL)
    # the ratio of medians alone: the outliers move a tenth of the mass up, the median of a from the 50th to about the 55th percentile of the clean
    # frame, whose ln a spreads over about 2: near 0.1 off (a statistic of the frame, not of the per-pixel ratios), and nothing is dropped
    assert abs(med["log_scale"][0] - 0.6) < 0.15 and med["count"][0] == H * W
    assert np.abs(med["field"]).max() > 0.02                                                                          # ... so the field carries the outliers
    gated = aref.fit(m, a, fit="median", cell=CELL, reject=0.5)
    assert gated["count"][0] == H * W - bad.sum()
    assert abs(gated["log_scale"][0] - med["log_scale"][0]) == 0 and np.abs(gated["log_scale"][0] + aref.field_at_pixels(gated["field"], H, W, CELL) - 0.6).max() < 1e-3


def test_lambda_pulls_the_field_down_where_anchors_are_few():
    m = log_map("lambda")
    v = resampled(m)
    a = np.zeros((1, H, W), dtype=np.float32)
    ys, xs = np.meshgrid(np.arange(CELL // 2, H, CELL), np.arange(CELL // 2, W // 2, CELL), indexing="ij")           # one anchor per cell, left half only
    a[0, ys, xs] = np.exp(v[0, ys, xs] + 0.3).astype(np.float32)
    kw = dict(prior=np.zeros(1), fit="none", cell=CELL, sigma=2.0)
    free, held = aref.fit(m, a, lam=0.0, **kw)["field"][0], aref.fit(m, a, lam=1.0, **kw)["field"][0]
    gx = W // CELL
    assert np.abs(free[:, :gx // 2 + 6] - 0.3).max() < 1e-6                 # without lambda the mean is carried as far as a tap reaches (Rg = 6 cells)
    assert (free[:, gx // 2 + 6:] == 0).all() and (held[:, gx // 2 + 6:] == 0).all()
    assert np.abs(held[:, gx // 2 + 5:]).max() < 0.02                       # six cells from the last anchors W is g[6] * sum g = 0.011 * 5: 0.3 * W / (W + 1)
    assert 0.2 < held[:, :gx // 2 - 4].min() and held.max() < 0.3           # amid the anchors W is about 2 pi sigma^2 = 25 (a quarter of it in a corner): most of the offset


def test_a_perturbed_logarithm_stays_inside_the_derived_bound():
    """the bound tests/test_gpu_anchor.py holds the device to (anchor_ref.ln_bounds), tried on the reference itself: every ln moved by up to
    one ulp either way (two apart at most) keeps s_c, ls and the field inside it; the largest deviation is printed as the yardstick"""
    m = log_map("bound", 2)
    a = np.exp(resampled(m, 37, 53) + filler.uniform("anchor.cpu.bound", (2, 37, 53), -0.3, 0.9, dtype=np.float64)).astype(np.float32)
    a[filler.unit("anchor.cpu.bound.holes", 2 * 37 * 53).reshape(2, 37, 53) < 0.3] = 0.0
    move = (filler.unit("anchor.cpu.bound.move", 2 * 37 * 53).reshape(2, 37, 53) * 3.0).astype(np.int64) - 1

    def moved(x):
        y = np.log(x)
        return np.where(move > 0, np.nextafter(y, np.inf), np.where(move < 0, np.nextafter(y, -np.inf), y))
    prior = np.array([0.2, -0.1])
    for fit in ("logmean", "none"):
        base = aref.fit(m, a, prior=prior, fit=fit, cell=8, sigma=1.5, lam=0.5)
        pert = aref.fit(m, a, prior=prior, fit=fit, cell=8, sigma=1.5, lam=0.5, log=moved)
        E = aref.ln_bounds(m, a, 8, prior=prior, fit=aref.FIT_LOGMEAN if fit == "logmean" else aref.FIT_NONE, sigma=1.5, lam=0.5)
        np.testing.assert_array_equal(base["n"], pert["n"])
        dev = {k: np.abs(base[k] - pert[k]) for k in ("s", "field")}
        dev["ls"] = np.abs(base["log_scale"] - pert["log_scale"])
        print(fit, {k: "%.3g of %.3g" % (dev[k].max(), E[k].max()) for k in dev})
        assert dev["s"].max() > 0
        for k in dev:
            assert (dev[k] <= E[k]).all(), (fit, k)
            assert E[k].max() < 1e-12                                        # and the bound is a rounding-level one


def test_lane_tree_order_is_the_headers():
    vals = filler.uniform("anchor.cpu.tree", (200,), -1.0, 1.0, dtype=np.float64)
    t = [0.0] * 64
    for p, x in enumerate(vals):
        t[p % 64] = t[p % 64] + x
    for o in (32, 16, 8, 4, 2, 1):
        for l in range(o):
            t[l] = t[l] + t[l + o]
    assert aref.lane_tree_sum(vals) == t[0] and aref.lane_tree_sum([]) == 0.0
    g = aref.taps(2.0)
    assert len(g) == 7 and g[0] == 1.0 and g[6] == math.exp(-36.0 / 8.0) and len(aref.taps(0.0)) == 1 and len(aref.taps(0.1)) == 2


def test_zero_field_changes_nothing_and_bilinear_is_exact_at_centres():
    m = log_map("frames", 2)
    ls = np.array([0.4, -0.2])
    plain = dref.reference(m, 37, 53, view=(2.5, -3.25, 41.0, 48.5), log_scale_in=ls)
    zero = aref.frames(m, 37, 53, ls, np.zeros((2, 5, 7)), 8, view=(2.5, -3.25, 41.0, 48.5))
    for k in ("D", "f32", "u16"):
        assert plain[k].tobytes() == zero[k].tobytes(), k
    F = filler.uniform("anchor.cpu.field", (1, 3, 4), -0.5, 0.5, dtype=np.float64)
    c = aref.field_at_pixels(F, 12, 16, 4)                                   # even cell: centres at x.5; the pixels either side are 1/8 from it
    assert c.shape == (1, 12, 16) and (c[0, 0, :2] == F[0, 0, 0]).all() and (c[0, -1, -2:] == F[0, -1, -1]).all()      # clamped: constant outside the outer centres
    c3 = aref.field_at_pixels(F, 9, 12, 3)                                   # odd cell: pixel 3 i + 1 IS the centre of cell i
    np.testing.assert_array_equal(c3[0, 1::3, 1::3], F[0])


def test_wrapper_parameter_rules():
    from md_rdm_amd import anchor
    assert anchor.check_params(16, 2.0, 1.0, None) is None and anchor.check_params(1, 0.0, 0.0, 0.5) is None and anchor.check_params(16, 32.0, 1.0, None) is None
    for bad, word in (((0, 2.0, 1.0, None), "cell"), ((16, -1.0, 1.0, None), "sigma"), ((16, math.nan, 1.0, None), "sigma"), ((16, math.inf, 1.0, None), "sigma"),
                      ((16, 32.5, 1.0, None), "radius"), ((16, 2.0, -0.5, None), "lambda"), ((16, 2.0, math.inf, None), "lambda"), ((16, 2.0, 1.0, 0.0), "reject"),
                      ((16, 2.0, 1.0, math.nan), "reject")):
        assert word in anchor.check_params(*bad), bad
    assert anchor.view_rows(480, 640, (9.6, 12.49, 460.8, 615.02)) == (10, 12, 470, 628)
    assert anchor.view_rows(37, 53, (2.5, -3.25, 41.0, 48.5)) == (2, 0, 37, 45) and anchor.view_rows(9, 11, (4.25, 5.125, 0.5, 0.25)) is None
    for h, w, view in ((37, 53, (2.5, -3.25, 41.0, 48.5)), (480, 640, (9.6, 12.49, 460.8, 615.02))):
        y0, x0, y1, x1 = anchor.view_rows(h, w, view)
        want = np.zeros((h, w), dtype=bool)
        want[y0:y1, x0:x1] = True
        np.testing.assert_array_equal(dref.inside_mask(h, w, view), want)
    with pytest.raises(Exception, match="MI355X only"):
        anchor.fit(np.zeros((1, 1, 128, 128)), np.zeros((1, 5, 7), dtype=np.float32))


def test_command_line_flag_rules(tmp_path):
    from md_rdm_amd import predict
    parse = predict.build_parser().parse_args
    ok = parse(["a.npy", "--out", "o", "--metric", "--native", "--anchors", "a_d.png", "--anchor_fit", "median", "--anchor_reject", "0.5", "--max_depth", "10"])
    predict.check_ply_args(ok)
    predict.check_anchor_args(ok)
    assert predict.anchor_options(ok) == {"fit": "median", "reject": 0.5, "max_depth": 10.0, "field": True}
    predict.check_anchor_args(parse(["--synthetic", "2", "--out", "o", "--metric", "--full_res", "--anchors", "a.npy", "b.npy", "--anchor_no_field"]))
    predict.check_anchor_args(parse(["a.npy", "--out", "o"]))
    for argv, word in ((["a.npy", "--out", "o", "--metric", "--native", "--anchor_cell", "8"], "need --anchors"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchor_no_field"], "need --anchors"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchor_unit", "0.001"], "need --anchors"),
                       (["a.npy", "--out", "o", "--native", "--anchors", "d.npy"], "needs --metric"),
                       (["a.npy", "--out", "o", "--metric", "--anchors", "d.npy"], "--native for file inputs"),
                       (["a.npy", "--out", "o", "--metric", "--full_res", "--anchors", "d.npy"], "--native for file inputs"),
                       (["--synthetic", "1", "--out", "o", "--metric", "--anchors", "d.npy"], "--full_res for --synthetic"),
                       (["a.npy", "b.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy"], "one file per input (got 1 files for 2 inputs)"),
                       (["--synthetic", "2", "--out", "o", "--metric", "--full_res", "--anchors", "d.npy"], "one file per input"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_cell", "0"], "cell must be >= 1"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_sigma", "-1"], "sigma must be finite"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_sigma", "40"], "radius"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_lambda", "nan"], "lambda must be finite"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_reject", "0"], "reject must be > 0"),
                       (["a.npy", "--out", "o", "--metric", "--native", "--anchors", "d.npy", "--anchor_unit", "0"], "--anchor_unit must be positive")):
        with pytest.raises(SystemExit) as e:
            predict.check_anchor_args(parse(argv))
        assert word in str(e.value), (argv, str(e.value))
    with pytest.raises(SystemExit) as e:                                    # without --ply, a view or anchors the depth range has no taker
        predict.check_ply_args(parse(["a.npy", "--out", "o", "--metric", "--native", "--max_depth", "10"]))
    assert "need --ply" in str(e.value)
    # anchor files: float32 .npy as it is, 16-bit PNG in steps of the unit; a wrong dtype is refused
    np.save(str(tmp_path / "d.npy"), np.full((1, 5, 7), 2.5, dtype=np.float32))
    assert predict.load_anchor(str(tmp_path / "d.npy"), 1e-3).shape == (5, 7)
    np.save(str(tmp_path / "e.npy"), np.zeros((5, 7)))
    with pytest.raises(SystemExit, match="float32"):
        predict.load_anchor(str(tmp_path / "e.npy"), 1e-3)
    from md_rdm_amd import viz
    steps = (filler.unit("anchor.cpu.png", 35) * 65536.0).astype(np.uint16).reshape(5, 7)
    viz.write_png16(str(tmp_path / "d.png"), steps)
    got = predict.load_anchor(str(tmp_path / "d.png"), 0.002)
    assert got.dtype == np.float32 and (got == (steps.astype(np.float64) * 0.002).astype(np.float32)).all()
    (tmp_path / "bad.png").write_bytes(b"not a png")
    with pytest.raises(SystemExit, match="not a PNG"):
        predict.load_anchor(str(tmp_path / "bad.png"), 1e-3)


def _png16(rows_with_filters, w):
    """a 16-bit greyscale PNG from (filter, bytes of the FILTERED line) pairs"""
    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    raw = b"".join(bytes([f]) + bytes(line) for f, line in rows_with_filters)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, len(rows_with_filters), 16, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b"")


def test_read_png16_undoes_every_filter(tmp_path):
    from md_rdm_amd import viz
    w = 6
    img = (filler.unit("anchor.cpu.png16", 5 * w) * 65536.0).astype(np.uint16).reshape(5, w)
    by = img.astype(">u2").view(np.uint8).reshape(5, 2 * w).astype(np.int64)
    lines = []
    for y, f in enumerate((0, 1, 2, 3, 4)):
        prev = by[y - 1] if y else np.zeros(2 * w, dtype=np.int64)
        out = []
        for i in range(2 * w):
            a, b, c = (by[y, i - 2], prev[i], prev[i - 2]) if i >= 2 else (0, prev[i], 0)
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else b if pb <= pc else c)[f]
            out.append(int(by[y, i] - pred) & 255)
        lines.append((f, out))
    (tmp_path / "f.png").write_bytes(_png16(lines, w))
    np.testing.assert_array_equal(viz.read_png16(str(tmp_path / "f.png")), img)
    viz.write_png16(str(tmp_path / "g.png"), img)
    np.testing.assert_array_equal(viz.read_png16(str(tmp_path / "g.png")), img)
    rgb = b"\x89PNG\r\n\x1a\n" + _png16([(0, [0] * 6)], 1)[8:].replace(struct.pack(">IIBBBBB", 1, 1, 16, 0, 0, 0, 0), struct.pack(">IIBBBBB", 1, 1, 16, 2, 0, 0, 0))
    (tmp_path / "rgb.png").write_bytes(rgb)
    with pytest.raises(ValueError, match="16-bit greyscale"):
        viz.read_png16(str(tmp_path / "rgb.png"))


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    # declared == bound == exported, with the header's types: test_abi_cpu.py
    assert set(_lib.symbols("rdm_anchor.h")) == {"rdm_depth_anchor_cells", "rdm_depth_anchor_field", "rdm_depth_frames_corrected"}
    hip_h, depth_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read(), open(os.path.join(ROOT, "include", "rdm_depth.h")).read()
    assert "anchor" not in hip_h and "anchor" not in depth_h
    consts = dict(re.findall(r"#define RDM_ANCHOR_(\w+) (\d+)", open(HEADER).read()))
    assert consts == {"FIT_NONE": "0", "FIT_LOGMEAN": "1", "MAX_CELLS": str(_lib.ANCHOR_MAX_CELLS), "MAX_RADIUS": str(_lib.ANCHOR_MAX_RADIUS)}
    assert (_lib.ANCHOR_FIT["none"], _lib.ANCHOR_FIT["logmean"]) == (aref.FIT_NONE, aref.FIT_LOGMEAN) and (aref.MAX_CELLS, aref.MAX_RADIUS) == (5120, 96)
    assert 60 * 80 <= _lib.ANCHOR_MAX_CELLS                                                          # 480x640 at cell 8 fits
