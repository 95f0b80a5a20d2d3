"""-m gpu: rdm_eval_standard_f64 (csrc/evalstd.hip, include/rdm_eval.h) through the C ABI, metrics.StandardMetrics, harness.evaluate and the
evaluate command under the standard protocol, against the float64 numpy restatement tests/evalstd_ref.py (oracle resize, math.fsum sums).

Which bound holds where (every comparison prints its observed figure before it asserts):
* columns 0 (n) and 14 (clamped pixels): EQUAL.  Column 12 under median alignment (an order statistic of the input): EQUAL bit for bit.
* columns 1-3: EQUAL, on inputs on which the restatement reports every pixel's max-ratio at least 1e-9 (relative) away from 1.25^k; the
  seeds below were searched on the CPU for that and the test asserts it of the restatement before it looks at the device.
* columns 11 and 13 (and 12 under log-mean alignment): rtol 1e-13, the project's bound for a quantity that passes through the device exp
  (tests/test_gpu_evalmetrics.py); pred_out likewise.
* columns 4-10: rtol 1e-11, the project's bound for metric sums in another order, on rows whose mean |q-d|/d is at least 1e-2 (asserted of
  every row of the shape cases).  A row below that (a perfect prediction; one valid pixel under an alignment, where q = d) is held to
  atol n * 2^-50 * max_depth instead: q = s * exp(ln d) is d within a few roundings.  Every call of compare() names the rows it expects on
  that path (none in the shape cases) and compare() asserts that exactly those take it, so a change of the inputs cannot move a row from
  one bound to the other unseen.  Column 8 is the one SIGNED sum; log-mean alignment without clamping would make it zero by construction and
  an rtol meaningless, so the inputs clamp (see log_map) and compare() asserts of every row that |sum g| is at least 1e-3 of sum |g|.
Depth range of the tests: (0.25, 8) on data spanning [0.1, 12], so both ends of the range exclude pixels and the prediction clamps at both."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import evalstd_ref as ref
import stream_probe as sp
from conftest import ROOT
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
LO, HI = 0.25, 8.0
ALIGNS = ("none", "median", "logmean")
SHAPES = [(3, 128, 128), (3, 37, 53), (3, 226, 226), (2, 480, 640)]
SEEDS = {(3, 128, 128): 1, (3, 37, 53): 1, (3, 226, 226): 1, (2, 480, 640): 1}     # searched on the CPU: see the module docstring


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def log_map(tag, B):
    """over [-2.5, 5.5) with a long upper tail: wide enough to clamp at both ends of (LO, HI) after an alignment too, and more at the upper end,
    which keeps column 8, the signed sum, away from cancelling"""
    return (-2.5 + 8.0 * filler.unit("evalstd.map/%s/%d" % (tag, B), B * 128 * 128) ** 2).reshape(B, 1, 128, 128)


def make_inputs(B, h, w, seed):
    """float32 depth: sample 0 all valid; the last sample about half holes, millimetre-quantised (runs of equal keys for the radix select) with
    NaN, +-inf, negative, == LO and == HI entries; a middle sample (B = 3) raw over [0.1, 12], so the range itself excludes pixels"""
    tag = "%d/%dx%dx%d" % (seed, B, h, w)
    d = filler.log_uniform("evalstd.d/" + tag, (B, 1, h, w), 0.1, 12.0)
    d[0] = filler.log_uniform("evalstd.d0/" + tag, (1, h, w), 0.3, 7.5)
    last = np.round(d[B - 1].astype(np.float64) * 1000.0) / 1000.0
    last[filler.unit("evalstd.hole/" + tag, h * w).reshape(1, h, w) < 0.5] = 0.0
    d[B - 1] = last.astype(np.float32)
    d[B - 1, 0, 1, :6] = [np.nan, np.inf, -np.inf, -2.0, LO, HI]
    return d, log_map(tag, B)


@functools.lru_cache(maxsize=None)
def shape_case(B, h, w):
    d, m = make_inputs(B, h, w, SEEDS[(B, h, w)])
    return d, m, {a: ref.reference(m, d, a, LO, HI) for a in ALIGNS}


def raw(dev, m, d, align="median", lo=LO, hi=HI, crop=None, want_out=True, rows=None, ws_bytes=None):
    """the entry point itself -> (status, rows, pred_out or None); outputs pre-filled with a sentinel"""
    import ctypes as C
    from md_rdm_amd import _lib
    L = _lib.lib()
    m = m if torch.is_tensor(m) else T(m, dev)
    d = d if torch.is_tensor(d) else T(d, dev)
    B, _, h, w = d.shape
    if rows is None:
        rows = torch.full((B, 16), -777.0, dtype=torch.float64, device=dev)
    out = torch.full((B, 1, h, w), -777.0, dtype=torch.float64, device=dev) if want_out else None
    need = L.rdm_eval_standard_workspace_bytes(B, h, w)
    assert need == B * h * w * 8
    ws = torch.empty(B * h * w, dtype=torch.float64, device=dev)
    c = (C.c_int32 * 4)(*crop) if crop is not None else None
    rc = L.rdm_eval_standard_f64(_lib.ptr(m), _lib.ptr(d), int(d.dtype == torch.float64), B, h, w, _lib.EVAL_ALIGN[align], lo, hi, c, _lib.ptr(rows), _lib.ptr(out),
                                 _lib.ptr(ws), need if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, rows, out


def compare(got, r, align, what, hi=HI, atol_rows=()):
    """device rows against the restatement's dict, by the bounds of the module docstring; atol_rows: the samples whose mean |q-d|/d is below
    1e-2 and which are therefore held to the absolute bound - exactly these, every other row is held to rtol 1e-11"""
    want = r["rows"]
    assert got.shape == want.shape and not (got == -777.0).any(), what
    np.testing.assert_array_equal(got[:, [0, 14, 15]], want[:, [0, 14, 15]], err_msg=what)
    for b in range(want.shape[0]):
        n = want[b, 0]
        if n == 0 or np.isnan(want[b, 1]):
            np.testing.assert_array_equal(got[b], want[b], err_msg="%s sample %d" % (what, b))
            continue
        print("%s sample %d: n %d, margin %.3e, mean abs_rel %.3e, |sum g| / sum |g| %.3e, clamped low %d high %d" % (
            what, b, n, r["margin"][b], r["abs_rel"][b], abs(want[b, 8]) / max(r["g_abs"][b], 1e-300), r["sp_low"][b], r["sp_high"][b]))
        assert r["margin"][b] >= 1e-9, "the restatement itself has a pixel within 1e-9 of a delta threshold: pick another seed"
        np.testing.assert_array_equal(got[b, 1:4], want[b, 1:4])
        rel = np.abs(got[b, [11, 13]] / want[b, [11, 13]] - 1) if align != "none" else np.zeros(2)
        print("    columns 11, 13: rel %s" % rel)
        if align == "median":
            assert got[b, 12] == want[b, 12]                                     # bit for bit
        else:
            np.testing.assert_allclose(got[b, 12], want[b, 12], rtol=1e-13, atol=0)
        np.testing.assert_allclose(got[b, [11, 13]], want[b, [11, 13]], rtol=1e-13, atol=0)
        plain = r["abs_rel"][b] >= 1e-2
        assert plain == (b not in atol_rows), "sample %d: mean abs_rel %.3e is not on the side of 1e-2 this case states" % (b, r["abs_rel"][b])
        with np.errstate(divide="ignore", invalid="ignore"):
            print("    columns 4-10: rel %s" % np.abs(got[b, 4:11] / want[b, 4:11] - 1))
        if plain:
            assert abs(want[b, 8]) >= 1e-3 * r["g_abs"][b], "column 8 cancels on this input: an rtol says nothing about it"
            np.testing.assert_allclose(got[b, 4:11], want[b, 4:11], rtol=1e-11, atol=0)
        else:
            np.testing.assert_allclose(got[b, 4:11], want[b, 4:11], rtol=0, atol=n * 2.0 ** -50 * hi)


def compare_out(out, r, what):
    got = out.cpu().numpy()
    assert not (got == -777.0).any()
    with np.errstate(invalid="ignore"):
        print("%s pred_out: max rel %.3e" % (what, np.nanmax(np.abs(got / r["q"] - 1))))
    np.testing.assert_allclose(got, r["q"], rtol=1e-13, atol=0, equal_nan=True)


# ---- the shapes: identity, fewer pixels than one pass, the loader's size, many pixels per thread ---------------------------------------------
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("B,h,w", SHAPES)
def test_shapes_against_the_restatement(dev, B, h, w, align):
    d, m, refs = shape_case(B, h, w)
    r = refs[align]
    valid = r["rows"][:, 0]
    assert valid[0] == h * w and 0.25 * h * w < valid[B - 1] < 0.6 * h * w and not r["valid"][B - 1, 0, 1, :6].any()
    assert (r["sp_low"] > 0).all() and (r["sp_high"] > 0).all()                    # the prediction clamps at both ends in every sample
    dq = d[B - 1][r["valid"][B - 1]]
    assert len(np.unique(dq)) < 0.9 * len(dq) or h * w < 4096                      # ties among the millimetre-quantised depths
    rc, rows32, out32 = raw(dev, m, d, align)
    assert rc == 0
    what = "%dx%dx%d %s" % (B, h, w, align)
    compare(rows32.cpu().numpy(), r, align, what)
    compare_out(out32, r, what)
    rc, rows64, out64 = raw(dev, m, d.astype(np.float64), align)                   # the same values as float64: bit for bit
    assert rc == 0 and sp.same_bits(rows32, rows64) and sp.same_bits(out32, out64)


# ---- few valid pixels, parity of the count, ties across the median, genuine float64 ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern_case():
    h, w = 37, 53
    base = filler.log_uniform("evalstd.pat", (1, 1, h, w), 0.3, 7.5).astype(np.float64)
    one, two, none = np.zeros_like(base), np.zeros_like(base), np.zeros_like(base)
    one[0, 0, 20, 31] = base[0, 0, 20, 31]
    two[0, 0, 3, 4], two[0, 0, 30, 50] = base[0, 0, 3, 4], base[0, 0, 30, 50]
    none[0, 0, 0, 0], none[0, 0, 5, 5] = np.nan, 9.0
    tied = np.round(base * 4.0) / 4.0                                              # quarter-metre steps: about 30 distinct values over 1961 pixels
    tied[tied <= LO] = 0.5
    odd, even = tied.copy(), tied.copy()
    even[0, 0, 0, 0] = 0.0
    fine = base * (1.0 + 2.0 ** -30)                                               # bits below float32's last place
    d = np.concatenate([one, two, none, odd, even, fine])
    assert ((odd > LO) & (odd < HI)).sum() % 2 == 1 and ((even > LO) & (even < HI)).sum() % 2 == 0
    assert (fine.astype(np.float32).astype(np.float64) != fine).any()
    m = log_map("pat", 6)
    return d, m, {a: ref.reference(m, d, a, LO, HI) for a in ALIGNS}


@pytest.mark.parametrize("align", ALIGNS)
def test_valid_pixel_patterns(dev, align):
    d, m, refs = pattern_case()
    r = refs[align]
    assert r["rows"][:3, 0].tolist() == [1, 2, 0] and not r["rows"][2].any()
    if align == "median":                                                          # the medians of the tied samples sit inside runs of equal keys
        for b in (3, 4):
            dv = d[b][r["valid"][b]]
            assert (dv == r["rows"][b, 12]).sum() > 10 or r["rows"][b, 12] not in dv
            assert r["rows"][b, 12] == np.median(dv)
    rc, rows, out = raw(dev, m, d, align)
    assert rc == 0
    compare(rows.cpu().numpy(), r, align, "patterns %s" % align, atol_rows=() if align == "none" else (0,))    # one valid pixel, aligned: q = d
    compare_out(out, r, "patterns %s" % align)


def test_an_even_count_whose_middle_pair_straddles_two_values(dev):
    """the upper middle element is NOT in the selected key's run: the extra minimum pass of the select"""
    h, w = 9, 7
    d = np.zeros((2, 1, h, w))
    d[0, 0, 0, :4] = [1.0, 3.0, 2.0, 5.0]                                           # median (2 + 3) / 2
    d[1, 0, 2, :6] = [4.0, 1.5, 1.5, 4.0, 4.0, 1.5]                                 # median (1.5 + 4) / 2, both in runs
    m = log_map("straddle", 2)
    r = ref.reference(m, d, "median", LO, HI)
    assert r["rows"][:, 12].tolist() == [2.5, 2.75]
    rc, rows, out = raw(dev, m, d, "median")
    assert rc == 0
    compare(rows.cpu().numpy(), r, "median", "straddle")
    compare_out(out, r, "straddle")


@pytest.mark.parametrize("align", ALIGNS)
def test_a_prediction_equal_to_the_depth(dev, align):
    d = filler.log_uniform("evalstd.perfect", (2, 1, 128, 128), 0.3, 7.5).astype(np.float64)
    m = np.log(d)
    d[:, :, ::5, ::3] = 0.0
    r = ref.reference(m, d, align, LO, HI)
    assert (r["abs_rel"] < 1e-14).all()
    rc, rows, _ = raw(dev, m, d, align)
    got = rows.cpu().numpy()
    assert rc == 0 and (got[:, 1:4] == got[:, :1]).all()
    n = got[:, :1]
    print("perfect prediction, %s: sums %s" % (align, got[:, 4:11]))
    np.testing.assert_array_equal(got[:, 0], r["rows"][:, 0])
    np.testing.assert_allclose(got[:, 4:11], r["rows"][:, 4:11], rtol=0, atol=float(n.max()) * 2.0 ** -50 * HI)
    np.testing.assert_allclose(got[:, 11], 1.0, rtol=1e-13)


# ---- crop -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [(5, 7, 30, 50), (12, 0, 13, 53), (0, 0, 37, 53), (36, 52, 37, 53)])
def test_crop(dev, crop):
    d, m, _ = shape_case(3, 37, 53)
    d = d.copy()
    d[:, 0, 36, 52] = 3.0
    for align in ("median", "none"):
        r = ref.reference(m, d, align, LO, HI, crop)
        assert (r["rows"][:, 0] == r["valid"][:, :, crop[0]:crop[2], crop[1]:crop[3]].sum(axis=(1, 2, 3))).all() and (r["rows"][:, 0] > 0).all()
        rc, rows, out = raw(dev, m, d, align, crop=crop)
        assert rc == 0
        one_pixel_aligned = crop == (36, 52, 37, 53) and align == "median"                 # q = d in all three samples
        compare(rows.cpu().numpy(), r, align, "crop %s %s" % (crop, align), atol_rows=(0, 1, 2) if one_pixel_aligned else ())
        compare_out(out, r, "crop %s" % (crop,))                                   # the whole frame, outside the crop too
    if crop == (0, 0, 37, 53):
        assert sp.same_bits(rows, raw(dev, m, d, "none")[1])


# ---- a NaN in the map -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,y,x", [(128, 128, 60, 60), (37, 53, 17, 24)])
def test_nan_in_the_map(dev, h, w, y, x):
    """map pixel (60, 60): at 128x128 it is frame pixel (60, 60) alone; at 37x53 its cubic taps reach the frame pixels around (17, 24)"""
    d, m, _ = shape_case(3, h, w)
    d, m = d.copy(), m.copy()
    d[:, 0, y, x] = 2.0                                                            # valid in every sample
    bad = m.copy()
    bad[1, 0, 60, 60] = np.nan
    r = ref.reference(bad, d, "median", LO, HI)
    assert np.isnan(r["rows"][1, 1:14]).all() and r["rows"][1, 0] > 0 and not np.isnan(r["rows"][[0, 2]]).any()
    for align in ALIGNS:
        rc, rows, out = raw(dev, bad, d, align)
        got = rows.cpu().numpy()
        assert rc == 0 and got[1, 0] == r["rows"][1, 0] and np.isnan(got[1, 1:14]).all() and (got[1, 14:] == 0).all()
        assert sp.same_bits(rows[[0, 2]], raw(dev, m, d, align)[1][[0, 2]])         # the other samples do not see it
    compare_out(out, ref.reference(bad, d, "logmean", LO, HI), "nan row")            # that sample's pred_out is formed with s = 1
    hole = d.copy()
    r0, r1, c0, c1 = (y, y + 1, x, x + 1) if h == 128 else (y - 4, y + 5, x - 4, x + 5)
    hole[1, 0, r0:r1, c0:c1] = 0.0
    p = ref.prediction(bad, h, w)[1, 0]
    assert np.isnan(p).any() and not np.isnan(p[ref.valid_mask(hole, LO, HI)[1, 0]]).any()      # every NaN of the resized map lies in the hole
    for align in ALIGNS:
        rc, rows, _ = raw(dev, bad, hole, align)
        rc2, rows2, _ = raw(dev, m, hole, align)
        assert rc == 0 and rc2 == 0 and not torch.isnan(rows).any() and sp.same_bits(rows, rows2), align


# ---- determinism, batch independence, the optional output ------------------------------------------------------------------------------------
def test_repeated_alone_and_without_pred_out(dev):
    d, m, _ = shape_case(3, 226, 226)
    dt, mt = T(d, dev), T(m, dev)
    for align in ALIGNS:
        rc, rows, out = raw(dev, mt, dt, align)
        rc2, rows2, out2 = raw(dev, mt, dt, align)
        assert rc == 0 and rc2 == 0 and sp.same_bits(rows, rows2) and sp.same_bits(out, out2)
        rc3, rows3, out3 = raw(dev, mt, dt, align, want_out=False)
        assert rc3 == 0 and out3 is None and sp.same_bits(rows3, rows)
        for b in range(3):
            rc1, r1, o1 = raw(dev, mt[b:b + 1].contiguous(), dt[b:b + 1].contiguous(), align)
            assert rc1 == 0 and sp.same_bits(r1[0], rows[b]) and sp.same_bits(o1[0], out[b]), (align, b)


def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    d, m, _ = shape_case(3, 37, 53)
    dt, mt = T(d, dev), T(m, dev)
    rows = torch.full((3, 16), -777.0, dtype=torch.float64, device=dev)
    for kw, word in ((dict(align="median", lo=-1.0), b"min_depth"), (dict(lo=3.0, hi=3.0), b"min_depth"), (dict(crop=(4, 4, 4, 9)), b"crop"),
                     (dict(crop=(0, 0, 38, 53)), b"crop"), (dict(crop=(0, 50, 37, 54)), b"crop"), (dict(ws_bytes=3 * 37 * 53 * 8 - 8), b"workspace")):
        rc, _, out = raw(dev, mt, dt, rows=rows, **kw)
        assert rc == -1 and word in L.rdm_last_error_string(), (kw, L.rdm_last_error_string())
        assert bool((out == -777.0).all())
    P, st = _lib.ptr, _lib.stream()
    ws = torch.empty(3 * 37 * 53, dtype=torch.float64, device=dev)
    good = [P(mt), P(dt), 0, 3, 37, 53, 1, LO, HI, None, P(rows), None, P(ws), ws.numel() * 8, st]
    for pos, val, word in ((0, None, b"NULL"), (1, None, b"NULL"), (10, None, b"NULL"), (12, None, b"NULL"), (3, 0, b"batch"), (4, -37, b"batch"), (5, 0, b"batch"),
                           (6, 3, b"align"), (6, -1, b"align")):
        args = list(good)
        args[pos] = val
        assert L.rdm_eval_standard_f64(*args) == -1 and word in L.rdm_last_error_string(), (pos, val, L.rdm_last_error_string())
    torch.cuda.synchronize()
    assert bool((rows == -777.0).all())


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -----------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib
    from md_rdm_amd.metrics import StandardMetrics
    d, m, _ = shape_case(3, 37, 53)
    sm = StandardMetrics(min_depth=LO, max_depth=HI)
    ins = dict(m=T(m, dev), d=T(d, dev))
    scratch = dict(rows=torch.empty(3, 16, dtype=torch.float64, device=dev), out=torch.empty(3, 1, 37, 53, dtype=torch.float64, device=dev),
                   ws=torch.empty(3 * 37 * 53, dtype=torch.float64, device=dev))

    def call(b, st):
        _lib.check(_lib.lib().rdm_eval_standard_f64(_lib.ptr(b["m"]), _lib.ptr(b["d"]), 0, 3, 37, 53, 1, LO, HI, None, _lib.ptr(b["rows"]), _lib.ptr(b["out"]),
                                                    _lib.ptr(b["ws"]), b["ws"].numel() * 8, st))
        return dict(wrapped=sm.compute_rows(b["m"], b["d"]))                       # the product wrapper resolves the caller's stream itself
    return sp.Case(ins, call, outs=("rows", "out"), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    _, _, refs = shape_case(3, 37, 53)
    compare(got["rows"].cpu().numpy(), refs["median"], "median", "stream")
    assert sp.same_bits(got["wrapped"], got["rows"])


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- harness.evaluate and the command --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


def batches_of(x, y, bs):
    return [(x[i:i + bs], y[i:i + bs]) for i in range(0, x.shape[0], bs)]


def test_harness_evaluate_standard(dev, model):
    from md_rdm_amd import evaluate, harness, viz
    from md_rdm_amd.metrics import StandardMetrics
    xs, ys = evaluate.synthetic_samples(5, 226, 226)
    x, y = T(xs, dev), T(ys, dev)
    sm = StandardMetrics()
    got_rows = []
    res, maps = harness.evaluate(model, batches_of(x, y, 5), sm, return_maps=True, rows_out=got_rows, rows_max=2)
    assert res["n"] == 5 and res["skipped"] == 0 and list(res)[:len(sm.names)] == sm.names
    for bs in (1, 2):
        assert harness.evaluate(model, batches_of(x, y, bs), sm) == res, bs
    rows = sm.compute_rows(maps, y).cpu().numpy()
    r = ref.reference(maps.cpu().numpy(), ys, "median")
    compare(rows, r, "median", "evaluate")
    vals = np.array(ref.values_from_rows(rows))
    for k, name in enumerate(sm.names):
        print("%s: evaluate %.15g, mean of the restatement's values %.15g" % (name, res[name], vals[:, k].mean()))
        np.testing.assert_allclose(res[name], vals[:, k].mean(), rtol=1e-14, atol=0)
    q = torch.empty(2, 1, 226, 226, dtype=torch.float64, device=dev)
    sm.compute_rows(maps[:2], y[:2], pred_out=q)
    want = viz.comparison_rows(x[:2], y[:2], q).cpu().numpy()                      # input | depth | q over one colour range
    assert len(got_rows) == 2 and want.shape == (2, 226, 678, 3)
    np.testing.assert_array_equal(np.stack(got_rows), want)
    # samples without a valid pixel are left out and counted; all of them: an error
    y2 = y.clone()
    y2[3] = 0.0
    res2 = harness.evaluate(model, batches_of(x, y2, 2), sm)
    assert res2["n"] == 4 and res2["skipped"] == 1
    keep = [0, 1, 2, 4]
    for k, name in enumerate(sm.names):
        np.testing.assert_allclose(res2[name], vals[keep, k].mean(), rtol=1e-14, atol=0)
    with pytest.raises(ValueError, match="valid pixel"):
        harness.evaluate(model, batches_of(x, torch.zeros_like(y), 5), sm)
    with pytest.raises(ValueError, match="exp_pred"):
        harness.evaluate(model, batches_of(x, y, 5), sm, exp_pred=True)


def run_cli(tmp_path, name, extra):
    out = tmp_path / name
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "md_rdm_amd.evaluate", "--synthetic", "4", "--out", str(out)] + extra, cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(out.read_text()), r.stdout


def test_cli_standard_protocol(dev, model, tmp_path):
    from md_rdm_amd import evaluate, harness
    from md_rdm_amd.metrics import StandardMetrics
    rec, stdout = run_cli(tmp_path, "r.json", ["--protocol", "standard"])
    assert (rec["protocol"], rec["align"], rec["min_depth"], rec["max_depth"], rec["crop"], rec["skipped"], rec["n"]) == ("standard", "median", 1e-3, 10.0, None, 0, 4)
    assert list(rec["metrics"]) == list(ref.NAMES) and "skipped 0" in stdout
    xs, ys = evaluate.synthetic_samples(4, 226, 226)
    res = harness.evaluate(model, batches_of(T(xs, dev), T(ys, dev), 8), StandardMetrics())
    for name in ref.NAMES:
        assert rec["metrics"][name] == res[name] and ("%s %.6f" % (name, res[name])) in stdout, name


def test_cli_reference_protocol_writes_what_it_wrote(dev, model, tmp_path):
    from md_rdm_amd import evaluate, harness
    rec, _ = run_cli(tmp_path, "r.json", ["--protocol", "reference"])
    assert set(rec) == {"split", "n", "batch_size", "precision", "size", "exp_pred", "relative_decoders", "checkpoint", "world", "metrics", "protocol"}
    assert rec["protocol"] == "reference" and rec["n"] == 4 and rec["exp_pred"] is False
    xs, ys = evaluate.synthetic_samples(4, 226, 226)
    res = harness.evaluate(model, batches_of(T(xs, dev), T(ys, dev), 8), evaluate.DEFAULT_METRICS)
    assert "skipped" not in res and rec["metrics"] == {k: res[k] for k in evaluate.DEFAULT_METRICS}
