"""The standard evaluation protocol without a GPU: the command's new flags and their errors, StandardMetrics.values_from_rows on hand-made
rows, the numpy restatement (tests/evalstd_ref.py) against numpy's median and against the protocol's invariants, and the C-ABI boundary of
include/rdm_eval.h (declared == bound == exported; every refusal is a status code before the launch)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import evalstd_ref as ref
from conftest import ROOT
from md_rdm_amd import filler

HEADER = os.path.join(ROOT, "include", "rdm_eval.h")


# ---- the command ---------------------------------------------------------------------------------------------------------------------------
def test_new_flags_and_defaults():
    from md_rdm_amd import evaluate
    P = evaluate.build_parser()
    a = P.parse_args([])
    assert (a.protocol, a.align, a.min_depth, a.max_depth, a.crop) == ("reference", "median", 1e-3, 10.0, None)
    assert a.metrics == evaluate.DEFAULT_METRICS                                  # the parse-time default stays the reference's list
    a = P.parse_args(["--protocol", "standard", "--align", "logmean", "--min_depth", "0.5", "--max_depth", "80", "--crop", "45", "41", "471", "601"])
    assert (a.protocol, a.align, a.min_depth, a.max_depth, a.crop) == ("standard", "logmean", 0.5, 80.0, [45, 41, 471, 601])
    for argv in (["--protocol", "eigen"], ["--align", "mean"], ["--crop", "1", "2", "3"]):
        with pytest.raises(SystemExit):
            P.parse_args(argv)
    text = P.format_help()
    assert "--protocol {reference,standard}" in text and "--crop Y0 X0 Y1 X1" in text and "--align {none,median,logmean}" in text


def test_make_computer_picks_the_protocol():
    from md_rdm_amd import evaluate
    from md_rdm_amd.metrics import MetricComputation, StandardMetrics
    P = evaluate.build_parser()
    mc = evaluate.make_computer(P.parse_args([]))
    assert isinstance(mc, MetricComputation) and mc.names == evaluate.DEFAULT_METRICS
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard"]))          # --metrics left at its default: the standard list
    assert isinstance(sm, StandardMetrics) and sm.names == list(ref.NAMES) and (sm.align, sm.min_depth, sm.max_depth, sm.crop) == ("median", 1e-3, 10.0, None)
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard", "--metrics", "silog", "rmse", "--align", "none", "--crop", "2", "3", "200", "226", "--max_depth", "80"]))
    assert sm.names == ["silog", "rmse"] and (sm.align, sm.max_depth, sm.crop) == ("none", 80.0, (2, 3, 200, 226))


@pytest.mark.parametrize("argv,word", [
    (["--protocol", "standard", "--exp_pred"], "--exp_pred belongs to --protocol reference"),
    (["--protocol", "standard", "--metrics", "mse"], "not built in the standard protocol"),
    (["--protocol", "standard", "--metrics", "absrel"], "abs_rel"),                                   # the message lists the available names
    (["--protocol", "standard", "--min_depth", "3", "--max_depth", "3"], "min_depth < max_depth"),
    (["--protocol", "standard", "--min_depth", "-1"], "min_depth < max_depth"),
    (["--protocol", "standard", "--crop", "10", "10", "10", "20"], "--crop"),
    (["--protocol", "standard", "--crop", "0", "0", "227", "226"], "--crop"),
    (["--metrics", "silog"], "is not built"),                                                         # the reference protocol has no silog
])
def test_flag_errors_come_before_the_gpu(argv, word):
    from md_rdm_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--synthetic", "2"] + argv)
    assert word in str(e.value) and "no GPU" not in str(e.value), e.value


# ---- StandardMetrics ------------------------------------------------------------------------------------------------------------------------
def test_standard_metrics_surface():
    from md_rdm_amd.metrics import StandardMetrics
    sm = StandardMetrics()
    assert sm.names == list(ref.NAMES) and tuple(StandardMetrics.available) == ref.NAMES
    with pytest.raises(KeyError) as e:
        StandardMetrics(["delta1", "mse"])
    assert "mse" in str(e.value) and all(n in str(e.value) for n in ref.NAMES)
    for kw in (dict(align="mean"), dict(min_depth=2.0, max_depth=1.0), dict(min_depth=-0.1), dict(crop=(0, 0, 0, 5)), dict(crop=(3, 0, 2, 5)), dict(crop=(0, 0, 5))):
        with pytest.raises(ValueError):
            StandardMetrics(**kw)
    doc = " ".join(StandardMetrics.__doc__.split())
    assert "TRUE root mean square" in doc and "not the reference's metric of the same name" in doc
    import torch
    from md_rdm_amd import _lib
    with pytest.raises(_lib.RdmError):                                              # no CPU fallback
        sm.compute_rows(torch.zeros(1, 1, 128, 128, dtype=torch.float64), torch.ones(1, 1, 8, 8))


def test_values_from_rows_on_hand_made_rows():
    from md_rdm_amd.metrics import StandardMetrics
    sm = StandardMetrics()
    rows = np.zeros((4, 16))
    rows[0] = [8, 2, 4, 8, 1.0, 0.5, 32.0, 2.0, 2.0, 0.25, 4.0, 1.5, 3.0, 2.0, 1, 0]
    rows[2] = [4, 4, 4, 4, 0.4, 0.04, 0.16, 1.0, 2.0 + 1e-9, 0.2, 0.8, 0.75, 1.5, 2.0, 0, 0]    # mean g^2 < (mean g)^2 by rounding: silog clamps at 0
    rows[3] = [5] + [np.nan] * 13 + [0, 0]
    vals = sm.values_from_rows(rows)
    assert vals[1] is None                                                                     # n = 0: skipped
    v = dict(zip(sm.names, vals[0]))
    assert v == dict(delta1=0.25, delta2=0.5, delta3=1.0, abs_rel=0.125, sq_rel=0.0625, rmse=2.0, rmse_log=0.5, silog=100 * np.sqrt(0.25 - 0.0625), log10=0.03125, mae=0.5,
                     scale=1.5)
    v = dict(zip(sm.names, vals[2]))
    assert v["silog"] == 0.0 and v["rmse_log"] == 0.5 and v["rmse"] == 0.2
    assert all(np.isnan(x) for x in vals[3])
    import torch
    assert sm.values_from_rows(torch.from_numpy(rows[:3])) == vals[:3]
    assert StandardMetrics(["scale", "delta2"]).values_from_rows(rows[:1]) == [[1.5, 0.5]]      # a subset, in the caller's order
    np.testing.assert_array_equal(np.array(ref.values_from_rows(rows[[0, 2]])), np.array([vals[0], vals[2]]))
    assert ref.values_from_rows(rows)[1] is None


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 10, 101, 1000])
def test_restatement_median_is_numpys(n):
    a = filler.log_uniform("evalstd.med/%d" % n, (n,), 0.3, 9.0).astype(np.float64)
    assert ref.median(a) == float(np.median(a))
    q = np.round(a * 4) / 4                                                                    # heavy ties, across the middle as well
    assert ref.median(q) == float(np.median(q))
    assert ref.median(np.full(n, 2.5)) == 2.5


def small_case(h, w, tag="a"):
    d = filler.log_uniform("evalstd.cpu.d/%s/%dx%d" % (tag, h, w), (2, 1, h, w), 0.3, 12.0).astype(np.float64)
    d[:, :, ::3, ::4] = 0.0
    m = filler.uniform("evalstd.cpu.m/%s/%dx%d" % (tag, h, w), (2, 1, 128, 128), -1.0, 2.0, dtype=np.float64)
    return m, d


@pytest.mark.parametrize("h,w", [(128, 128), (37, 53)])
def test_a_constant_added_to_the_map_changes_only_the_scale(h, w):
    m, d = small_case(h, w)
    shift = 0.625
    for align in ("median", "logmean"):
        a, b = ref.reference(m, d, align), ref.reference(m + shift, d, align)
        np.testing.assert_array_equal(a["rows"][:, :4], b["rows"][:, :4])
        va, vb = np.array(ref.values_from_rows(a["rows"])), np.array(ref.values_from_rows(b["rows"]))
        np.testing.assert_allclose(vb[:, :-1], va[:, :-1], rtol=1e-12, atol=0)
        np.testing.assert_allclose(vb[:, -1], va[:, -1] * np.exp(-shift), rtol=1e-12, atol=0)
    a, b = ref.reference(m, d, "none"), ref.reference(m + shift, d, "none")
    va, vb = np.array(ref.values_from_rows(a["rows"])), np.array(ref.values_from_rows(b["rows"]))
    assert (va[:, -1] == 1.0).all() and (vb[:, -1] == 1.0).all()
    assert (np.abs(vb[:, 3:-1] / va[:, 3:-1] - 1) > 1e-3).all()                                  # without alignment the errors move


@pytest.mark.parametrize("align", ["none", "median", "logmean"])
def test_a_prediction_equal_to_the_depth_has_no_error(align):
    _, d = small_case(128, 128, "perfect")
    d = np.maximum(d, 0.0)
    with np.errstate(divide="ignore"):
        m = np.where(d > 0, np.log(d), 0.25)                                                    # the holes hold anything
    r = ref.reference(m, d, align)
    n = r["rows"][:, 0]
    assert (n == ((d > 1e-3) & (d < 10.0)).sum(axis=(1, 2, 3))).all() and (n > 0).all()
    v = np.array(ref.values_from_rows(r["rows"]))
    assert (v[:, :3] == 1.0).all()
    assert np.abs(v[:, 3:10]).max() < 1e-14, v                                                  # exp(log d) is d within a rounding or two
    np.testing.assert_allclose(v[:, 10], 1.0, rtol=1e-15)


def test_restatement_masks_and_special_rows():
    m, d = small_case(37, 53, "mask")
    d[0, 0, 5, 5:11] = [np.nan, np.inf, -np.inf, -2.0, 1e-3, 10.0]                              # all invalid: == min_depth and == max_depth too
    base = ref.valid_mask(d, 1e-3, 10.0)
    assert not base[0, 0, 5, 5:11].any() and base.sum() == ((d > 1e-3) & (d < 10.0)).sum()
    c = ref.valid_mask(d, 1e-3, 10.0, (4, 7, 5, 40))
    assert c.sum() == base[:, :, 4:5, 7:40].sum() and not c[:, :, 5:].any()
    none = ref.reference(m, np.zeros_like(d))
    assert not none["rows"].any() and np.isinf(none["margin"]).all()
    np.testing.assert_array_equal(none["q"], np.clip(none["p"], 1e-3, 10.0))                    # s = 1 there
    m2 = m.copy()
    m2[1, 0, 60, 60] = np.nan
    r = ref.reference(m2, d)
    assert r["rows"][0, 1] == ref.reference(m, d)["rows"][0, 1]
    assert r["rows"][1, 0] > 0 and np.isnan(r["rows"][1, 1:14]).all() and (r["rows"][1, 14:] == 0).all()


# ---- the C ABI of include/rdm_eval.h --------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    names = set(_lib.symbols("rdm_eval.h"))                # declared == bound == exported, with the header's types: test_abi_cpu.py
    assert names == {"rdm_eval_standard_workspace_bytes", "rdm_eval_standard_f64"}
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    for name in names:
        assert name not in hip_h                                                                # rdm_hip.h keeps its declaration set
    hdr = open(HEADER).read()
    assert '#include "rdm_hip.h"' in hdr
    assert {k: int(re.search(r"#define RDM_EVAL_ALIGN_%s (\d)" % k.upper(), hdr).group(1)) for k in _lib.EVAL_ALIGN} == _lib.EVAL_ALIGN


def test_workspace_bytes_and_argument_errors_are_status_codes():
    """every refusal happens before the launch: callable without a GPU"""
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    W = L.rdm_eval_standard_workspace_bytes
    assert W(3, 37, 53) == 3 * 37 * 53 * 8 and W(1, 1, 1) == 8 and W(2, 480, 640) == 2 * 480 * 640 * 8
    assert W(0, 4, 4) == 0 and W(1, -4, 4) == 0 and W(1, 4, 0) == 0 and W(1, 0x10000, 0x10000) == 0
    assert W(1, 1, 0x7fffffff) == 8 * 0x7fffffff
    p = C.c_void_p(4096)
    crop = lambda *v: (C.c_int32 * 4)(*v)
    good = dict(m=p, d=p, f64=0, batch=2, h=8, w=9, align=1, lo=1e-3, hi=10.0, crop=None, rows=p, out=None, ws=p, wsb=2 * 8 * 9 * 8)
    changes = [(dict(m=None), b"NULL"), (dict(d=None), b"NULL"), (dict(rows=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(batch=0), b"batch"), (dict(h=-1), b"batch"),
               (dict(w=0), b"batch"), (dict(h=0x10000, w=0x10000), b"32-bit"), (dict(align=3), b"align"), (dict(align=-1), b"align"), (dict(lo=-1e-3), b"min_depth"),
               (dict(lo=10.0), b"min_depth"), (dict(lo=float("nan")), b"min_depth"), (dict(hi=float("nan")), b"min_depth"), (dict(crop=crop(2, 2, 2, 5)), b"crop"),
               (dict(crop=crop(0, 0, 9, 9)), b"crop"), (dict(crop=crop(0, 0, 8, 10)), b"crop"), (dict(crop=crop(-1, 0, 8, 9)), b"crop"), (dict(crop=crop(0, 5, 8, 4)), b"crop"),
               (dict(wsb=2 * 8 * 9 * 8 - 1), b"workspace"), (dict(wsb=0), b"workspace"),
               (dict(m=C.c_void_p(4100)), b"aligned"), (dict(rows=C.c_void_p(4100)), b"aligned"), (dict(ws=C.c_void_p(4100)), b"aligned"),
               (dict(out=C.c_void_p(4097)), b"aligned"), (dict(d=C.c_void_p(4098)), b"aligned"), (dict(d=C.c_void_p(4100), f64=1), b"aligned")]
    assert L.rdm_eval_standard_f64(None, C.c_void_p(4100), 0, 2, 8, 9, 1, 1e-3, 10.0, None, p, None, p, 2 * 8 * 9 * 8, None) == -1      # float32 depth at a 4-byte address
    assert b"NULL" in L.rdm_last_error_string()                                                  # ... passes the alignment check and is refused for the NULL map
    for change, word in changes:
        kw = dict(good, **change)
        rc = L.rdm_eval_standard_f64(kw["m"], kw["d"], kw["f64"], kw["batch"], kw["h"], kw["w"], kw["align"], kw["lo"], kw["hi"], kw["crop"], kw["rows"], kw["out"], kw["ws"],
                                     kw["wsb"], None)
        assert rc == -1 and b"eval_standard" in L.rdm_last_error_string() and word in L.rdm_last_error_string(), (change, rc, L.rdm_last_error_string())
