"""Native-resolution scoring without a GPU: the view-aware restatement (tests/evalview_ref.py) against the oracle's resize and the C library's
fma, the loader's views, the named crops, the command's new flags and refusals, the definition of flip averaging, and the C-ABI boundary of
include/rdm_eval_view.h (declared == bound == exported; every refusal is a status code before the launch)."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import evalstd_ref as ref
import evalview_ref as vref
from conftest import ROOT
from md_rdm_amd import filler
from oracle import computations_cpu as ocp

HEADER = os.path.join(ROOT, "include", "rdm_eval_view.h")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_emulated_fma_is_the_c_librarys():
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype, libm.fma.argtypes = C.c_double, [C.c_double] * 3
    n = 4000
    rng = np.random.default_rng(20)                                                # full 53-bit mantissas: the products are inexact
    a, b, c = rng.uniform(-3.0, 3.0, n), rng.uniform(-3.0, 3.0, n), rng.uniform(-9.0, 9.0, n)
    c[::4] = -(a[::4] * b[::4])                                                    # cancellation: the result is the product's rounding error
    c[1::8] = -(a[1::8] * b[1::8]) * (1.0 + 2.0 ** -40)
    a[2::16], c[2::16] = 1.0 + 2.0 ** -30, 2.0 ** -53                             # half-way cases of the final rounding
    b[2::16] = 1.0 - 2.0 ** -30
    want = np.array([libm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    np.testing.assert_array_equal(vref.fma(a, b, c), want)
    assert (want != a * b + c).sum() > n // 8                                      # the fused result does differ from two roundings


@pytest.mark.parametrize("h,w", [(7, 5), (37, 53), (128, 128), (480, 640)])
def test_full_view_sampler_is_the_oracle_resize(h, w):
    m = filler.uniform("evalview.cpu.m/%dx%d" % (h, w), (2, 1, 128, 128), -2.5, 5.5, dtype=np.float64)
    want = ocp.resize(m, (h, w))
    np.testing.assert_array_equal(vref.resize_view(m, h, w), want)
    np.testing.assert_array_equal(vref.resize_view(m, h, w, (0.0, 0.0, float(h), float(w))), want)
    if (h, w) != (128, 128):
        np.testing.assert_array_equal(vref.prediction(m, h, w, vref.full_view(h, w)), ref.prediction(m, h, w))
    else:
        np.testing.assert_array_equal(vref.prediction(m, h, w), np.exp(m))          # read as it is


def test_view_sampler_places_the_map():
    """a view with integer corners and sizes is the oracle resize to (vh, vw) pasted at (vy0, vx0), bit for bit: (y + 0.5) - vy0 is then
    (y - vy0) + 0.5 exactly; outside it the map's edge is replicated (the cubic coefficients sum to 1 within roundings)"""
    m = filler.uniform("evalview.cpu.place", (2, 1, 128, 128), -2.5, 5.5, dtype=np.float64)
    h, w, view = 61, 83, (9.0, 20.0, 37.0, 53.0)
    r = vref.resize_view(m, h, w, view)
    np.testing.assert_array_equal(r[:, :, 9:46, 20:73], ocp.resize(m, (37, 53)))
    np.testing.assert_allclose(r[:, :, :8, 20:73], np.broadcast_to(r[:, :, :1, 20:73], (2, 1, 8, 53)), rtol=0, atol=1e-13)     # rows whose taps are all map row 0
    np.testing.assert_allclose(r[:, :, 47:, 20:73], np.broadcast_to(r[:, :, 60:, 20:73], (2, 1, 14, 53)), rtol=0, atol=1e-13)
    np.testing.assert_allclose(r[:, :, :8, :19], np.broadcast_to(m[:, :, :1, :1], (2, 1, 8, 19)), rtol=0, atol=1e-13)             # the corner pixel
    a = vref.reference(m, np.full((2, 1, h, w), 2.0), "none", view=view)
    b = vref.reference(m, np.full((2, 1, h, w), 2.0), "none")
    assert ref.prediction.__module__ == "evalstd_ref" and (a["p"] != b["p"]).any() and a["rows"][0, 0] == h * w
    np.testing.assert_array_equal(a["p"], np.exp(r))


# ---- the loader's views ---------------------------------------------------------------------------------------------------------------------
def test_loader_views():
    from md_rdm_amd.dataloaders import nyu
    assert nyu.test_view((480, 640)) == (9.6, 13 * 640 / 666, 460.8, 640 * 640 / 666)
    p = nyu.test_params((480, 640), (226, 226))
    assert list(p.crop2) == [10, 13, 480, 640]                                     # the crop the view maps back, of the 500x666 resize
    v = nyu.test_view((480, 640))
    assert v[0] < 45 and v[0] + v[2] == pytest.approx(470.4) and 470 + 0.5 > v[0] + v[2] > 469 + 0.5      # row 470 of the Eigen crop is outside
    assert v[1] < 41 and v[1] + v[3] > 601                                          # its columns are all inside
    # validation: Resize(250) -> CenterCrop((226, 226)) of 480x640: 250x333, top 12, left round(53.5) = 54 (Python rounds half to even)
    assert nyu.val_view((480, 640), 250, (226, 226)) == (12 * 480 / 250, 54 * 640 / 333, 226 * 480 / 250, 226 * 640 / 333)
    q = nyu.identity_params((480, 640), 250, (226, 226))
    assert (q.top, q.left, q.h2, q.w2) == (12, 54, 250, 333)
    assert nyu.val_view((480, 640), 250, (228, 304)) == (11 * 480 / 250, 14 * 640 / 333, 228 * 480 / 250, 304 * 640 / 333)
    assert nyu.val_view((640, 480), 250, (226, 226)) == (54 * 640 / 333, 12 * 480 / 250, 226 * 640 / 333, 226 * 480 / 250)     # a portrait frame
    assert nyu.test_view((300, 640))[2] == 480 * 300 / 500                         # 500x1066 after the resize
    with pytest.raises(ValueError):
        nyu.test_view((300, 300))                                                  # 500x500: narrower than the crop
    with pytest.raises(ValueError):
        nyu.val_view((480, 640), 250, (260, 260))


def test_native_depth_is_for_val_and_test():
    from md_rdm_amd.dataloaders import NYUDataset, PrefetchLoader
    raw = [(np.zeros((480, 640, 3), np.uint8), np.ones((480, 640), np.float32))]
    with pytest.raises(ValueError, match="native_depth"):
        PrefetchLoader(NYUDataset(raw, split="train"), 1, device="cpu", native_depth=True)
    for split in ("val", "test"):
        ld = PrefetchLoader(NYUDataset(raw, split=split, output_size=(226, 226)), 1, device="cpu", native_depth=True)     # touches no device
        assert ld.native_depth and ld.view is None
    assert not PrefetchLoader(NYUDataset(raw, split="val"), 1, device="cpu").native_depth


# ---- named crops and the view of StandardMetrics ---------------------------------------------------------------------------------------------
def test_named_crops():
    from md_rdm_amd import metrics
    from md_rdm_amd.metrics import StandardMetrics
    sm = StandardMetrics(crop="eigen")
    assert sm.crop == "eigen" and sm.resolve_crop(480, 640) == (45, 41, 471, 601)
    for hw in ((226, 226), (640, 480), (480, 641)):
        with pytest.raises(ValueError, match="480x640"):
            sm.resolve_crop(*hw)
    g = StandardMetrics(crop="garg")
    assert g.resolve_crop(352, 1216) == (143, 43, 349, 1172)                       # 143.65 43.71 349.15 1172.29, truncated
    assert g.resolve_crop(375, 1242) == (153, 44, 371, 1197)                       # the figures of the usual KITTI scripts
    assert "TRUNCATED" in metrics.named_crop.__doc__
    assert StandardMetrics(crop=(1, 2, 3, 4)).resolve_crop(9, 9) == (1, 2, 3, 4) and StandardMetrics().resolve_crop(9, 9) is None
    with pytest.raises(ValueError):
        StandardMetrics(crop="kitti")


def test_standard_metrics_view():
    from md_rdm_amd.metrics import StandardMetrics
    assert StandardMetrics().view is None
    sm = StandardMetrics(view=[9.6, 12, 460.8, 615])
    assert sm.view == (9.6, 12.0, 460.8, 615.0)
    sm.view = None
    assert sm.view is None
    for bad in ((0, 0, 0, 5), (0, 0, 5, -1), (0, float("nan"), 5, 5), (float("inf"), 0, 5, 5), (0, 0, 5)):
        with pytest.raises(ValueError, match="view"):
            StandardMetrics(view=bad)


# ---- the command ----------------------------------------------------------------------------------------------------------------------------
def test_new_flags_parse():
    from md_rdm_amd import evaluate, predict
    P = evaluate.build_parser()
    a = P.parse_args([])
    assert (a.native, a.flip, a.crop) == (False, False, None) and not hasattr(a, "crop_name")
    a = P.parse_args(["--protocol", "standard", "--native", "--flip", "--crop", "eigen"])
    assert (a.native, a.flip, a.crop) == (True, True, "eigen")
    assert P.parse_args(["--crop=garg"]).crop == "garg"
    assert P.parse_args(["--crop", "45", "41", "471", "601"]).crop == [45, 41, 471, 601]
    for argv in (["--crop", "kitti"], ["--crop", "eigen", "1"], ["--crop", "eigen", "--crop", "1", "2", "3", "4"]):
        with pytest.raises(SystemExit):
            P.parse_args(argv)
    text = " ".join(P.format_help().split())
    assert "--native" in text and "--flip" in text and "eigen" in text and "garg" in text and "crop_name" not in text
    Q = predict.build_parser()
    assert Q.parse_args(["--out", "d"]).flip is False and Q.parse_args(["--out", "d", "--flip"]).flip is True


def test_make_computer_with_names_and_native():
    from md_rdm_amd import evaluate
    P = evaluate.build_parser()
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard", "--native", "--nyu_path", "d", "--crop", "eigen"]))
    assert sm.crop == "eigen" and sm.view is None                                  # the view arrives with the first batch
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard", "--size", "480", "640", "--crop", "eigen"]))
    assert sm.resolve_crop(480, 640) == (45, 41, 471, 601)
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard", "--crop", "garg"]))
    assert sm.resolve_crop(226, 226) == (92, 8, 224, 217)
    sm = evaluate.make_computer(P.parse_args(["--protocol", "standard", "--native", "--nyu_path", "d", "--crop", "45", "41", "471", "601"]))
    assert sm.crop == (45, 41, 471, 601)                                           # beyond --size: the raw frame decides


@pytest.mark.parametrize("argv,word", [
    (["--synthetic", "2", "--native"], "--native needs --protocol standard"),
    (["--nyu_path", "d", "--native", "--protocol", "reference"], "--native needs --protocol standard"),
    (["--synthetic", "2", "--native", "--protocol", "standard"], "--native needs --nyu_path"),
    (["--synthetic", "2", "--crop", "eigen"], "--crop eigen belongs to --protocol standard"),
    (["--synthetic", "2", "--crop", "garg", "--protocol", "reference"], "--crop garg belongs to --protocol standard"),
    (["--synthetic", "2", "--protocol", "standard", "--crop", "eigen"], "480x640"),                    # scored at --size, 226x226
    (["--nyu_path", "d", "--protocol", "standard", "--native", "--crop", "5", "5", "5", "9"], "--crop"),
    (["--nyu_path", "d", "--protocol", "standard", "--native", "--rows", "r"], "--rows with --native"),
])
def test_flag_errors_come_before_the_gpu(argv, word):
    from md_rdm_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(argv)
    assert word in str(e.value) and "no GPU" not in str(e.value), e.value


# ---- flip -----------------------------------------------------------------------------------------------------------------------------------
def closed_form(x):
    """a 'network' whose map is known: the running sum of the red channel along the width, which a mirror does not commute with"""
    return torch_cumsum(x[:, :1].double())


def torch_cumsum(t):
    import torch
    return torch.cumsum(t, dim=-1) * torch.arange(1, t.shape[-2] + 1, dtype=torch.float64)[:, None]


def test_flip_is_its_defining_expression():
    import torch
    from md_rdm_amd import harness
    from md_rdm_amd.metrics import StandardMetrics
    from md_rdm_amd.network.RDM_Net import mirror_average
    x = torch.from_numpy(filler.uniform("evalview.flip.x", (2, 3, 128, 128), 0.0, 1.0, dtype=np.float32))
    want = 0.5 * (closed_form(x) + closed_form(x.flip(-1)).flip(-1))
    assert torch.equal(mirror_average(closed_form, x), want) and not torch.equal(want, closed_form(x))
    # in closed form: cumsum from the left and cumsum from the right of the same row, halved
    r = x[:, :1].double()
    alt = 0.5 * (torch.cumsum(r, -1) + torch.cumsum(r.flip(-1), -1).flip(-1)) * torch.arange(1, 129, dtype=torch.float64)[:, None]
    assert torch.equal(want, alt)
    calls = []

    class Stub:
        def predict(self, v, flip=False):                                          # what DepthEstimationNet.predict does with flip
            calls.append((tuple(v.shape), flip))
            return mirror_average(closed_form, v) if flip else closed_form(v)

    class Rows(StandardMetrics):
        def compute_rows(self, pred, depth, pred_out=None):                       # a host stand-in for the launch: n = 1, everything else the map's sum
            import torch
            rows = torch.zeros(pred.shape[0], 16, dtype=torch.float64)
            rows[:, 0] = 1
            rows[:, 11] = pred.sum(dim=(1, 2, 3))
            return rows

    sm = Rows(["scale"])
    batches = [(x[:1], x[:1, :1]), (x[1:], x[1:, :1])]
    res, maps = harness.evaluate(Stub(), batches, sm, return_maps=True, flip=True)
    assert calls == [((1, 3, 128, 128), True)] * 2 and torch.equal(maps, want)
    assert res["scale"] == (float(want[0].sum()) + float(want[1].sum())) / 2
    del calls[:]
    res0, maps0 = harness.evaluate(Stub(), batches, sm, return_maps=True)
    assert calls == [((1, 3, 128, 128), False)] * 2 and torch.equal(maps0, closed_form(x)) and res0["scale"] != res["scale"]


def test_predict_signature_has_flip():
    import inspect
    from md_rdm_amd import harness
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    assert inspect.signature(DepthEstimationNet.predict).parameters["flip"].default is False
    assert inspect.signature(harness.evaluate).parameters["flip"].default is False


# ---- the C ABI of include/rdm_eval_view.h ---------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_eval_view.h")) == {"rdm_eval_standard_view_f64"}    # declared == bound == exported, with the header's types: test_abi_cpu.py
    assert '#include "rdm_eval.h"' in open(HEADER).read()
    old, new = _lib.HEADERS["rdm_eval.h"]["rdm_eval_standard_f64"][1], _lib.HEADERS["rdm_eval_view.h"]["rdm_eval_standard_view_f64"][1]
    assert len(new) == 16 and new[:10] == old[:10] and new[11:] == old[10:]          # the same arguments plus the view, after the crop


def test_view_refusals_are_status_codes():
    """every refusal happens before the launch: callable without a GPU"""
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    p = C.c_void_p(4096)
    view = lambda *v: (C.c_double * 4)(*v)
    crop = lambda *v: (C.c_int32 * 4)(*v)
    good = dict(m=p, d=p, f64=0, batch=2, h=8, w=9, align=1, lo=1e-3, hi=10.0, crop=None, view=view(0.5, 0.5, 7, 8), rows=p, out=None, ws=p, wsb=2 * 8 * 9 * 8)
    nan, inf = float("nan"), float("inf")
    changes = [(dict(view=view(nan, 0, 8, 9)), b"view"), (dict(view=view(0, nan, 8, 9)), b"view"), (dict(view=view(0, 0, nan, 9)), b"view"),
               (dict(view=view(0, 0, 8, nan)), b"view"), (dict(view=view(inf, 0, 8, 9)), b"view"), (dict(view=view(0, -inf, 8, 9)), b"view"),
               (dict(view=view(0, 0, inf, 9)), b"view"), (dict(view=view(0, 0, 8, inf)), b"view"), (dict(view=view(0, 0, 0, 9)), b"view"),
               (dict(view=view(0, 0, 8, 0)), b"view"), (dict(view=view(0, 0, -8, 9)), b"view"), (dict(view=view(0, 0, 8, -9)), b"view"),
               # what the old entry refuses, with and without a view
               (dict(m=None), b"NULL"), (dict(rows=None, view=None), b"NULL"), (dict(batch=0), b"batch"), (dict(h=0x10000, w=0x10000), b"32-bit"),
               (dict(align=3), b"align"), (dict(lo=10.0), b"min_depth"), (dict(crop=crop(0, 0, 9, 9)), b"crop"), (dict(wsb=2 * 8 * 9 * 8 - 1, view=None), b"workspace"),
               (dict(ws=C.c_void_p(4100)), b"aligned")]
    for change, word in changes:
        kw = dict(good, **change)
        rc = L.rdm_eval_standard_view_f64(kw["m"], kw["d"], kw["f64"], kw["batch"], kw["h"], kw["w"], kw["align"], kw["lo"], kw["hi"], kw["crop"], kw["view"], kw["rows"],
                                          kw["out"], kw["ws"], kw["wsb"], None)
        assert rc == -1 and b"eval_standard" in L.rdm_last_error_string() and word in L.rdm_last_error_string(), (change, rc, L.rdm_last_error_string())
