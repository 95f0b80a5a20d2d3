"""-m gpu: rdm_eval_standard_view_f64 (csrc/evalstd.hip, include/rdm_eval_view.h) through the C ABI, StandardMetrics with a view and a named crop,
PrefetchLoader(native_depth=True), predict(flip=True) and the evaluate command with --native --crop eigen --flip, against the float64 numpy
restatement tests/evalview_ref.py (its own view-aware sampler with explicit fma steps; steps 2 to 5 from tests/evalstd_ref.py).

The bounds are those of tests/test_gpu_evalstd.py, applied by ITS compare() and compare_out() (imported, not restated): counts and the median of the
depth equal, columns 11 / 13 and pred_out rtol 1e-13, the sums rtol 1e-11 on rows with a mean |q-d|/d of at least 1e-2 and atol n 2^-50 max_depth on the
rows named as below that, the three delta counts equal on inputs whose restatement keeps every pixel 1e-9 away from a threshold.  compare()
asserts all of that of the restatement before it looks at the device; the seeds below were run through it on the CPU (the restatement's rows
against themselves).  With the full view, or none, the new entry must give the BYTES of rdm_eval_standard_f64."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import evalstd_ref as ref
import evalview_ref as vref
import stream_probe as sp
import test_gpu_evalstd as base
from conftest import ROOT
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
LO, HI, ALIGNS, T = base.LO, base.HI, base.ALIGNS, base.T
EIGEN = (45, 41, 471, 601)
TEST_VIEW = (9.6, 13 * 640 / 666, 460.8, 640 * 640 / 666)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def raw_view(dev, m, d, align="median", lo=LO, hi=HI, crop=None, view=None, want_out=True, rows=None):
    """rdm_eval_standard_view_f64 itself -> (status, rows, pred_out or None); outputs pre-filled with a sentinel.  view None = a NULL pointer"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    m = m if torch.is_tensor(m) else T(m, dev)
    d = d if torch.is_tensor(d) else T(d, dev)
    B, _, h, w = d.shape
    if rows is None:
        rows = torch.full((B, 16), -777.0, dtype=torch.float64, device=dev)
    out = torch.full((B, 1, h, w), -777.0, dtype=torch.float64, device=dev) if want_out else None
    need = L.rdm_eval_standard_workspace_bytes(B, h, w)                            # unchanged by the view
    ws = torch.empty(B * h * w, dtype=torch.float64, device=dev)
    c = (C.c_int32 * 4)(*crop) if crop is not None else None
    v = (C.c_double * 4)(*view) if view is not None else None
    rc = L.rdm_eval_standard_view_f64(_lib.ptr(m), _lib.ptr(d), int(d.dtype == torch.float64), B, h, w, _lib.EVAL_ALIGN[align], lo, hi, c, v, _lib.ptr(rows),
                                      _lib.ptr(out), _lib.ptr(ws), need, _lib.stream())
    torch.cuda.synchronize()
    return rc, rows, out


def small_inputs(B, h, w, tag):
    """float32 depth over [0.1, 12] (the range (LO, HI) itself excludes pixels) with zeros, a NaN and an infinity where there is room"""
    d = filler.log_uniform("evalview.d/%s/%dx%dx%d" % (tag, B, h, w), (B, 1, h, w), 0.1, 12.0)
    if h * w >= 16:
        d[filler.unit("evalview.hole/%s/%dx%dx%d" % (tag, B, h, w), B * h * w).reshape(B, 1, h, w) < 0.2] = 0.0
        d[B - 1, 0, h // 2, :2] = [np.nan, np.inf]
    return d, base.log_map("view/%s/%dx%d" % (tag, h, w), B)


# ---- the full view: the bytes of rdm_eval_standard_f64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("h,w,crop", [(128, 128, (5, 7, 100, 120)), (1, 1, (0, 0, 1, 1)), (7, 5, (1, 1, 6, 4)), (37, 53, (5, 7, 30, 50))])
def test_full_view_gives_the_old_entrys_bytes(dev, h, w, crop, align):
    d, m = small_inputs(3, h, w, "id")
    if (h, w) == (1, 1):
        d[:, 0, 0, 0] = [2.0, 0.5, 9.0]                                              # valid, valid, beyond HI
    dt, mt = T(d, dev), T(m, dev)
    for c in (None, crop):
        rc0, rows0, out0 = base.raw(dev, mt, dt, align, crop=c)
        assert rc0 == 0 and bool((rows0[:2, 0] > 0).all()), (c, rows0[:, 0])
        for view in (None, (0.0, 0.0, float(h), float(w))):
            rc, rows, out = raw_view(dev, mt, dt, align, crop=c, view=view)
            assert rc == 0 and sp.same_bits(rows, rows0) and sp.same_bits(out, out0), (c, view)
        rc, rows, out = raw_view(dev, mt, dt, align, crop=c, want_out=False)
        assert rc == 0 and out is None and sp.same_bits(rows, rows0)
    if (h, w) == (128, 128) and align == "none":                                   # only the FULL view reads the map as it is
        rc, _, shifted = raw_view(dev, mt, dt, "none", view=(0.25, 0.0, 128.0, 128.0))
        assert rc == 0 and not torch.equal(shifted, out0)


# ---- fractional views against the restatement ------------------------------------------------------------------------------------------------
VIEWS = {
    "test transform at a tenth": (3, 48, 64, (0.96, 1.25, 46.08, 61.5)),
    "partly outside the frame": (3, 37, 53, (-5.5, 10.25, 30.0, 60.0)),
    "a frame inside one map pixel's reach": (3, 48, 64, (-100.0, -120.0, 300.0, 400.0)),            # vh = 300 on h = 48: 0.43 map pixels per depth pixel
    "the map inside one depth pixel": (3, 48, 64, (20.25, 30.5, 0.5, 0.75)),                          # vh = 0.5: 256 map pixels per depth pixel
}
VIEW_SEEDS = {"test transform at a tenth": 1, "partly outside the frame": 1, "a frame inside one map pixel's reach": 1, "the map inside one depth pixel": 1}


@functools.lru_cache(maxsize=None)
def view_case(name):
    B, h, w, view = VIEWS[name]
    d, m = small_inputs(B, h, w, "%s/%d" % (name, VIEW_SEEDS[name]))
    return d, m, view, {a: vref.reference(m, d, a, LO, HI, view=view) for a in ALIGNS}


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_fractional_views_against_the_restatement(dev, name, align):
    d, m, view, refs = view_case(name)
    r = refs[align]
    assert (r["rows"][:, 0] > 0).all() and (r["p"] != ref.prediction(m, d.shape[2], d.shape[3])).any()      # the view does move the prediction
    rc, rows, out = raw_view(dev, m, d, align, view=view)
    assert rc == 0
    base.compare(rows.cpu().numpy(), r, align, "%s %s" % (name, align))
    base.compare_out(out, r, name)
    rc, rows64, out64 = raw_view(dev, m, d.astype(np.float64), align, view=view)   # the same values as float64: bit for bit
    assert rc == 0 and sp.same_bits(rows, rows64) and sp.same_bits(out, out64)


@functools.lru_cache(maxsize=None)
def one_pixel_case():
    d = np.array([2.0, 0.5, 9.0], dtype=np.float32).reshape(3, 1, 1, 1)            # valid, valid, beyond HI: a row of zeros
    m = base.log_map("view/1x1", 3)
    view = (0.25, 0.125, 0.5, 0.75)                                                 # the pixel's centre falls between map pixels (63.5, 63.5)
    return d, m, view, {a: vref.reference(m, d, a, LO, HI, view=view) for a in ALIGNS}


@pytest.mark.parametrize("align", ALIGNS)
def test_a_one_pixel_depth_under_a_view(dev, align):
    d, m, view, refs = one_pixel_case()
    r = refs[align]
    assert r["rows"][:, 0].tolist() == [1, 1, 0] and not r["rows"][2].any()
    rc, rows, out = raw_view(dev, m, d, align, view=view)
    assert rc == 0
    base.compare(rows.cpu().numpy(), r, align, "1x1 %s" % align, atol_rows=() if align == "none" else (0, 1))      # one valid pixel, aligned: q = d
    base.compare_out(out, r, "1x1")


# ---- the native frame ------------------------------------------------------------------------------------------------------------------------
NATIVE_SEED = 1


@functools.lru_cache(maxsize=None)
def native_case():
    """B = 2 at 480x640 under the test transform's view and the Eigen crop, median alignment; zeros and NaNs sprinkled over the depth"""
    tag = "native/%d" % NATIVE_SEED
    d = filler.log_uniform("evalview.d/" + tag, (2, 1, 480, 640), 0.1, 12.0)
    u = filler.unit("evalview.hole/" + tag, 2 * 480 * 640).reshape(2, 1, 480, 640)
    d[u < 0.15] = 0.0
    d[u > 0.97] = np.nan
    m = base.log_map("view/" + tag, 2)
    return d, m, vref.reference(m, d, "median", LO, HI, crop=EIGEN, view=TEST_VIEW)


def test_native_frame_with_the_eigen_crop(dev):
    from md_rdm_amd.dataloaders import nyu
    from md_rdm_amd.metrics import StandardMetrics
    d, m, r = native_case()
    assert nyu.test_view((480, 640)) == TEST_VIEW
    n = r["rows"][:, 0]
    assert (n > 0.7 * 426 * 560 * 0.8).all() and (n < 426 * 560).all() and np.isnan(d).sum() > 1000 and (d == 0).sum() > 1000
    assert r["valid"][:, :, 470, 41:601].any() and not r["valid"][:, :, 471:].any()                # row 470 is scored, against the replicated edge
    rc, rows, out = raw_view(dev, m, d, "median", crop=EIGEN, view=TEST_VIEW)
    assert rc == 0
    base.compare(rows.cpu().numpy(), r, "median", "native")
    base.compare_out(out, r, "native")
    sm = StandardMetrics(min_depth=LO, max_depth=HI, crop="eigen", view=nyu.test_view((480, 640)))
    q = torch.empty(2, 1, 480, 640, dtype=torch.float64, device=dev)
    assert sp.same_bits(sm.compute_rows(T(m, dev), T(d, dev), pred_out=q), rows) and sp.same_bits(q, out)
    with pytest.raises(ValueError, match="480x640"):
        sm.compute_rows(T(m, dev), T(d[:, :, :, :639].copy(), dev))
    plain = StandardMetrics(min_depth=LO, max_depth=HI, crop=EIGEN)                  # no view: the old entry, the map stretched over the frame
    assert sp.same_bits(plain.compute_rows(T(m, dev), T(d, dev)), base.raw(dev, m, d, "median", crop=EIGEN)[1])
    assert not torch.equal(plain.compute_rows(T(m, dev), T(d, dev)), rows)


def stream_case(dev):
    from md_rdm_amd import _lib
    from md_rdm_amd.metrics import StandardMetrics
    d, m, _ = native_case()
    sm = StandardMetrics(min_depth=LO, max_depth=HI, crop="eigen", view=TEST_VIEW)
    ins = dict(m=T(m, dev), d=T(d, dev))
    scratch = dict(rows=torch.empty(2, 16, dtype=torch.float64, device=dev), out=torch.empty(2, 1, 480, 640, dtype=torch.float64, device=dev),
                   ws=torch.empty(2 * 480 * 640, dtype=torch.float64, device=dev))
    crop, view = (C.c_int32 * 4)(*EIGEN), (C.c_double * 4)(*TEST_VIEW)

    def call(b, st):
        _lib.check(_lib.lib().rdm_eval_standard_view_f64(_lib.ptr(b["m"]), _lib.ptr(b["d"]), 0, 2, 480, 640, 1, LO, HI, crop, view, _lib.ptr(b["rows"]), _lib.ptr(b["out"]),
                                                         _lib.ptr(b["ws"]), b["ws"].numel() * 8, st))
        return dict(wrapped=sm.compute_rows(b["m"], b["d"]))                       # the product wrapper resolves the caller's stream itself
    return sp.Case(ins, call, outs=("rows", "out"), scratch=scratch)


def test_native_frame_on_a_late_non_default_stream(dev):
    got = sp.check(stream_case(dev), sp.Delay(dev))
    _, _, r = native_case()
    base.compare(got["rows"].cpu().numpy(), r, "median", "native, stream")
    assert sp.same_bits(got["wrapped"], got["rows"])


# ---- determinism, batch independence ---------------------------------------------------------------------------------------------------------
def test_repeated_and_alone(dev):
    d, m, view, _ = view_case("test transform at a tenth")
    dt, mt = T(d, dev), T(m, dev)
    for align in ALIGNS:
        rc, rows, out = raw_view(dev, mt, dt, align, view=view, crop=(4, 4, 44, 60))
        rc2, rows2, out2 = raw_view(dev, mt, dt, align, view=view, crop=(4, 4, 44, 60))
        assert rc == 0 and rc2 == 0 and sp.same_bits(rows, rows2) and sp.same_bits(out, out2)
        rc1, r1, o1 = raw_view(dev, mt[1:2].contiguous(), dt[1:2].contiguous(), align, view=view, crop=(4, 4, 44, 60))
        assert rc1 == 0 and sp.same_bits(r1[0], rows[1]) and sp.same_bits(o1[0], out[1]), align


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_bad_views_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    d, m, _, _ = view_case("partly outside the frame")
    dt, mt = T(d, dev), T(m, dev)
    rows = torch.full((3, 16), -777.0, dtype=torch.float64, device=dev)
    nan, inf = float("nan"), float("inf")
    for view in ((nan, 0, 37, 53), (0, 0, 37, nan), (inf, 0, 37, 53), (0, -inf, 37, 53), (0, 0, inf, 53), (0, 0, 0, 53), (0, 0, 37, -53), (0, 0, -1e-300, 53)):
        rc, _, out = raw_view(dev, mt, dt, rows=rows, view=view)
        assert rc == -1 and b"view" in L.rdm_last_error_string(), (view, rc, L.rdm_last_error_string())         # RDM_ERR_BAD_ARGUMENT
        assert bool((out == -777.0).all())
    rc, _, out = raw_view(dev, mt, dt, rows=rows, view=(0, 0, 37, 53), crop=(0, 0, 38, 53))                     # what the old entry refuses
    assert rc == -1 and b"crop" in L.rdm_last_error_string() and bool((out == -777.0).all())
    assert bool((rows == -777.0).all())


# ---- predict(flip=True) ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


def test_predict_flip_is_its_defining_expression(dev, model):
    """tests/test_gpu_predict.py holds two predict calls on one input to torch.equal, so the expression formed from plain calls is held to that"""
    from md_rdm_amd.network import computations as cp
    x = torch.from_numpy(filler.synthetic_batch(2, 226, 226, seed=filler.MARGIN_SEEDS["eval226"])[0]).to(dev)
    want = 0.5 * (model.predict(x) + model.predict(x.flip(-1)).flip(-1))
    got, counts = model.predict(x, flip=True, return_counts=True)
    assert got.dtype == torch.float64 and got.shape == (2, 1, 128, 128) and torch.equal(got, want)
    assert not torch.equal(got, model.predict(x)) and torch.equal(counts, model.predict(x, return_counts=True)[1])
    assert torch.equal(model.predict(x, flip=True, size=(48, 64)), cp.resize(want, (48, 64)))            # averaged before size and linear apply
    assert torch.equal(model.predict(x, flip=True, linear=True), torch.exp(want).float())


# ---- the loader, harness.evaluate and the command --------------------------------------------------------------------------------------------
def write_samples(folder, n=3):
    depths = []
    for i in range(n):
        rgb = (filler.unit("evalview.e2e.rgb/%d" % i, 480 * 640 * 3) * 256).astype(np.uint8).reshape(480, 640, 3)
        dep = filler.log_uniform("evalview.e2e.d/%d" % i, (480, 640), 0.4, 9.0)
        dep[filler.unit("evalview.e2e.hole/%d" % i, 480 * 640).reshape(480, 640) < 0.1] = 0.0
        np.savez(os.path.join(folder, "s%02d.npz" % i), rgb=rgb, depth=dep)
        depths.append(dep)
    return np.stack(depths)[:, None]


def test_cli_native_eigen_flip_end_to_end(dev, model, tmp_path):
    from md_rdm_amd import harness
    from md_rdm_amd.dataloaders import NYUDataset, PrefetchLoader
    from md_rdm_amd.metrics import StandardMetrics
    data = tmp_path / "nyu"
    data.mkdir()
    depths = write_samples(str(data))
    out = tmp_path / "r.json"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "md_rdm_amd.evaluate", "--nyu_path", str(data), "--protocol", "standard", "--native", "--crop",
                        "eigen", "--flip", "--split", "test", "--batch_size", "2", "--out", str(out)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(out.read_text())
    assert (rec["protocol"], rec["native"], rec["flip"], rec["crop"], rec["view"], rec["n"], rec["skipped"], rec["split"]) == (
        "standard", True, True, list(EIGEN), list(TEST_VIEW), 3, 0, "test")
    # the same evaluation, directly
    sm = StandardMetrics(crop="eigen")
    loader = PrefetchLoader(NYUDataset(str(data), split="test", output_size=(226, 226)), 2, shuffle=False, device=dev, drop_last=False, indices=range(3), native_depth=True)
    assert loader.view is None
    seen = []

    def batches():
        for x, y in loader:
            assert loader.view == TEST_VIEW and x.shape[1:] == (3, 226, 226) and y.shape[1:] == (1, 480, 640) and y.dtype == torch.float32
            sm.view = loader.view
            seen.append(y)
            yield x, y
    res, maps = harness.evaluate(model, batches(), sm, return_maps=True, flip=True)
    y = torch.cat(seen)
    np.testing.assert_array_equal(y.cpu().numpy(), depths)                          # the raw depth, untouched
    assert res["n"] == 3 and res["skipped"] == 0
    for name in ref.NAMES:
        assert rec["metrics"][name] == res[name], name
    # and the restatement on the maps that were scored
    r64 = vref.reference(maps.cpu().numpy(), depths, "median", crop=EIGEN, view=TEST_VIEW)
    rows = sm.compute_rows(maps, y).cpu().numpy()
    base.compare(rows, r64, "median", "end to end", hi=10.0)
    vals = np.array(ref.values_from_rows(rows))
    for k, name in enumerate(sm.names):
        print("%s: evaluate %.15g, mean of the restatement's values %.15g" % (name, res[name], vals[:, k].mean()))
        np.testing.assert_allclose(res[name], vals[:, k].mean(), rtol=1e-14, atol=0)
