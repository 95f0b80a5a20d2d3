"""rdm_depth_frames (include/rdm_depth.h) and md_rdm_amd.depth on the MI355X against the numpy statement of the contract (tests/depthframe_ref.py).

Tolerances, derived from the contract:
  scale_out   bit for bit (one integer sum, five IEEE float64 operations in a stated order, A and Bc from the C library's log on both sides);
  depth_f32   within one float32 ulp: the resampled log value is bit-exact (tests/evalview_ref.py), the float64 exponentials of the device and
              of numpy differ by a few float64 ulps, far below a float32 ulp, so at most the final rounding flips;
  depth_u16   equal, except at ROUNDING-CRITICAL pixels (quotient within 1e-9 * max(q, 1) of a half-integer), where it may differ by 1; such pixels
              may be at most 0.1 % of a case (the hash-generated cases here have none, which every comparison asserts of the reference);
  outside     exactly 0.
Every call writes between guard elements, which must stay untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import depthframe_ref as dref
import stream_probe as sp
from md_rdm_amd import filler
from md_rdm_amd.dataloaders import nyu

pytestmark = pytest.mark.gpu
G = 8                                            # guard elements on either side of an output: 32 / 16 bytes, so shift = 0 keeps the 16 / 8-byte alignment
F_GUARD, U_GUARD = -777.0, 0x7A7A
TEST_VIEW = nyu.test_view((480, 640))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def log_map(key, B):
    return filler.uniform("dframe.map/" + key, (B, 1, 128, 128), -1.5, 1.5, dtype=np.float64)


def head_counts(key, B, n, K=90):
    return (filler.unit("dframe.counts/" + key, B * n) * (K + 1)).astype(np.int64).reshape(B, n)


def raw(dev, m, h, w, view=None, counts=None, ls=None, sid="nyu", offset=0.0, unit=1e-3, outside=0, want=("f32", "u16", "scale"), split=0, shift=0, argv=None):
    """one call of the C entry -> (rc, f32 (B,h,w) | None, u16 | None, scale (B,) | None); asserts the guards.  ``argv``: {position: value} overrides"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    m = m if isinstance(m, torch.Tensor) else T(m, dev)
    B, n = m.shape[0], m.shape[0] * h * w
    fbuf = torch.full((G + shift + n + G,), F_GUARD, dtype=torch.float32, device=dev)
    ubuf = torch.full((G + shift + n + G,), U_GUARD, dtype=torch.int16, device=dev)
    sbuf = torch.full((1 + B + 1,), F_GUARD, dtype=torch.float64, device=dev)
    c = None if counts is None else counts if isinstance(counts, torch.Tensor) else T(np.asarray(counts, dtype=np.int64).reshape(B, -1), dev)
    lst = None if ls is None else T(np.asarray(ls, dtype=np.float64), dev)
    par = (C.c_double * 4)(*(dref.SID[sid] if isinstance(sid, str) else sid), offset) if c is not None else None
    v = (C.c_double * 4)(*view) if view is not None else None
    args = [_lib.ptr(m), _lib.ptr(c), c.shape[1] if c is not None else 0, _lib.ptr(lst), par, B, h, w, v, outside, unit,
            C.c_void_p(fbuf.data_ptr() + 4 * (G + shift)) if "f32" in want else None, C.c_void_p(ubuf.data_ptr() + 2 * (G + shift)) if "u16" in want else None,
            C.c_void_p(sbuf.data_ptr() + 8) if "scale" in want else None, split, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_depth_frames(*args)
    torch.cuda.synchronize()
    f, u, s = fbuf.cpu().numpy(), ubuf.cpu().numpy().view(np.uint16), sbuf.cpu().numpy()
    lo, hi = G + shift, G + shift + n
    assert (f[:lo] == np.float32(F_GUARD)).all() and (f[hi:] == np.float32(F_GUARD)).all(), "float32 guards"
    assert (u[:lo] == U_GUARD).all() and (u[hi:] == U_GUARD).all(), "uint16 guards"
    assert s[0] == F_GUARD and s[-1] == F_GUARD, "scale guards"
    if rc != 0 or "f32" not in want:
        assert (f == np.float32(F_GUARD)).all()
    if rc != 0 or "u16" not in want:
        assert (u == U_GUARD).all()
    if rc != 0 or "scale" not in want:
        assert (s == F_GUARD).all()
    return (rc, f[lo:hi].reshape(B, h, w) if "f32" in want else None, u[lo:hi].reshape(B, h, w) if "u16" in want else None, s[1:-1] if "scale" in want else None)


def ulps32(a, b):
    """largest distance in float32 steps between two non-negative float32 arrays; NaN must meet NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    assert (nan == np.isnan(b)).all(), "NaN pattern"
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return int(d[~nan].max()) if (~nan).any() else 0


def compare(got, r, what):
    rc, f, u, s = got
    assert rc == 0, what
    assert r["critical"].mean() <= 1e-3, (what, "the reference itself has too many rounding-critical pixels")
    if s is not None:
        np.testing.assert_array_equal(s.view(np.int64), r["ls"].view(np.int64), err_msg=what)
    if f is not None:
        assert ulps32(f, r["f32"]) <= 1, (what, ulps32(f, r["f32"]))
        assert (f[:, ~r["inside"]] == 0).all() or what.endswith("edge")
    if u is not None:
        d = np.abs(u.astype(np.int64) - r["u16"].astype(np.int64))
        assert (d[~r["critical"]] == 0).all() and (d <= 1).all(), (what, int(d.max()), int((d != 0).sum()))


# ---- frames and views -------------------------------------------------------------------------------------------------------------------------
FRAMES = [("1x1", 1, 1, None), ("5x7", 5, 7, None), ("128x128", 128, 128, None), ("37x53 fractional", 37, 53, (2.5, -3.25, 41.0, 48.5)),
          ("sub-pixel view", 9, 11, (4.25, 5.125, 0.5, 0.25))]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name,h,w,view", FRAMES, ids=[f[0] for f in FRAMES])
def test_frames_and_views(dev, name, h, w, view, B):
    m = log_map(name, B)
    ls = filler.uniform("dframe.ls/" + name, (B,), -0.5, 1.0, dtype=np.float64)
    for outside in ("zero", "edge"):
        r = dref.reference(m, h, w, view=view, log_scale_in=ls, outside=outside)
        if name == "37x53 fractional":                                              # rows 2.5 .. 43.5 (past the bottom), columns -3.25 .. 45.25 (past the left edge)
            assert r["inside"].any() and not r["inside"].all()
        compare(raw(dev, m, h, w, view=view, ls=ls, outside={"zero": 0, "edge": 1}[outside]), r, "%s B=%d %s" % (name, B, outside))


def test_subpixel_views(dev):
    """rows 4.25 .. 4.75 hold the centre 4.5; columns 5.125 .. 5.375 hold no centre (every pixel is 0), columns 5.125 .. 5.625 hold 5.5 alone"""
    m = log_map("sub-pixel view", 1)
    r = dref.reference(m, 9, 11, view=(4.25, 5.125, 0.5, 0.25))
    assert not r["inside"].any()
    got = raw(dev, m, 9, 11, view=(4.25, 5.125, 0.5, 0.25))
    assert got[0] == 0 and (got[1] == 0).all() and (got[2] == 0).all()
    r = dref.reference(m, 9, 11, view=(4.25, 5.125, 0.5, 0.5))
    assert r["inside"].sum() == 1 and r["inside"][4, 5]
    compare(raw(dev, m, 9, 11, view=(4.25, 5.125, 0.5, 0.5)), r, "one pixel inside")


@functools.lru_cache(maxsize=None)
def native_case():
    m = log_map("native", 2)
    c = head_counts("native", 2, 64)
    return m, c, dref.reference(m, 480, 640, view=TEST_VIEW, counts=c)


def test_native_frame(dev):
    m, c, r = native_case()
    got = raw(dev, m, 480, 640, view=TEST_VIEW, counts=c)
    compare(got, r, "native")
    assert (got[1][:, :10] == 0).all() and (got[1][:, 470:] == 0).all() and (got[1][:, 10:470, 13:627] > 0).all()      # rows 9.6 .. 470.4, columns 12.49 .. 627.51
    assert (got[2][:, :10] == 0).all() and (got[2][:, 470:] == 0).all() and (got[2][:, :, :12] == 0).all() and (got[2][:, :, 628:] == 0).all()


# ---- store tails and alignment ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("w", [1, 2, 3, 5, 7, 9])
def test_store_tails(dev, w, shift):
    """h = 3, B = 2: rows and the second sample start at every element offset mod 4; shift = 1 moves both outputs one element off their allocation"""
    m = log_map("tails", 2)
    r = dref.reference(m, 3, w)
    compare(raw(dev, m, 3, w, shift=shift), r, "3x%d shift %d" % (w, shift))


# ---- the scale --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 63, 418])
def test_scale_head_sizes(dev, n):
    m = log_map("scale", 3)
    for sid in dref.SID:
        K = int(dref.SID[sid][2])
        for offset in (0.0, 0.5):
            c = head_counts("%s/%d" % (sid, n), 3, n, K)
            c[1] = 0                                                                # all counts 0: alpha metres; all K: beta metres
            c[2] = K
            r = dref.reference(m, 5, 7, counts=c, sid=sid, offset=offset)
            got = raw(dev, m, 5, 7, counts=c, sid=sid, offset=offset)
            compare(got, r, "%s n=%d offset %g" % (sid, n, offset))
            if offset == 0.0:
                assert got[3][1] == np.log(dref.SID[sid][0]) and abs(got[3][2] - np.log(dref.SID[sid][1])) < 1e-14


def test_scale_sources(dev):
    from md_rdm_amd import depth
    m, mt = log_map("sources", 3), T(log_map("sources", 3), dev)
    c = head_counts("sources", 3, 64)
    ls = np.array([0.75, -0.25, -0.0])
    for counts, extra in ((None, ls), (c, None), (c, ls), (None, None)):
        r = dref.reference(m, 37, 53, counts=counts, log_scale_in=extra)
        compare(raw(dev, mt, 37, 53, counts=counts, ls=extra), r, "counts %s log_scale %s" % (counts is not None, extra is not None))
        out = depth.metric_frames(mt, (37, 53), counts=None if counts is None else T(c.reshape(3, 1, 8, 8), dev), log_scale=None if extra is None else T(extra, dev),
                                  want=("f32", "u16", "log_scale"))
        assert out["f32"].shape == (3, 37, 53) and out["u16"].dtype == torch.uint16 and out["log_scale"].dtype == torch.float64
        compare((0, out["f32"].cpu().numpy(), out["u16"].cpu().numpy(), out["log_scale"].cpu().numpy()), r, "metric_frames")
        if counts is not None and extra is None:
            assert sp.same_bits(depth.sid_log_scale(T(c.reshape(3, 1, 8, 8), dev)), out["log_scale"])
    # neither: exp of the map stretched over the frame, predict(linear=True, size=...)'s resize + exp + cast, to the same one-ulp bound
    from md_rdm_amd.network import computations as cp
    lin = torch.exp(cp.resize(mt, (37, 53))).float()[:, 0]
    assert ulps32(raw(dev, mt, 37, 53, want=("f32",))[1], lin.cpu().numpy()) <= 1


# ---- quantisation -----------------------------------------------------------------------------------------------------------------------------
def test_quantisation(dev):
    m = log_map("quant", 2)
    for unit in (1e-3, 1.0 / 256.0):
        compare(raw(dev, m, 37, 53, unit=unit), dref.reference(m, 37, 53, unit=unit), "unit %g" % unit)
    ls = np.array([3.0, 8.0])                                                       # e^(8 - 1.5 - the cubic's overshoot) > 65.535 m: sample 1 saturates everywhere
    r = dref.reference(m, 37, 53, log_scale_in=ls)
    assert (r["u16"][1] == 65535).all() and (r["u16"][0] == 65535).any() and (r["u16"][0] < 65535).any()
    compare(raw(dev, m, 37, 53, ls=ls), r, "saturation")
    only_f, only_u = raw(dev, m, 37, 53, want=("f32",)), raw(dev, m, 37, 53, want=("u16",))
    both = raw(dev, m, 37, 53)
    assert only_f[0] == 0 and only_u[0] == 0 and only_f[2] is None and only_u[1] is None
    np.testing.assert_array_equal(only_f[1].view(np.int32), both[1].view(np.int32))
    np.testing.assert_array_equal(only_u[2], both[2])


def test_nan_and_inf_in_the_map(dev):
    """128x128 under the full view reads the map with weights 0 and 1: the poisoned pixel itself is NaN -> (NaN, 0) or +inf -> (inf, 65535); pixels
    whose 4x4 taps do not reach it are untouched"""
    m = log_map("nonfinite", 2).copy()
    clean = raw(dev, m, 128, 128)
    m[0, 0, 60, 60] = np.nan
    m[1, 0, 20, 100] = np.inf
    rc, f, u, _ = raw(dev, m, 128, 128)
    assert rc == 0 and np.isnan(f[0, 60, 60]) and u[0, 60, 60] == 0 and f[1, 20, 100] == np.inf and u[1, 20, 100] == 65535
    far = np.ones((2, 128, 128), dtype=bool)
    far[0, 57:64, 57:64] = False
    far[1, 17:24, 97:104] = False
    np.testing.assert_array_equal(f[far].view(np.int32), clean[1][far].view(np.int32))
    np.testing.assert_array_equal(u[far], clean[2][far])


# ---- determinism ------------------------------------------------------------------------------------------------------------------------------
def test_repeated_alone_and_split(dev):
    m, c = log_map("det", 3), head_counts("det", 3, 64)
    view = (2.5, -3.25, 41.0, 48.5)
    base = raw(dev, m, 37, 53, view=view, counts=c)
    for split in (0, 1, 2, 7, 64):
        got = raw(dev, m, 37, 53, view=view, counts=c, split=split)
        assert got[0] == 0
        for a, b in zip(got[1:], base[1:]):
            assert a.tobytes() == b.tobytes(), split
    for b in range(3):
        one = raw(dev, m[b:b + 1], 37, 53, view=view, counts=c[b:b + 1])
        assert one[1][0].tobytes() == base[1][b].tobytes() and one[2][0].tobytes() == base[2][b].tobytes() and one[3][0] == base[3][b], b
    m2, c2, _ = native_case()
    big = raw(dev, m2, 480, 640, view=TEST_VIEW, counts=c2)
    for split in (1, 7, 480, 1000):
        got = raw(dev, m2, 480, 640, view=TEST_VIEW, counts=c2, split=split)
        assert got[1].tobytes() == big[1].tobytes() and got[2].tobytes() == big[2].tobytes(), split


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -------------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib, depth
    m, c = log_map("stream", 2), head_counts("stream", 2, 64).reshape(2, 1, 8, 8)
    ins = dict(m=T(m, dev), c=T(c, dev))
    scratch = dict(f=torch.empty(2, 37, 53, dtype=torch.float32, device=dev), u=torch.empty(2, 37, 53, dtype=torch.int16, device=dev),
                   s=torch.empty(2, dtype=torch.float64, device=dev))
    par, view = (C.c_double * 4)(*dref.SID["nyu"], 0.0), (C.c_double * 4)(2.5, -3.25, 41.0, 48.5)

    def call(b, st):
        _lib.check(_lib.lib().rdm_depth_frames(_lib.ptr(b["m"]), _lib.ptr(b["c"]), 64, None, par, 2, 37, 53, view, 1, 1e-3, _lib.ptr(b["f"]), _lib.ptr(b["u"]), _lib.ptr(b["s"]), 0, st))
        out = depth.metric_frames(b["m"], (37, 53), view=(2.5, -3.25, 41.0, 48.5), counts=b["c"], outside="edge", want=("f32", "u16"))   # the wrapper resolves the stream itself
        return dict(wrapped_f=out["f32"], wrapped_u=out["u16"].view(torch.int16))
    return sp.Case(ins, call, outs=("f", "u", "s"), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    m, c = log_map("stream", 2), head_counts("stream", 2, 64)
    r = dref.reference(m, 37, 53, view=(2.5, -3.25, 41.0, 48.5), counts=c, outside="edge")
    compare((0, got["f"].cpu().numpy(), got["u"].cpu().numpy().view(np.uint16), got["s"].cpu().numpy()), r, "stream edge")
    assert sp.same_bits(got["wrapped_f"], got["f"]) and sp.same_bits(got["wrapped_u"], got["u"])


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    m, c = T(log_map("bad", 2), dev), T(head_counts("bad", 2, 64), dev)
    D4 = C.c_double * 4
    nan, inf = float("nan"), float("inf")
    # positions: 0 log_map, 1 counts, 2 count_n, 3 log_scale, 4 sid, 5 batch, 6 h, 7 w, 8 view, 9 outside, 10 unit, 11 f32, 12 u16, 13 scale_out, 14 split
    bad = [({0: None}, b"log_map"), ({11: None, 12: None}, b"depth_f32"), ({5: 0}, b"batch"), ({5: -1}, b"batch"), ({6: 0}, b"h"), ({7: -3}, b"w"),
           ({2: 0}, b"count_n"), ({4: None}, b"sid"), ({4: D4(nan, 10, 90, 0)}, b"sid"), ({4: D4(0.02, inf, 90, 0)}, b"sid"), ({4: D4(0.02, 10, 90, nan)}, b"sid"),
           ({4: D4(0.0, 10, 90, 0)}, b"alpha"), ({4: D4(-1.0, 10, 90, 0)}, b"alpha"), ({4: D4(0.02, 0.02, 90, 0)}, b"beta"), ({4: D4(0.02, 0.01, 90, 0)}, b"beta"),
           ({4: D4(0.02, 10, 0, 0)}, b"K"), ({10: 0.0}, b"unit"), ({10: -1e-3}, b"unit"), ({10: nan}, b"unit"), ({10: inf}, b"unit"), ({9: 2}, b"outside"), ({9: -1}, b"outside"),
           ({14: -1}, b"split"), ({8: D4(nan, 0, 5, 7)}, b"view"), ({8: D4(0, inf, 5, 7)}, b"view"), ({8: D4(0, 0, 0, 7)}, b"vh"), ({8: D4(0, 0, 5, -1)}, b"vw"),
           ({8: D4(0, 0, nan, 7)}, b"view")]
    for argv, word in bad:
        rc = raw(dev, m, 5, 7, counts=c, argv=argv)[0]                              # raw() asserts that nothing at all was written
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    rc = L.rdm_depth_frames(_lib.ptr(m), None, 0, None, None, 2, 65536, 32768, None, 0, 1e-3, _lib.ptr(m), None, None, 0, _lib.stream())      # h * w = 2^31: refused before a launch
    assert rc == -1 and b"h * w" in L.rdm_last_error_string()
    assert raw(dev, m, 5, 7, counts=None, argv={4: None, 2: 0})[0] == 0               # without counts neither sid nor count_n is read


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


@pytest.mark.parametrize("flip", [False, True])
def test_predict_metric_is_predict_then_metric_frames(dev, model, flip):
    from md_rdm_amd import depth, evaluate
    x = T(evaluate.synthetic_samples(2, 226, 226)[0], dev)
    got = model.predict_metric(x, (480, 640), view=TEST_VIEW, flip=flip, want=("f32", "u16", "log_scale"))
    lm, counts = model.predict(x, return_counts=True, flip=flip)
    want = depth.metric_frames(lm, (480, 640), view=TEST_VIEW, counts=counts, want=("f32", "u16", "log_scale"))
    assert set(got) == {"f32", "u16", "log_scale"} and got["f32"].shape == (2, 480, 640)
    for k in want:
        assert sp.same_bits(got[k].view(torch.int16) if k == "u16" else got[k], want[k].view(torch.int16) if k == "u16" else want[k]), k
    assert sp.same_bits(counts, model.predict(x, return_counts=True)[1])            # under flip: the unmirrored pass's counts
    assert bool((got["f32"][:, 10:470, 13:627] > 0).all()) and bool((got["f32"][:, :10] == 0).all())


def test_predict_command_metric_native_png16(dev, tmp_path, monkeypatch):
    from PIL import Image
    from md_rdm_amd import depth, predict
    frames = (filler.unit("dframe.frames", 2 * 480 * 640 * 3) * 256.0).astype(np.uint8).reshape(2, 480, 640, 3)
    for i in range(2):
        np.save(str(tmp_path / ("frame%d.npy" % i)), frames[i])
    calls, real = [], depth.metric_frames

    def recording(log_map, frame_hw, **kw):                                        # the command's own launch: its arguments and the planes the kernel wrote
        calls.append((tuple(frame_hw), kw, real(log_map, frame_hw, **kw)))
        return calls[-1][2]
    monkeypatch.setattr(depth, "metric_frames", recording)
    out = tmp_path / "maps"
    assert predict.main([str(tmp_path / "frame0.npy"), str(tmp_path / "frame1.npy"), "--out", str(out), "--metric", "--native", "--png16"]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["frame0.npy", "frame0_depth.png", "frame1.npy", "frame1_depth.png"]
    assert len(calls) == 1                                                          # one launch for the batch of two
    frame_hw, kw, planes = calls[0]
    assert frame_hw == (480, 640) and tuple(kw["view"]) == TEST_VIEW and kw["counts"].shape == (2, 1, 8, 8) and kw["outside"] == "zero" and kw["unit"] == 1e-3
    assert kw["sid"] == "nyu" and kw["offset"] == 0.0 and set(kw["want"]) == {"f32", "u16"}
    for i in range(2):
        d = np.load(str(out / ("frame%d.npy" % i)))
        assert d.dtype == np.float32 and d.shape == (1, 480, 640)
        np.testing.assert_array_equal(d[0], planes["f32"][i].cpu().numpy())
        with Image.open(str(out / ("frame%d_depth.png" % i))) as im:
            assert im.mode == "I;16"
            png = np.asarray(im)
        np.testing.assert_array_equal(png, planes["u16"][i].cpu().numpy())        # the PNG is the kernel's u16 plane
        assert (png[:10] == 0).all() and (png[470:] == 0).all() and (d[0, :10] == 0).all() and (d[0, 470:] == 0).all()      # above row 9.6 and below row 470.4
        assert (d[0, 10:470, 13:627] > 0).all()
        # the two planes are one launch's: the u16 plane quantises the float64 depth that the float32 plane holds to half a float32 ulp
        q = d[0].astype(np.float64) / 1e-3
        assert (np.abs(png.astype(np.float64) - np.minimum(q, 65535.0)) <= 0.5 + q * 2.0 ** -23).all()


def test_evaluate_scale_sid(dev, model):
    from md_rdm_amd import depth, evaluate, harness
    from md_rdm_amd.metrics import StandardMetrics
    xs, ys = evaluate.synthetic_samples(3, 226, 226)
    x, y = T(xs, dev), T(ys, dev)
    batches = [(x[:2], y[:2]), (x[2:], y[2:])]
    sm = StandardMetrics(align="none")
    plain, maps = harness.evaluate(model, batches, sm, return_maps=True)
    assert harness.evaluate(model, batches, sm, scale=None) == plain == harness.evaluate(model, batches, sm)
    res, shifted = harness.evaluate(model, batches, sm, scale="sid", return_maps=True)
    rows = []
    for lo, hi in ((0, 2), (2, 3)):
        counts = model.predict(x[lo:hi], return_counts=True)[1]
        by_hand = maps[lo:hi] + depth.sid_log_scale(counts).reshape(-1, 1, 1, 1)
        assert sp.same_bits(by_hand, shifted[lo:hi])
        rows.append(sm.compute_rows(by_hand, y[lo:hi]))
    from md_rdm_amd.metrics import mean_over_shards
    values = sm.values_from_rows(torch.cat(rows).cpu())
    assert res["n"] == len(values) == 3 and res["skipped"] == 0 and None not in values
    sums = [0.0] * len(sm.names)
    for v in values:                                                                # per-sample values summed in order, as evaluate does
        for i, s in enumerate(v):
            sums[i] += s
    means, n = mean_over_shards([(sums, 3)])
    assert n == 3 and [res[name] for name in sm.names] == list(means)
    assert res != plain
    k = harness.evaluate(model, batches, sm, scale="sid", sid="kitti", sid_offset=0.5)
    assert k != res
