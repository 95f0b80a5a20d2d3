"""include/rdm_anchor.h and md_rdm_amd.anchor on the MI355X against the numpy statement of the contract (tests/anchor_ref.py).

Tolerances, derived from the contract and never from what the kernels return:
  n_cells, count_out   equal: integers.  The validity tests and the gate compare the same float64 values on both sides, except that |r| carries
                       the logarithm's error: every case asserts of the reference that no |r| lies within 1e-9 of the gate.
  s_cells, log_scale_out, field
                       the only operation that is not a correctly rounded IEEE operation in a stated order (on a tap table both sides form with
                       the C library's exp) is the float64 ln: the device's (ROCm's device library documents 1 ulp for log) and numpy's (the C
                       library's, below 1 ulp) may be 2 ulp apart at the largest |ln a| of the inputs.  anchor_ref.ln_bounds carries that per
                       residual (plus one ulp for each of the two subtractions, which may round the other way on a perturbed operand) through
                       the fixed-order sums (perturbations add up; each addition may round the other way), the fit, the re-centring and the
                       normalised weighted mean, element by element; its docstring states every step.  For these cases the bounds come to a
                       few 1e-13 for s_c (a cell of 64 pixels; they grow with the anchors in a cell) and 1e-14 for the scale and the field.  tests/test_anchor_cpu.py tries the same bound on the reference
                       with a perturbed ln and prints the yardstick (deviations of 4e-15, 2e-16 and 1e-16).
  bit for bit          what no ln enters: a sample without anchors (field +0.0, ls = prior), a zero field through rdm_depth_frames_corrected
                       against rdm_depth_frames (float32 and uint16), repeated calls, a sample alone against the same sample in a batch.
  corrected frames     fed a reference-made field: float32 within one float32 ulp and uint16 equal except at rounding-critical pixels, as
                       tests/test_gpu_depthframe.py holds rdm_depth_frames (the log-domain value is bit-exact, the exponentials differ by ulps).
  fit="median"         ln(median(a) / median(exp(v))): the two exponentials (1 ulp each, relative 2^-52) and the two divisions make the ratio
                       relative 3 * 2^-52 apart at most, which is the distance of the logarithms; plus the 2 ulp of the ln itself.
Every call writes between guard elements, which must stay untouched; a refused call must leave its poisoned outputs untouched."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import anchor_ref as aref
import depthframe_ref as dref
import evalview_ref as vref
import stream_probe as sp
from md_rdm_amd import filler
from md_rdm_amd.dataloaders import nyu

pytestmark = pytest.mark.gpu
F_GUARD, I_GUARD, U_GUARD = -777.0, -0x11111112, 0x7A7A
INF = math.inf
VIEW = (2.5, -3.25, 41.0, 48.5)                  # of a 37x53 frame: rows 2.5 .. 43.5 (past the bottom), columns -3.25 .. 45.25 (past the left edge)
TEST_VIEW = nyu.test_view((480, 640))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def guarded(dev, shape, dtype, fill):
    """(buffer with one guard element at either end, pointer to the payload)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2,), fill, dtype=dtype, device=dev)
    return buf, C.c_void_p(buf.data_ptr() + buf.element_size())


def payload(buf, shape, fill, written):
    a = buf.cpu().numpy()
    assert a[0] == fill and a[-1] == fill, "guards"
    if not written:
        assert (a == fill).all(), "a refused call wrote"
    return a[1:-1].reshape(shape)


# positions: 0 log_map, 1 anchors, 2 prior, 3 batch, 4 h, 5 w, 6 view, 7 cell, 8 min_depth, 9 max_depth, 10 reject, 11 n_cells, 12 s_cells
def raw_cells(dev, m, a, cell, view=None, prior=None, min_depth=0.0, max_depth=INF, reject=INF, argv=None):
    from md_rdm_amd import _lib
    B, h, w = a.shape
    gy, gx = aref.cdiv(h, cell), aref.cdiv(w, cell)
    mt, at, pt = T(m, dev), T(a, dev), None if prior is None else T(np.asarray(prior, np.float64), dev)
    nbuf, nptr = guarded(dev, (B, gy, gx), torch.int32, I_GUARD)
    sbuf, sptr = guarded(dev, (B, gy, gx), torch.float64, F_GUARD)
    args = [_lib.ptr(mt), _lib.ptr(at), _lib.ptr(pt), B, h, w, (C.c_double * 4)(*view) if view is not None else None, cell, min_depth, max_depth, reject, nptr, sptr,
            _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = _lib.lib().rdm_depth_anchor_cells(*args)
    torch.cuda.synchronize()
    return rc, payload(nbuf, (B, gy, gx), I_GUARD, rc == 0), payload(sbuf, (B, gy, gx), F_GUARD, rc == 0)


# positions: 0 n_cells, 1 s_cells, 2 prior, 3 batch, 4 gy, 5 gx, 6 fit, 7 sigma, 8 lambda, 9 log_scale_out, 10 count_out, 11 field
def raw_field(dev, n, s, prior=None, fit=aref.FIT_LOGMEAN, sigma=2.0, lam=1.0, want_field=True, argv=None):
    from md_rdm_amd import _lib
    B, gy, gx = n.shape
    nt, st, pt = T(n.astype(np.int32), dev), T(s, dev), None if prior is None else T(np.asarray(prior, np.float64), dev)
    lbuf, lptr = guarded(dev, (B,), torch.float64, F_GUARD)
    cbuf, cptr = guarded(dev, (B,), torch.int32, I_GUARD)
    fbuf, fptr = guarded(dev, (B, gy, gx), torch.float64, F_GUARD)
    args = [_lib.ptr(nt), _lib.ptr(st), _lib.ptr(pt), B, gy, gx, fit, sigma, lam, lptr, cptr, fptr if want_field else None, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = _lib.lib().rdm_depth_anchor_field(*args)
    torch.cuda.synchronize()
    return rc, payload(lbuf, (B,), F_GUARD, rc == 0), payload(cbuf, (B,), I_GUARD, rc == 0), payload(fbuf, (B, gy, gx), F_GUARD, rc == 0 and want_field)


# positions: 0 log_map .. 14 split as rdm_depth_frames (tests/test_gpu_depthframe.py), 15 field, 16 gy, 17 gx, 18 cell
def raw_frames(dev, m, h, w, ls, F, cell, view=None, outside=0, unit=1e-3, want=("f32", "u16"), corrected=True, argv=None):
    from md_rdm_amd import _lib
    B = m.shape[0]
    mt, lt = T(m, dev), T(np.asarray(ls, np.float64), dev)
    fbuf, fptr = guarded(dev, (B, h, w), torch.float32, F_GUARD)
    ubuf, uptr = guarded(dev, (B, h, w), torch.int16, U_GUARD)
    args = [_lib.ptr(mt), None, 0, _lib.ptr(lt), None, B, h, w, (C.c_double * 4)(*view) if view is not None else None, outside, unit, fptr if "f32" in want else None,
            uptr if "u16" in want else None, None, 0]
    if corrected:
        Ft = T(np.asarray(F, np.float64), dev)
        args += [_lib.ptr(Ft), Ft.shape[1], Ft.shape[2], cell]
    args.append(_lib.stream())
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = (_lib.lib().rdm_depth_frames_corrected if corrected else _lib.lib().rdm_depth_frames)(*args)
    torch.cuda.synchronize()
    return rc, payload(fbuf, (B, h, w), np.float32(F_GUARD), rc == 0 and "f32" in want), payload(ubuf, (B, h, w), U_GUARD, rc == 0 and "u16" in want).view(np.uint16)


def ulps32(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


# ---- the cases: the smallest frames at which the kernels can go wrong ---------------------------------------------------------------------------
# 37x53: w no multiple of 4, ragged last cells at cell 8 (5 x 7 cells of which the last row is 5 pixels and the last column 5 pixels), 35 cells = more
# than one workgroup of four; sample 1 of 3 has no valid anchor; 70x90: crosses k_depth_frames' 32-row chunks twice and the 64-lane stride of a 16x16 cell
CASES = {
    "ragged cells":  dict(B=3, h=37, w=53, view=None, cell=8, fit="logmean", sigma=1.5, lam=0.5, reject=INF),
    "partial view":  dict(B=3, h=37, w=53, view=VIEW, cell=8, fit="none", sigma=1.0, lam=1.0, reject=0.6),
    "one cell":      dict(B=3, h=37, w=53, view=VIEW, cell=64, fit="none", sigma=2.0, lam=1.0, reject=INF),          # (logmean would leave one cell a field of rounding)
    "sigma 0":       dict(B=3, h=37, w=53, view=None, cell=8, fit="logmean", sigma=0.0, lam=0.0, reject=INF),
    "wide sigma":    dict(B=3, h=37, w=53, view=None, cell=8, fit="none", sigma=4.0, lam=1.0, reject=INF),       # Rg = 12 > 7 x 5 cells
    "70x90 chunks":  dict(B=2, h=70, w=90, view=(1.5, 2.25, 66.0, 85.5), cell=16, fit="logmean", sigma=1.0, lam=1.0, reject=1.5),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and the reference of a case, computed once and shared by the tests"""
    c = CASES[name]
    B, h, w = c["B"], c["h"], c["w"]
    key = "anchor.gpu/%s" % name
    m = filler.uniform(key + "/map", (B, 1, 128, 128), -1.5, 1.5, dtype=np.float64)
    v = vref.resize_view(m, h, w, c["view"])[:, 0]
    tilt = 0.4 * ((np.arange(h) + 0.5) / h - 0.5)[None, :, None]                      # something for the field to find: -0.2 at the top to 0.2 at the bottom
    a = np.exp(v + tilt + filler.uniform(key + "/off", (B, h, w), -0.3, 0.9, dtype=np.float64)).astype(np.float32)
    a[filler.unit(key + "/holes", B * h * w).reshape(B, h, w) < 0.3] = 0.0
    if B == 3:
        a[1] = 0.0
        a[1, 3, 4], a[1, 5, 6], a[1, 7, 8] = np.nan, -2.0, np.inf                   # not anchors either
    prior = filler.uniform(key + "/prior", (B,), 0.1, 0.5, dtype=np.float64)
    fit = aref.FIT_LOGMEAN if c["fit"] == "logmean" else aref.FIT_NONE
    r, keep, _ = aref.residuals(m, a, c["view"], prior, reject=c["reject"])
    valid = aref.residuals(m, a, c["view"], prior)[1]
    assert (np.abs(np.abs(r[valid]) - c["reject"]) > 1e-9).all() if math.isfinite(c["reject"]) else True
    n, s = aref.cells(m, a, c["cell"], c["view"], prior, reject=c["reject"])
    ls, count, F = aref.field(n, s, prior, fit, c["sigma"], c["lam"])
    E = aref.ln_bounds(m, a, c["cell"], c["view"], prior, fit, c["sigma"], c["lam"], c["reject"])
    assert E["s"].max() < 1e-11 * max(1, c["cell"] // 16) ** 2 and E["ls"].max() < 1e-12 and E["field"].max() < 1e-12      # rounding-level bounds, whatever the case
    return dict(c, m=m, a=a, prior=prior, fitc=fit, keep=keep, valid=valid, n=n, s=s, ls=ls, count=count, F=F, E=E)


@pytest.mark.parametrize("name", list(CASES))
def test_cells_fit_and_field(dev, name):
    c = case(name)
    if name == "partial view":
        inside = dref.inside_mask(c["h"], c["w"], c["view"])
        assert (c["a"][0][~inside] > 0).any() and not c["valid"][:, ~inside].any()    # anchors outside the view exist and are ignored
        assert c["valid"].sum() > c["keep"].sum() > 0                                 # and the gate drops some of the others
    if c["B"] == 3:
        assert c["count"][1] == 0 and c["count"][0] > 0 and c["count"][2] > 0
    rc, n, s = raw_cells(dev, c["m"], c["a"], c["cell"], c["view"], c["prior"], reject=c["reject"])
    assert rc == 0
    np.testing.assert_array_equal(n, c["n"])
    print(name, "s_c: %.3g of %.3g" % (np.abs(s - c["s"]).max(), c["E"]["s"].max()))
    assert (np.abs(s - c["s"]) <= c["E"]["s"]).all()
    assert (s[c["n"] == 0] == 0).all() and not np.signbit(s[c["n"] == 0]).any()
    # launch 2 on the DEVICE's cell sums (the chain a caller runs) and on the reference's (launch 2 alone: every step stated, so bit for bit)
    rc, ls, count, F = raw_field(dev, n, s, c["prior"], c["fitc"], c["sigma"], c["lam"])
    assert rc == 0
    np.testing.assert_array_equal(count, c["count"])
    print(name, "ls: %.3g of %.3g, field: %.3g of %.3g" % (np.abs(ls - c["ls"]).max(), c["E"]["ls"].max(), np.abs(F - c["F"]).max(), c["E"]["field"].max()))
    assert (np.abs(ls - c["ls"]) <= c["E"]["ls"]).all() and (np.abs(F - c["F"]) <= c["E"]["field"]).all()
    rc, ls2, count2, F2 = raw_field(dev, c["n"], c["s"], c["prior"], c["fitc"], c["sigma"], c["lam"])
    assert rc == 0 and ls2.tobytes() == c["ls"].tobytes() and count2.tobytes() == c["count"].tobytes() and F2.tobytes() == c["F"].tobytes()
    if c["B"] == 3:                                                                   # the sample without anchors: no ln involved
        assert ls[1] == c["prior"][1] and (F[1] == 0).all() and not np.signbit(F[1]).any()
    only = raw_field(dev, n, s, c["prior"], c["fitc"], c["sigma"], c["lam"], want_field=False)       # field NULL: the fit alone, nothing else written
    assert only[0] == 0 and only[1].tobytes() == ls.tobytes() and only[2].tobytes() == count.tobytes()


def test_no_prior_and_depth_range(dev):
    c = case("ragged cells")
    rc, n, s = raw_cells(dev, c["m"], c["a"], 8, min_depth=0.5, max_depth=2.0)
    rn, rs = aref.cells(c["m"], c["a"], 8, min_depth=0.5, max_depth=2.0)
    E = aref.ln_bounds(c["m"], c["a"], 8, min_depth=0.5, max_depth=2.0)
    assert rc == 0 and 0 < rn.sum() < c["valid"].sum()
    np.testing.assert_array_equal(n, rn)
    assert (np.abs(s - rs) <= E["s"]).all()
    rc, ls, count, F = raw_field(dev, n, s)
    rls, rcount, rF = aref.field(rn, rs)
    assert rc == 0 and (count == rcount).all() and ls[1] == 0 and (np.abs(ls - rls) <= E["ls"]).all() and (np.abs(F - rF) <= E["field"]).all()


@pytest.mark.parametrize("name", ["ragged cells", "partial view", "one cell", "70x90 chunks"])
def test_corrected_frames(dev, name):
    c = case(name)
    h, w, cell, view = c["h"], c["w"], c["cell"], c["view"]
    zeros = np.zeros_like(c["F"])
    for outside in (0, 1):
        plain = raw_frames(dev, c["m"], h, w, c["ls"], None, cell, view, outside, corrected=False)
        zero = raw_frames(dev, c["m"], h, w, c["ls"], zeros, cell, view, outside)
        assert plain[0] == 0 and zero[0] == 0 and plain[1].tobytes() == zero[1].tobytes() and plain[2].tobytes() == zero[2].tobytes()
        r = aref.frames(c["m"], h, w, c["ls"], c["F"], cell, view, outside=("zero", "edge")[outside])
        assert r["critical"].mean() <= 1e-3 and np.abs(c["F"]).max() > 0.01
        rc, f, u = raw_frames(dev, c["m"], h, w, c["ls"], c["F"], cell, view, outside)
        assert rc == 0 and ulps32(f, r["f32"]) <= 1, (name, outside, ulps32(f, r["f32"]))
        d = np.abs(u.astype(np.int64) - r["u16"].astype(np.int64))
        assert (d[~r["critical"]] == 0).all() and (d <= 1).all()
        if outside == 0:
            assert (f[:, ~r["inside"]] == 0).all() and (u[:, ~r["inside"]] == 0).all()
        assert ulps32(plain[1], r["f32"]) > 1                                         # the field is not a no-op
    only_f = raw_frames(dev, c["m"], h, w, c["ls"], c["F"], cell, view, want=("f32",))
    both = raw_frames(dev, c["m"], h, w, c["ls"], c["F"], cell, view)
    assert only_f[0] == 0 and only_f[1].tobytes() == both[1].tobytes()


def test_repeated_and_alone(dev):
    c = case("partial view")
    m, a, p = c["m"], c["a"], c["prior"]
    first = raw_cells(dev, m, a, 8, VIEW, p, reject=0.6)
    again = raw_cells(dev, m, a, 8, VIEW, p, reject=0.6)
    assert first[0] == 0 and first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    f1 = raw_field(dev, first[1], first[2], p, aref.FIT_LOGMEAN, 1.0, 1.0)
    f2 = raw_field(dev, first[1], first[2], p, aref.FIT_LOGMEAN, 1.0, 1.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(f1[1:], f2[1:]))
    d1 = raw_frames(dev, m, 37, 53, f1[1], f1[3], 8, VIEW)
    d2 = raw_frames(dev, m, 37, 53, f1[1], f1[3], 8, VIEW)
    assert d1[1].tobytes() == d2[1].tobytes() and d1[2].tobytes() == d2[2].tobytes()
    for b in range(3):
        one = raw_cells(dev, m[b:b + 1], a[b:b + 1], 8, VIEW, p[b:b + 1], reject=0.6)
        assert one[1][0].tobytes() == first[1][b].tobytes() and one[2][0].tobytes() == first[2][b].tobytes(), b
        fo = raw_field(dev, first[1][b:b + 1], first[2][b:b + 1], p[b:b + 1], aref.FIT_LOGMEAN, 1.0, 1.0)
        assert fo[1][0] == f1[1][b] and fo[2][0] == f1[2][b] and fo[3][0].tobytes() == f1[3][b].tobytes(), b
        do = raw_frames(dev, m[b:b + 1], 37, 53, f1[1][b:b + 1], f1[3][b:b + 1], 8, VIEW)
        assert do[1][0].tobytes() == d1[1][b].tobytes() and do[2][0].tobytes() == d1[2][b].tobytes(), b


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -------------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib
    c = case("partial view")
    ins = dict(m=T(c["m"], dev), a=T(c["a"], dev), p=T(c["prior"], dev))
    scratch = dict(n=torch.empty(3, 5, 7, dtype=torch.int32, device=dev), s=torch.empty(3, 5, 7, dtype=torch.float64, device=dev),
                   ls=torch.empty(3, dtype=torch.float64, device=dev), count=torch.empty(3, dtype=torch.int32, device=dev),
                   F=torch.empty(3, 5, 7, dtype=torch.float64, device=dev), f=torch.empty(3, 37, 53, dtype=torch.float32, device=dev),
                   u=torch.empty(3, 37, 53, dtype=torch.int16, device=dev))
    view = (C.c_double * 4)(*VIEW)

    def call(b, st):
        L = _lib.lib()
        _lib.check(L.rdm_depth_anchor_cells(_lib.ptr(b["m"]), _lib.ptr(b["a"]), _lib.ptr(b["p"]), 3, 37, 53, view, 8, 0.0, INF, 0.6, _lib.ptr(b["n"]), _lib.ptr(b["s"]), st))
        _lib.check(L.rdm_depth_anchor_field(_lib.ptr(b["n"]), _lib.ptr(b["s"]), _lib.ptr(b["p"]), 3, 5, 7, 1, 1.0, 1.0, _lib.ptr(b["ls"]), _lib.ptr(b["count"]), _lib.ptr(b["F"]), st))
        _lib.check(L.rdm_depth_frames_corrected(_lib.ptr(b["m"]), None, 0, _lib.ptr(b["ls"]), None, 3, 37, 53, view, 0, 1e-3, _lib.ptr(b["f"]), _lib.ptr(b["u"]), None, 0,
                                                _lib.ptr(b["F"]), 5, 7, 8, st))
        from md_rdm_amd import anchor                                                 # the wrappers resolve the stream themselves
        fitted = anchor.fit(b["m"], b["a"], view=VIEW, prior=b["p"], cell=8, sigma=1.0, lam=1.0, reject=0.6)
        out = anchor.metric_frames(b["m"], (37, 53), fitted, view=VIEW, want=("f32", "u16"))
        return dict(w_ls=fitted["log_scale"], w_count=fitted["count"], w_F=fitted["field"], w_f=out["f32"], w_u=out["u16"].view(torch.int16))
    return sp.Case(ins, call, outs=tuple(scratch), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_three_launches_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    c = case("partial view")
    np.testing.assert_array_equal(got["n"].cpu().numpy(), c["n"])
    for k, w in (("ls", "w_ls"), ("count", "w_count"), ("F", "w_F"), ("f", "w_f"), ("u", "w_u")):
        assert sp.same_bits(got[k], got[w]), k


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    c = case("ragged cells")
    D4, nan, odd = C.c_double * 4, math.nan, lambda t, k: C.c_void_p(t.data_ptr() + k)
    keep = T(np.zeros(64), dev)
    bad = [({0: None}, b"log_map"), ({1: None}, b"anchors"), ({11: None}, b"n_cells"), ({12: None}, b"s_cells"), ({0: odd(keep, 4)}, b"8-byte"), ({2: odd(keep, 4)}, b"8-byte"),
           ({12: odd(keep, 4)}, b"8-byte"), ({1: odd(keep, 2)}, b"4-byte"), ({11: odd(keep, 2)}, b"4-byte"), ({3: 0}, b"batch"), ({4: 0}, b"h"), ({5: -1}, b"w"),
           ({3: 65536}, b"grid limit"), ({7: 0}, b"cell"), ({7: -8}, b"cell"), ({8: -1.0}, b"min_depth"), ({8: nan}, b"min_depth"), ({9: nan}, b"max_depth"),
           ({8: 2.0, 9: 1.0}, b"max_depth"), ({10: nan}, b"reject"), ({10: 0.0}, b"reject"), ({10: -1.0}, b"reject"), ({10: 0.5, 2: None}, b"needs a prior"),
           ({6: D4(nan, 0, 5, 7)}, b"view"), ({6: D4(0, 0, 0, 7)}, b"vh"), ({6: D4(0, 0, 5, -1)}, b"vw"), ({6: D4(0, math.inf, 5, 7)}, b"view")]
    for argv, word in bad:
        rc = raw_cells(dev, c["m"], c["a"], 8, None, c["prior"], argv=argv)[0]      # raw_cells asserts that nothing at all was written
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    assert raw_cells(dev, c["m"], c["a"], 8, None, None, reject=INF)[0] == 0         # reject off needs no prior
    bad = [({0: None}, b"n_cells"), ({1: None}, b"s_cells"), ({9: None}, b"log_scale_out"), ({10: None}, b"count_out"), ({1: odd(keep, 4)}, b"8-byte"),
           ({2: odd(keep, 4)}, b"8-byte"), ({9: odd(keep, 4)}, b"8-byte"), ({11: odd(keep, 4)}, b"8-byte"), ({0: odd(keep, 2)}, b"4-byte"), ({10: odd(keep, 2)}, b"4-byte"),
           ({3: 0}, b"batch"), ({4: 0}, b"gy"), ({5: -1}, b"gx"), ({3: 65536}, b"grid limit"), ({4: 5121, 5: 1}, b"LDS"), ({4: 65, 5: 80}, b"LDS"), ({6: 2}, b"fit"),
           ({6: -1}, b"fit"), ({7: -0.5}, b"sigma"), ({7: nan}, b"sigma"), ({7: math.inf}, b"sigma"), ({7: 32.5}, b"radius"), ({8: -1.0}, b"lambda"), ({8: nan}, b"lambda"),
           ({8: math.inf}, b"lambda")]
    for argv, word in bad:
        rc = raw_field(dev, c["n"], c["s"], c["prior"], argv=argv)[0]
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    bad = [({15: None}, b"field"), ({15: odd(keep, 4)}, b"field"), ({18: 0}, b"cell"), ({16: 4}, b"ceil"), ({17: 8}, b"ceil"), ({18: 16}, b"ceil"), ({0: None}, b"log_map"),
           ({11: None, 12: None}, b"depth_f32"), ({5: 0}, b"batch"), ({6: 0}, b"h"), ({10: 0.0}, b"unit"), ({9: 2}, b"outside"), ({14: -1}, b"split"),
           ({8: D4(0, 0, nan, 7)}, b"view")]
    for argv, word in bad:
        rc = raw_frames(dev, c["m"], 37, 53, c["ls"], c["F"], 8, argv=argv)[0]
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    rc, n, s = raw_cells(dev, c["m"][:1], np.full((1, 60 * 8, 80 * 8), 1.5, np.float32), 8)       # 60 x 80 cells, the native frame at cell 8, fits the LDS
    assert rc == 0 and raw_field(dev, n, s)[0] == 0


# ---- the wrapper --------------------------------------------------------------------------------------------------------------------------------
def test_fit_wrapper_and_median(dev):
    from md_rdm_amd import _lib, anchor
    c = case("partial view")
    mt, at, pt = T(c["m"], dev), T(c["a"], dev), T(c["prior"], dev)
    f = anchor.fit(mt, at, view=VIEW, prior=pt, fit="none", cell=8, sigma=1.0, lam=1.0, reject=0.6)
    assert f["cell"] == 8 and f["count"].dtype == torch.int32 and f["field"].shape == (3, 5, 7)
    np.testing.assert_array_equal(f["count"].cpu().numpy(), c["count"])
    assert (np.abs(f["log_scale"].cpu().numpy() - c["ls"]) <= c["E"]["ls"]).all() and (np.abs(f["field"].cpu().numpy() - c["F"]) <= c["E"]["field"]).all()
    assert anchor.fit(mt, at, view=VIEW, prior=pt, field=False)["field"] is None
    # median: ln of the ratio of medians, to 4 * 2^-52 + 2 ulp(|ln|); the sample without a valid anchor keeps its prior, bit for bit
    for prior in (pt, None):
        med = anchor.fit(mt, at, view=VIEW, prior=prior, fit="median", cell=8, sigma=1.0, lam=1.0, reject=0.6, max_depth=50.0)
        want = aref.median_log_scale(c["m"], c["a"], VIEW, None if prior is None else c["prior"], 0.0, 50.0)
        got = med["log_scale"].cpu().numpy()
        assert (np.abs(got - want) <= 4 * 2.0 ** -52 + 2 * np.spacing(np.abs(want))).all(), (got, want)
        assert got[1] == (c["prior"][1] if prior is not None else 0.0) and np.isfinite(got).all()
        r = aref.fit(c["m"], c["a"], VIEW, None if prior is None else c["prior"], "median", 8, 1.0, 1.0, 0.6, 0.0, 50.0)
        np.testing.assert_array_equal(med["count"].cpu().numpy(), r["count"])
        assert np.abs(med["field"].cpu().numpy() - r["field"]).max() < 1e-12
    only_scale = anchor.metric_frames(mt, (37, 53), anchor.fit(mt, at, view=VIEW, prior=pt, field=False), view=VIEW)
    from md_rdm_amd import depth
    assert sp.same_bits(only_scale["f32"], depth.metric_frames(mt, (37, 53), view=VIEW, log_scale=anchor.fit(mt, at, view=VIEW, prior=pt, field=False)["log_scale"])["f32"])
    for kw, word in ((dict(fit="mean"), "fit"), (dict(cell=0), "cell"), (dict(sigma=40.0), "radius"), (dict(reject=0.5), "needs a prior"), (dict(cell=1, view=None), "cells")):
        with pytest.raises(_lib.RdmError, match=word):
            anchor.fit(mt, T(np.zeros((3, 80, 80), np.float32), dev) if word == "cells" else at, **kw)


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


def test_predict_metric_with_anchors(dev, model):
    from md_rdm_amd import evaluate
    x = T(evaluate.synthetic_samples(2, 226, 226)[0], dev)
    plain = model.predict_metric(x, (480, 640), view=TEST_VIEW, want=("f32", "u16", "log_scale"))
    u = plain["f32"].cpu().numpy().astype(np.float64)
    inside = dref.inside_mask(480, 640, TEST_VIEW)
    assert np.isfinite(u).all() and (u[:, inside] > 0).all()
    mask = filler.unit("anchor.gpu/e2e", 2 * 480 * 640).reshape(2, 480, 640) < 0.005
    A = np.where(mask, u * 1.37, 0.0).astype(np.float32)
    assert np.isfinite(A).all() and 0.004 < mask.mean() < 0.006
    got = model.predict_metric(x, (480, 640), view=TEST_VIEW, want=("f32", "u16", "log_scale"), anchors=T(A, dev))
    g = got["f32"].cpu().numpy().astype(np.float64)
    target = 1.37 * u
    assert (np.abs(g - target)[:, inside] < np.abs(u - target)[:, inside]).all()     # closer to the anchored scale at EVERY pixel inside the view
    assert (g[:, ~inside] == 0).all()
    assert np.abs((got["log_scale"] - plain["log_scale"]).cpu().numpy() - math.log(1.37)).max() < 1e-6
    again = model.predict_metric(x, (480, 640), view=TEST_VIEW, want=("f32", "u16", "log_scale"), anchors=None)
    for k in plain:
        assert sp.same_bits(again[k].view(torch.int16) if k == "u16" else again[k], plain[k].view(torch.int16) if k == "u16" else plain[k]), k
    no_field = model.predict_metric(x, (480, 640), view=TEST_VIEW, anchors=T(A, dev), anchor=dict(fit="median", field=False, reject=0.5))
    assert (np.abs(no_field["f32"].cpu().numpy() - target)[:, inside] < 0.37 * u[:, inside]).all()
    from md_rdm_amd import _lib
    with pytest.raises(_lib.RdmError, match="need anchors"):
        model.predict_metric(x, (480, 640), anchor=dict(cell=8))
    with pytest.raises(_lib.RdmError, match="anchor must be a dict"):
        model.predict_metric(x, (480, 640), anchors=T(A, dev), anchor=dict(radius=3))


def test_predict_command_anchors(dev, tmp_path, monkeypatch):
    from md_rdm_amd import anchor, predict, viz
    frames = (filler.unit("anchor.gpu/frames", 2 * 480 * 640 * 3) * 256.0).astype(np.uint8).reshape(2, 480, 640, 3)
    steps = np.where(filler.unit("anchor.gpu/cmd", 2 * 480 * 640).reshape(2, 480, 640) < 0.01, 2500, 0).astype(np.uint16)      # 2.5 m at 1 % of the pixels
    for i in range(2):
        np.save(str(tmp_path / ("frame%d.npy" % i)), frames[i])
    np.save(str(tmp_path / "a0.npy"), (steps[0].astype(np.float64) * 1e-3).astype(np.float32))
    viz.write_png16(str(tmp_path / "a1.png"), steps[1])
    calls, real_fit, real_frames = [], anchor.fit, anchor.metric_frames

    def fit(log_map, anchors, **kw):
        calls.append(("fit", anchors, kw, real_fit(log_map, anchors, **kw)))
        return calls[-1][3]

    def metric_frames(log_map, frame_hw, fitted, **kw):
        calls.append(("frames", tuple(frame_hw), kw, real_frames(log_map, frame_hw, fitted, **kw)))
        return calls[-1][3]
    monkeypatch.setattr(anchor, "fit", fit)
    monkeypatch.setattr(anchor, "metric_frames", metric_frames)
    out = tmp_path / "maps"
    assert predict.main([str(tmp_path / "frame0.npy"), str(tmp_path / "frame1.npy"), "--out", str(out), "--metric", "--native", "--png16", "--anchors",
                         str(tmp_path / "a0.npy"), str(tmp_path / "a1.png"), "--anchor_cell", "8", "--anchor_sigma", "1.5", "--max_depth", "10"]) == 0
    assert [c[0] for c in calls] == ["fit", "frames"]                                # one fit and one frame launch for the batch of two
    _, anchors, kw, fitted = calls[0]
    np.testing.assert_array_equal(anchors.cpu().numpy(), (steps.astype(np.float64) * 1e-3).astype(np.float32))      # the .npy and the PNG read alike
    assert kw["cell"] == 8 and kw["sigma"] == 1.5 and kw["max_depth"] == 10.0 and kw["field"] is True and tuple(kw["view"]) == TEST_VIEW and kw["prior"].shape == (2,)
    inside = dref.inside_mask(480, 640, TEST_VIEW)
    np.testing.assert_array_equal(fitted["count"].cpu().numpy(), (steps > 0)[:, inside].sum(axis=1))
    _, frame_hw, kw, planes = calls[1]
    assert frame_hw == (480, 640) and set(kw["want"]) == {"f32", "u16"}
    for i in range(2):
        d = np.load(str(out / ("frame%d.npy" % i)))
        np.testing.assert_array_equal(d[0], planes["f32"][i].cpu().numpy())          # the .npy is the anchored plane
        np.testing.assert_array_equal(viz.read_png16(str(out / ("frame%d_depth.png" % i))), planes["u16"][i].cpu().numpy())
        assert (d[0][~inside] == 0).all() and (d[0][inside] > 0).all()
    with pytest.raises(SystemExit, match="the anchors are 5x7"):
        np.save(str(tmp_path / "small.npy"), np.zeros((5, 7), np.float32))
        predict.main([str(tmp_path / "frame0.npy"), "--out", str(out), "--metric", "--native", "--anchors", str(tmp_path / "small.npy")])
