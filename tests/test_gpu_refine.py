"""rdm_depth_refine (include/rdm_refine.h) and md_rdm_amd.refine on the MI355X against the numpy statement of the contract (tests/refine_ref.py).

EXACT cases are compared bit for bit: with both sigmas +inf every weight is 1.0, with small-integer depths both sums are exact, and the quotient
and the two conversions are correctly rounded on both sides - an indexing, halo, validity or tap-skipping mistake has no slack to hide in.
GENERAL cases (finite sigmas) differ from the reference only in the last bits of `exp` in the tables (the device's against numpy's): that moves the
float64 D by a relative 1e-14 at most over 289 taps, which changes the float32 rounding only at a rounding boundary and then by one step - so
the bound is ONE float32 step, derived, and the test prints how many elements differ at all (`worst` keeps the module's figures; measured: see
DESIGN.md 4.12).  The uint16 plane must equal the reference wherever the reference's q is farther than 1e-9 from a half-integer, and the test asserts
that for its seeds that is everywhere.  The set of invalid pixels must be equal outright.
Every call writes between guard elements in front of and behind both planes, which must stay untouched; the base addresses are shifted by 0..3
elements."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import refine_ref as rref
import stream_probe as sp
from conftest import ROOT
from md_rdm_amd import filler
from md_rdm_amd.dataloaders import nyu

pytestmark = pytest.mark.gpu
G, FGUARD, UGUARD = 64, 0x5A5A5A5A, 0xA5A5                 # guard elements in front and behind; their bits
INF = math.inf
PARAMS = [(1, 1), (3, 4), (8, 3), (2, 12)]                  # (radius, step): halo 1, the default 12, and 24 reached both ways
worst = {"f32_steps": 0, "f32_differing": 0, "f32_elements": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)              # a copy: the cached frames are read-only


@functools.lru_cache(maxsize=None)
def frame(key, B, h, w, exact=False, guide="random", dead=None):
    """(depth (B,h,w) float32, guide (B,h,w,3) uint8), hash-generated; read-only.  Depth in [0.5, 9.5) (exact: the integers 1..9) with a quarter
    of zeros and, where the batch has room, one NaN, one inf and one negative; ``dead``: that sample has no valid depth at all.
    guide "blocks": constant over 4x4 blocks, so equal colours occur."""
    d = filler.uniform("refine.depth/" + key, (B, h, w), 0.5, 9.5).astype(np.float32)
    if exact:
        d = np.floor(filler.uniform("refine.depth/" + key, (B, h, w), 1.0, 10.0)).astype(np.float32)
    d[filler.unit("refine.mask/" + key, B * h * w).reshape(B, h, w) < 0.25] = 0.0
    n = B * h * w
    if n >= 16:
        flat = d.reshape(-1)
        at = (filler.unit("refine.special/" + key, 3) * n).astype(np.int64)
        flat[at[0]], flat[at[1]], flat[at[2]] = np.nan, np.inf, -2.0
    if dead is not None:
        d[dead] = 0.0
    g = (filler.unit("refine.rgb/" + key, n * 3) * 256.0).astype(np.uint8).reshape(B, h, w, 3)
    if guide == "blocks":
        yy, xx = np.mgrid[0:h, 0:w]
        g = g[:, (yy // 4) * 4, (xx // 4) * 4]
    g = np.ascontiguousarray(g)
    d.setflags(write=False)
    g.setflags(write=False)
    return d, g


@functools.lru_cache(maxsize=None)
def reference(key, B, h, w, exact, guide, dead, radius, step, ss, sc, fill, unit=1e-3):
    d, g = frame(key, B, h, w, exact, guide, dead)
    out = rref.reference(d, g, radius, step, ss, sc, fill, unit)
    for v in out.values():
        v.setflags(write=False)
    return out


def raw(dev, d, g, radius, step, ss, sc, fill, unit=1e-3, f32=True, u16=True, shift=0, argv=None):
    """one call of the C entry -> (rc, f32 (B,h,w) | None, u16 (B,h,w) | None); asserts the guards"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    dt = d if isinstance(d, torch.Tensor) else T(d, dev)
    gt = g if isinstance(g, torch.Tensor) else T(g, dev)
    B, h, w = dt.shape
    n = B * h * w
    fbuf = torch.full((G + shift + n + G,), FGUARD, dtype=torch.int32, device=dev)
    ubuf = torch.full((G + shift + n + G,), UGUARD - 65536, dtype=torch.int16, device=dev)
    assert fbuf.data_ptr() % 16 == 0 and ubuf.data_ptr() % 16 == 0
    args = [_lib.ptr(dt), _lib.ptr(gt), B, h, w, radius, step, ss, sc, 1 if fill else 0, unit, C.c_void_p(fbuf.data_ptr() + 4 * (G + shift)) if f32 else None,
            C.c_void_p(ubuf.data_ptr() + 2 * (G + shift)) if u16 else None, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_depth_refine(*args)
    torch.cuda.synchronize()
    fo, uo = fbuf.cpu().numpy(), ubuf.cpu().numpy().view(np.uint16)
    lo, hi = G + shift, G + shift + n
    assert (fo[:lo] == FGUARD).all() and (fo[hi:] == FGUARD).all(), "guards around the float32 plane"
    assert (uo[:lo] == UGUARD).all() and (uo[hi:] == UGUARD).all(), "guards around the uint16 plane"
    if rc != 0 or not f32:
        assert (fo == FGUARD).all(), "the float32 buffer was written"
    if rc != 0 or not u16:
        assert (uo == UGUARD).all(), "the uint16 buffer was written"
    if rc != 0:
        return rc, None, None
    return rc, fo[lo:hi].view(np.float32).reshape(B, h, w).copy() if f32 else None, uo[lo:hi].reshape(B, h, w).copy() if u16 else None


def steps_between(a, b):
    """distance in float32 steps, elementwise (both finite)"""
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))
    return np.abs(key(np.ascontiguousarray(a)) - key(np.ascontiguousarray(b)))


def compare_exact(got, want, what):
    rc, f, u = got
    assert rc == 0, what
    np.testing.assert_array_equal(f.view(np.int32), want["f32"].view(np.int32), err_msg=what + ": float32 plane")
    np.testing.assert_array_equal(u, want["u16"], err_msg=what + ": uint16 plane")


def compare_general(got, want, what):
    rc, f, u = got
    assert rc == 0, what
    assert np.isfinite(f).all(), what
    np.testing.assert_array_equal(f != 0, want["ok"], err_msg=what + ": the set of invalid pixels")        # a valid D is > 0
    assert (u[~want["ok"]] == 0).all() and (f[~want["ok"]] == 0).all(), what
    st = steps_between(f, want["f32"])
    worst["f32_steps"] = max(worst["f32_steps"], int(st.max()))
    worst["f32_differing"] += int((st > 0).sum())
    worst["f32_elements"] += st.size
    print("%s: float32 plane: %d of %d elements differ, by at most %d step(s) (module: %d of %d, worst %d)" % (
        what, int((st > 0).sum()), st.size, int(st.max()), worst["f32_differing"], worst["f32_elements"], worst["f32_steps"]))
    q = want["q"][want["ok"]]
    clear = np.abs(q - np.floor(q) - 0.5) > 1e-9
    assert clear.all(), "%s: %d reference pixels lie within 1e-9 of a half-integer: choose another seed" % (what, int((~clear).sum()))
    print("%s: uint16 plane: %d of %d elements differ" % (what, int((u != want["u16"]).sum()), u.size))
    assert int(st.max()) <= 1, what
    np.testing.assert_array_equal(u, want["u16"], err_msg=what + ": uint16 plane")


# ---- exact cases: both sigmas +inf, small-integer depths, bit for bit --------------------------------------------------------------------------
# (1,1); two frames smaller than the halo in one or both directions; one 32 x 16 tile exactly; one tile plus 1 row and 3 columns; several ragged tiles
FRAMES = [(1, 1), (5, 7), (3, 200), (16, 32), (17, 35), (37, 53)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_exact_frames(dev, h, w, B):
    dead = 1 if B == 3 else None                                  # an all-invalid sample inside the batch
    d, g = frame("exact", B, h, w, True, "random", dead)
    dt, gt = T(d, dev), T(g, dev)
    for shift, (radius, step) in enumerate(PARAMS):
        for fill in (False, True):
            want = reference("exact", B, h, w, True, "random", dead, radius, step, INF, INF, fill)
            if dead is not None:
                assert not want["ok"][dead].any() and (want["f32"][dead] == 0).all()
            compare_exact(raw(dev, dt, gt, radius, step, INF, INF, fill, shift=shift), want, "%dx%d B=%d r=%d s=%d fill=%d" % (h, w, B, radius, step, fill))


def test_exact_with_the_colour_term_alone_switched_off_by_equal_colours(dev):
    """a constant guide makes every E factor E[0] = 1.0 whatever sigma_color is: still exact, and the E reads all hit one address"""
    d, _ = frame("const", 2, 37, 53, True)
    g = np.full((2, 37, 53, 3), 201, dtype=np.uint8)
    for radius, step in PARAMS:
        want = rref.reference(d, g, radius, step, INF, 3.0, True)
        compare_exact(raw(dev, d, g, radius, step, INF, 3.0, True), want, "constant guide r=%d s=%d" % (radius, step))


# ---- general cases: finite sigmas, within one float32 step -------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", ["random", "blocks"])
@pytest.mark.parametrize("radius,step", PARAMS, ids=["r%ds%d" % p for p in PARAMS])
def test_general(dev, radius, step, guide):
    for B, h, w in ((3, 37, 53), (1, 17, 35)):
        d, g = frame("general", B, h, w, False, guide)
        dt, gt = T(d, dev), T(g, dev)
        for ss, sc, fill in ((None, 12.0, False), (None, 12.0, True), (2.5 * radius * step, 40.0, True), (INF, 25.0, False)):
            want = reference("general", B, h, w, False, guide, None, radius, step, ss, sc, fill)
            s_ = radius * step / 2.0 if ss is None else ss
            compare_general(raw(dev, dt, gt, radius, step, s_, sc, fill), want, "%dx%d B=%d %s r=%d s=%d ss=%r sc=%r fill=%d" % (h, w, B, guide, radius, step, ss, sc, fill))


def test_unit_and_saturation(dev):
    d, g = frame("unit", 2, 17, 35, False, "blocks")
    for unit in (1e-3, 1e-4, 0.25):                                 # 1e-4: depths above 6.5535 m saturate
        want = reference("unit", 2, 17, 35, False, "blocks", None, 3, 4, 6.0, 12.0, True, unit)
        compare_general(raw(dev, d, g, 3, 4, 6.0, 12.0, True, unit=unit), want, "unit %g" % unit)
    assert (reference("unit", 2, 17, 35, False, "blocks", None, 3, 4, 6.0, 12.0, True, 1e-4)["u16"] == 65535).any()


# ---- memory and launch ----------------------------------------------------------------------------------------------------------------------------
def test_repeated_and_alone(dev):
    d, g = frame("det", 3, 37, 53, False, "blocks")
    base = raw(dev, d, g, 3, 4, 6.0, 12.0, True)
    again = raw(dev, d, g, 3, 4, 6.0, 12.0, True, shift=3)
    assert base[0] == 0 and base[1].tobytes() == again[1].tobytes() and base[2].tobytes() == again[2].tobytes()
    for b in range(3):
        one = raw(dev, d[b:b + 1], g[b:b + 1], 3, 4, 6.0, 12.0, True, shift=b)
        assert one[1][0].tobytes() == base[1][b].tobytes() and one[2][0].tobytes() == base[2][b].tobytes(), b


def test_shifted_outputs_and_single_planes(dev):
    """odd w, bases shifted by 0..3 elements: the wide stores fall back to scalars where the address is not aligned, and nothing leaves a plane
    (raw() asserts the guards); a call for one plane writes that plane alone, the same bytes"""
    for (h, w) in ((37, 53), (16, 32)):
        d, g = frame("shift", 2, h, w, True)
        want = reference("shift", 2, h, w, True, "random", None, 3, 4, INF, INF, True)
        for shift in (0, 1, 2, 3):
            compare_exact(raw(dev, d, g, 3, 4, INF, INF, True, shift=shift), want, "%dx%d shift %d" % (h, w, shift))
            rc, f, u = raw(dev, d, g, 3, 4, INF, INF, True, u16=False, shift=shift)             # raw() asserts that the other buffer stays untouched
            assert rc == 0 and u is None and f.tobytes() == want["f32"].tobytes()
            rc, f, u = raw(dev, d, g, 3, 4, INF, INF, True, f32=False, shift=shift)
            assert rc == 0 and f is None and u.tobytes() == want["u16"].tobytes()


def test_wrapper(dev):
    from md_rdm_amd import _lib, refine
    d, g = frame("wrapper", 2, 37, 53, False, "blocks")
    dt, gt = T(d, dev), T(g, dev)
    want = raw(dev, dt, gt, 3, 4, 6.0, 12.0, False)
    out = refine.joint_bilateral(dt, gt, want=("f32", "u16"))                                 # the defaults: 3, 4, sigma_space = 6, 12.0, no fill
    assert set(out) == {"f32", "u16"} and out["f32"].dtype == torch.float32 and out["u16"].dtype == torch.uint16 and out["f32"].shape == (2, 37, 53)
    assert out["f32"].cpu().numpy().tobytes() == want[1].tobytes() and out["u16"].cpu().numpy().tobytes() == want[2].tobytes()
    only = refine.joint_bilateral(dt.unsqueeze(1), gt, want="u16", fill=True, radius=8, step=3, sigma_space=INF, sigma_color=INF, unit=1e-2)
    assert set(only) == {"u16"}
    assert only["u16"].cpu().numpy().tobytes() == raw(dev, dt, gt, 8, 3, INF, INF, True, unit=1e-2)[2].tobytes()
    for bad in (lambda: refine.joint_bilateral(dt.double(), gt), lambda: refine.joint_bilateral(dt[0], gt), lambda: refine.joint_bilateral(dt, gt[:, :, :, :2]),
                lambda: refine.joint_bilateral(dt, gt.float()), lambda: refine.joint_bilateral(dt, torch.from_numpy(g.copy())), lambda: refine.joint_bilateral(dt, gt[:1]),
                lambda: refine.joint_bilateral(dt, gt, radius=0), lambda: refine.joint_bilateral(dt, gt, radius=5, step=5), lambda: refine.joint_bilateral(dt, gt, step=17, radius=1),
                lambda: refine.joint_bilateral(dt, gt, sigma_color=0.0), lambda: refine.joint_bilateral(dt, gt, sigma_space=math.nan), lambda: refine.joint_bilateral(dt, gt, unit=0.0),
                lambda: refine.joint_bilateral(dt, gt, want=()), lambda: refine.joint_bilateral(dt, gt, want=("f64",))):
        with pytest.raises(_lib.RdmError):
            bad()


def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    d, g = frame("bad", 2, 5, 7, True)
    dt = T(d, dev)
    for argv, word in (({0: None}, b"depth"), ({1: None}, b"guide"), ({11: None, 12: None}, b"both be NULL"), ({11: _lib.ptr(dt)}, b"in place"), ({5: 9}, b"radius"),
                       ({6: 0}, b"step"), ({5: 5, 6: 5}, b"radius * step"), ({7: 0.0}, b"sigma_space"), ({8: math.nan}, b"sigma_color"), ({9: 2}, b"fill"), ({10: 0.0}, b"unit")):
        rc = raw(dev, dt, g, 3, 4, 6.0, 12.0, False, argv=argv)[0]                             # raw() asserts that nothing at all was written
        assert rc == -1 and word in _lib.lib().rdm_last_error_string(), (argv, _lib.lib().rdm_last_error_string())


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -------------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib, refine
    d, g = frame("stream", 2, 37, 53, False, "blocks")
    ins = dict(d=T(d, dev), g=T(g, dev))
    scratch = dict(f32=torch.empty(2, 37, 53, dtype=torch.float32, device=dev), u16=torch.empty(2, 37, 53, dtype=torch.int16, device=dev))

    def call(b, st):
        _lib.check(_lib.lib().rdm_depth_refine(_lib.ptr(b["d"]), _lib.ptr(b["g"]), 2, 37, 53, 3, 4, 6.0, 12.0, 1, 1e-3, _lib.ptr(b["f32"]), _lib.ptr(b["u16"]), st))
        return dict(wrapped=refine.joint_bilateral(b["d"], b["g"], fill=True)["f32"])          # the wrapper resolves the stream itself
    return sp.Case(ins, call, outs=("f32", "u16"), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    d, g = frame("stream", 2, 37, 53, False, "blocks")
    want = raw(dev, d, g, 3, 4, 6.0, 12.0, True)                                               # the default-stream result
    assert got["f32"].cpu().numpy().tobytes() == want[1].tobytes() == got["wrapped"].cpu().numpy().tobytes()
    assert got["u16"].cpu().numpy().view(np.uint16).tobytes() == want[2].tobytes()


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
FRAME_HW = (50, 64)                                                                            # a small frame that nyu.test_params accepts: Resize(500) makes it 500 x 640


@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                                     # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


def block_frames(n, h, w):
    """uint8 (n,h,w,3), constant over 8x8 blocks: a guide under which the filter mixes pixels"""
    g = (filler.unit("refine.product.rgb", n * h * w * 3) * 256.0).astype(np.uint8).reshape(n, h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(g[:, (yy // 8) * 8, (xx // 8) * 8])


def test_predict_metric_and_cloud_refine(dev, model):
    from md_rdm_amd import _lib, cloud, evaluate, refine
    x = T(evaluate.synthetic_samples(2, 226, 226)[0], dev)
    h, w = 120, 160
    view = nyu.test_view((480, 640))
    view = tuple(v / 4.0 for v in view)
    rgb = T(block_frames(2, h, w), dev)
    plain = model.predict_metric(x, (h, w), view=view, want=("f32", "u16", "log_scale"))
    got = model.predict_metric(x, (h, w), view=view, want=("f32", "u16", "log_scale"), refine=True, guide=rgb)
    want = refine.joint_bilateral(plain["f32"], rgb, want=("f32", "u16"))
    assert set(got) == {"f32", "u16", "log_scale"} and sp.same_bits(got["f32"], want["f32"]) and sp.same_bits(got["u16"], want["u16"])
    assert sp.same_bits(got["log_scale"], plain["log_scale"]) and not torch.equal(got["f32"], plain["f32"])
    opts = dict(radius=2, step=3, sigma_color=30.0, fill=True)
    got = model.predict_metric(x, (h, w), view=view, unit=1e-2, want=("u16", "f32"), refine=opts, guide=rgb)
    want2 = refine.joint_bilateral(plain["f32"], rgb, unit=1e-2, want=("f32", "u16"), **opts)
    assert set(got) == {"f32", "u16"} and sp.same_bits(got["u16"], want2["u16"]) and sp.same_bits(got["f32"], want2["f32"])
    assert int((got["f32"] > 0).sum()) > int((plain["f32"] > 0).sum())                          # the band around the view was filled
    assert set(model.predict_metric(x, (h, w), view=view, want="u16", refine=opts, guide=rgb)) == {"u16"}
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 480.0, 640.0), (h, w))
    records, counts = model.predict_cloud(x, (h, w), intr, view=view, rgb=rgb, normals=True, refine=True)
    wrec, wcnt = cloud.point_cloud(want["f32"], intr, rgb=rgb, normals=True)
    assert sp.same_bits(counts, wcnt) and int(counts.min()) > 0
    for b, n in enumerate(counts.cpu().tolist()):
        assert sp.same_bits(records[b, :n * 27], wrec[b, :n * 27])
    for bad in (lambda: model.predict_metric(x, (h, w), view=view, refine=True), lambda: model.predict_metric(x, (h, w), view=view, refine=True, guide=rgb[:, :-1]),
                lambda: model.predict_metric(x, (h, w), view=view, refine=True, guide=rgb.float()), lambda: model.predict_metric(x, (h, w), view=view, refine={"sigma": 1.0}, guide=rgb),
                lambda: model.predict_metric(x, (h, w), view=view, refine=3, guide=rgb), lambda: model.predict_cloud(x, (h, w), intr, view=view, refine=True)):
        with pytest.raises(_lib.RdmError):
            bad()


def test_predict_command_refine_files_are_the_library_calls(dev, tmp_path, monkeypatch):
    """the command in this process, its metric launch recorded: the three files are joint_bilateral of that plane and point_cloud of the result, bit for bit"""
    from PIL import Image
    from md_rdm_amd import cloud, depth, predict, refine
    H, W = FRAME_HW
    frames = block_frames(2, H, W)
    for i in range(2):
        np.save(str(tmp_path / ("frame%d.npy" % i)), frames[i])
    calls, real = [], depth.metric_frames

    def recording(log_map, frame_hw, **kw):
        calls.append((tuple(frame_hw), kw, real(log_map, frame_hw, **kw)))
        return dict(calls[-1][2])
    monkeypatch.setattr(depth, "metric_frames", recording)
    out = tmp_path / "maps"
    assert predict.main([str(tmp_path / "frame0.npy"), str(tmp_path / "frame1.npy"), "--out", str(out), "--metric", "--native", "--refine", "--refine_fill", "--png16", "--ply"]) == 0
    assert len(calls) == 1 and calls[0][0] == (H, W) and tuple(calls[0][1]["view"]) == nyu.test_view((H, W)) and set(calls[0][1]["want"]) == {"f32"}
    rgb = T(frames, dev)
    want = refine.joint_bilateral(calls[0][2]["f32"], rgb, fill=True, want=("f32", "u16"))
    records, counts = cloud.point_cloud(want["f32"], cloud.INTRINSICS["nyu"], rgb=rgb)
    assert int((want["f32"] > 0).sum()) > int((calls[0][2]["f32"] > 0).sum())                  # --refine_fill filled the band around the view
    for i in range(2):
        saved = np.load(str(out / ("frame%d.npy" % i)))
        assert saved.dtype == np.float32 and saved.shape == (1, H, W) and saved[0].tobytes() == want["f32"][i].cpu().numpy().tobytes()
        with Image.open(str(out / ("frame%d_depth.png" % i))) as im:
            assert im.mode == "I;16"
            np.testing.assert_array_equal(np.asarray(im), want["u16"][i].cpu().numpy())
        n = int(counts[i])
        head, _, body = open(str(out / ("frame%d.ply" % i)), "rb").read().partition(b"end_header\n")
        assert ("element vertex %d" % n).encode() in head and n > 0 and body == records[i, :n * 15].cpu().numpy().tobytes()


def test_predict_command_refine(dev, tmp_path):
    """`--metric --native --refine --png16 --ply` in a fresh process.  The command's model runs with unordered reductions, so its forward is not bit for
    bit a second process's; what IS exact is checked exactly - the .ply is `cloud.point_cloud` of the saved (refined) plane under the input frame, and the
    PNG's steps are those of the float64 depth that the saved float32 holds to half a float32 step (one launch wrote both) - and the saved plane is
    compared with `joint_bilateral(predict_metric(...)["f32"], rgb)` of this process at the tolerance of the command test of tests/test_gpu_predict.py,
    against which the unrefined plane must be far off."""
    from PIL import Image
    from md_rdm_amd import cloud, refine
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    H, W = FRAME_HW
    frames = block_frames(2, H, W)
    for i in range(2):
        np.save(str(tmp_path / ("frame%d.npy" % i)), frames[i])
    out = tmp_path / "maps"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.predict", str(tmp_path / "frame0.npy"), str(tmp_path / "frame1.npy"), "--out", str(out), "--metric", "--native",
                        "--refine", "--png16", "--ply"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(p.name for p in out.iterdir()) == ["frame0.npy", "frame0.ply", "frame0_depth.png", "frame1.npy", "frame1.ply", "frame1_depth.png"]
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    rgb = T(frames, dev)
    pre = nyu.NyuGpuPreprocessor(resize=500, output_size=(226, 226), device=dev)
    x, _ = pre(rgb, torch.zeros(2, H, W, dtype=torch.float32, device=dev), [nyu.test_params((H, W), (226, 226)) for _ in range(2)])
    plain = m.predict_metric(x, (H, W), view=nyu.test_view((H, W)))["f32"]
    want = refine.joint_bilateral(plain, rgb)["f32"].cpu().numpy()
    saved = np.stack([np.load(str(out / ("frame%d.npy" % i))) for i in range(2)])
    assert saved.dtype == np.float32 and saved.shape == (2, 1, H, W)
    saved = saved[:, 0]
    err, moved = np.abs(saved - want).max(), np.abs(plain.cpu().numpy() - want).max()
    print("command: max |saved - refined here| = %.3e, max |unrefined - refined| = %.3e, max depth %.3e" % (err, moved, want.max()))
    assert err <= 1e-4 * want.max() and moved >= 100 * max(err, 1e-6 * want.max())
    np.testing.assert_array_equal(saved == 0, want == 0)                                        # the pixels without a measurement are the same
    records, counts = cloud.point_cloud(T(saved, dev), cloud.INTRINSICS["nyu"], rgb=rgb)
    for i in range(2):
        n = int(counts[i])
        data = open(str(out / ("frame%d.ply" % i)), "rb").read()
        head, _, body = data.partition(b"end_header\n")
        assert head.decode("ascii").split("\n")[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % n] and b"uchar red" in head and n > 0
        assert body == records[i, :n * 15].cpu().numpy().tobytes()
        with Image.open(str(out / ("frame%d_depth.png" % i))) as im:
            assert im.mode == "I;16"
            png = np.asarray(im)
        q = saved[i].astype(np.float64) / 1e-3
        assert png.shape == (H, W) and (np.abs(png.astype(np.float64) - np.minimum(q, 65535.0)) <= 0.5 + q * 2.0 ** -23).all()
        assert ((png == 0) == (saved[i] == 0)).all()
