"""rdm_depth_cloud (include/rdm_cloud.h) and md_rdm_amd.cloud on the MI355X against the numpy statement of the contract (tests/cloud_ref.py).

The comparison is BIT FOR BIT, records and counts: the header's arithmetic is float64 subtraction, multiplication, division and square root, each
correctly rounded on the device and in numpy, in one stated order, followed by one rounding to float32; validity is comparisons; colours are
copies; the order is the pixels' own.  (`worst_normal_ulps` keeps the largest distance of a normal component in float32 steps seen by this module
and every comparison prints it before it asserts: measured 0.)
Every call writes between guard bytes - in front of the buffer, between the samples (the stride is longer than a sample can need), behind each
sample's count * rec bytes and behind the buffer - which must stay untouched; the base address is shifted by 0..3 bytes."""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest
import torch

import cloud_ref as cref
import stream_probe as sp
from md_rdm_amd import filler
from md_rdm_amd.dataloaders import nyu

pytestmark = pytest.mark.gpu
G, GAP, GUARD, CGUARD = 64, 37, 0xA5, 0x5A5A5A5A      # guard bytes in front and behind; unused bytes behind every sample's region; their values
INTR = (97.5, 101.25, 25.75, 17.5)
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]           # (normals, colour): 12, 15, 24, 27 bytes
worst_normal_ulps = [0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                                  # a copy: the cached frames are read-only


@functools.lru_cache(maxsize=None)
def frame(key, B, h, w, pattern="random"):
    """(depth (B,h,w) float32, rgb (B,h,w,3) uint8), hash-generated; read-only"""
    d = filler.uniform("cloud.depth/" + key, (B, h, w), 0.5, 6.0).astype(np.float32)
    u = filler.unit("cloud.mask/" + key, B * h * w).reshape(B, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    if pattern == "random":                          # about half
        d[u < 0.5] = 0.0
    elif pattern == "none":
        d[:] = 0.0
    elif pattern == "checkerboard":
        d[:, (yy + xx) % 2 == 1] = 0.0
    elif pattern == "last":
        last = d[:, -1, -1].copy()
        d[:] = 0.0
        d[:, -1, -1] = last
    elif pattern == "nonfinite":                     # 0, negatives, NaN and both infinities, a fifth each of about 60 %
        for k, v in enumerate((0.0, -1.5, np.nan, np.inf, -np.inf)):
            d[(u >= 0.12 * k) & (u < 0.12 * (k + 1))] = v
        d[0, 0, 0] = -0.0
    else:
        assert pattern == "all"
    rgb = (filler.unit("cloud.rgb/" + key, B * h * w * 3) * 256.0).astype(np.uint8).reshape(B, h, w, 3)
    d.setflags(write=False)
    rgb.setflags(write=False)
    return d, rgb


@functools.lru_cache(maxsize=None)
def reference(key, B, h, w, pattern, normals, colour, min_depth=0.0, max_depth=math.inf, step=1, intr=INTR):
    d, rgb = frame(key, B, h, w, pattern)
    return cref.reference(d, intr, rgb if colour else None, normals, min_depth, max_depth, step)


def raw(dev, d, rgb, normals, intr=INTR, min_depth=0.0, max_depth=math.inf, step=1, split=0, shift=0, argv=None):
    """one call of the C entry -> (rc, [the bytes of sample b's records], counts (B,) int32 | None, base address of sample 0, stride); asserts the guards"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    dt = d if isinstance(d, torch.Tensor) else T(d, dev)
    ct = None if rgb is None else rgb if isinstance(rgb, torch.Tensor) else T(rgb, dev)
    B, h, w = dt.shape
    rec = cref.record_bytes(normals, rgb is not None)
    need = -(-h // step) * -(-w // step) * rec
    stride = need + GAP
    buf = torch.full((G + shift + B * stride + G,), GUARD, dtype=torch.uint8, device=dev)
    cnt = torch.full((1 + B + 1,), CGUARD, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    base = buf.data_ptr() + G + shift
    args = [_lib.ptr(dt), _lib.ptr(ct), B, h, w, (C.c_double * 4)(*intr), min_depth, max_depth, step, 1 if normals else 0, C.c_void_p(base), stride,
            C.c_void_p(cnt.data_ptr() + 4), split, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_depth_cloud(*args)
    torch.cuda.synchronize()
    out, c = buf.cpu().numpy(), cnt.cpu().numpy()
    assert (out[:G + shift] == GUARD).all() and (out[G + shift + B * stride:] == GUARD).all(), "guards around the buffer"
    assert c[0] == CGUARD and c[-1] == CGUARD, "count guards"
    if rc != 0:
        assert (out == GUARD).all() and (c == CGUARD).all(), "a refused call wrote"
        return rc, None, None, base, stride
    recs = []
    for b in range(B):
        region = out[G + shift + b * stride:G + shift + (b + 1) * stride]
        assert 0 <= c[1 + b] * rec <= need, (b, c[1 + b])
        assert (region[c[1 + b] * rec:] == GUARD).all(), "sample %d: bytes behind count * rec were touched" % b
        recs.append(region[:c[1 + b] * rec].tobytes())
    return rc, recs, c[1:-1].copy(), base, stride


def fields(data, normals, colour):
    """record bytes -> (xyz (n,3) f32, normals (n,3) f32 | None, rgb (n,3) u8 | None)"""
    rec = cref.record_bytes(normals, colour)
    a = np.frombuffer(data, dtype=np.uint8).reshape(-1, rec)
    f = lambda lo: a[:, lo:lo + 12].copy().view("<f4")
    return f(0), f(12) if normals else None, a[:, rec - 3:].copy() if colour else None


def compare(got, want, normals, colour, what):
    rc, recs, counts = got[:3]
    wrecs, wcounts = want
    assert rc == 0, what
    np.testing.assert_array_equal(counts, wcounts, err_msg=what)
    for b, (g, r) in enumerate(zip(recs, wrecs)):
        gx, gn, gc = fields(g, normals, colour)
        rx, rn, rc_ = fields(r, normals, colour)
        np.testing.assert_array_equal(gx.view(np.int32), rx.view(np.int32), err_msg="%s: positions of sample %d" % (what, b))
        if colour:
            np.testing.assert_array_equal(gc, rc_, err_msg="%s: colours of sample %d" % (what, b))
        if normals and len(g):
            key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))   # monotone in the float
            steps = int(np.abs(key(gn) - key(rn)).max())
            worst_normal_ulps[0] = max(worst_normal_ulps[0], steps)
            print("%s: sample %d: normals differ by at most %d float32 steps (module worst %d)" % (what, b, steps, worst_normal_ulps[0]))
        assert g == r, "%s: the records of sample %d differ" % (what, b)


# ---- frames, batches and layouts ------------------------------------------------------------------------------------------------------------
FRAMES = [(1, 1), (1, 2), (3, 3), (5, 7), (37, 53), (64, 65)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", FRAMES, ids=["%dx%d" % f for f in FRAMES])
def test_frames_and_layouts(dev, h, w, B):
    for pattern in ("all", "random"):
        d, rgb = frame("frames", B, h, w, pattern)
        for shift, (normals, colour) in enumerate(LAYOUTS):
            want = reference("frames", B, h, w, pattern, normals, colour)
            compare(raw(dev, d, rgb if colour else None, normals, shift=shift), want, normals, colour, "%dx%d B=%d %s rec %d" % (h, w, B, pattern, cref.record_bytes(normals, colour)))


@pytest.mark.parametrize("pattern", ["all", "none", "checkerboard", "random", "last", "nonfinite"])
def test_validity_patterns(dev, pattern):
    d, rgb = frame("patterns", 3, 37, 53, pattern)
    for normals, colour in LAYOUTS:
        want = reference("patterns", 3, 37, 53, pattern, normals, colour)
        n = want[1].tolist()
        assert {"all": n == [37 * 53] * 3, "none": n == [0] * 3, "checkerboard": n == [981] * 3, "last": n == [1] * 3}.get(pattern, all(0 < k < 37 * 53 for k in n)), n
        got = raw(dev, d, rgb if colour else None, normals)                          # raw() asserts that a count of 0 leaves the whole region untouched
        compare(got, want, normals, colour, pattern)


def test_depth_bounds_are_inclusive(dev):
    d, rgb = frame("bounds", 2, 37, 53, "all")
    lo, hi = float(np.sort(d.reshape(-1))[500]), float(np.sort(d.reshape(-1))[3000])  # two depths of the frame, exactly
    assert lo < hi and (d == np.float32(lo)).any() and (d == np.float32(hi)).any()
    for mn, mx in ((lo, hi), (lo, math.inf), (0.0, hi), (hi, hi), (float(np.nextafter(np.float32(lo), np.float32(9))), float(np.nextafter(np.float32(hi), np.float32(0))))):
        want = reference("bounds", 2, 37, 53, "all", True, True, mn, mx)
        compare(raw(dev, d, rgb, True, min_depth=mn, max_depth=mx), want, True, True, "bounds [%r, %r]" % (mn, mx))
    a = reference("bounds", 2, 37, 53, "all", True, True, lo, hi)[1]
    b = reference("bounds", 2, 37, 53, "all", True, True, float(np.nextafter(np.float32(lo), np.float32(9))), float(np.nextafter(np.float32(hi), np.float32(0))))[1]
    assert a.sum() == 2501 and b.sum() == 2499                                     # the two bounds themselves are in


@pytest.mark.parametrize("step", [1, 2, 3])
def test_step_keeps_full_resolution_neighbours(dev, step):
    for h, w in ((5, 7), (37, 53), (64, 65)):                                       # no side is a multiple of 2 and of 3 at once; 64 = 2 * 32, 65 = 5 * 13
        d, rgb = frame("step", 3, h, w, "random")
        for normals, colour in ((True, True), (True, False), (False, True)):
            want = reference("step", 3, h, w, "random", normals, colour, 0.0, math.inf, step)
            compare(raw(dev, d, rgb if colour else None, normals, step=step), want, normals, colour, "%dx%d step %d" % (h, w, step))
        if step > 1:                                                                # the normals are those of the same pixels at step 1, not of the thinned frame
            full = cref.sample_arrays(d[0], INTR, None, True)
            thin = cref.sample_arrays(d[0], INTR, None, True, step=step)
            keep = np.zeros((h, w), dtype=bool)
            keep[::step, ::step] = True
            np.testing.assert_array_equal(thin["normals"], full["normals"][keep[cref.valid_mask(d[0])]])


# ---- runs: the output does not depend on split, and run boundaries fall on every byte residue ---------------------------------------------
SPLITS = (0, 1, 2, 7, 97, 5000)                                                     # 5000 > 64 * 65 sampled pixels: one pixel per workgroup


@pytest.mark.parametrize("normals,colour", [(False, True), (True, True)], ids=["rec15", "rec27"])
def test_split_and_run_boundaries(dev, normals, colour):
    d, rgb = frame("split", 3, 64, 65, "random")
    want = reference("split", 3, 64, 65, "random", normals, colour)
    rec = cref.record_bytes(normals, colour)
    seen = set()
    for split in SPLITS:
        for shift in ((0, 1, 2, 3) if split in (7, 97) else (0,)):
            got = raw(dev, d, rgb, normals, split=split, shift=shift)
            compare(got, want, normals, colour, "rec %d split %d shift %d" % (rec, split, shift))
            if split:
                for b in range(3):
                    starts = cref.run_starts(cref.valid_mask(d[b]), split)
                    seen |= {int((got[3] + b * got[4] + s * rec) % 16) for s in starts}
    assert seen == set(range(16)), sorted(seen)                                    # every residue mod 16 (and so mod 4) is a run's first or last byte address


# ---- determinism ------------------------------------------------------------------------------------------------------------------------------
def test_repeated_and_alone(dev):
    d, rgb = frame("det", 3, 37, 53, "random")
    base = raw(dev, d, rgb, True)
    again = raw(dev, d, rgb, True, shift=3)
    assert base[0] == 0 and again[1] == base[1] and (again[2] == base[2]).all()
    for b in range(3):
        one = raw(dev, d[b:b + 1], rgb[b:b + 1], True, shift=b)
        assert one[1][0] == base[1][b] and one[2][0] == base[2][b], b


# ---- the native frame -------------------------------------------------------------------------------------------------------------------------
def test_native_frame(dev):
    """480x640, B = 2, 27-byte records: what --native gives - a metric frame that is 0 outside the view of the test transform - at the toolbox camera"""
    from md_rdm_amd import cloud
    d, rgb = frame("native", 2, 480, 640, "all")
    d = d.copy()
    vy0, vx0, vh, vw = nyu.test_view((480, 640))
    yy, xx = np.mgrid[0:480, 0:640] + 0.5
    d[:, ~((yy >= vy0) & (yy < vy0 + vh) & (xx >= vx0) & (xx < vx0 + vw))] = 0.0
    assert (d[:, :10] == 0).all() and (d[:, 10:470, 13:627] > 0).all()
    intr = cloud.INTRINSICS["nyu"]
    want = cref.reference(d, intr, rgb, True)
    assert want[1].tolist() == [460 * 616] * 2                                      # rows 10 .. 469, columns 12 .. 627: centres 12.5 >= 12.49.., 627.5 < 627.50..
    compare(raw(dev, d, rgb, True, intr=intr), want, True, True, "native")
    records, counts = cloud.point_cloud(T(d, dev), "nyu", rgb=T(rgb, dev), normals=True)
    assert records.shape == (2, 480 * 640 * 27) and records.dtype == torch.uint8 and counts.dtype == torch.int32
    assert counts.cpu().tolist() == want[1].tolist()
    for b in range(2):
        assert records[b, :len(want[0][b])].cpu().numpy().tobytes() == want[0][b]


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -------------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib, cloud
    d, rgb = frame("stream", 2, 37, 53, "all")                                      # all valid: every byte of both outputs is written
    ins = dict(d=T(d, dev), rgb=T(rgb, dev))
    scratch = dict(rec=torch.empty(2, 37 * 53 * 27, dtype=torch.uint8, device=dev), cnt=torch.empty(2, dtype=torch.int32, device=dev))
    intr = (C.c_double * 4)(*INTR)

    def call(b, st):
        _lib.check(_lib.lib().rdm_depth_cloud(_lib.ptr(b["d"]), _lib.ptr(b["rgb"]), 2, 37, 53, intr, 0.0, math.inf, 1, 1, _lib.ptr(b["rec"]), 37 * 53 * 27, _lib.ptr(b["cnt"]), 0, st))
        records, counts = cloud.point_cloud(b["d"], INTR, rgb=b["rgb"], normals=True)            # the wrapper resolves the stream itself
        return dict(wrapped_cnt=counts)
    return sp.Case(ins, call, outs=("rec", "cnt"), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    want = reference("stream", 2, 37, 53, "all", True, True)
    assert got["cnt"].cpu().tolist() == want[1].tolist() == got["wrapped_cnt"].cpu().tolist()
    for b in range(2):
        assert got["rec"][b].cpu().numpy().tobytes() == want[0][b]


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- refusals on the device: nothing is written ------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib, cloud
    d, rgb = frame("bad", 2, 5, 7, "all")
    D4 = C.c_double * 4
    for argv, word in (({0: None}, b"depth"), ({8: 0}, b"step"), ({9: 2}, b"normals"), ({11: 5 * 7 * 27 - 1}, b"sample_stride_bytes"), ({5: D4(0, 1, 0, 0)}, b"fx"),
                       ({6: -1.0}, b"min_depth"), ({6: 2.0, 7: 1.0}, b"max_depth"), ({13: -1}, b"split")):
        rc = raw(dev, d, rgb, True, argv=argv)[0]                                   # raw() asserts that nothing at all was written
        assert rc == -1 and word in _lib.lib().rdm_last_error_string(), (argv, _lib.lib().rdm_last_error_string())
    t = T(d, dev)
    for bad in (lambda: cloud.point_cloud(t.double(), INTR), lambda: cloud.point_cloud(t[0], INTR), lambda: cloud.point_cloud(t, INTR, rgb=T(rgb, dev)[:, :, :, :2]),
                lambda: cloud.point_cloud(t, INTR, rgb=T(rgb, dev).float()), lambda: cloud.point_cloud(t, INTR, rgb=torch.from_numpy(rgb.copy())), lambda: cloud.point_cloud(t, INTR, step=0),
                lambda: cloud.point_cloud(t, (1.0, 0.0, 0.0, 0.0)), lambda: cloud.point_cloud(t, INTR, min_depth=3.0, max_depth=2.0)):
        with pytest.raises(_lib.RdmError):
            bad()


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


def test_predict_cloud_is_predict_metric_then_point_cloud(dev, model):
    from md_rdm_amd import cloud, evaluate
    x = T(evaluate.synthetic_samples(2, 226, 226)[0], dev)
    view = nyu.test_view((480, 640))
    rgb = T(frame("product", 2, 480, 640, "all")[1], dev)
    intr = cloud.INTRINSICS["nyu"]
    records, counts = model.predict_cloud(x, (480, 640), intr, view=view, rgb=rgb, normals=True, min_depth=0.1, step=2)
    planes = model.predict_metric(x, (480, 640), view=view, want=("f32",))
    wrec, wcnt = cloud.point_cloud(planes["f32"], intr, rgb=rgb, normals=True, min_depth=0.1, step=2)
    assert records.shape == (2, 240 * 320 * 27) and sp.same_bits(counts, wcnt) and int(counts.min()) > 0
    for b, n in enumerate(counts.cpu().tolist()):
        assert sp.same_bits(records[b, :n * 27], wrec[b, :n * 27])
    ref = cref.reference(planes["f32"].cpu().numpy(), intr, rgb.cpu().numpy(), True, 0.1, math.inf, 2)     # and both are the contract's
    compare((0, [records[b, :n * 27].cpu().numpy().tobytes() for b, n in enumerate(counts.cpu().tolist())], counts.cpu().numpy()), ref, True, True, "predict_cloud")


def test_predict_command_synthetic_ply(dev, tmp_path):
    from md_rdm_amd import cloud, predict
    out = tmp_path / "maps"
    assert predict.main(["--synthetic", "2", "--out", str(out), "--metric", "--ply", "--ply_normals"]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["synthetic_0000.npy", "synthetic_0000.ply", "synthetic_0001.npy", "synthetic_0001.ply"]
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 226.0, 226.0), (128, 128))      # the raw frame of a synthetic input is the network input
    for i in range(2):
        d = np.load(str(out / ("synthetic_%04d.npy" % i)))
        assert d.dtype == np.float32 and d.shape == (1, 128, 128)
        recs, counts = cref.reference(d, intr, None, True)
        data = open(str(out / ("synthetic_%04d.ply" % i)), "rb").read()
        head, _, body = data.partition(b"end_header\n")
        assert head.decode("ascii").split("\n")[:3] == ["ply", "format binary_little_endian 1.0", "element vertex %d" % counts[0]] and counts[0] == 128 * 128
        assert b"property float nx" in head and b"uchar" not in head
        compare((0, [body], counts), (recs, counts), True, False, "synthetic_%04d.ply" % i)
        assert len(list(struct.iter_unpack("<6f", body))) == counts[0]
