"""rdm_depth_warp (include/rdm_warp.h) and md_rdm_amd.warp on the MI355X against the numpy statement of the contract (tests/warp_ref.py).

The comparison is BIT FOR BIT on every plane - depth, colour, index, mask: the arithmetic is float64 multiplication, division, addition,
subtraction and floor, each correctly rounded on the device and in numpy and written in one order, one rounding to float32, and an integer minimum.
No tolerance exists.  Every call writes between guard elements in front of and behind every plane and the workspace, which must stay untouched."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import stream_probe as sp
import warp_ref as wref
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
G = 16                                                                             # guard elements at both ends of every buffer
POISON = {"depth": -123.5, "rgb": 0xA5, "index": 0x5A5A5A5A, "mask": 0x77}
DTYPE = {"depth": torch.float32, "rgb": torch.uint8, "index": torch.int32, "mask": torch.uint8}
INTR = (61.5, 63.25, 25.75, 17.5)                                                  # of the 37x53 source
INTR_T = (47.0, 45.5, 13.25, 21.5)                                                 # of a 41x29 target
INTR_W = (12.0, 12.5, 10.0, 17.5)                                                  # a wide-angle 37x53 target
MIN_D, MAX_D = 0.5, 8.0
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
ALL = ("rgb", "index", "mask")


def rodrigues(r, t):
    from md_rdm_amd import warp
    return warp.pose_from_rt(r, t)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def frame(key, B, h, w, pattern="mixed"):
    """(B,h,w) float32 and (B,h,w,3) uint8, hash-generated, read-only.  "mixed": depths in [1.5, 4], about 2 % each 0, negative, NaN, +inf, below MIN_D
    and above MAX_D.  "layers": a background at about 4 m with a block at about 1.5 m in the middle.  "plane": the constant 2.  "holes": "mixed" with
    rows 3 and 4 and the first three and last four columns without a measurement."""
    d = filler.uniform("warp.depth/" + key, (B, h, w), 1.5, 4.0).astype(np.float32)
    u = filler.unit("warp.mask/" + key, B * h * w).reshape(B, h, w)
    if pattern in ("mixed", "holes"):
        for k, bad in enumerate((0.0, -1.5, np.nan, np.inf, 0.3, 9.0)):
            d[(u >= 0.02 * k) & (u < 0.02 * (k + 1))] = bad
        if pattern == "holes":
            d[:, 3:5, :] = 0.0
            d[:, :, :3] = np.nan
            d[:, :, -4:] = -1.0
    elif pattern == "layers":
        d = (np.float32(4.0) + np.float32(0.1) * (d - np.float32(1.5))).astype(np.float32)
        d[:, h // 4:3 * h // 4, w // 3:2 * w // 3] -= np.float32(2.5)
    else:
        assert pattern == "plane"
        d[:] = 2.0
    rgb = (filler.unit("warp.rgb/" + key, B * h * w * 3) * 256.0).astype(np.uint8).reshape(B, h, w, 3)
    d.setflags(write=False)
    rgb.setflags(write=False)
    return d, rgb


def guarded(dev, name, shape):
    n = int(np.prod(shape))
    return torch.full((G + n + G,), POISON[name], dtype=DTYPE[name], device=dev)


def raw(dev, d, rgb, poses, intr=INTR, intr_out=None, out_hw=None, splat=1, fill=0, planes=ALL, min_depth=MIN_D, max_depth=MAX_D, ws=None, argv=None):
    """one call of the C entry -> (rc, {plane: numpy}); asserts the guards; `ws`: a workspace tensor (int64, G guards at both ends) to use as it is"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    B, h, w = d.shape
    th, tw = (h, w) if out_hw is None else out_hw
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
    assert P.shape[0] in (1, B)
    dt, ct, pt = torch.from_numpy(np.array(d)).to(dev), None if rgb is None else torch.from_numpy(np.array(rgb)).to(dev), torch.from_numpy(P).to(dev)
    shapes = {"depth": (B, th, tw), "rgb": (B, th, tw, 3), "index": (B, th, tw), "mask": (B, th, tw)}
    bufs = {k: guarded(dev, k, shapes[k]) for k in ("depth",) + tuple(planes)}
    at = lambda k: C.c_void_p(bufs[k].data_ptr() + G * bufs[k].element_size()) if k in bufs else None
    need = L.rdm_depth_warp_workspace_bytes(B, th, tw)
    assert need == B * th * tw * 8
    if ws is None:
        ws = torch.full((G + B * th * tw + G,), 0x1234567812345678, dtype=torch.int64, device=dev)
    before = ws.clone()
    src, dst = (C.c_double * 4)(*intr), (C.c_double * 4)(*(intr if intr_out is None else intr_out))
    args = [_lib.ptr(dt), _lib.ptr(ct), B, h, w, src, dst, _lib.ptr(pt), 12 if P.shape[0] > 1 else 0, min_depth, max_depth, th, tw, splat, fill,
            at("depth"), at("rgb"), at("index"), at("mask"), C.c_void_p(ws.data_ptr() + 8 * G), need, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_depth_warp(*args)
    torch.cuda.synchronize()
    assert torch.equal(ws[:G], before[:G]) and torch.equal(ws[-G:], before[-G:]), "workspace guards"
    host = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k, v in host.items():
        p = np.array(POISON[k]).astype(v.dtype)
        assert (v[:G] == p).all() and (v[-G:] == p).all(), "guards around %s" % k
        if rc != 0:
            assert (v == p).all(), "a refused call wrote %s" % k
    if rc != 0:
        assert torch.equal(ws, before), "a refused call wrote the workspace"
        return rc, None
    return rc, {k: v[G:-G].reshape(shapes[k]) for k, v in host.items()}


def compare(got, want, what):
    rc, planes = got
    assert rc == 0, what
    for k, v in planes.items():
        r = want[k]
        assert v.dtype == r.dtype and v.shape == r.shape, (what, k, v.dtype, r.dtype, v.shape, r.shape)
        if v.tobytes() != r.tobytes():
            where = np.argwhere(v.view(np.uint32 if k == "depth" else v.dtype) != r.view(np.uint32 if k == "depth" else r.dtype))
            first = tuple(where[0])
            assert False, "%s: plane %s differs in %d places, first at %r: %r, reference %r" % (what, k, len(where), first, v[first], r[first])


@functools.lru_cache(maxsize=None)
def ref(key, B, h, w, pattern, pose_key, intr_out, out_hw, splat, fill):
    d, rgb = frame(key, B, h, w, pattern)
    return wref.reference(d, INTR, POSES[pose_key], rgb, out_hw=out_hw, intr_dst=intr_out, min_depth=MIN_D, max_depth=MAX_D, splat=splat, fill=fill)


POSES = {
    "ident": IDENT,
    "small": rodrigues((0.02, -0.05, 0.01), (0.08, -0.03, 0.05)),
    "per": np.stack([rodrigues((0.02, -0.05, 0.01), (0.08, -0.03, 0.05)), rodrigues((-0.04, 0.03, 0.1), (-0.1, 0.02, -0.2)), rodrigues((0.0, 0.0, 0.0), (0.06, 0.0, 0.0))]),
    "minify": rodrigues((0.0, 0.0, 0.0), (0.0, 0.0, 4.0)),                          # a plane at 2 m is then at 6 m: the image shrinks 3x
    "roty": rodrigues((0.0, 0.3, 0.0), (-0.9, 0.05, 0.1)),
    "behind": rodrigues((0.0, 1.3, 0.0), (0.0, 0.0, 0.2)),                          # the right part of the frame is behind the turned camera
    "other": rodrigues((0.05, 0.1, -0.02), (0.3, 0.1, -0.1)),
    # R is used as given: a scaled identity leaves u and v alone and scales Qz.  Depths of 1.5 .. 4 times 3e-46 straddle half the smallest float32
    # denormal (7.0e-46): zf rounds to 0 for some pixels and to 1.4e-45 for others; times 1e38 they straddle the largest float32 (3.4e38)
    "denormal": np.concatenate([3e-46 * np.eye(3), np.zeros((3, 1))], axis=1),
    "overflow": np.concatenate([1e38 * np.eye(3), np.zeros((3, 1))], axis=1),
}


# ---- the frames that exercise the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose_key", ["small", "per"])
@pytest.mark.parametrize("target", [(INTR_T, (41, 29)), (None, None)], ids=["41x29", "37x53"])
def test_hash_frame_with_invalid_sources(dev, target, pose_key):
    d, rgb = frame("a", 3, 37, 53)
    assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d == 0).any() and (d == np.float32(0.3)).any() and (d == np.float32(9.0)).any()
    want = ref("a", 3, 37, 53, "mixed", pose_key, target[0], target[1], 1, 3)
    assert (want["mask"] == 0).any() and (want["mask"] == 1).any() and (want["mask"] == 2).any()
    src = want["index"][want["mask"] == 1]
    assert wref.valid(d, MIN_D, MAX_D).reshape(3, -1)[np.nonzero(want["mask"] == 1)[0], src].all()          # only valid sources are ever kept
    compare(raw(dev, d, rgb, POSES[pose_key], intr_out=target[0], out_hw=target[1], fill=3), want, "37x53 -> %r, %s" % (target[1], pose_key))


def test_minifying_pose_breaks_ties_by_index_under_contention(dev):
    d, rgb = frame("plane", 3, 37, 53, "plane")
    want = ref("plane", 3, 37, 53, "plane", "minify", None, None, 1, 0)
    kept = want["mask"] == 1
    assert (want["depth"][kept] == np.float32(6.0)).all() and 37 * 53 // 12 < kept[0].sum() < 37 * 53 // 6          # about nine sources on every kept cell
    compare(raw(dev, d, rgb, POSES["minify"]), want, "minify")
    compare(raw(dev, d, rgb, POSES["minify"], splat=3, fill=64), ref("plane", 3, 37, 53, "plane", "minify", None, None, 3, 64), "minify splat 3 fill 64")


@pytest.mark.parametrize("fill", [0, 1, 5, 64])
def test_rotation_over_two_depth_layers(dev, fill):
    d, rgb = frame("layers", 3, 37, 53, "layers")
    want = ref("layers", 3, 37, 53, "layers", "roty", None, None, 1, fill)
    near = want["depth"][(want["mask"] == 1)] < 2.5
    assert near.any() and (~near).any() and (want["mask"] == 0).any() == (fill < 64) and ((want["mask"] == 2).any() == (fill > 0))
    compare(raw(dev, d, rgb, POSES["roty"], fill=fill), want, "two layers, fill %d" % fill)


def test_frame_partly_behind_the_camera_and_partly_outside(dev):
    d, rgb = frame("a", 3, 37, 53)
    T = wref.pose12(POSES["behind"])
    xs = (np.arange(53) - INTR[2]) / INTR[0]
    qz = T[8] * xs * 2.0 + T[10] * 2.0 + T[11]                                     # of a point at 2 m in column x
    assert (qz < 0).any() and (qz > 0).any()
    want = ref("a", 3, 37, 53, "mixed", "behind", INTR_W, None, 2, 2)
    assert 0 < (want["mask"] == 1).sum() < wref.valid(d, MIN_D, MAX_D).sum() // 2 and 0 < len(np.unique(want["index"][want["mask"] == 1])) < 3 * 37 * 53 // 2
    compare(raw(dev, d, rgb, POSES["behind"], intr_out=INTR_W, splat=2, fill=2), want, "behind")


@pytest.mark.parametrize("pose_key", ["denormal", "overflow"])
def test_target_depths_at_the_ends_of_float32(dev, pose_key):
    d, rgb = frame("a", 3, 37, 53)
    want = ref("a", 3, 37, 53, "mixed", pose_key, None, None, 1, 0)
    ok = wref.valid(d, MIN_D, MAX_D)
    kept = want["mask"] == 1
    assert 0 < kept.sum() < ok.sum() and not (kept & ~ok).any()                  # the rounding to float32 decides: some valid sources are dropped, some kept
    if pose_key == "denormal":
        assert (want["depth"][kept].view(np.uint32) == 1).all()                 # the smallest denormal, > 0
    else:
        assert np.isfinite(want["depth"]).all() and want["depth"].max() > np.float32(3e38)
    compare(raw(dev, d, rgb, POSES[pose_key]), want, pose_key)


@pytest.mark.parametrize("splat", [1, 2, 3, 4])
def test_splat_footprints_cross_every_border(dev, splat):
    d, rgb = frame("a", 3, 37, 53)
    intr_out, out_hw = (61.5, 63.25, 17.25, 12.0), (25, 33)                        # the same scale on a smaller grid: the source overhangs all four borders
    want = ref("a", 3, 37, 53, "mixed", "ident", intr_out, out_hw, splat, 0)
    m = want["mask"] == 1
    assert m[:, 0].any() and m[:, -1].any() and m[:, :, 0].any() and m[:, :, -1].any()
    compare(raw(dev, d, rgb, IDENT, intr_out=intr_out, out_hw=out_hw, splat=splat), want, "splat %d" % splat)
    want = ref("a", 3, 37, 53, "mixed", "other", INTR_T, (41, 29), splat, 1)
    compare(raw(dev, d, rgb, POSES["other"], intr_out=INTR_T, out_hw=(41, 29), splat=splat, fill=1), want, "splat %d, moved" % splat)


@pytest.mark.parametrize("fill", [0, 1, 5, 64])
def test_fill_with_empty_rows_and_holes_at_both_row_ends(dev, fill):
    d, rgb = frame("holes", 3, 37, 53, "holes")
    want = ref("holes", 3, 37, 53, "holes", "ident", None, None, 1, fill)
    assert not want["mask"][:, 3:5].any() and (want["index"][:, 3:5] == -1).all()           # rows without a point stay holes whatever F is
    assert (want["mask"] == 2).any() == (fill > 0) and (want["mask"][:, :, 0] == 0).any() and (want["mask"][:, :, -1] == 0).any()          # (rows 3 and 4)
    if fill >= 5:                                                                  # the holes at both row ends are reached from inside the row
        assert (want["mask"][:, :, 0] == 2).any() and (want["mask"][:, :, -1] == 2).any()
    compare(raw(dev, d, rgb, IDENT, fill=fill), want, "holes, fill %d" % fill)


# a single pixel, one row, one column; rows longer than one 256-cell segment (the fill reaches across the segment's edge) and more rows than one
SHAPES = [("one", 1, 1), ("row", 1, 40), ("col", 40, 1), ("wide", 2, 700), ("tall", 300, 3)]


@pytest.mark.parametrize("key,h,w", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes(dev, key, h, w):
    d, rgb = frame(key, 2, h, w)
    intr = (0.7 * w + 3.0, 0.7 * h + 3.0, (w - 1) / 2.0, (h - 1) / 2.0)
    pose = rodrigues((0.0, 0.0, 0.0), (0.02, 0.01, 0.1)) if min(h, w) > 1 else IDENT
    for splat, fill in ((1, 0), (2, 64), (4, 5)):
        want = wref.reference(d, intr, pose, rgb, min_depth=MIN_D, max_depth=MAX_D, splat=splat, fill=fill)
        assert (want["mask"] == 1).any() or (h, w) == (1, 1)
        compare(raw(dev, d, rgb, pose, intr=intr, splat=splat, fill=fill), want, "%dx%d splat %d fill %d" % (h, w, splat, fill))
    d1 = np.full((1, 1, 1), 2.0, np.float32)                                      # the single valid pixel
    compare(raw(dev, d1, rgb[:1], IDENT, intr=(5.0, 5.0, 0.0, 0.0), splat=3, fill=4), wref.reference(d1, (5.0, 5.0, 0.0, 0.0), IDENT, rgb[:1], splat=3, fill=4), "1x1")


# ---- the workspace, batches, determinism, NULL planes ----------------------------------------------------------------------------------------
def test_workspace_contents_do_not_matter(dev):
    d, rgb = frame("a", 3, 37, 53)
    ws = torch.zeros(G + 3 * 41 * 29 + G, dtype=torch.int64, device=dev)           # zeros: smaller than every key
    compare(raw(dev, d, rgb, POSES["per"], intr_out=INTR_T, out_hw=(41, 29), fill=3, ws=ws), ref("a", 3, 37, 53, "mixed", "per", INTR_T, (41, 29), 1, 3), "zeroed workspace")
    assert ws[G:-G].ne(0).all()                                                   # it was used
    compare(raw(dev, d, rgb, POSES["other"], intr_out=INTR_T, out_hw=(41, 29), splat=2, fill=1, ws=ws), ref("a", 3, 37, 53, "mixed", "other", INTR_T, (41, 29), 2, 1),
            "the same workspace, another pose")


def test_batch_alone_and_repeated(dev):
    d, rgb = frame("a", 3, 37, 53)
    base = raw(dev, d, rgb, POSES["per"], intr_out=INTR_T, out_hw=(41, 29), splat=2, fill=5)
    compare(base, ref("a", 3, 37, 53, "mixed", "per", INTR_T, (41, 29), 2, 5), "batch of 3")
    again = raw(dev, d, rgb, POSES["per"], intr_out=INTR_T, out_hw=(41, 29), splat=2, fill=5)
    for k in base[1]:
        assert again[1][k].tobytes() == base[1][k].tobytes(), k
    for b in range(3):
        one = raw(dev, d[b:b + 1], rgb[b:b + 1], POSES["per"][b], intr_out=INTR_T, out_hw=(41, 29), splat=2, fill=5)
        for k in base[1]:
            assert one[1][k][0].tobytes() == base[1][k][b].tobytes(), (b, k)


def test_null_planes_and_want_subsets(dev):
    from md_rdm_amd import _lib, warp
    d, rgb = frame("a", 3, 37, 53)
    want = ref("a", 3, 37, 53, "mixed", "small", None, None, 1, 3)
    for planes in ((), ("mask",), ("index",), ("rgb",), ("rgb", "mask")):
        compare(raw(dev, d, rgb, POSES["small"], fill=3, planes=planes), want, "planes %r" % (planes,))
    compare(raw(dev, d, None, POSES["small"], fill=3, planes=("index", "mask")), want, "no colours")
    dt, ct = torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(np.array(rgb)).to(dev)
    for names, colours in ((warp.PLANES, ct), (("depth",), ct), ("mask", None), (("index", "rgb"), ct), (warp.PLANES, None)):
        out = warp.render(dt, INTR, POSES["small"], rgb=colours, min_depth=MIN_D, max_depth=MAX_D, fill=3, want=names)
        expect = {k for k in ((names,) if isinstance(names, str) else names) if k != "rgb" or colours is not None}
        assert set(out) == expect
        compare((0, {k: v.cpu().numpy() for k, v in out.items()}), want, "render want=%r" % (names,))
    out = warp.render(dt, INTR, torch.from_numpy(POSES["per"]).float().to(dev), rgb=ct, out_hw=(41, 29), intrinsics_out=INTR_T, min_depth=MIN_D, max_depth=MAX_D, splat=2)
    P32 = POSES["per"].astype(np.float32).astype(np.float64)                       # a float32 tensor pose is widened, not re-derived
    compare((0, {k: v.cpu().numpy() for k, v in out.items()}), wref.reference(d, INTR, P32, rgb, out_hw=(41, 29), intr_dst=INTR_T, min_depth=MIN_D, max_depth=MAX_D, splat=2),
            "render, per-sample tensor poses")
    for bad in (lambda: warp.render(dt.double(), INTR, IDENT), lambda: warp.render(dt[0], INTR, IDENT), lambda: warp.render(dt, INTR, IDENT, rgb=ct[:, :, :, :2]),
                lambda: warp.render(dt, INTR, IDENT, rgb=ct.cpu()), lambda: warp.render(dt, INTR, np.stack([IDENT] * 2)), lambda: warp.render(dt, INTR, IDENT, splat=5)):
        with pytest.raises(_lib.RdmError):
            bad()


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control ------------------------------------------------
# Two cases: the C entry alone, which allocates nothing, and the wrapper, which resolves the stream itself and allocates its planes and workspace.
# Every test proves a stream of its own to run beside the null stream (a fresh stream_probe.Delay), and the controls assert their two
# preconditions themselves: that the stream still runs beside the null stream, and that the delay was still running when the call had been enqueued.
STREAM_ARGS = dict(out_hw=(41, 29), intrinsics_out=INTR_T, min_depth=MIN_D, max_depth=MAX_D, splat=2, fill=5)


def stream_case(dev, wrapped):
    from md_rdm_amd import _lib, warp
    L = _lib.lib()
    d, rgb = frame("a", 3, 37, 53)
    wsb = L.rdm_depth_warp_workspace_bytes(3, 41, 29)
    src, dst = (C.c_double * 4)(*INTR), (C.c_double * 4)(*INTR_T)
    ins = dict(d=torch.from_numpy(np.array(d)).to(dev), rgb=torch.from_numpy(np.array(rgb)).to(dev), poses=torch.from_numpy(POSES["per"].reshape(3, 12).copy()).to(dev))
    if wrapped:                                                                    # a pose on the device never visits the host
        return sp.Case(ins, lambda b, st: warp.render(b["d"], INTR, b["poses"].view(3, 3, 4), rgb=b["rgb"], **STREAM_ARGS))
    scratch = dict(depth=torch.empty(3, 41, 29, dtype=torch.float32, device=dev), rgb=torch.empty(3, 41, 29, 3, dtype=torch.uint8, device=dev),
                   index=torch.empty(3, 41, 29, dtype=torch.int32, device=dev), mask=torch.empty(3, 41, 29, dtype=torch.uint8, device=dev),
                   ws=torch.empty(wsb // 8, dtype=torch.int64, device=dev))
    ins["colours"] = ins.pop("rgb")

    def call(b, st):
        _lib.check(L.rdm_depth_warp(_lib.ptr(b["d"]), _lib.ptr(b["colours"]), 3, 37, 53, src, dst, _lib.ptr(b["poses"]), 12, MIN_D, MAX_D, 41, 29, 2, 5, _lib.ptr(b["depth"]),
                                    _lib.ptr(b["rgb"]), _lib.ptr(b["index"]), _lib.ptr(b["mask"]), _lib.ptr(b["ws"]), wsb, st))
    return sp.Case(ins, call, outs=warp.PLANES, scratch=scratch)


@pytest.fixture
def delay(dev):
    return sp.Delay(dev)


def beside_null(delay):
    """stream_probe.Delay's proof, repeated now: a fill on the null stream finishes while a sleep on delay.S is still running"""
    probe = torch.zeros(64, device=delay.dev)
    null = torch.cuda.default_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(delay.S):
        delay.enqueue(20.0)
    with torch.cuda.stream(null):
        probe.add_(1.0)
    null.synchronize()
    beside = not delay.S.query()
    delay.S.synchronize()
    return beside


@pytest.mark.parametrize("wrapped", [False, True], ids=["c_entry", "wrapper"])
def test_call_on_a_late_non_default_stream(dev, delay, wrapped):
    got = sp.check(stream_case(dev, wrapped), delay)
    want = ref("a", 3, 37, 53, "mixed", "per", INTR_T, (41, 29), 2, 5)
    assert set(got) == set(want)
    for k in want:
        assert got[k].cpu().numpy().tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("wrapped", [False, True], ids=["c_entry", "wrapper"])
def test_control_call_on_the_null_stream_is_detected(dev, delay, wrapped):
    """The C entry writes into the harness's poisoned buffers: stream_probe.control as it stands (different from the reference AND poisoned).  The
    wrapper allocates its planes itself, so nothing of its result can carry the harness's poison: there the call made on the null stream reads the
    poisoned inputs (NaN depths and poses: no point is kept) and every plane must differ from the reference."""
    case = stream_case(dev, wrapped)
    assert beside_null(delay), "the stream does not run beside the null stream: the control could prove nothing"
    inner, seen = case.call, {}

    def call(b, st):
        out = inner(b, st)
        seen["delay_running"] = not delay.S.query()                                 # the host has enqueued the whole call: is S still in its delay?
        return out
    case.call = call
    if wrapped:
        ref_planes = sp.reference_run(case)
        snap = sp.late_run(case, delay, wrong_stream=True)
        assert sorted(sp.mismatches(case, snap, ref_planes)) == sorted(ref_planes), "a wrapper call on the wrong stream went undetected"
        assert not any(bool(v.any()) for k, v in snap.items() if k != "index") and bool((snap["index"] == -1).all())          # it saw the poisoned inputs
    else:
        sp.control(case, delay)
    assert seen["delay_running"], "the delay had run out before the call was enqueued: the host was held up inside the call"


# ---- refusals on the device: nothing is written ------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    d, rgb = frame("bad", 2, 5, 7)
    nan, inf = float("nan"), float("inf")
    I4 = lambda *v: (C.c_double * 4)(*v)
    # positions: 0 depth, 1 rgb, 2 batch, 3 h, 4 w, 5 intr_src, 6 intr_dst, 7 poses, 8 pose_stride, 9 min_depth, 10 max_depth, 11 th, 12 tw, 13 splat, 14 fill,
    # 15 depth_out, 16 rgb_out, 17 index_out, 18 mask_out, 19 workspace, 20 workspace_bytes, 21 stream
    rows = (({0: None}, b"depth"), ({5: None}, b"intr_src"), ({6: None}, b"intr_dst"), ({7: None}, b"poses"), ({15: None}, b"depth_out"), ({19: None}, b"workspace"),
            ({1: None}, b"rgb_out needs rgb"), ({2: 0}, b"batch"), ({3: 0}, b"h"), ({4: -1}, b"w"), ({11: 0}, b"th"), ({12: 0}, b"tw"), ({2: 65536}, b"65535"),
            ({3: 65536, 4: 32768}, b"h * w"), ({11: 65536, 12: 32768}, b"th * tw"), ({8: 6}, b"pose_stride"), ({13: 0}, b"splat"), ({13: 5}, b"splat"),
            ({14: -1}, b"fill"), ({14: 65}, b"fill"), ({20: 2 * 5 * 7 * 8 - 1}, b"workspace_bytes"), ({5: I4(nan, 1, 0, 0)}, b"intr_src"), ({5: I4(0, 1, 0, 0)}, b"intr_src"),
            ({6: I4(1, 0, 0, 0)}, b"intr_dst"), ({6: I4(1, 1, 0, inf)}, b"intr_dst"), ({9: -1.0}, b"min_depth"), ({9: nan}, b"min_depth"), ({10: nan}, b"max_depth"),
            ({9: 2.0, 10: 1.0}, b"max_depth"))
    for argv, word in rows:
        rc = raw(dev, d, rgb, POSES["per"][:2], argv=argv)[0]                       # raw() asserts that nothing at all was written
        assert rc == -1 and word in _lib.lib().rdm_last_error_string(), (argv, _lib.lib().rdm_last_error_string())
    ws = torch.full((G + 2 * 5 * 7 + G,), 0x1234567812345678, dtype=torch.int64, device=dev)
    rc = raw(dev, d, rgb, POSES["per"][:2], ws=ws, argv={19: C.c_void_p(ws.data_ptr() + 8 * G + 4)})[0]
    assert rc == -1 and b"aligned" in _lib.lib().rdm_last_error_string()


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
def test_predict_view_is_render_of_predict_metric(dev):
    from md_rdm_amd import cloud, evaluate, warp
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    x = torch.from_numpy(np.array(evaluate.synthetic_samples(2, 226, 226)[0])).to(dev)
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 226.0, 226.0), (128, 128))
    rgb = torch.from_numpy((filler.unit("warp.predict.rgb", 2 * 128 * 128 * 3) * 256.0).astype(np.uint8).reshape(2, 128, 128, 3)).to(dev)
    plane = m.predict_metric(x, (128, 128), want=("f32",))["f32"]
    pose = warp.stereo_pose(0.06)
    got = m.predict_view(x, (128, 128), intr, pose, rgb=rgb, splat=2, fill=4)
    direct = warp.render(plane, intr, pose, rgb=rgb, splat=2, fill=4)
    assert set(got) == set(direct) == set(warp.PLANES)
    for k in got:
        assert sp.same_bits(got[k], direct[k]), k
    want = wref.reference(plane.cpu().numpy(), intr, pose, rgb.cpu().numpy(), splat=2, fill=4)
    compare((0, {k: v.cpu().numpy() for k, v in got.items()}), want, "predict_view")
    assert (want["mask"] == 1).any()


def test_predict_command_synthetic_stereo(dev, tmp_path):
    from md_rdm_amd import predict
    out = tmp_path / "maps"
    assert predict.main(["--synthetic", "2", "--out", str(out), "--metric", "--full_res", "--stereo", "0.06", "--png16"]) == 0
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted("synthetic_000%d%s" % (i, s) for i in range(2) for s in (".npy", "_depth.png", "_right.png", "_right_depth.png")), names
    for p in out.iterdir():
        assert p.suffix != ".png" or p.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
