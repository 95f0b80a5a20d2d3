"""rdm_tsdf_integrate / rdm_tsdf_extract (include/rdm_fuse.h) and md_rdm_amd.fuse on the MI355X against the numpy statement of the contract
(tests/fuse_ref.py, whose statement tests/test_fuse_cpu.py checks on scenes known by hand).

The comparison is BIT FOR BIT on every plane and every record: the arithmetic is float64 multiplication, division, addition, subtraction, floor and
square root, each correctly rounded on the device and in numpy and written in one order, with one rounding to float32.  No tolerance exists.  Every
call writes between guard elements in front of and behind every plane, the records, count and the workspace, which must stay untouched."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import fuse_ref as fref
import stream_probe as sp
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
G = 16                                                                             # guard elements at both ends of every buffer
P_F32, P_U8, P_I64 = -123.5, 0xA5, 0x5A5A5A5A5A5A5A5A
INTR = (61.5, 63.25, 25.75, 17.5)                                                  # of the 37x53 frames
MIN_D, MAX_D = 0.5, 8.0
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
DIMS, GEOM = (19, 13, 11), (-0.9, -0.6, 1.2, 0.1, 0.4)                             # at 2 m the 37x53 frame spans x -0.84 .. 0.89, y -0.55 .. 0.62: a rim of voxels is outside it
INF = math.inf


def rodrigues(r, t):
    from md_rdm_amd import warp
    return warp.pose_from_rt(r, t)


POSES = {
    "ident": IDENT,
    "per": np.stack([rodrigues((0.02, -0.05, 0.01), (0.08, -0.03, 0.05)), rodrigues((-0.04, 0.03, 0.1), (-0.1, 0.02, -0.2)), rodrigues((0.0, 0.0, 0.0), (0.06, 0.0, 0.0))]),
    "aside": rodrigues((0.0, 0.0, 0.0), (50.0, 0.0, 0.0)),                          # every voxel in front of the camera, none inside its frame
    "behind": rodrigues((0.0, 0.0, 0.0), (0.0, 0.0, -10.0)),                        # every Qz < 0
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def frame(key, B, h, w, pattern="mixed"):
    """(B,h,w) float32 and (B,h,w,3) uint8, hash-generated, read-only.  "mixed": depths in [1.5, 4], about 2 % each 0, negative, NaN, +inf, below MIN_D
    and above MAX_D.  "near": depths in [1.3, 2.4], the band of DIMS / GEOM."""
    lo, hi = (1.5, 4.0) if pattern == "mixed" else (1.3, 2.4)
    d = filler.uniform("fuse.depth/" + key, (B, h, w), lo, hi).astype(np.float32)
    if pattern == "mixed":
        u = filler.unit("fuse.mask/" + key, B * h * w).reshape(B, h, w)
        for k, bad in enumerate((0.0, -1.5, np.nan, np.inf, 0.3, 9.0)):
            d[(u >= 0.02 * k) & (u < 0.02 * (k + 1))] = bad
    rgb = (filler.unit("fuse.rgb/" + key, B * h * w * 3) * 256.0).astype(np.uint8).reshape(B, h, w, 3)
    d.setflags(write=False)
    rgb.setflags(write=False)
    return d, rgb


@functools.lru_cache(maxsize=None)
def hash_planes(key, dims, special=False):
    """T in [-1, 1], W in [0, 5], C in [0, 255], so that an untouched voxel is visible.  special (for the extraction): T also exactly 0, -0, 1, -1, NaN, +inf
    and just inside 1; W also exactly 2.5 (the min_weight of those tests), 0 and NaN; C also NaN, below 0, above 255 and on a half."""
    nx, ny, nz = dims
    T = filler.uniform("fuse.T/" + key, (nz, ny, nx), -1.0, 1.0).astype(np.float32)
    W = filler.uniform("fuse.W/" + key, (nz, ny, nx), 0.0, 5.0).astype(np.float32)
    Cc = filler.uniform("fuse.C/" + key, (nz, ny, nx, 3), 0.0, 255.0).astype(np.float32)
    if special:
        u = filler.unit("fuse.special/" + key, nx * ny * nz).reshape(nz, ny, nx)
        for k, v in enumerate((0.0, -0.0, 1.0, -1.0, np.nan, np.inf, np.float32(0.99999994), np.float32(-0.99999994))):
            T[(u >= 0.02 * k) & (u < 0.02 * (k + 1))] = v
        u = filler.unit("fuse.specialW/" + key, nx * ny * nz).reshape(nz, ny, nx)
        for k, v in enumerate((2.5, 0.0, np.nan, np.float32(2.4999998), np.inf)):
            W[(u >= 0.03 * k) & (u < 0.03 * (k + 1))] = v
        u = filler.unit("fuse.specialC/" + key, nx * ny * nz * 3).reshape(nz, ny, nx, 3)
        for k, v in enumerate((np.nan, -5.0, 300.0, 254.5, 0.5, -np.inf)):
            Cc[(u >= 0.02 * k) & (u < 0.02 * (k + 1))] = v
    for a in (T, W, Cc):
        a.setflags(write=False)
    return T, W, Cc


def fresh(dims):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32)


def guarded(dev, a, poison):
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(np.concatenate([np.full(G, poison, a.dtype), a, np.full(G, poison, a.dtype)])).to(dev)


def interior(t, poison, what):
    v = t.cpu().numpy()
    p = np.array(poison).astype(v.dtype)
    assert (v[:G] == p).all() and (v[-G:] == p).all(), "guards around %s" % what
    return v[G:-G]


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        iv = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        where = np.argwhere(got.view(iv) != want.view(iv))
        first = tuple(where[0])
        assert False, "%s differs in %d places, first at %r: %r, reference %r" % (what, len(where), first, got[first], want[first])


def raw_integrate(dev, d, rgb, poses, dims, geom, planes, intr=INTR, colour=True, min_depth=MIN_D, max_depth=MAX_D, obs_weight=1.0, max_weight=64.0, argv=None):
    """one call of the C entry -> (rc, (T, W, C | None)); asserts the guards, and that a refused call wrote nothing"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    B, h, w = d.shape
    nx, ny, nz = dims
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
    assert P.shape[0] in (1, B)
    dt, ct, pt = torch.from_numpy(np.array(d)).to(dev), None if rgb is None else torch.from_numpy(np.array(rgb)).to(dev), torch.from_numpy(P).to(dev)
    bufs = [guarded(dev, planes[0], P_F32), guarded(dev, planes[1], P_F32), guarded(dev, planes[2], P_F32) if colour else None]
    at = lambda t: None if t is None else C.c_void_p(t.data_ptr() + 4 * G)
    args = [_lib.ptr(dt), _lib.ptr(ct), B, h, w, (C.c_double * 4)(*intr), _lib.ptr(pt), 12 if P.shape[0] > 1 else 0, min_depth, max_depth, obs_weight, max_weight,
            nx, ny, nz, (C.c_double * 5)(*geom), at(bufs[0]), at(bufs[1]), at(bufs[2]), _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_tsdf_integrate(*args)
    torch.cuda.synchronize()
    out = [None if t is None else interior(t, P_F32, "plane %d" % k).reshape(planes[k].shape) for k, t in enumerate(bufs)]
    if rc != 0:
        for k, v in enumerate(out):
            assert v is None or v.tobytes() == np.ascontiguousarray(planes[k]).tobytes(), "a refused call wrote plane %d" % k
        return rc, None
    return rc, tuple(out)


def compare_planes(got, want, what):
    rc, planes = got
    assert rc == 0, what
    for name, v, r in zip(("tsdf", "weight", "color"), planes, want):
        if v is not None:
            same(v, r, "%s: %s" % (what, name))


@functools.lru_cache(maxsize=None)
def ref_integrate(frame_key, B, pattern, pose_key, plane_key, colour=True, dims=DIMS, geom=GEOM, obs_weight=1.0, max_weight=64.0):
    d, rgb = frame(frame_key, B, 37, 53, pattern)
    T, W, Cc = hash_planes(plane_key, dims)
    out = fref.integrate(d, rgb if colour else None, INTR, POSES[pose_key], dims, geom, T, W, Cc if colour else None, MIN_D, MAX_D, obs_weight, max_weight)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


# ---- integration -------------------------------------------------------------------------------------------------------------------------------
def test_one_mixed_frame_into_hash_planes(dev):
    d, rgb = frame("a", 1, 37, 53)
    assert np.isnan(d).any() and np.isinf(d).any() and (d < 0).any() and (d == 0).any() and (d == np.float32(0.3)).any() and (d == np.float32(9.0)).any()
    T0, W0, C0 = hash_planes("a", DIMS)
    want = ref_integrate("a", 1, "mixed", "ident", "a")
    touched = want[1] != W0
    assert 0.3 < touched.mean() < 0.95 and (want[0][~touched].tobytes() == T0[~touched].tobytes()) and (want[2][~touched].tobytes() == C0[~touched].tobytes())
    assert not touched[0, :, 0].any() and not touched[0, :, 18].any()              # x = -0.9 and 0.9 at z = 1.2: u = -20.4 and 71.9, outside the 53 columns
    compare_planes(raw_integrate(dev, d, rgb, IDENT, DIMS, GEOM, (T0, W0, C0)), want, "mixed frame")
    # fresh planes: T' = s itself, so the clamp and the band are visible
    wf = fref.integrate(d, rgb, INTR, IDENT, DIMS, GEOM, *fresh(DIMS), MIN_D, MAX_D)
    seen = wf[1] > 0
    assert (wf[0][seen] == 1).any() and ((wf[0][seen] > -1) & (wf[0][seen] < 1)).any() and (wf[0][seen] >= -1).all()
    compare_planes(raw_integrate(dev, d, rgb, IDENT, DIMS, GEOM, fresh(DIMS)), wf, "mixed frame, fresh planes")


def test_three_frames_in_one_call_are_three_calls(dev):
    d, rgb = frame("b", 3, 37, 53, "near")
    start = hash_planes("b", DIMS)
    want = ref_integrate("b", 3, "near", "per", "b")
    once = raw_integrate(dev, d, rgb, POSES["per"], DIMS, GEOM, start)
    compare_planes(once, want, "B = 3, per-sample poses")
    assert ((want[1] - start[1]) == 3).any() and ((want[1] - start[1]) == 1).any()          # voxels seen by all three frames and by one
    planes = start
    for b in range(3):
        rc, planes = raw_integrate(dev, d[b:b + 1], rgb[b:b + 1], POSES["per"][b], DIMS, GEOM, planes)
        assert rc == 0
    compare_planes((0, planes), want, "three single-frame calls")
    again = raw_integrate(dev, d, rgb, POSES["per"], DIMS, GEOM, start)
    for a, b in zip(again[1], once[1]):
        assert a.tobytes() == b.tobytes()


def test_pose_stride_zero_and_no_colour(dev):
    d, rgb = frame("b", 3, 37, 53, "near")
    start = hash_planes("b", DIMS)
    one = POSES["per"][0]
    want = fref.integrate(d, rgb, INTR, one, DIMS, GEOM, *start, MIN_D, MAX_D)
    compare_planes(raw_integrate(dev, d, rgb, one, DIMS, GEOM, start), want, "one pose for three frames")
    assert want[1].tobytes() != ref_integrate("b", 3, "near", "per", "b")[1].tobytes()
    want = ref_integrate("b", 3, "near", "per", "b", colour=False)
    for colours in (rgb, None):                                                   # color NULL: rgb is not read, given or not
        got = raw_integrate(dev, d, colours, POSES["per"], DIMS, GEOM, start, colour=False)
        compare_planes(got, want, "no colour plane")
        assert got[1][2] is None
    same(want[0], ref_integrate("b", 3, "near", "per", "b")[0], "T does not depend on the colour plane")


@pytest.mark.parametrize("pose_key", ["aside", "behind"])
def test_a_camera_that_sees_nothing_changes_nothing(dev, pose_key):
    d, rgb = frame("b", 3, 37, 53, "near")
    start = hash_planes("c", DIMS)
    want = fref.integrate(d, rgb, INTR, POSES[pose_key], DIMS, GEOM, *start, MIN_D, MAX_D)
    for a, b in zip(want, start):
        assert a.tobytes() == b.tobytes()
    compare_planes(raw_integrate(dev, d, rgb, POSES[pose_key], DIMS, GEOM, start), start, pose_key)


def test_exact_edges_of_the_band_the_clamp_the_cap_and_the_pixel_rounding(dev):
    # (1) the band: d = 2, voxel 0.25, trunc 0.5, Pz = 1 .. 3 exactly.  sdf = 0.5 gives s exactly 1, sdf = -0.5 == -trunc is kept, Pz = 2.75 is hidden.
    dims, geom, intr = (3, 3, 9), (-0.25, -0.25, 1.0, 0.25, 0.5), (20.0, 20.0, 15.5, 11.5)
    d = np.full((1, 24, 32), 2.0, np.float32)
    wf = fref.integrate(d, None, intr, IDENT, dims, geom, *fresh(dims)[:2], None, 0.0, INF)
    assert wf[0][:, 1, 1].tolist() == [1.0, 1.0, 1.0, 0.5, 0.0, -0.5, -1.0, 1.0, 1.0] and wf[1][:, 1, 1].tolist() == [1.0] * 7 + [0.0] * 2
    compare_planes(raw_integrate(dev, d, None, IDENT, dims, geom, fresh(dims), intr=intr, colour=False, min_depth=0.0, max_depth=INF), wf + (None,), "band, fresh planes")
    start = hash_planes("band", dims)
    # (2) the cap: W in [0, 5] under max_weight 3 with observations of weight 1: below, reaching and beyond the cap, also with W set exactly to 2 and 3
    W = np.array(start[1])
    W[:, 0, 0], W[:, 2, 2] = 2.0, 3.0
    want = fref.integrate(d, None, intr, IDENT, dims, geom, start[0], W, None, 0.0, INF, 1.0, 3.0)
    assert (want[1][:7, 0, 0] == 3.0).all() and (want[1][:7, 2, 2] == 3.0).all() and (want[1][:7] <= 3.0).all() and (want[1][:7] < 3.0).any() and (W[:7] > 3.0).any()
    compare_planes(raw_integrate(dev, d, None, IDENT, dims, geom, (start[0], W, start[2]), intr=intr, colour=False, min_depth=0.0, max_depth=INF, max_weight=3.0), want,
                   "band, hash planes, cap 3")
    # (3) the pixel: Pz = 2, fx = fy = 4, cx = cy = 0, P = -0.25 + idx * 0.25: u = (i - 1) / 2 and v = (j - 1) / 2 exactly.  u = -0.5 rounds up to column 0;
    # u = 0.5, 1.5 .. round up; u = 6.5 = w - 0.5 rounds up to column 7, outside the 5x7 frame.  d = 2 + (x + 8 y) / 64 and trunc 1: T' = (c + 8 r) / 64 exactly
    dims, geom, intr = (16, 12, 1), (-0.25, -0.25, 2.0, 0.25, 1.0), (4.0, 4.0, 0.0, 0.0)
    ys, xs = np.mgrid[0:5, 0:7]
    d = (2.0 + (xs + 8 * ys) / 64.0).astype(np.float32)[None]
    wf = fref.integrate(d, None, intr, IDENT, dims, geom, *fresh(dims)[:2], None, 0.0, INF)
    col = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]                              # floor((i - 1) / 2 + 0.5) for i = 0 .. 13
    row = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert wf[1][0].tolist() == [[1.0] * 14 + [0.0] * 2] * 10 + [[0.0] * 16] * 2
    assert wf[0][0, :10, :14].tolist() == [[(c + 8 * r) / 64.0 for c in col] for r in row]
    compare_planes(raw_integrate(dev, d, None, IDENT, dims, geom, fresh(dims), intr=intr, colour=False, min_depth=0.0, max_depth=INF), wf + (None,), "pixel rounding")
    start = hash_planes("pixel", dims)
    want = fref.integrate(d, None, intr, IDENT, dims, geom, start[0], start[1], None, 0.0, INF)
    compare_planes(raw_integrate(dev, d, None, IDENT, dims, geom, start, intr=intr, colour=False, min_depth=0.0, max_depth=INF), want, "pixel rounding, hash planes")


def test_integrate_rows_longer_than_one_workgroup(dev):
    dims, geom = (300, 3, 2), (-0.7, -0.1, 1.9, 0.005, 0.3)                         # 300 voxels along x: two segments of 256, the second ragged
    d, rgb = frame("b", 3, 37, 53, "near")
    start = hash_planes("wide", dims)
    want = fref.integrate(d, rgb, INTR, POSES["per"], dims, geom, *start, MIN_D, MAX_D)
    assert (want[1][:, :, 256:] != start[1][:, :, 256:]).any() and (want[1][:, :, :256] != start[1][:, :, :256]).any() and (want[1] == start[1]).any()
    compare_planes(raw_integrate(dev, d, rgb, POSES["per"], dims, geom, start), want, "300x3x2")


# ---- extraction --------------------------------------------------------------------------------------------------------------------------------
GB = 64                                                                            # guard bytes around the records


def raw_extract(dev, planes, dims, geom, min_weight=1.0, normals=1, colour=True, capacity=0, null_records=False, shift=3, argv=None):
    """one call of the C entry -> (rc, the capacity * rec bytes of the records buffer, count); asserts the guards; `shift`: the records start at an address that
    is `shift` mod 16"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    nx, ny, nz = dims
    rec = 12 + 12 * normals + (3 if colour else 0)
    tT, tW = torch.from_numpy(np.array(planes[0])).to(dev), torch.from_numpy(np.array(planes[1])).to(dev)
    tC = torch.from_numpy(np.array(planes[2])).to(dev) if colour else None
    nb = capacity * rec
    recbuf = torch.full((16 + GB + nb + GB,), P_U8, dtype=torch.uint8, device=dev)
    start = (-recbuf.data_ptr()) % 16 + shift + GB                                  # offset of the first record in recbuf
    cnt = torch.full((G + 1 + G,), P_I64, dtype=torch.int64, device=dev)
    need = L.rdm_tsdf_extract_workspace_bytes(nx, ny, nz)
    assert need == ny * nz * 8
    ws = torch.full((G + ny * nz + G,), 0x1234567812345678, dtype=torch.int64, device=dev)
    before = ws.clone()
    args = [_lib.ptr(tT), _lib.ptr(tW), _lib.ptr(tC), nx, ny, nz, (C.c_double * 5)(*geom), min_weight, normals,
            None if null_records else C.c_void_p(recbuf.data_ptr() + start), capacity, C.c_void_p(cnt.data_ptr() + 8 * G), C.c_void_p(ws.data_ptr() + 8 * G), need, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_tsdf_extract(*args)
    torch.cuda.synchronize()
    assert torch.equal(ws[:G], before[:G]) and torch.equal(ws[-G:], before[-G:]), "workspace guards"
    host, count = recbuf.cpu().numpy(), cnt.cpu().numpy()
    assert (host[:start] == P_U8).all() and (host[start + nb:] == P_U8).all(), "guards around the records"
    assert (count[:G] == P_I64).all() and (count[-G:] == P_I64).all(), "guards around count"
    assert torch.equal(tT.view(torch.int32), torch.from_numpy(np.array(planes[0])).to(dev).view(torch.int32)), "the volume is read only"
    if rc != 0 or null_records:
        assert (host == P_U8).all(), "records were written"
    if rc != 0:
        assert torch.equal(ws, before) and count[G] == P_I64, "a refused call wrote the workspace or count"
        return rc, None, None
    return rc, host[start:start + nb].tobytes(), int(count[G])


def check_extract(dev, planes, dims, geom, what, min_weight=1.0, layouts=((1, True),), slack=5, shift=3):
    """every layout against the reference, with `slack` records of room beyond the total: they stay untouched.  -> the total"""
    total = None
    for normals, colour in layouts:
        rec = 12 + 12 * normals + (3 if colour else 0)
        payload, n = fref.extract(planes[0], planes[1], planes[2] if colour else None, dims, geom, min_weight, bool(normals))
        assert len(payload) == n * rec and (total is None or n == total)
        total = n
        rc, got, count = raw_extract(dev, planes, dims, geom, min_weight, normals, colour, capacity=n + slack, shift=shift)
        assert rc == 0 and count == n, (what, normals, colour, count, n)
        if got[:n * rec] != payload:
            a, b = np.frombuffer(got[:n * rec], np.uint8).reshape(n, rec), np.frombuffer(payload, np.uint8).reshape(n, rec)
            bad = np.nonzero((a != b).any(axis=1))[0]
            assert False, "%s (normals %d, colour %d): %d of %d records differ, first %d: %r, reference %r" % (what, normals, colour, len(bad), n, bad[0], a[bad[0]].tolist(), b[bad[0]].tolist())
        assert got[n * rec:] == bytes([P_U8]) * (slack * rec), "%s: bytes beyond the last record were written" % what
    return total


ALL_LAYOUTS = ((0, False), (0, True), (1, False), (1, True))


def test_extract_the_fused_volume_in_all_four_layouts(dev):
    d, rgb = frame("b", 3, 37, 53, "near")
    planes = fref.integrate(d, rgb, INTR, POSES["per"], DIMS, GEOM, *fresh(DIMS), MIN_D, MAX_D)
    n = check_extract(dev, planes, DIMS, GEOM, "fused volume", layouts=ALL_LAYOUTS)
    assert n > 200                                                                 # random depths: a rough surface with many crossings
    assert 0 < check_extract(dev, planes, DIMS, GEOM, "fused volume, seen by all three", min_weight=3.0) < n


@pytest.mark.parametrize("shift", [0, 3, 13])
def test_extract_a_hash_volume_with_special_values(dev, shift):
    planes = hash_planes("x", DIMS, True)
    T, W, Cc = planes
    assert (T == 0).any() and np.signbit(T[T == 0]).any() and (T == 1).any() and (T == -1).any() and np.isnan(T).any() and np.isinf(T).any()
    assert (W == np.float32(2.5)).any() and (W == np.float32(2.4999998)).any() and np.isnan(W).any() and np.isnan(Cc).any() and (Cc > 255).any() and (Cc < 0).any()
    n = check_extract(dev, planes, DIMS, GEOM, "hash volume", min_weight=2.5, layouts=ALL_LAYOUTS if shift == 3 else ((1, True), (0, True)), shift=shift)
    assert 300 < n < 19 * 13 * 11 * 3 // 2
    assert check_extract(dev, planes, DIMS, GEOM, "hash volume, every weight", min_weight=-INF) > n


def test_capacity_below_the_total_null_records_and_no_crossing(dev):
    planes = hash_planes("x", DIMS, True)
    payload, n = fref.extract(*planes, DIMS, GEOM, 2.5, True)
    for cap in (0, 1, 7, 300, n - 1, n):                                           # 300: inside a row's chunk and across rows
        rc, got, count = raw_extract(dev, planes, DIMS, GEOM, 2.5, 1, True, capacity=cap + 4)
        assert rc == 0 and count == n
        rc, got, count = raw_extract(dev, planes, DIMS, GEOM, 2.5, 1, True, capacity=cap + 4, argv={10: cap})          # room for cap + 4, told cap
        assert rc == 0 and count == n, (cap, count, n)
        assert got[:cap * 27] == payload[:cap * 27] and got[cap * 27:] == bytes([P_U8]) * (4 * 27), "capacity %d" % cap
    rc, got, count = raw_extract(dev, planes, DIMS, GEOM, 2.5, 1, True, capacity=n, null_records=True)
    assert rc == 0 and count == n
    empty = fresh(DIMS)
    assert fref.extract(*empty, DIMS, GEOM, 1.0, True) == (b"", 0)
    rc, got, count = raw_extract(dev, empty, DIMS, GEOM, 1.0, 1, True, capacity=8)
    assert rc == 0 and count == 0 and got == bytes([P_U8]) * (8 * 27)
    seen = (empty[0], np.ones_like(empty[1]), empty[2])                            # observed everywhere, T = 1 everywhere: no crossing
    rc, got, count = raw_extract(dev, seen, DIMS, GEOM, 1.0, 1, True, capacity=8)
    assert rc == 0 and count == 0 and got == bytes([P_U8]) * (8 * 27)


# one voxel along x; x beyond one wavefront; 1200 rows, beyond one block of the scan; x beyond the writer's 256-voxel chunk, dense enough for several
# hundred records per chunk; a single voxel
SHAPES = [("nx1", (1, 13, 11)), ("x70", (70, 9, 5)), ("rows1200", (3, 40, 30)), ("x300", (300, 3, 2)), ("x600", (600, 1, 1)), ("one", (1, 1, 1)), ("col", (1, 1, 40))]


@pytest.mark.parametrize("key,dims", SHAPES, ids=[s[0] for s in SHAPES])
def test_extract_shapes(dev, key, dims):
    planes = hash_planes("shape." + key, dims, True)
    geom = (0.3, -0.2, 1.0, 0.05, 0.2)
    n = check_extract(dev, planes, dims, geom, key, min_weight=2.5, layouts=((1, True), (0, False)))
    assert n > 0 or key == "one"
    if key in ("x300", "x600"):                                                   # every weight counts: a chunk of 256 voxels hands over more records than a wavefront has lanes
        m = check_extract(dev, planes, dims, geom, key + ", every weight", min_weight=-INF)
        assert m > 100 * dims[1] * dims[2]


def test_extract_twice_gives_the_same_bytes(dev):
    planes = hash_planes("x", DIMS, True)
    n = fref.extract(*planes, DIMS, GEOM, 2.5, True)[1]
    a, b = (raw_extract(dev, planes, DIMS, GEOM, 2.5, 1, True, capacity=n) for _ in range(2))
    assert a[0] == 0 and a == b


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control ------------------------------------------------
def integrate_case(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    d, rgb = frame("b", 3, 37, 53, "near")
    T, W, Cc = hash_planes("b", DIMS)
    intr, geom = (C.c_double * 4)(*INTR), (C.c_double * 5)(*GEOM)
    ins = dict(d=torch.from_numpy(np.array(d)).to(dev), rgb=torch.from_numpy(np.array(rgb)).to(dev), poses=torch.from_numpy(POSES["per"].reshape(3, 12).copy()).to(dev),
               tsdf=torch.from_numpy(np.array(T)).to(dev), weight=torch.from_numpy(np.array(W)).to(dev), color=torch.from_numpy(np.array(Cc)).to(dev))

    def call(b, st):
        _lib.check(L.rdm_tsdf_integrate(_lib.ptr(b["d"]), _lib.ptr(b["rgb"]), 3, 37, 53, intr, _lib.ptr(b["poses"]), 12, MIN_D, MAX_D, 1.0, 64.0, 19, 13, 11, geom,
                                        _lib.ptr(b["tsdf"]), _lib.ptr(b["weight"]), _lib.ptr(b["color"]), st))
    return sp.Case(ins, call, outs=("tsdf", "weight", "color"))


def extract_case(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    T, W, Cc = hash_planes("x", DIMS, True)
    n = fref.extract(T, W, Cc, DIMS, GEOM, 2.5, True)[1]
    geom = (C.c_double * 5)(*GEOM)
    wsb = L.rdm_tsdf_extract_workspace_bytes(19, 13, 11)
    ins = dict(tsdf=torch.from_numpy(np.array(T)).to(dev), weight=torch.from_numpy(np.array(W)).to(dev), color=torch.from_numpy(np.array(Cc)).to(dev))
    scratch = dict(records=torch.empty(n * 27, dtype=torch.uint8, device=dev), count=torch.empty(1, dtype=torch.int64, device=dev),
                   ws=torch.empty(wsb // 8, dtype=torch.int64, device=dev))

    def call(b, st):
        _lib.check(L.rdm_tsdf_extract(_lib.ptr(b["tsdf"]), _lib.ptr(b["weight"]), _lib.ptr(b["color"]), 19, 13, 11, geom, 2.5, 1, _lib.ptr(b["records"]), n, _lib.ptr(b["count"]),
                                      _lib.ptr(b["ws"]), wsb, st))
    return sp.Case(ins, call, outs=("records", "count"), scratch=scratch)


@pytest.fixture(scope="module")
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


def watched(case, delay):
    """the case, its call noting whether delay.S was still in its delay when the host had enqueued the whole call -> (case, {"delay_running": bool})"""
    inner, seen = case.call, {}

    def call(b, st):
        out = inner(b, st)
        seen["delay_running"] = not delay.S.query()
        return out
    case.call = call
    return case, seen


def test_integrate_on_a_late_non_default_stream(dev, delay):
    got = sp.check(integrate_case(dev), delay)
    want = ref_integrate("b", 3, "near", "per", "b")
    for k, r in zip(("tsdf", "weight", "color"), want):
        assert got[k].cpu().numpy().tobytes() == r.tobytes(), k


def test_extract_on_a_late_non_default_stream(dev, delay):
    got = sp.check(extract_case(dev), delay)
    payload, n = fref.extract(*hash_planes("x", DIMS, True), DIMS, GEOM, 2.5, True)
    assert int(got["count"].item()) == n and got["records"].cpu().numpy().tobytes() == payload


def test_control_calls_on_the_null_stream_are_detected(dev, delay):
    """extract writes into the harness's poisoned buffers: stream_probe.control as it stands (count differs from the reference AND is poisoned).  integrate
    updates planes in place and stores nothing where it sees the poisoned inputs (NaN depths and poses: every frame is skipped), so nothing of its result can
    carry the poison: there the planes, snapshotted as the late copies left them, must all differ from the reference."""
    assert beside_null(delay), "the stream does not run beside the null stream: the controls could prove nothing"
    case, seen = watched(extract_case(dev), delay)
    sp.control(case, delay)
    assert seen["delay_running"], "the delay had run out before the call was enqueued: the host was held up inside the call"
    case, seen = watched(integrate_case(dev), delay)
    ref_planes = sp.reference_run(case)
    snap = sp.late_run(case, delay, wrong_stream=True)
    assert seen["delay_running"], "the delay had run out before the call was enqueued: the host was held up inside the call"
    assert sorted(sp.mismatches(case, snap, ref_planes)) == sorted(ref_planes), "an integrate call on the wrong stream went undetected"
    for k in snap:
        assert sp.same_bits(snap[k], case.staged[k]), k                             # it saw the poisoned inputs and changed nothing


# ---- refusals on the device: nothing is written ------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    d, rgb = frame("bad", 2, 37, 53, "near")
    planes = hash_planes("bad", DIMS)
    nan, inf = float("nan"), float("inf")
    I4, G5 = lambda *v: (C.c_double * 4)(*v), lambda *v: (C.c_double * 5)(*v)
    # positions: 0 depth, 1 rgb, 2 batch, 3 h, 4 w, 5 intr, 6 poses, 7 pose_stride, 8 min_depth, 9 max_depth, 10 obs_weight, 11 max_weight, 12 nx, 13 ny, 14 nz, 15 geom,
    # 16 tsdf, 17 weight, 18 color, 19 stream
    rows = (({0: None}, b"depth"), ({5: None}, b"intr"), ({6: None}, b"poses"), ({15: None}, b"geom"), ({16: None}, b"tsdf"), ({17: None}, b"weight"), ({1: None}, b"color needs rgb"),
            ({2: 0}, b"batch"), ({2: 65536}, b"65535"), ({3: 0}, b"h"), ({4: -1}, b"w"), ({3: 65536, 4: 32768}, b"h * w"), ({5: I4(nan, 1, 0, 0)}, b"intr"),
            ({5: I4(1, 0, 0, 0)}, b"intr"), ({8: -1.0}, b"min_depth"), ({8: nan}, b"min_depth"), ({9: nan}, b"max_depth"), ({8: 2.0, 9: 1.0}, b"max_depth"), ({7: 6}, b"pose_stride"),
            ({12: 0}, b"nx"), ({13: 0}, b"ny"), ({14: -1}, b"nz"), ({12: 2048, 13: 2048, 14: 512}, b"nx * ny * nz"), ({15: G5(0, nan, 0, 0.1, 0.4)}, b"geom"),
            ({15: G5(0, 0, 0, 0, 0.4)}, b"voxel"), ({15: G5(0, 0, 0, 0.1, 0)}, b"trunc"), ({15: G5(0, 0, 0, 0.1, inf)}, b"trunc"), ({10: 0.0}, b"obs_weight"),
            ({10: inf}, b"obs_weight"), ({10: nan}, b"obs_weight"), ({11: nan}, b"max_weight"), ({11: 0.5}, b"max_weight"))
    for argv, word in rows:
        rc = raw_integrate(dev, d, rgb, POSES["per"][:2], DIMS, GEOM, planes, argv=argv)[0]          # raw_integrate asserts that nothing at all was written
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    # positions: 0 tsdf, 1 weight, 2 color, 3 nx, 4 ny, 5 nz, 6 geom, 7 min_weight, 8 normals, 9 records, 10 capacity, 11 count, 12 workspace, 13 workspace_bytes, 14 stream
    rows = (({0: None}, b"tsdf"), ({1: None}, b"weight"), ({6: None}, b"geom"), ({11: None}, b"count"), ({12: None}, b"workspace"), ({3: 0}, b"nx"), ({4: -1}, b"ny"), ({5: 0}, b"nz"),
            ({3: 2048, 4: 2048, 5: 512}, b"nx * ny * nz"), ({6: G5(inf, 0, 0, 0.1, 0.4)}, b"geom"), ({6: G5(0, 0, 0, -1, 0.4)}, b"voxel"), ({6: G5(0, 0, 0, 0.1, nan)}, b"trunc"),
            ({7: nan}, b"min_weight"), ({8: 2}, b"normals"), ({10: -1}, b"capacity"), ({13: 13 * 11 * 8 - 1}, b"workspace_bytes"))
    for argv, word in rows:
        rc = raw_extract(dev, planes, DIMS, GEOM, capacity=16, argv=argv)[0]                          # raw_extract asserts that nothing at all was written
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, L.rdm_last_error_string())
    ws = torch.zeros(13 * 11 + 2, dtype=torch.int64, device=dev)
    rc = raw_extract(dev, planes, DIMS, GEOM, capacity=16, argv={12: C.c_void_p(ws.data_ptr() + 4)})[0]
    assert rc == -1 and b"aligned" in L.rdm_last_error_string() and not ws.any()


# ---- through the product ----------------------------------------------------------------------------------------------------------------------
def test_volume_wrapper_is_the_c_entries(dev):
    from md_rdm_amd import _lib, fuse
    d, rgb = frame("b", 3, 37, 53, "near")
    dt, ct = torch.from_numpy(np.array(d)).to(dev), torch.from_numpy(np.array(rgb)).to(dev)
    vol = fuse.Volume(DIMS, GEOM[:3], GEOM[3], device=dev)
    assert vol.trunc == 4.0 * GEOM[3] and vol.tsdf.eq(1).all() and not vol.weight.any() and not vol.color.any()
    assert vol.integrate(dt[:2], INTR, POSES["per"][:2], rgb=ct[:2], min_depth=MIN_D, max_depth=MAX_D) is vol
    vol.integrate(dt[2:], INTR, torch.from_numpy(POSES["per"][2]).to(dev), rgb=ct[2:], min_depth=MIN_D, max_depth=MAX_D)          # a pose on the device stays there
    want = fref.integrate(d, rgb, INTR, POSES["per"], DIMS, GEOM, *fresh(DIMS), MIN_D, MAX_D)
    compare_planes((0, (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy())), want, "Volume.integrate")
    for normals in (True, False):
        records, n = vol.extract(normals=normals)
        payload, m = fref.extract(*want, DIMS, GEOM, 1.0, normals)
        assert n == m > 0 and records.dtype == torch.uint8 and records.cpu().numpy().tobytes() == payload
    plain = fuse.Volume(DIMS, GEOM[:3], GEOM[3], trunc=GEOM[4], color=False, max_weight=2.0, device=dev).integrate(dt, INTR, POSES["per"], min_depth=MIN_D, max_depth=MAX_D)
    want = fref.integrate(d, None, INTR, POSES["per"], DIMS, GEOM, *fresh(DIMS)[:2], None, MIN_D, MAX_D, 1.0, 2.0)
    compare_planes((0, (plain.tsdf.cpu().numpy(), plain.weight.cpu().numpy(), None)), want, "Volume without colour")
    records, n = plain.extract(normals=True, min_weight=2.0)
    assert (records.cpu().numpy().tobytes(), n) == fref.extract(want[0], want[1], None, DIMS, GEOM, 2.0, True) and plain.color is None
    for bad in (lambda: vol.integrate(dt, INTR, IDENT), lambda: vol.integrate(dt.cpu(), INTR, IDENT, rgb=ct), lambda: vol.integrate(dt, INTR, np.stack([IDENT] * 2), rgb=ct),
                lambda: vol.integrate(dt, INTR, IDENT, rgb=ct, weight=0.0), lambda: vol.integrate(dt, INTR, IDENT, rgb=ct, min_depth=2.0, max_depth=1.0),
                lambda: vol.integrate(dt.double(), INTR, IDENT, rgb=ct), lambda: vol.extract(min_weight=math.nan)):
        with pytest.raises(_lib.RdmError):
            bad()


def test_volume_write_ply(dev, tmp_path):
    from md_rdm_amd import cloud, fuse
    d, rgb = frame("b", 3, 37, 53, "near")
    vol = fuse.Volume(DIMS, GEOM[:3], GEOM[3], device=dev)
    vol.integrate(torch.from_numpy(np.array(d)).to(dev), INTR, POSES["per"], rgb=torch.from_numpy(np.array(rgb)).to(dev), min_depth=MIN_D, max_depth=MAX_D)
    n = vol.write_ply(str(tmp_path / "v.ply"), normals=True)
    payload, m = fref.extract(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy(), DIMS, GEOM, 1.0, True)
    assert n == m > 0 and (tmp_path / "v.ply").read_bytes() == cloud.ply_header(n, True, True) + payload


def test_predict_fused_is_integrate_of_predict_metric(dev):
    from md_rdm_amd import cloud, evaluate, fuse
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    x = torch.from_numpy(np.array(evaluate.synthetic_samples(2, 226, 226)[0])).to(dev)
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 226.0, 226.0), (128, 128))
    rgb = torch.from_numpy((filler.unit("fuse.predict.rgb", 2 * 128 * 128 * 3) * 256.0).astype(np.uint8).reshape(2, 128, 128, 3)).to(dev)
    plane = m.predict_metric(x, (128, 128), want=("f32",))["f32"]
    host = plane.cpu().numpy()
    ok = fref.valid(host)
    assert ok.any()
    z = float(np.median(host[ok]))                                                  # the hash-filled model's maps are not depth: the volume goes where its values are
    voxel = z / 16.0
    dims, origin = (16, 16, 12), (-8.0 * voxel, -8.0 * voxel, z - 6.0 * voxel)
    poses = POSES["per"][:2]
    a, b = fuse.Volume(dims, origin, voxel, device=dev), fuse.Volume(dims, origin, voxel, device=dev)
    fused = m.predict_fused(x, (128, 128), intr, poses, a, rgb=rgb)
    assert sp.same_bits(fused, plane)
    b.integrate(plane, intr, poses, rgb=rgb)
    for k in ("tsdf", "weight", "color"):
        assert sp.same_bits(getattr(a, k), getattr(b, k)), k
    want = fref.integrate(host, rgb.cpu().numpy(), intr, poses, dims, origin + (voxel, 4.0 * voxel), *fresh(dims))
    compare_planes((0, (a.tsdf.cpu().numpy(), a.weight.cpu().numpy(), a.color.cpu().numpy())), want, "predict_fused")
    assert (want[1] > 0).any()


def test_predict_command_synthetic_fuse(dev, tmp_path):
    from md_rdm_amd import predict
    out = tmp_path / "maps"
    poses = tmp_path / "poses.txt"
    np.savetxt(str(poses), POSES["per"].reshape(3, 12))
    assert predict.main(["--synthetic", "3", "--out", str(out), "--metric", "--full_res", "--batch_size", "2", "--fuse", "--poses", str(poses), "--max_depth", "10",
                         "--fuse_voxel", "0.25", "--ply_normals"]) == 0
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(["synthetic_000%d.npy" % i for i in range(3)] + ["fused.ply"]), names
    blob = (out / "fused.ply").read_bytes()
    head, payload = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and "property float nx" in lines and "property uchar red" in lines
    count = int([ln for ln in lines if ln.startswith("element vertex ")][0].split()[-1])
    assert len(payload) == count * 27
