"""rdm_depth_mesh (include/rdm_mesh.h) and md_rdm_amd.mesh on the MI355X against the numpy statement of the contract (tests/mesh_ref.py).

The comparison is BIT FOR BIT - faces, face_count and vertex_count, both layouts: every output is an integer, the only arithmetic is float64
subtraction, fabs and one float64 multiplication, each correctly rounded on the device and in numpy.  No tolerance exists.
Every call writes between guard bytes - in front of the buffer, between the samples (the stride is longer than a sample can need, and odd), behind
each sample's face_count * rec bytes and behind the buffer - which must stay untouched; the base address is shifted by 0..3 bytes."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import cloud_ref as cref
import mesh_ref as mref
import stream_probe as sp
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
G, GAP, GUARD, CGUARD = 64, 37, 0xA5, 0x5A5A5A5A      # guard bytes in front and behind; unused bytes behind every sample's region; their values
INTR = (97.5, 101.25, 25.75, 17.5)
LAYOUTS = ("i32", "ply")
MIN_D, MAX_D = 0.5, 8.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def T(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                                  # a copy: the cached frames are read-only


@functools.lru_cache(maxsize=None)
def frame(key, B, h, w, pattern="mixed", holes=0.25):
    """(B,h,w) float32, hash-generated, read-only.  "mixed": depths in [2, 2.1] (neighbours differ by up to 5 %), a seventh of them doubled (steps
    no ratio below 1.9 bridges), `holes` of the pixels 0 and about 1 % each NaN, +inf, negative, below MIN_D and above MAX_D; sample b's holes are
    drawn apart from the others'.  "all": no holes, no steps.  "none": every pixel 0."""
    d = filler.uniform("mesh.depth/" + key, (B, h, w), 2.0, 2.1).astype(np.float32)
    if pattern == "mixed":
        u = filler.unit("mesh.mask/" + key, B * h * w).reshape(B, h, w)
        v = filler.unit("mesh.step/" + key, B * h * w).reshape(B, h, w)
        d[v < 1.0 / 7.0] *= np.float32(2.0)
        d[u < holes] = 0.0
        for k, bad in enumerate((np.nan, np.inf, -1.5, 0.3, 9.0)):
            d[(u >= holes + 0.01 * k) & (u < holes + 0.01 * (k + 1))] = bad
    elif pattern == "none":
        d[:] = 0.0
    else:
        assert pattern == "all"
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def samples(key, B, h, w, pattern, holes, step, ratio):
    """mesh_ref.sample_faces of every sample of a frame, computed once"""
    d = frame(key, B, h, w, pattern, holes)
    return tuple(mref.sample_faces(d[b], MIN_D, MAX_D, step, ratio) for b in range(B))


def want(key, B, h, w, pattern, holes, step, ratio, layout):
    ss = samples(key, B, h, w, pattern, holes, step, ratio)
    return [mref.pack(s["faces"], layout) for s in ss], [len(s["faces"]) for s in ss], [s["vertex_count"] for s in ss]


def raw(dev, d, step=1, ratio=1.05, layout="i32", shift=0, argv=None, vertex_count=True):
    """one call of the C entry -> (rc, [the bytes of sample b's faces], face counts, vertex counts | None); asserts the guards"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    dt = d if isinstance(d, torch.Tensor) else T(d, dev)
    B, h, w = dt.shape
    rec = mref.face_bytes(layout)
    need = 2 * (-(-h // step) - 1) * (-(-w // step) - 1) * rec
    stride = need + GAP + (need + GAP + 1) % 2                                    # larger than needed, and odd
    assert stride % 2 == 1
    buf = torch.full((G + shift + B * stride + G,), GUARD, dtype=torch.uint8, device=dev)
    cnt = torch.full((2, 1 + B + 1), CGUARD, dtype=torch.int32, device=dev)
    wsb = L.rdm_depth_mesh_workspace_bytes(B, h, w, step)
    assert wsb > 0
    ws = torch.full((wsb // 4 + 2,), CGUARD, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    base = buf.data_ptr() + G + shift
    args = [_lib.ptr(dt), B, h, w, MIN_D, MAX_D, step, ratio, _lib.MESH_FACES[layout], C.c_void_p(base), stride, C.c_void_p(cnt[0].data_ptr() + 4),
            C.c_void_p(cnt[1].data_ptr() + 4) if vertex_count else None, C.c_void_p(ws.data_ptr() + 4), wsb, _lib.stream()]
    for pos, val in (argv or {}).items():
        args[pos] = val
    rc = L.rdm_depth_mesh(*args)
    torch.cuda.synchronize()
    out, c, wsh = buf.cpu().numpy(), cnt.cpu().numpy(), ws.cpu().numpy()
    assert (out[:G + shift] == GUARD).all() and (out[G + shift + B * stride:] == GUARD).all(), "guards around the buffer"
    assert (c[:, 0] == CGUARD).all() and (c[:, -1] == CGUARD).all(), "count guards"
    assert wsh[0] == CGUARD and wsh[-1] == CGUARD, "workspace guards"
    if rc != 0:
        assert (out == GUARD).all() and (c == CGUARD).all() and (wsh == CGUARD).all(), "a refused call wrote"
        return rc, None, None, None
    if not vertex_count:
        assert (c[1] == CGUARD).all()
    recs = []
    for b in range(B):
        region = out[G + shift + b * stride:G + shift + (b + 1) * stride]
        assert 0 <= c[0, 1 + b] * rec <= need, (b, c[0, 1 + b])
        assert (region[c[0, 1 + b] * rec:] == GUARD).all(), "sample %d: bytes behind face_count * rec were touched" % b
        recs.append(region[:c[0, 1 + b] * rec].tobytes())
    return rc, recs, c[0, 1:-1].tolist(), c[1, 1:-1].tolist() if vertex_count else None


def compare(got, wanted, what):
    rc, recs, fc, vc = got
    wrecs, wfc, wvc = wanted
    assert rc == 0, what
    assert fc == wfc, "%s: face counts %r, reference %r" % (what, fc, wfc)
    assert vc is None or vc == wvc, "%s: vertex counts %r, reference %r" % (what, vc, wvc)
    for b, (g, r) in enumerate(zip(recs, wrecs)):
        if g != r:
            rec = len(r) // max(wfc[b], 1)
            k = next(i for i in range(len(r)) if g[i] != r[i]) // rec
            assert False, "%s: sample %d differs first at face %d: %r, reference %r" % (what, b, k, g[k * rec:(k + 1) * rec], r[k * rec:(k + 1) * rec])


# ---- (a) the frame that exercises the contract, and (f) its indices against the cloud's records -------------------------------------------------
RATIOS = (1.02, 1.5, math.inf)


def exercised(s):
    """what one sample's reference output contains: names of the contract's cases"""
    vA, vB, vC, vD = (s["valid"][:-1, :-1], s["valid"][:-1, 1:], s["valid"][1:, :-1], s["valid"][1:, 1:])
    four = vA & vB & vC & vD
    emitted = np.zeros(s["ad"].shape + (2,), bool)
    emitted.reshape(-1, 2)[s["cell"], s["cand"]] = True
    seen = set()
    if (four & s["ad"]).any():
        seen.add("AD")
    if (four & ~s["ad"]).any():
        seen.add("BC")
    for name, others, cand in (("no A", vB & vC & vD & ~vA, 1), ("no B", vA & vC & vD & ~vB, 0), ("no C", vA & vB & vD & ~vC, 1), ("no D", vA & vB & vC & ~vD, 0)):
        if (others & emitted[..., cand]).any():
            seen.add(name)
        assert not (others & emitted[..., 1 - cand]).any()
    if s["cut"].any():
        seen.add("cut")
    if len(s["faces"]):
        seen.add("faces")
    return seen


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("ratio", RATIOS, ids=["r1.02", "r1.5", "rinf"])
def test_hash_frame_with_holes_and_steps(dev, ratio, step):
    d = frame("a", 1, 37, 53)
    s = samples("a", 1, 37, 53, "mixed", 0.25, step, ratio)[0]
    need = {"AD", "BC", "no A", "no B", "no C", "no D", "faces"} | ({"cut"} if ratio < math.inf else set())
    assert exercised(s) >= need, sorted(need - exercised(s))            # otherwise a passing comparison shows nothing
    assert not np.isfinite(d).all() and (d < 0).any() and (d == np.float32(0.3)).any() and (d == np.float32(9.0)).any() and 0.2 < (d == 0).mean() < 0.3
    for shift, layout in enumerate(LAYOUTS):
        compare(raw(dev, d, step, ratio, layout, shift=shift + step), want("a", 1, 37, 53, "mixed", 0.25, step, ratio, layout), "37x53 step %d ratio %r %s" % (step, ratio, layout))


@pytest.mark.parametrize("step", [1, 3])
def test_indices_are_the_clouds_record_numbers(dev, step):
    from md_rdm_amd import cloud, mesh
    d = frame("a", 1, 37, 53)
    s = samples("a", 1, 37, 53, "mixed", 0.25, step, 1.5)[0]
    tri, fc, vc = mesh.faces(T(d, dev), MIN_D, MAX_D, step, 1.5, "i32")
    records, counts = cloud.point_cloud(T(d, dev), INTR, min_depth=MIN_D, max_depth=MAX_D, step=step)
    assert vc.cpu().tolist() == counts.cpu().tolist() == [s["vertex_count"]] and fc.cpu().tolist() == [len(s["faces"])]
    got = mref.unpack(tri[0, :len(s["faces"]) * 12].cpu().numpy().tobytes(), "i32")
    np.testing.assert_array_equal(got, s["faces"])
    xyz = records[0, :s["vertex_count"] * 12].cpu().numpy().view("<f4").reshape(-1, 3)
    pts = cref.points(d[0], INTR).astype(np.float32)
    sw1 = s["ad"].shape[1]
    i, j = s["cell"] // sw1, s["cell"] % sw1
    ad = s["ad"][i, j]
    A, B, Cc, D = (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
    pick = lambda yes, p, q: (np.where(yes, p[0], q[0]), np.where(yes, p[1], q[1]))
    first = s["cand"] == 0
    corners = (pick(ad | first, A, B),                                            # (A, C, D) (A, D, B) | (A, C, B) (B, C, D)
               pick(ad, pick(first, Cc, D), Cc),
               pick(ad, pick(first, D, B), pick(first, B, D)))
    for k, (ci, cj) in enumerate(corners):                                        # the cloud's record at the index is the record of the corner's pixel
        np.testing.assert_array_equal(xyz[got[:, k]].view(np.int32), pts[ci * step, cj * step].view(np.int32))


# ---- (b), (c), (d): long rows, many rows, degenerate grids ---------------------------------------------------------------------------------------
# 3x521 and 2x700: 520 and 699 cells, a cell row longer than two 256-thread chunks; 300x5: 299 table entries ahead of the last row, more than one per thread
SHAPES = [("b", 3, 521, "mixed", 1), ("c", 300, 5, "mixed", 1), ("b", 3, 521, "mixed", 2), ("all", 19, 23, "all", 1), ("none", 19, 23, "none", 1), ("row", 1, 40, "mixed", 1),
          ("col", 40, 1, "mixed", 1), ("steprow", 3, 40, "all", 3), ("stepcol", 40, 2, "all", 2), ("one", 1, 1, "all", 1), ("wide", 2, 700, "all", 1)]


@pytest.mark.parametrize("key,h,w,pattern,step", SHAPES, ids=["%s-%dx%d-s%d" % (k, h, w, s) for k, h, w, _, s in SHAPES])
def test_shapes(dev, key, h, w, pattern, step):
    d = frame(key, 2, h, w, pattern, 0.1)
    ratio = 1.06 if pattern == "all" else 1.04                                  # "all" spans [2, 2.1]: 1.06 keeps every face, 1.04 cuts some of the others'
    for layout in LAYOUTS:
        wanted = want(key, 2, h, w, pattern, 0.1, step, ratio, layout)
        sh, sw = -(-h // step), -(-w // step)
        if pattern == "all":
            assert wanted[1] == [2 * (sh - 1) * (sw - 1)] * 2 and wanted[2] == [sh * sw] * 2
        elif pattern == "none":
            assert wanted[1] == [0, 0] and wanted[2] == [0, 0]
        else:
            assert all(0 < v < sh * sw for v in wanted[2]) and (min(sh, sw) == 1 or all(0 < f < 2 * (sh - 1) * (sw - 1) for f in wanted[1]))
        if min(sh, sw) == 1:
            assert wanted[1] == [0, 0]
        compare(raw(dev, d, step, ratio, layout, shift=3), wanted, "%dx%d step %d %s %s" % (h, w, step, pattern, layout))


# ---- (e) batches, determinism, untouched bytes ---------------------------------------------------------------------------------------------------
def test_batch_alone_repeated_and_without_vertex_count(dev):
    d = frame("e", 3, 37, 53)
    assert not (d[0] == d[1]).all() and len({(d[b] == 0).tobytes() for b in range(3)}) == 3                 # three different hole patterns
    for layout in LAYOUTS:
        wanted = want("e", 3, 37, 53, "mixed", 0.25, 1, 1.04, layout)
        base = raw(dev, d, 1, 1.04, layout)                                      # raw() asserts the sentinel behind face_count * rec and the odd, larger stride
        compare(base, wanted, "batch of 3 %s" % layout)
        assert len(set(wanted[1])) == 3
        again = raw(dev, d, 1, 1.04, layout, shift=1)
        assert again[1:] == base[1:]
        for b in range(3):
            one = raw(dev, d[b:b + 1], 1, 1.04, layout, shift=b)
            assert one[1][0] == base[1][b] and one[2][0] == base[2][b] and one[3][0] == base[3][b], b
        compare(raw(dev, d, 1, 1.04, layout, vertex_count=False), wanted, "vertex_count NULL %s" % layout)


# ---- (g) the stream argument: tests/stream_probe.py's late producer, with the null-stream control -------------------------------------------------
def stream_case(dev):
    from md_rdm_amd import _lib, mesh
    L = _lib.lib()
    d = frame("stream", 2, 37, 53, "all")                                         # all valid and flat: every byte of every output is written
    wsb = L.rdm_depth_mesh_workspace_bytes(2, 37, 53, 1)
    stride = 2 * 36 * 52 * 13
    scratch = dict(faces=torch.empty(2, stride, dtype=torch.uint8, device=dev), fc=torch.empty(2, dtype=torch.int32, device=dev),
                   vc=torch.empty(2, dtype=torch.int32, device=dev), ws=torch.empty(wsb // 4, dtype=torch.int32, device=dev))

    def call(b, st):
        _lib.check(L.rdm_depth_mesh(_lib.ptr(b["d"]), 2, 37, 53, 0.0, math.inf, 1, 1.06, 1, _lib.ptr(b["faces"]), stride, _lib.ptr(b["fc"]), _lib.ptr(b["vc"]), _lib.ptr(b["ws"]),
                                    wsb, st))
        tri, fc, vc = mesh.faces(b["d"], edge_ratio=1.06, layout="ply")           # the wrapper resolves the stream itself
        return dict(wrapped_faces=tri, wrapped_fc=fc, wrapped_vc=vc)
    return sp.Case(dict(d=T(d, dev)), call, outs=("faces", "fc", "vc"), scratch=scratch)


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay):
    got = sp.check(stream_case(dev), delay)
    d = frame("stream", 2, 37, 53, "all")
    recs, fc, vc = mref.reference(d, 0.0, math.inf, 1, 1.06, "ply")
    assert fc.tolist() == [2 * 36 * 52] * 2 and got["fc"].cpu().tolist() == fc.tolist() == got["wrapped_fc"].cpu().tolist()
    assert got["vc"].cpu().tolist() == vc.tolist() == got["wrapped_vc"].cpu().tolist()
    for b in range(2):
        assert got["faces"][b].cpu().numpy().tobytes() == recs[b] == got["wrapped_faces"][b].cpu().numpy().tobytes()


def test_control_call_on_the_null_stream_is_detected(dev, delay):
    sp.control(stream_case(dev), delay)


# ---- refusals on the device: nothing is written ------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib, mesh
    d = frame("bad", 2, 5, 7, "all")
    for argv, word in (({0: None}, b"depth"), ({6: 0}, b"step"), ({7: 0.5}, b"edge_ratio"), ({7: float("nan")}, b"edge_ratio"), ({8: 2}, b"layout"),
                       ({10: 2 * 4 * 6 * 12 - 1}, b"sample_stride_bytes"), ({4: -1.0}, b"min_depth"), ({4: 2.0, 5: 1.0}, b"max_depth"), ({14: 4}, b"workspace_bytes"),
                       ({13: None}, b"workspace")):
        rc = raw(dev, d, argv=argv)[0]                                             # raw() asserts that nothing at all was written
        assert rc == -1 and word in _lib.lib().rdm_last_error_string(), (argv, _lib.lib().rdm_last_error_string())
    t = T(d, dev)
    for bad in (lambda: mesh.faces(t.double()), lambda: mesh.faces(t[0]), lambda: mesh.faces(t, step=0), lambda: mesh.faces(t, edge_ratio=0.9),
                lambda: mesh.faces(t, layout="obj"), lambda: mesh.faces(t, min_depth=3.0, max_depth=2.0)):
        with pytest.raises(_lib.RdmError):
            bad()


# ---- (h) through the product ----------------------------------------------------------------------------------------------------------------------
def parse_ply(data, rec):
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[-2] == "property list uchar int vertex_indices"
    nv, nf = int(lines[2].split()[2]), int(lines[-3].split()[2])
    assert lines[2].startswith("element vertex ") and lines[-3].startswith("element face ") and len(body) == nv * rec + nf * 13
    return nv, nf, body[:nv * rec], body[nv * rec:]


def test_predict_mesh_and_write_ply(dev, tmp_path):
    from md_rdm_amd import cloud, evaluate, mesh
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    m.deterministic = True                                                          # ordered reductions: two forwards of one input give the same bits
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).eval()
    x = T(evaluate.synthetic_samples(2, 226, 226)[0], dev)
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 226.0, 226.0), (128, 128))
    plane = m.predict_metric(x, (128, 128), want=("f32",))["f32"]
    d = plane.cpu().numpy()
    zs = np.sort(d.reshape(-1))
    lo, hi = float(zs[len(zs) // 50]), float(zs[-len(zs) // 50])                   # bounds that drop a fiftieth of the pixels at each end: holes in the mesh
    ratio = float(np.quantile(np.maximum(d[:, :, 1:], d[:, :, :-1]) / np.minimum(d[:, :, 1:], d[:, :, :-1]), 0.9))      # cuts about a tenth of the horizontal edges
    assert lo > 0 and ratio >= 1
    records, vcounts, tri, fcounts = m.predict_mesh(x, (128, 128), intr, normals=True, min_depth=lo, max_depth=hi, step=2, edge_ratio=ratio)
    wrec, wcnt = cloud.point_cloud(plane, intr, normals=True, min_depth=lo, max_depth=hi, step=2)
    assert sp.same_bits(vcounts, wcnt) and all(sp.same_bits(records[b, :n * 24], wrec[b, :n * 24]) for b, n in enumerate(wcnt.cpu().tolist()))
    refs, rfc, rvc = mref.reference(d, lo, hi, 2, ratio, "ply")
    assert fcounts.cpu().tolist() == rfc.tolist() and vcounts.cpu().tolist() == rvc.tolist()
    print("predict_mesh: %r faces of %d cells, %r vertices, edge_ratio %r" % (rfc.tolist(), 63 * 63, rvc.tolist(), ratio))
    assert all(f > 0 for f in rfc.tolist()), rfc
    for b in range(2):
        p = str(tmp_path / ("mesh%d.ply" % b))
        mesh.write_ply(p, records[b], rvc[b], True, False, tri[b], rfc[b])
        nv, nf, vbody, fbody = parse_ply(open(p, "rb").read(), 24)
        assert (nv, nf) == (rvc[b], rfc[b]) and fbody == refs[b] and vbody == wrec[b, :nv * 24].cpu().numpy().tobytes()
        assert mref.unpack(fbody, "ply").max() < nv


def test_predict_command_synthetic_mesh(dev, tmp_path):
    from md_rdm_amd import cloud, predict
    out = tmp_path / "maps"
    assert predict.main(["--synthetic", "2", "--out", str(out), "--metric", "--ply", "--ply_step", "2", "--mesh", "--mesh_edge_ratio", "1.01"]) == 0
    assert sorted(p.name for p in out.iterdir()) == ["synthetic_0000.npy", "synthetic_0000.ply", "synthetic_0001.npy", "synthetic_0001.ply"]
    intr = cloud.intrinsics_in_view(cloud.INTRINSICS["nyu"], (0.0, 0.0, 226.0, 226.0), (128, 128))
    for i in range(2):
        d = np.load(str(out / ("synthetic_%04d.npy" % i)))
        assert d.dtype == np.float32 and d.shape == (1, 128, 128)
        vrecs, vcounts = cref.reference(d, intr, None, False, step=2)
        frecs, fc, vc = mref.reference(d, step=2, edge_ratio=1.01, layout="ply")
        nv, nf, vbody, fbody = parse_ply(open(str(out / ("synthetic_%04d.ply" % i)), "rb").read(), 12)
        print("synthetic_%04d.ply: %d vertices, %d faces of %d cells" % (i, nv, nf, 63 * 63))
        assert (nv, nf) == (vc[0], fc[0]) and nv == vcounts[0] == 64 * 64 and vbody == vrecs[0] and fbody == frecs[0]
