"""Triangle meshes without a GPU: the numpy statement of include/rdm_mesh.h (tests/mesh_ref.py) on frames whose faces are known by hand, the PLY
writer, the rules of the command-line flags, the host-tensor refusals, and the C-ABI boundary of include/rdm_mesh.h (declared == bound ==
exported, not in rdm_hip.h or any other table; every bad argument a status code with a message, before any device call)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import cloud_ref as cref
import mesh_ref as mref
from conftest import ROOT
from md_rdm_amd import filler

HEADER = os.path.join(ROOT, "include", "rdm_mesh.h")
INTR = (500.0, 510.0, 3.25, 2.5)
INF = math.inf


def F(depth, **kw):
    """the faces of one frame as a list of index triples; the loop statement and the vectorised one must agree on every frame a test uses"""
    d = np.asarray(depth, dtype=np.float32)
    s = mref.sample_faces(d, **kw)
    np.testing.assert_array_equal(s["faces"], mref.loops(d, **kw))
    return s["faces"].tolist()


# ---- the numpy statement of the contract ----------------------------------------------------------------------------------------------------
def test_constant_plane_uses_the_ad_diagonal_everywhere():
    # 2x3: vertices 0 1 2 / 3 4 5; cell 0: A0 B1 C3 D4, cell 1: A1 B2 C4 D5; the tie goes to AD: (A, C, D), (A, D, B)
    assert F(np.full((2, 3), 2.0)) == [[0, 3, 4], [0, 4, 1], [1, 4, 5], [1, 5, 2]]
    for sh, sw in ((2, 2), (3, 5), (7, 4)):
        s = mref.sample_faces(np.full((sh, sw), 1.25, np.float32))
        assert len(s["faces"]) == 2 * (sh - 1) * (sw - 1) and s["ad"].all() and s["vertex_count"] == sh * sw and not s["cut"].any()
        assert s["cell"].tolist() == np.repeat(np.arange((sh - 1) * (sw - 1)), 2).tolist() and s["cand"].tolist() == [0, 1] * ((sh - 1) * (sw - 1))


@pytest.mark.parametrize("hole,want", [("A", [0, 1, 2]), ("B", [0, 1, 2]), ("C", [0, 2, 1]), ("D", [0, 2, 1])])
def test_one_invalid_corner_leaves_the_triangle_of_the_other_three(hole, want):
    """A B / C D with one hole: the remaining vertices are numbered 0 1 2 in row-major order.  A missing: (B, C, D) = 0 1 2; B missing: (A, C, D) =
    0 1 2; C missing: (A, D, B) = 0 2 1; D missing: (A, C, B) = 0 2 1."""
    for bad in (0.0, np.nan, -1.0, np.inf):
        d = np.full((2, 2), 3.0, np.float32)
        d["ABCD".index(hole) // 2, "ABCD".index(hole) % 2] = bad
        assert F(d, edge_ratio=1.0) == [want]
    d = np.full((2, 2), 3.0, np.float32)
    d["ABCD".index(hole) // 2, "ABCD".index(hole) % 2] = 9.0        # out of range is invalid too
    assert F(d, max_depth=5.0) == [want]
    d["ABCD".index(hole) // 2, "ABCD".index(hole) % 2] = 0.5
    assert F(d, min_depth=1.0) == [want]


def test_two_invalid_corners_and_checkerboard_give_vertices_without_faces():
    assert F([[1, 0], [0, 1]]) == [] and F([[0, 1], [1, 0]]) == [] and F([[1, 1], [0, 0]]) == [] and F([[0, 0], [0, 0]]) == []
    yy, xx = np.mgrid[0:6, 0:9]
    d = np.where((yy + xx) % 2 == 0, 2.0, 0.0).astype(np.float32)
    s = mref.sample_faces(d)
    assert s["vertex_count"] == 27 and len(s["faces"]) == 0 and F(d) == []


def test_edge_test_boundaries():
    d = np.array([[1.0, 1.5], [1.0, 1.5]], np.float32)               # a step 1.0 | 1.5, exactly representable; |dA - dD| = |dB - dC|: AD
    full = [[0, 2, 3], [0, 3, 1]]
    assert F(d, edge_ratio=1.5) == full                              # hi == lo * ratio passes
    assert F(d, edge_ratio=float(np.nextafter(1.5, 1.0))) == []      # one float64 step below: both triangles span the step
    assert F(d, edge_ratio=float(np.nextafter(1.5, 2.0))) == full and F(d, edge_ratio=INF) == full and F(d, edge_ratio=1.0) == []
    d = np.array([[1.0, 1.0, 1.5], [1.0, 1.0, 1.5]], np.float32)     # the flat cell stays, the cell across the step goes
    assert F(d, edge_ratio=1.25) == [[0, 3, 4], [0, 4, 1]]
    s = mref.sample_faces(d, edge_ratio=1.25)
    assert s["cut"].tolist() == [[[False, False], [True, True]]]
    # float32 depths that are not round numbers: lo = 1 + 2^-22, hi = 1.5 * lo exactly (3 * 2^-23 is a float32 step count); equality passes, hi one
    # float32 step up does not
    lo = np.float32(1.0 + 2.0 ** -22)
    hi = np.float32(1.5) * lo
    assert float(hi) == 1.5 * float(lo)
    assert F([[lo, hi], [lo, hi]], edge_ratio=1.5) == full and F([[lo, np.nextafter(hi, np.float32(9))], [lo, hi]], edge_ratio=1.5) == [[0, 2, 3]]


def test_diagonal_follows_the_smaller_depth_difference():
    d = np.array([[1.0, 2.0, 1.0], [2.0, 1.0, 2.0]], np.float32)     # both cells: |dA - dD| = 0 = |dB - dC|: the tie goes to AD
    s = mref.sample_faces(d, edge_ratio=INF)
    assert s["ad"].tolist() == [[True, True]]
    d = np.array([[1.0, 2.0, 1.0], [2.0, 1.1, 2.0]], np.float32)     # cell 0: |1 - 1.1| > |2 - 2| -> BC; cell 1: |2 - 2| <= |1 - 1.1| -> AD
    s = mref.sample_faces(d, edge_ratio=INF)
    assert s["ad"].tolist() == [[False, True]]
    # vertices 0 1 2 / 3 4 5; cell 0 (BC): (A, C, B) = (0, 3, 1), (B, C, D) = (1, 3, 4); cell 1 (AD): (A, C, D) = (1, 4, 5), (A, D, B) = (1, 5, 2)
    assert F(d, edge_ratio=INF) == [[0, 3, 1], [1, 3, 4], [1, 4, 5], [1, 5, 2]]
    # with a tight ratio the BC cell keeps nothing (every triangle holds a 1 and a 2), and the AD cell neither
    assert F(d, edge_ratio=1.5) == []
    d = np.array([[1.0, 1.0], [1.0, 3.0]], np.float32)               # |dA - dD| = 2 > |dB - dC| = 0 -> BC: the flat triangle survives a ratio the other does not
    assert F(d, edge_ratio=2.0) == [[0, 2, 1]] and mref.sample_faces(d, edge_ratio=2.0)["cut"].tolist() == [[[False, True]]]


def test_every_triangle_faces_the_camera():
    """x right, y down, z forward, positive fx and fy: a triangle whose cross(p1 - p0, p2 - p0) points at the camera projects to pixel coordinates
    with a NEGATIVE z component of (q1 - q0) x (q2 - q0) (x right, y down), and so does every emitted face of a frame with both diagonals and holes;
    the 3-D normal's dot product with the view ray is negative as well."""
    d = filler.uniform("mesh.cpu.winding", (9, 13), 1.0, 4.0).astype(np.float32)
    d[filler.unit("mesh.cpu.winding.mask", 9 * 13).reshape(9, 13) < 0.2] = 0.0
    s = mref.sample_faces(d, edge_ratio=INF)
    assert s["ad"].any() and (~s["ad"]).any() and len(s["faces"]) > 40
    arr = cref.sample_arrays(d, INTR)
    P = arr["xyz"].astype(np.float64)
    ys, xs = np.nonzero(s["valid"])
    q = np.stack([xs, ys], axis=1).astype(np.float64)                # vertex index -> pixel
    t = s["faces"]
    e1, e2 = q[t[:, 1]] - q[t[:, 0]], q[t[:, 2]] - q[t[:, 0]]
    area = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    assert (area == -1.0).all()                                      # half a pixel cell each, one sign
    n = np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]])
    assert ((n * P[t[:, 0]]).sum(1) < 0).all()


def test_degenerate_grids_have_no_faces():
    for shape in ((1, 7), (7, 1), (1, 1)):
        s = mref.sample_faces(np.full(shape, 2.0, np.float32))
        assert len(s["faces"]) == 0 and s["vertex_count"] == shape[0] * shape[1]
    assert F(np.full((3, 5), 2.0), step=3) == [] and F(np.full((5, 3), 2.0), step=4) == []      # one sampled row / column through the step
    recs, fc, vc = mref.reference(np.full((2, 1, 4), 2.0, np.float32), layout="ply")
    assert recs == [b"", b""] and fc.tolist() == [0, 0] and vc.tolist() == [4, 4]


def test_step_three_indices_point_at_the_cloud_records():
    d = filler.uniform("mesh.cpu.step", (20, 31), 1.0, 1.3).astype(np.float32)
    d[filler.unit("mesh.cpu.step.mask", 20 * 31).reshape(20, 31) < 0.15] = 0.0
    s = mref.sample_faces(d, step=3, edge_ratio=1.2)
    assert s["valid"].shape == (7, 11) and 0 < len(s["faces"]) < 2 * 6 * 10
    np.testing.assert_array_equal(s["faces"], mref.loops(d, step=3, edge_ratio=1.2))
    arr = cref.sample_arrays(d, INTR, step=3)
    assert s["vertex_count"] == len(arr["xyz"]) == int(cref.reference(d[None], INTR, step=3)[1][0])
    pts = cref.points(d, INTR)
    for (cell, cand), tri in zip(zip(s["cell"].tolist(), s["cand"].tolist()), s["faces"].tolist()):
        i, j = divmod(cell, 10)
        A, B, Cc, D = (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
        corners = (((A, Cc, D), (A, D, B)) if s["ad"][i, j] else ((A, Cc, B), (B, Cc, D)))[cand]
        for v, (ri, rj) in zip(tri, corners):                        # the record at the index is the record of the corner's pixel
            np.testing.assert_array_equal(arr["xyz"][v], pts[ri * 3, rj * 3].astype(np.float32))
            assert arr["xyz"][v][2] == d[ri * 3, rj * 3]


def test_layouts_and_pack_round_trip():
    tri = np.array([[0, 1, 2], [70000, 3, 2 ** 31 - 1]], np.int32)
    assert mref.pack(tri, "i32") == tri.astype("<i4").tobytes() and len(mref.pack(tri, "ply")) == 26
    assert mref.pack(tri, "ply")[:13] == b"\x03" + tri[0].astype("<i4").tobytes() and mref.pack(tri, "ply")[13:14] == b"\x03"
    for layout in ("i32", "ply"):
        np.testing.assert_array_equal(mref.unpack(mref.pack(tri, layout), layout), tri)


# ---- write_ply -------------------------------------------------------------------------------------------------------------------------------
def parse_ply(data):
    """-> (vcount, fcount, vertex property lines, vertex payload, face payload); asserts the header's shape"""
    head, sep, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert sep and lines[:2] == ["ply", "format binary_little_endian 1.0"] and lines[-1] == ""
    assert lines[2].startswith("element vertex ") and lines[-3].startswith("element face ") and lines[-2] == "property list uchar int vertex_indices"
    vcount, fcount, props = int(lines[2].split()[2]), int(lines[-3].split()[2]), lines[3:-3]
    rec = sum(4 if p.startswith("property float ") else 1 for p in props)
    assert all(p.startswith("property float ") or p.startswith("property uchar ") for p in props)
    assert len(body) == vcount * rec + fcount * 13
    return vcount, fcount, props, body[:vcount * rec], body[vcount * rec:]


@pytest.mark.parametrize("normals,colour", [(False, False), (False, True), (True, False), (True, True)])
def test_write_ply_round_trip(tmp_path, normals, colour):
    from md_rdm_amd import cloud, mesh
    assert mesh.face_bytes("i32") == mref.face_bytes("i32") == 12 and mesh.face_bytes("ply") == mref.face_bytes("ply") == 13
    d = filler.uniform("mesh.cpu.ply", (4, 6), 1.0, 1.04).astype(np.float32)
    d[1, 2] = 0.0
    rgb = (filler.unit("mesh.cpu.rgb", 4 * 6 * 3) * 256.0).astype(np.uint8).reshape(4, 6, 3)
    vertices = cref.pack(cref.sample_arrays(d, INTR, rgb if colour else None, normals))
    s = mref.sample_faces(d)
    tri, nv, nf = mref.pack(s["faces"], "ply"), 23, len(s["faces"])
    assert nf == 2 * 15 - 4 and s["vertex_count"] == nv                # each of the four cells around the hole keeps the one triangle of its other corners
    assert mesh.ply_header(nv, nf, normals, colour) == cloud.ply_header(nv, normals, colour)[:-len(b"end_header\n")] + (
        b"element face %d\nproperty list uchar int vertex_indices\nend_header\n" % nf)
    vrow, frow = np.frombuffer(vertices + b"\xEE" * 40, np.uint8), np.frombuffer(tri + b"\xDD" * 29, np.uint8)        # regions longer than their used prefixes
    for k, (vs, fs) in enumerate(((vrow, frow), (torch.from_numpy(vrow.copy()), torch.from_numpy(frow.copy())), (vertices + b"\xEE", tri + b"\xDD"))):
        p = str(tmp_path / ("m%d.ply" % k))
        mesh.write_ply(p, vs, nv, normals, colour, fs, nf)
        gv, gf, props, vbody, fbody = parse_ply(open(p, "rb").read())
        assert (gv, gf) == (nv, nf) and vbody == vertices and fbody == tri
        assert len(vbody) == nv * cloud.record_bytes(normals, colour) and ("property float nx" in props) == normals and ("property uchar red" in props) == colour
        np.testing.assert_array_equal(mref.unpack(fbody, "ply"), s["faces"])
        assert mref.unpack(fbody, "ply").max() < nv
    mesh.write_ply(str(tmp_path / "empty.ply"), vrow, nv, normals, colour, b"", 0)
    assert parse_ply(open(str(tmp_path / "empty.ply"), "rb").read())[:2] == (nv, 0)
    for bad in (lambda p: mesh.write_ply(p, vertices, nv + 1, normals, colour, tri, nf), lambda p: mesh.write_ply(p, vertices, nv, normals, colour, tri, nf + 1),
                lambda p: mesh.write_ply(p, vertices, nv, normals, colour, torch.zeros(2, 13, dtype=torch.uint8), 1)):
        with pytest.raises(ValueError):
            bad(str(tmp_path / "short.ply"))
        assert not os.path.exists(str(tmp_path / "short.ply"))


def test_host_tensors_are_refused():
    from md_rdm_amd import _lib, mesh
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        mesh.faces(torch.ones(1, 4, 4))
    with pytest.raises(_lib.RdmError):
        mesh.faces(np.ones((1, 4, 4), np.float32))
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        mesh.depth_mesh(torch.ones(1, 4, 4), INTR)
    with pytest.raises(_lib.RdmError):
        mesh.face_bytes("obj")


# ---- the command's rules: refused before anything touches a GPU ---------------------------------------------------------------------------
def test_predict_mesh_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.mesh, a.mesh_edge_ratio) == (False, None)
    predict.check_mesh_args(a)
    a = P.parse_args(["--out", "d", "f.npy", "--metric", "--ply", "--ply_step", "2", "--mesh", "--mesh_edge_ratio", "1.1"])
    assert (a.mesh, a.mesh_edge_ratio, a.ply_step) == (True, 1.1, 2)
    predict.check_ply_args(a)
    predict.check_mesh_args(a)
    predict.check_mesh_args(P.parse_args(["--out", "d", "--synthetic", "2", "--metric", "--ply", "--mesh", "--mesh_edge_ratio", "inf"]))
    predict.check_mesh_args(P.parse_args(["--out", "d", "--synthetic", "2", "--metric", "--ply", "--mesh", "--mesh_edge_ratio", "1"]))
    files = ["--out", "d", "f.npy"]
    for argv, word in ((files + ["--mesh"], "--mesh needs --ply"), (files + ["--metric", "--mesh"], "--mesh needs --ply"), (files + ["--mesh", "--ply"], "--ply needs --metric"),
                       (files + ["--metric", "--ply", "--mesh_edge_ratio", "1.1"], "--mesh_edge_ratio needs --mesh"), (files + ["--mesh_edge_ratio", "2"], "--mesh_edge_ratio needs --mesh"),
                       (files + ["--metric", "--ply", "--mesh", "--mesh_edge_ratio", "0.99"], "--mesh_edge_ratio must be >= 1"),
                       (files + ["--metric", "--ply", "--mesh", "--mesh_edge_ratio", "nan"], "--mesh_edge_ratio must be >= 1"),
                       (files + ["--metric", "--ply", "--mesh", "--mesh_edge_ratio=-inf"], "--mesh_edge_ratio must be >= 1")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    text = P.format_help()
    for flag in ("--mesh", "--mesh_edge_ratio R"):
        assert flag in text, flag
    assert "--mesh" in predict.__doc__ and "--mesh_edge_ratio" in predict.__doc__ and "not been measured" in predict.__doc__


# ---- the C ABI of include/rdm_mesh.h ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


NAMES = {"rdm_depth_mesh", "rdm_depth_mesh_workspace_bytes"}


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    assert set(_lib.symbols("rdm_mesh.h")) == NAMES        # declared == bound == exported, with the header's types: test_abi_cpu.py
    assert re.search(r"#define\s+RDM_MESH_FACES_I32\s+0\b", text) and re.search(r"#define\s+RDM_MESH_FACES_PLY\s+1\b", text) and _lib.MESH_FACES == {"i32": 0, "ply": 1}
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_depth_mesh" not in hip_h and "rdm_mesh.h" not in hip_h
    assert "rdm_depth_mesh" not in open(os.path.join(ROOT, "include", "rdm_cloud.h")).read()
    assert "mesh.hip" in __import__("md_rdm_amd.build", fromlist=["sources"]).sources()


def test_workspace_bytes(L):
    ws = L.rdm_depth_mesh_workspace_bytes
    assert ws(1, 4, 6, 1) > 0 and ws(8, 480, 640, 1) >= ws(1, 480, 640, 1) > 0 and ws(3, 1, 1, 1) >= 0
    assert ws(8, 480, 640, 1) <= 8 * 480 * 640                        # tables per row, not a plane
    for bad in ((0, 4, 6, 1), (-1, 4, 6, 1), (1, 0, 6, 1), (1, 4, -6, 1), (1, 4, 6, 0), (65536, 4, 6, 1), (1, 65536, 32768, 1)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_are_status_codes_before_any_device_call(L):
    """Made-up pointers only: every refusal comes from the launcher's own checks, which precede the launches (this machine has no device to call)."""
    nan, inf = float("nan"), float("inf")
    P = C.c_void_p(256)
    need = L.rdm_depth_mesh_workspace_bytes(1, 4, 6, 1)
    assert need > 0
    # positions: 0 depth, 1 batch, 2 h, 3 w, 4 min_depth, 5 max_depth, 6 step, 7 edge_ratio, 8 layout, 9 faces, 10 sample_stride_bytes, 11 face_count, 12 vertex_count,
    # 13 workspace, 14 workspace_bytes, 15 stream
    good = [P, 1, 4, 6, 0.0, inf, 1, 1.05, 0, P, 2 * 3 * 5 * 12, P, None, P, need, None]
    bad = [({0: None}, b"depth"), ({9: None}, b"faces"), ({11: None}, b"face_count"), ({1: 0}, b"batch"), ({1: -1}, b"batch"), ({2: 0}, b"h"), ({3: -2}, b"w"),
           ({6: 0}, b"step"), ({6: -1}, b"step"), ({1: 65536}, b"65535"), ({2: 65536, 3: 32768, 10: 2 ** 31 - 1}, b"h * w"),
           ({4: -1e-9}, b"min_depth"), ({4: nan}, b"min_depth"), ({5: nan}, b"max_depth"), ({4: 2.0, 5: 1.0}, b"max_depth"), ({4: inf, 5: 1.0}, b"max_depth"),
           ({7: nan}, b"edge_ratio"), ({7: 0.999}, b"edge_ratio"), ({7: -inf}, b"edge_ratio"), ({7: 0.0}, b"edge_ratio"),
           ({8: 2}, b"layout"), ({8: -1}, b"layout"),
           ({10: 2 * 3 * 5 * 12 - 1}, b"sample_stride_bytes"), ({8: 1}, b"sample_stride_bytes"), ({8: 1, 10: 2 * 3 * 5 * 13 - 1}, b"sample_stride_bytes"),
           ({6: 2, 10: 2 * 1 * 2 * 12 - 1}, b"sample_stride_bytes"), ({10: 2 ** 31}, b"sample_stride_bytes"), ({10: -1}, b"sample_stride_bytes"),
           ({14: need - 1}, b"workspace_bytes"), ({14: 0}, b"workspace_bytes"), ({14: -5}, b"workspace_bytes"), ({13: None}, b"workspace")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_depth_mesh(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
