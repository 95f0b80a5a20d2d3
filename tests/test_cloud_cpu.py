"""Point clouds without a GPU: the numpy statement of include/rdm_cloud.h (tests/cloud_ref.py) on surfaces whose normals are known, the PLY
writer, the intrinsics of a view, the rules of the command-line flags, and the C-ABI boundary of include/rdm_cloud.h (declared == bound ==
exported, not in rdm_hip.h; every bad argument a status code with a message, before any device call)."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

import cloud_ref as cref
from conftest import ROOT
from md_rdm_amd import filler

INTR = (500.0, 510.0, 3.25, 2.5)
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]


# ---- the numpy statement of the contract ----------------------------------------------------------------------------------------------------
def test_fronto_parallel_plane_faces_the_camera_everywhere():
    d = np.full((5, 7), 2.0, dtype=np.float32)
    arr = cref.sample_arrays(d, INTR, normals=True)
    assert arr["xyz"].shape == (35, 3) and (arr["xyz"][:, 2] == 2.0).all()
    assert (arr["normals64"] == np.array([0.0, 0.0, -1.0])).all()                     # edges and corners included: one-sided differences
    assert (arr["normals"] == np.array([0.0, 0.0, -1.0], dtype=np.float32)).all()
    np.testing.assert_array_equal(arr["xyz"][:, 0].reshape(5, 7), (((np.arange(7.0) - 3.25) * 2.0) / 500.0).astype(np.float32)[None, :].repeat(5, 0))


def test_tilted_plane_gives_its_analytic_normal():
    """Z = 1 + 0.01 X (X the camera's x axis): the pixel (y, x) sees it at Z = 1 / (1 - 0.01 (x - cx) / fx), and its normal facing the camera is
    (0.01, 0, -1) / |.|.  Differences of points ON a plane lie in it, so the reference's float64 normal of the float64 points is the analytic one
    up to the points' own rounding: 1.1e-16 * |P| against a baseline of 2 / fx = 4e-3, 3e-14 per component and a few of them: 1e-12.  (A float32
    depth puts every point 6e-8 off the plane, which is why this goes through normals_of and not through a float32 frame.)"""
    fx, fy, cx, cy = INTR
    h, w = 9, 11
    xs, ys = np.arange(w, dtype=np.float64)[None, :].repeat(h, 0), np.arange(h, dtype=np.float64)[:, None].repeat(w, 1)
    Z = 1.0 / (1.0 - 0.01 * (xs - cx) / fx)
    P = np.stack([((xs - cx) * Z) / fx, ((ys - cy) * Z) / fy, Z], axis=-1)
    n = cref.normals_of(P, np.ones((h, w), dtype=bool))
    want = np.array([0.01, 0.0, -1.0]) / math.sqrt(1.0 + 1e-4)
    assert np.abs(n - want).max() <= 1e-12, np.abs(n - want).max()
    holes = np.ones((h, w), dtype=bool)                                               # one-sided differences next to holes stay in the plane too
    holes[::3, 2::3] = False                                                         # every valid pixel keeps a neighbour on each axis
    n = cref.normals_of(P, holes)
    assert np.abs(n[holes] - want).max() <= 1e-12


def test_lonely_pixel_has_no_normal():
    d = np.zeros((3, 3), dtype=np.float32)
    d[1, 1] = 1.5
    recs, counts = cref.reference(d[None], INTR, normals=True)
    assert counts.tolist() == [1] and len(recs[0]) == 24
    x, y, z, nx, ny, nz = struct.unpack("<6f", recs[0])
    assert (nx, ny, nz) == (0.0, 0.0, 0.0) and z == 1.5
    assert x == np.float32(((1.0 - 3.25) * 1.5) / 500.0) and y == np.float32(((1.0 - 2.5) * 1.5) / 510.0)
    d[1, 2] = 1.5                                                                     # a horizontal neighbour alone is not enough
    assert struct.unpack("<6f", cref.reference(d[None], INTR, normals=True)[0][0][:24])[3:] == (0.0, 0.0, 0.0)


def test_reference_validity_step_and_order():
    d = np.array([[1.0, 0.0, -1.0, np.nan, 2.0], [np.inf, -np.inf, 3.0, 0.5, 4.0], [5.0, 1.0, 1.0, 1.0, 6.0]], dtype=np.float32)
    recs, counts = cref.reference(d[None], INTR, min_depth=1.0, max_depth=5.0)
    z = np.frombuffer(recs[0], dtype="<f4").reshape(-1, 3)[:, 2]
    assert counts.tolist() == [8] and z.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 1.0, 1.0, 1.0]      # both bounds included, row-major
    recs, counts = cref.reference(d[None], INTR, step=2)
    assert np.frombuffer(recs[0], dtype="<f4").reshape(-1, 3)[:, 2].tolist() == [1.0, 2.0, 5.0, 1.0, 6.0]
    # 15 pixels in 4 runs: [0, 3), [3, 7), [7, 11), [11, 15) hold 1, 1, 4, 4 valid ones
    assert cref.run_starts(cref.valid_mask(d), 4).tolist() == [0, 1, 2, 6, 10] and cref.run_starts(cref.valid_mask(d), 99).size == 16


# ---- write_ply ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals,colour", LAYOUTS)
def test_write_ply_header_and_payload(tmp_path, normals, colour):
    from md_rdm_amd import cloud
    rec = cloud.record_bytes(normals, colour)
    assert rec == cref.record_bytes(normals, colour) == {(False, False): 12, (False, True): 15, (True, False): 24, (True, True): 27}[(normals, colour)]
    d = filler.uniform("cloud.cpu.depth", (4, 6), 0.5, 3.0).astype(np.float32)
    d[1, 2] = 0.0
    rgb = (filler.unit("cloud.cpu.rgb", 4 * 6 * 3) * 256.0).astype(np.uint8).reshape(4, 6, 3)
    arr = cref.sample_arrays(d, INTR, rgb if colour else None, normals)
    payload, n = cref.pack(arr), 23
    assert len(payload) == n * rec
    row = np.frombuffer(payload + b"\xEE" * 40, dtype=np.uint8)                       # a region longer than its used prefix
    for k, src in enumerate((row, torch.from_numpy(row.copy()), payload + b"\xEE" * 40)):
        p = str(tmp_path / ("c%d.ply" % k))
        cloud.write_ply(p, src, n, normals, colour)
        data = open(p, "rb").read()
        head, _, body = data.partition(b"end_header\n")
        lines = head.decode("ascii").split("\n")
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 23"] and lines[-1] == ""
        props = ["property float x", "property float y", "property float z"] + (["property float nx", "property float ny", "property float nz"] if normals else []) + (
            ["property uchar red", "property uchar green", "property uchar blue"] if colour else [])
        assert lines[3:-1] == props
        assert body == payload
        fmt = "<" + "f" * (6 if normals else 3) + ("BBB" if colour else "")
        assert struct.calcsize(fmt) == rec
        for i, v in enumerate(struct.iter_unpack(fmt, body)):
            assert v[:3] == tuple(arr["xyz"][i].tolist())
            if normals:
                assert v[3:6] == tuple(arr["normals"][i].tolist())
            if colour:
                assert v[-3:] == tuple(arr["rgb"][i].tolist())
    cloud.write_ply(str(tmp_path / "empty.ply"), row, 0, normals, colour)
    assert open(str(tmp_path / "empty.ply"), "rb").read().endswith(b"element vertex 0\n" + b"".join(l.encode() + b"\n" for l in props) + b"end_header\n")
    with pytest.raises(ValueError):
        cloud.write_ply(str(tmp_path / "short.ply"), payload, n + 1, normals, colour)
    assert not os.path.exists(str(tmp_path / "short.ply"))


# ---- intrinsics ----------------------------------------------------------------------------------------------------------------------------------
def test_intrinsics_in_view():
    from md_rdm_amd import _lib, cloud
    from md_rdm_amd.dataloaders import nyu
    raw = cloud.INTRINSICS["nyu"]
    assert cloud.intrinsics_params("nyu") == raw and cloud.intrinsics_params([1, 2, 3, 4]) == (1.0, 2.0, 3.0, 4.0)
    np.testing.assert_allclose(cloud.intrinsics_in_view(raw, (0, 0, 480, 640), (480, 640)), raw, rtol=0, atol=1e-12)      # the full view: the identity
    view = nyu.test_view((480, 640))                                                  # (9.6, 12.49.., 460.8, 615.01..): fractional
    for hw in ((128, 128), (480, 640), (226, 226)):
        fx, fy, cx, cy = cloud.intrinsics_in_view(raw, view, hw)
        assert abs(fx - raw[0] * hw[1] / view[3]) <= 1e-12 * fx and abs(fy - raw[1] * hw[0] / view[2]) <= 1e-12 * fy
        # the principal point is where the raw frame's is: a raw centre coordinate u is at (u + 0.5 - vx0) * W / vw - 0.5 of the view's frame
        assert abs(cx - ((raw[2] + 0.5 - view[1]) * hw[1] / view[3] - 0.5)) <= 1e-12 and abs(cy - ((raw[3] + 0.5 - view[0]) * hw[0] / view[2] - 0.5)) <= 1e-12
        for X, Y, Z in ((0.3, -0.2, 1.7), (-1.0, 0.4, 3.0)):                         # and every point projects to the mapped pixel of its raw pixel
            u, v = raw[0] * X / Z + raw[2], raw[1] * Y / Z + raw[3]
            assert abs((fx * X / Z + cx) - ((u + 0.5 - view[1]) * hw[1] / view[3] - 0.5)) <= 1e-9
            assert abs((fy * Y / Z + cy) - ((v + 0.5 - view[0]) * hw[0] / view[2] - 0.5)) <= 1e-9
    for bad in (lambda: cloud.intrinsics_params("kinect"), lambda: cloud.intrinsics_params((1, 2, 3)), lambda: cloud.intrinsics_in_view(raw, (0, 0, 0, 5), (4, 4))):
        with pytest.raises(_lib.RdmError):
            bad()


def test_host_tensors_are_refused():
    from md_rdm_amd import _lib, cloud
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        cloud.point_cloud(torch.ones(1, 4, 4), INTR)
    with pytest.raises(_lib.RdmError):
        cloud.point_cloud(np.ones((1, 4, 4), np.float32), INTR)


# ---- the command's rules: refused before anything touches a GPU ---------------------------------------------------------------------------
def test_predict_ply_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.ply, a.ply_normals, a.ply_step, a.camera, a.intrinsics, a.min_depth, a.max_depth) == (False, False, None, None, None, None, None)
    predict.check_ply_args(a)
    a = P.parse_args(["--out", "d", "f.npy", "--metric", "--ply", "--ply_normals", "--ply_step", "2", "--intrinsics", "500", "501", "320", "240", "--min_depth", "0.5",
                      "--max_depth", "8"])
    assert (a.ply, a.ply_normals, a.ply_step, a.intrinsics, a.min_depth, a.max_depth) == (True, True, 2, [500.0, 501.0, 320.0, 240.0], 0.5, 8.0)
    predict.check_ply_args(a)
    predict.check_ply_args(P.parse_args(["--out", "d", "--synthetic", "2", "--metric", "--ply", "--camera", "nyu"]))
    files, syn = ["--out", "d", "f.npy"], ["--out", "d", "--synthetic", "2"]
    for argv, word in ((files + ["--ply"], "--ply needs --metric"), (syn + ["--ply", "--ply_normals"], "--ply needs --metric"), (files + ["--metric", "--ply_normals"], "need --ply"),
                       (files + ["--metric", "--ply_step", "2"], "need --ply"), (files + ["--metric", "--camera", "nyu"], "need --ply"),
                       (files + ["--metric", "--intrinsics", "1", "1", "0", "0"], "need --ply"), (files + ["--metric", "--min_depth", "1"], "need --ply"),
                       (files + ["--metric", "--max_depth", "1"], "need --ply"), (files + ["--metric", "--ply", "--camera", "nyu", "--intrinsics", "1", "1", "0", "0"], "not both"),
                       (files + ["--metric", "--ply", "--camera", "kinect"], "--camera kinect"), (files + ["--metric", "--ply", "--intrinsics", "0", "1", "0", "0"], "--intrinsics"),
                       (files + ["--metric", "--ply", "--intrinsics", "1", "nan", "0", "0"], "--intrinsics"), (files + ["--metric", "--ply", "--ply_step", "0"], "--ply_step"),
                       (files + ["--metric", "--ply", "--min_depth", "-1"], "--min_depth"), (files + ["--metric", "--ply", "--min_depth", "nan"], "--min_depth"),
                       (files + ["--metric", "--ply", "--min_depth", "2", "--max_depth", "1"], "--max_depth"), (files + ["--metric", "--ply", "--max_depth", "nan"], "--max_depth")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    text = P.format_help()
    for flag in ("--ply", "--ply_normals", "--ply_step N", "--camera NAME", "--intrinsics FX FY CX CY", "--min_depth M", "--max_depth M"):
        assert flag in text, flag


# ---- the C ABI of include/rdm_cloud.h -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_cloud.h")) == {"rdm_depth_cloud"}       # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_depth_cloud" not in hip_h and "rdm_cloud.h" not in hip_h


def test_bad_arguments_are_status_codes_before_any_device_call(L):
    """Host or made-up pointers only: every refusal comes from the launcher's own checks, which precede the launch (this machine has no device to
    call)."""
    D4 = C.c_double * 4
    nan, inf = float("nan"), float("inf")
    P = C.c_void_p(256)
    # positions: 0 depth, 1 rgb, 2 batch, 3 h, 4 w, 5 intr, 6 min_depth, 7 max_depth, 8 step, 9 normals, 10 records, 11 sample_stride_bytes, 12 count, 13 split, 14 stream
    good = [P, None, 1, 4, 6, D4(*INTR), 0.0, inf, 1, 0, P, 4 * 6 * 12, P, 0, None]
    bad = [({0: None}, b"depth"), ({5: None}, b"intr"), ({10: None}, b"records"), ({12: None}, b"count"), ({2: 0}, b"batch"), ({2: -1}, b"batch"), ({3: 0}, b"h"), ({4: -2}, b"w"),
           ({8: 0}, b"step"), ({8: -1}, b"step"), ({2: 65536}, b"65535"), ({3: 65536, 4: 32768, 11: 2 ** 31 - 1}, b"h * w"),
           ({11: 4 * 6 * 12 - 1}, b"sample_stride_bytes"), ({1: P}, b"sample_stride_bytes"), ({9: 1}, b"sample_stride_bytes"), ({1: P, 9: 1, 11: 4 * 6 * 27 - 1}, b"sample_stride_bytes"),
           ({8: 2, 11: 2 * 3 * 12 - 1}, b"sample_stride_bytes"), ({8: 4, 11: 1 * 2 * 12 - 1}, b"sample_stride_bytes"), ({11: 2 ** 31}, b"sample_stride_bytes"), ({11: -1}, b"sample_stride_bytes"),
           ({5: D4(nan, 510, 3, 2)}, b"intr"), ({5: D4(500, inf, 3, 2)}, b"intr"), ({5: D4(500, 510, nan, 2)}, b"intr"), ({5: D4(500, 510, 3, -inf)}, b"intr"),
           ({5: D4(0, 510, 3, 2)}, b"fx"), ({5: D4(500, 0.0, 3, 2)}, b"fy"), ({6: -1e-9}, b"min_depth"), ({6: nan}, b"min_depth"), ({7: nan}, b"max_depth"),
           ({6: 2.0, 7: 1.0}, b"max_depth"), ({6: inf, 7: 1.0}, b"max_depth"), ({9: 2}, b"normals"), ({9: -1}, b"normals"), ({13: -1}, b"split")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_depth_cloud(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
