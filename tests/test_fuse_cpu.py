"""Depth fusion without a GPU: the numpy statement of include/rdm_fuse.h (tests/fuse_ref.py) on scenes whose surface is known by hand - so that the
STATEMENT is checked, not merely reproduced -, the pose and bounds helpers, the wrapper's refusals, the rules of the command-line flags, and the C-ABI
boundary of include/rdm_fuse.h (declared == bound == exported; every bad argument a status code with a message, before any device call)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import fuse_ref as fref
from conftest import ROOT

IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
INF = math.inf


def fresh(dims, colour=True):
    nx, ny, nz = dims
    return np.ones((nz, ny, nx), np.float32), np.zeros((nz, ny, nx), np.float32), np.zeros((nz, ny, nx, 3), np.float32) if colour else None


# ---- the statement of the contract ---------------------------------------------------------------------------------------------------------
def test_a_constant_depth_plane_is_recovered_exactly():
    """d = 2 everywhere, identity pose, voxel 0.25, trunc 0.5, every Pz a multiple of 0.25.  sdf = 2 - Pz is then exactly linear in Pz and exactly
    representable, s = sdf / 0.5 and T' = (0 * 1 + 1 * s) / 1 are exact, so the interpolated crossing is the plane up to the float32 rounding of T
    and of the coordinate: |z - 2| <= 1e-5, and the normal, a difference of exact values normalised, within 1e-6 of (0, 0, -1).  Derived, not measured."""
    h, w, intr = 24, 32, (20.0, 20.0, 15.5, 11.5)
    dims, geom = (9, 9, 9), (-1.0, -1.0, 1.0, 0.25, 0.5)
    depth = np.full((1, h, w), 2.0, np.float32)
    rgb = np.full((1, h, w, 3), (10, 120, 250), np.uint8)
    T, W, Cc = fref.integrate(depth, rgb, intr, IDENT, dims, geom, *fresh(dims))
    # by hand: the column of voxels through the optical axis (i = j = 4: Px = Py = 0) sees d = 2 at every Pz
    assert T[:, 4, 4].tolist() == [1.0, 1.0, 1.0, 0.5, 0.0, -0.5, -1.0, 1.0, 1.0]          # Pz = 1 .. 3; sdf == -trunc is kept, the next voxel is hidden
    assert W[:, 4, 4].tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert Cc[4, 4, 4].tolist() == [10.0, 120.0, 250.0] and not Cc[8].any()
    assert W[0, 4, 0] == 0 and T[0, 4, 0] == 1                                             # Pz = 1, Px = -1: u = -4.5, outside the frame
    payload, n = fref.extract(T, W, Cc, dims, geom, min_weight=1.0, normals=True)
    assert n > 20 and len(payload) == n * 27
    pos, nrm, col = fref.records_array(payload, n, True, True)
    assert np.abs(pos[:, 2] - 2.0).max() <= 1e-5
    assert np.abs(nrm - np.array([0.0, 0.0, -1.0], np.float32)).max() <= 1e-6
    assert (col == np.array([10, 120, 250], np.uint8)).all()
    # the points are the voxel centres of the plane z = 2 that the frame sees, in row-major order, each once (only z edges cross)
    assert (np.diff(np.round((pos[:, 1] + 1.0) / 0.25) * 9 + np.round((pos[:, 0] + 1.0) / 0.25)) > 0).all()
    for rec_normals, rec_colour in ((False, False), (False, True), (True, False)):
        p2, n2 = fref.extract(T, W, Cc if rec_colour else None, dims, geom, normals=rec_normals)
        assert n2 == n and fref.records_array(p2, n2, rec_normals, rec_colour)[0].tobytes() == pos.tobytes()
    assert fref.extract(T, W, Cc, dims, geom, min_weight=2.0)[1] == 0                      # nothing was seen twice


def plane_depth(h, w, intr, pose, z0=2.0):
    """the float32 depth frame of the world plane z = z0 from the camera of ``pose`` (world -> camera)"""
    fx, fy, cx, cy = intr
    R, t = pose[:, :3], pose[:, 3]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], axis=-1)
    return ((z0 + (R.T @ t)[2]) / (rays @ R)[..., 2]).astype(np.float32)               # (R^T (z r - t)).z = z0


def test_three_rotated_views_of_a_plane_agree_within_half_a_voxel():
    from md_rdm_amd import warp
    h, w, intr = 48, 64, (60.0, 60.0, 31.5, 23.5)
    dims, geom = (13, 9, 9), (-0.75, -0.5, 1.0, 0.125, 0.5)
    poses = np.stack([IDENT, warp.pose_from_rt((0.0, 0.2, 0.0), (0.4, 0.0, 0.1)), warp.pose_from_rt((0.15, -0.2, 0.0), (-0.4, 0.3, 0.1))])
    depth = np.stack([plane_depth(h, w, intr, p) for p in poses])
    assert np.isfinite(depth).all() and depth.min() > 1.0 and depth.max() < 3.5 and depth[1].std() > 0.05 and depth[0].std() == 0
    T, W, _ = fref.integrate(depth, None, intr, poses, dims, geom, *fresh(dims, colour=False))
    assert (W == 3).any() and (W == 0).any()
    payload, n = fref.extract(T, W, None, dims, geom, min_weight=1.0, normals=True)
    pos, nrm, _ = fref.records_array(payload, n, True, False)
    assert n >= 13 * 9 // 2
    assert np.abs(pos[:, 2] - 2.0).max() <= 0.125 / 2
    assert (nrm[:, 2] < -0.9).all()                                                       # toward the cameras
    # the same frames one call each: the same bytes
    planes = fresh(dims, colour=False)
    for b in range(3):
        planes = fref.integrate(depth[b:b + 1], None, intr, poses[b], dims, geom, *planes)
    assert planes[0].tobytes() == T.tobytes() and planes[1].tobytes() == W.tobytes()


def test_weight_cap_invalid_depths_and_untouched_voxels():
    dims, geom = (3, 1, 1), (0.0, 0.0, 2.0, 0.25, 0.5)
    intr = (4.0, 4.0, 0.0, 0.0)                                                           # Px = 0, 0.25, 0.5 at Pz = 2: u = 0, 0.5, 1 -> columns 0, 1, 1
    depth = np.array([[[2.25, np.nan]], [[2.25, 2.5]], [[0.0, 9.0]], [[2.25, 2.5]]], np.float32)
    T, W, _ = fref.integrate(depth, None, intr, IDENT, dims, geom, *fresh(dims, colour=False), max_depth=8.0, obs_weight=1.0, max_weight=2.0)
    assert T.reshape(-1).tolist() == [0.5, 1.0, 1.0] and W.reshape(-1).tolist() == [2.0, 2.0, 2.0]          # three, two and two frames; the cap at 2
    T2, W2, _ = fref.integrate(depth[2:3], None, intr, IDENT, dims, geom, T, W, None, max_depth=8.0)
    assert T2.tobytes() == T.tobytes() and W2.tobytes() == W.tobytes()                      # a frame without a valid depth changes nothing


# ---- the helpers ---------------------------------------------------------------------------------------------------------------------------------
def test_pose_inverse_round_trips():
    from md_rdm_amd import _lib, fuse, warp
    p = warp.pose_from_rt((0.3, -0.2, 0.5), (0.1, -0.4, 0.7))
    q = fuse.pose_inverse(p)
    assert q.dtype == np.float64 and q.shape == (3, 4)
    np.testing.assert_allclose(fuse.pose_inverse(q), p, atol=1e-15, rtol=0)
    full = np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]]) @ np.concatenate([q, [[0.0, 0.0, 0.0, 1.0]]])
    np.testing.assert_allclose(full, np.eye(4), atol=1e-15, rtol=0)
    both = fuse.pose_inverse(np.stack([p, IDENT]))
    assert both.shape == (2, 3, 4) and both[0].tobytes() == q.tobytes() and both[1].tolist() == IDENT.tolist()
    assert fuse.pose_inverse(torch.eye(4)).tolist() == IDENT.tolist()
    for bad in (np.eye(3), "abc", np.zeros((2, 2, 3, 4))):
        with pytest.raises(_lib.RdmError):
            fuse.pose_inverse(bad)


def test_bounds_hold_every_frustum_corner():
    from md_rdm_amd import _lib, fuse, warp
    h, w, intr, far, voxel = 37, 53, (61.5, 63.25, 25.75, 17.5), 3.5, 0.07
    poses = np.stack([IDENT, warp.pose_from_rt((0.2, -0.5, 0.1), (0.8, -0.3, 0.5)), warp.pose_from_rt((-0.4, 0.9, 0.3), (-1.0, 0.2, -0.2))])
    origin, dims = fuse.bounds((h, w), intr, poses, far, voxel)
    lo, hi = np.array(origin), np.array(origin) + (np.array(dims) - 1) * voxel
    n = 0
    for p in poses:                                                               # by hand: X_world = R^T (X_cam - t)
        R, t = p[:, :3], p[:, 3]
        for cam in [(0.0, 0.0, 0.0)] + [((x - intr[2]) * far / intr[0], (y - intr[3]) * far / intr[1], far) for x in (-0.5, w - 0.5) for y in (-0.5, h - 0.5)]:
            X = R.T @ (np.array(cam) - t)
            assert (X >= lo - 1e-12).all() and (X <= hi + 1e-12).all(), (cam, X, lo, hi)
            n += 1
    assert n == 15 and all(isinstance(v, int) and v > 1 for v in dims) and ((hi - lo) < (np.ptp(fuse.frustum_corners((h, w), intr, poses, far).reshape(-1, 3), axis=0) + voxel)).all()
    assert fuse.bounds((h, w), intr, IDENT, far, voxel)[0][2] == 0.0                # one (3,4) pose; the camera's centre is the near end
    for bad in (lambda: fuse.bounds((h, w), intr, poses, INF, voxel), lambda: fuse.bounds((h, w), intr, poses, far, 0.0), lambda: fuse.bounds((h, w), intr, poses, 1e6, 1e-3),
                lambda: fuse.bounds((0, w), intr, poses, far, voxel), lambda: fuse.bounds((h, w), (0.0, 1.0, 0.0, 0.0), poses, far, voxel)):
        with pytest.raises(_lib.RdmError):
            bad()


def test_volume_and_integrate_refuse_the_cpu():
    from md_rdm_amd import _lib, fuse
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        fuse.Volume((4, 4, 4), (0.0, 0.0, 0.0), 0.1, device="cpu")
    for kw in (dict(dims=(4, 4)), dict(dims=(0, 4, 4)), dict(dims=(2048, 2048, 2048)), dict(voxel=0.0), dict(voxel=math.nan), dict(trunc=-1.0), dict(origin=(0.0, INF, 0.0)),
               dict(max_weight=0.0)):
        args = dict(dims=(4, 4, 4), origin=(0.0, 0.0, 0.0), voxel=0.1, device="cpu")
        args.update(kw)
        with pytest.raises(_lib.RdmError) as e:
            fuse.Volume(**args)
        assert "no CPU fallback" not in str(e.value), kw                                # refused for its own reason, before the device is looked at
    assert fuse.VOXEL == 0.02 and fuse.TRUNC_VOXELS == 4.0 and fuse.MIN_WEIGHT == 1.0 and "not been measured" in fuse.__doc__


# ---- the command's rules: refused before anything touches a GPU ---------------------------------------------------------------------------
def test_predict_fuse_flags(tmp_path):
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.fuse, a.poses, a.poses_c2w, a.fuse_voxel, a.fuse_trunc, a.fuse_dims, a.fuse_origin, a.fuse_min_weight, a.fuse_max_weight) == (False, None, False) + (None,) * 6
    assert predict.check_fuse_args(a) is None
    three, two = str(tmp_path / "three.txt"), str(tmp_path / "two.npy")
    c2w = np.stack([IDENT, IDENT, IDENT]).reshape(3, 12)
    c2w[:, 3::4] = (1.0, 2.0, 3.0)
    np.savetxt(three, c2w)
    np.save(two, np.stack([IDENT, IDENT]))
    bad_rows = str(tmp_path / "bad.txt")
    np.savetxt(bad_rows, np.zeros((3, 11)))
    syn = ["--out", "d", "--synthetic", "3", "--metric", "--full_res", "--fuse", "--poses", three]
    files = ["--out", "d", "a.npy", "b.npy", "--metric", "--native", "--fuse", "--poses", two]
    checks = (predict.check_metric_args, predict.check_ply_args, predict.check_refine_args, predict.check_mesh_args, predict.check_view_args, predict.check_anchor_args)
    for argv in (syn + ["--max_depth", "6"], syn + ["--fuse_dims", "8", "9", "10", "--fuse_origin", "0", "0", "0", "--fuse_voxel", "0.05", "--fuse_trunc", "0.2"],
                 files + ["--max_depth", "6", "--min_depth", "0.2", "--ply_normals", "--intrinsics", "500", "500", "320", "240", "--refine", "--fuse_min_weight", "2",
                          "--fuse_max_weight", "16"],
                 files + ["--max_depth", "6", "--camera", "nyu", "--anchors", "x.npy", "y.npy", "--stereo", "0.06"]):
        a = P.parse_args(argv)
        for check in checks:
            check(a)
        poses = predict.check_fuse_args(a)
        assert poses.shape == (len(poses), 12) and poses.dtype == np.float64
    got = predict.check_fuse_args(P.parse_args(syn + ["--max_depth", "6", "--poses_c2w"]))
    assert got[:, 3::4].tolist() == [[-1.0, -2.0, -3.0]] * 3 and got[:, :3].tolist() == [[1.0, 0.0, 0.0]] * 3          # [R^T | -R^T t]
    plain = ["--out", "d", "f.npy"]
    for argv, word in ((plain + ["--poses", three], "need --fuse"), (plain + ["--poses_c2w"], "need --fuse"), (plain + ["--fuse_voxel", "0.1"], "need --fuse"),
                       (plain + ["--fuse_trunc", "0.1"], "need --fuse"), (plain + ["--fuse_dims", "1", "2", "3"], "need --fuse"),
                       (plain + ["--fuse_origin", "1", "2", "3"], "need --fuse"), (plain + ["--fuse_min_weight", "1"], "need --fuse"),
                       (plain + ["--metric", "--native", "--fuse_max_weight", "4"], "need --fuse"),
                       (plain + ["--fuse", "--poses", three], "--fuse needs --metric"),
                       (plain + ["--metric", "--fuse", "--poses", three, "--max_depth", "6"], "--fuse needs the colours"),
                       (["--out", "d", "--synthetic", "3", "--metric", "--fuse", "--poses", three, "--max_depth", "6"], "--fuse needs the colours"),
                       (plain + ["--metric", "--native", "--fuse", "--max_depth", "6"], "--fuse needs --poses"),
                       (syn, "give --max_depth"), (syn + ["--fuse_dims", "8", "8", "8"], "give --max_depth"),
                       (syn + ["--max_depth", "6", "--fuse_voxel", "0"], "--fuse_voxel must be"), (syn + ["--max_depth", "6", "--fuse_voxel", "inf"], "--fuse_voxel must be"),
                       (syn + ["--max_depth", "6", "--fuse_trunc", "-1"], "--fuse_trunc must be"), (syn + ["--max_depth", "6", "--fuse_dims", "0", "4", "4"], "--fuse_dims must be"),
                       (syn + ["--max_depth", "6", "--fuse_dims", "2048", "2048", "2048"], "--fuse_dims must be"),
                       (syn + ["--max_depth", "6", "--fuse_origin", "0", "nan", "0"], "--fuse_origin must be"),
                       (syn + ["--max_depth", "6", "--fuse_min_weight", "nan"], "--fuse_min_weight"), (syn + ["--max_depth", "6", "--fuse_max_weight", "0.5"], "--fuse_max_weight"),
                       (syn + ["--max_depth", "2", "--min_depth", "3"], "--max_depth"), (syn + ["--max_depth", "6", "--camera", "kinect"], "--camera kinect"),
                       (syn + ["--max_depth", "6", "--ply_step", "2"], "need --ply"),
                       (["--out", "d", "--synthetic", "2", "--metric", "--full_res", "--fuse", "--poses", three, "--max_depth", "6"], "one row per input frame (got 3 rows for 2 inputs)"),
                       (files[:2] + files[3:] + ["--max_depth", "6"], "one row per input frame (got 2 rows for 1 inputs)"),
                       (syn[:-1] + [bad_rows, "--max_depth", "6"], "rows of twelve"), (syn[:-1] + [str(tmp_path / "none.txt"), "--max_depth", "6"], "--poses")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit):
        P.parse_args(plain + ["--fuse_dims", "1", "2"])                                    # three values or none
    text = P.format_help()
    for flag in ("--fuse", "--poses FILE", "--poses_c2w", "--fuse_voxel M", "--fuse_trunc M", "--fuse_dims NX NY NZ", "--fuse_origin X Y Z", "--fuse_min_weight W", "--fuse_max_weight W"):
        assert flag in text, flag
    assert "not been measured" in " ".join(text.split()) and all(f in predict.__doc__ for f in ("--fuse", "--poses", "--poses_c2w", "--fuse_voxel", "fused.ply"))


# ---- the C ABI of include/rdm_fuse.h ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib, build
    assert _lib.symbols("rdm_fuse.h") == ["rdm_tsdf_integrate", "rdm_tsdf_extract_workspace_bytes", "rdm_tsdf_extract"]          # types and exports: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_tsdf" not in hip_h and "rdm_fuse.h" not in hip_h
    assert "fuse.hip" in build.sources()
    src = open(os.path.join(ROOT, "md_rdm_amd", "csrc", "fuse.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("namespace rdm {", 1)[1] and "hipMemset" not in src


def test_workspace_bytes(L):
    ws = L.rdm_tsdf_extract_workspace_bytes
    assert ws(19, 13, 11) == 13 * 11 * 8 and ws(256, 256, 256) == 256 * 256 * 8 and ws(1, 1, 1) == 8 and ws(1, 46340, 46340) == 46340 * 46340 * 8
    for bad in ((0, 4, 6), (-1, 4, 6), (4, 0, 6), (4, 6, -1), (2048, 2048, 512), (65536, 65536, 1)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_are_status_codes_before_any_device_call(L):
    """Made-up pointers only: every refusal comes from the launcher's own checks, which precede the launches (this machine has no device to call)."""
    nan, inf = float("nan"), float("inf")
    P = C.c_void_p(256)
    I4, G5 = lambda *v: (C.c_double * 4)(*v), lambda *v: (C.c_double * 5)(*v)
    intr, geom = I4(500.0, 510.0, 3.25, 2.5), G5(0.0, 0.0, 0.0, 0.1, 0.4)
    # positions: 0 depth, 1 rgb, 2 batch, 3 h, 4 w, 5 intr, 6 poses, 7 pose_stride, 8 min_depth, 9 max_depth, 10 obs_weight, 11 max_weight, 12 nx, 13 ny, 14 nz, 15 geom,
    # 16 tsdf, 17 weight, 18 color, 19 stream
    good = [P, P, 2, 4, 6, intr, P, 12, 0.0, inf, 1.0, 64.0, 5, 6, 7, geom, P, P, P, None]
    bad = [({0: None}, b"depth"), ({5: None}, b"intr"), ({6: None}, b"poses"), ({15: None}, b"geom"), ({16: None}, b"tsdf"), ({17: None}, b"weight"),
           ({1: None}, b"color needs rgb"), ({2: 0}, b"batch"), ({2: 65536}, b"65535"), ({3: 0}, b"h"), ({4: -2}, b"w"), ({3: 65536, 4: 32768}, b"h * w"),
           ({5: I4(nan, 1, 0, 0)}, b"intr"), ({5: I4(0, 1, 0, 0)}, b"intr"), ({5: I4(1, 1, 0, -inf)}, b"intr"), ({8: -1e-9}, b"min_depth"), ({8: nan}, b"min_depth"),
           ({9: nan}, b"max_depth"), ({8: 2.0, 9: 1.0}, b"max_depth"), ({7: 1}, b"pose_stride"), ({7: 24}, b"pose_stride"), ({7: -12}, b"pose_stride"),
           ({12: 0}, b"nx"), ({13: -1}, b"ny"), ({14: 0}, b"nz"), ({12: 2048, 13: 2048, 14: 512}, b"nx * ny * nz"), ({12: 65536, 13: 65536, 14: 1}, b"nx * ny * nz"),
           ({15: G5(nan, 0, 0, 0.1, 0.4)}, b"geom"), ({15: G5(0, inf, 0, 0.1, 0.4)}, b"geom"), ({15: G5(0, 0, 0, 0.0, 0.4)}, b"voxel"), ({15: G5(0, 0, 0, 0.1, -0.4)}, b"trunc"),
           ({15: G5(0, 0, 0, inf, 0.4)}, b"geom"), ({10: 0.0}, b"obs_weight"), ({10: inf}, b"obs_weight"), ({10: nan}, b"obs_weight"), ({10: -1.0}, b"obs_weight"),
           ({11: nan}, b"max_weight"), ({11: 0.5}, b"max_weight")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_tsdf_integrate(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
    need = L.rdm_tsdf_extract_workspace_bytes(5, 6, 7)
    assert need == 6 * 7 * 8
    # positions: 0 tsdf, 1 weight, 2 color, 3 nx, 4 ny, 5 nz, 6 geom, 7 min_weight, 8 normals, 9 records, 10 capacity, 11 count, 12 workspace, 13 workspace_bytes, 14 stream
    good = [P, P, P, 5, 6, 7, geom, 1.0, 1, P, 10, P, P, need, None]
    bad = [({0: None}, b"tsdf"), ({1: None}, b"weight"), ({6: None}, b"geom"), ({11: None}, b"count"), ({12: None}, b"workspace"), ({3: 0}, b"nx"), ({4: 0}, b"ny"), ({5: -3}, b"nz"),
           ({3: 2048, 4: 2048, 5: 512, 13: 2 ** 40}, b"nx * ny * nz"), ({6: G5(0, 0, nan, 0.1, 0.4)}, b"geom"), ({6: G5(0, 0, 0, -0.1, 0.4)}, b"voxel"),
           ({6: G5(0, 0, 0, 0.1, 0.0)}, b"trunc"), ({7: nan}, b"min_weight"), ({8: 2}, b"normals"), ({8: -1}, b"normals"), ({10: -1}, b"capacity"),
           ({13: need - 1}, b"workspace_bytes"), ({13: 0}, b"workspace_bytes"), ({12: C.c_void_p(260)}, b"aligned")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_tsdf_extract(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
