"""Novel views without a GPU: the numpy statement of include/rdm_warp.h (tests/warp_ref.py) on frames whose views are known by hand, the pose
helpers, the wrapper's refusals, the rules of the command-line flags, and the C-ABI boundary of include/rdm_warp.h (declared == bound == exported,
in no other table; every bad argument a status code with a message, before any device call)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import warp_ref as wref
from conftest import ROOT
from md_rdm_amd import filler

INTR = (40.0, 44.0, 5.25, 3.5)
IDENT = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
INF = math.inf


def both(d, intr, pose, **kw):
    """warp_ref.sample, which must agree with the pixel-by-pixel statement on every frame a test uses"""
    a, b = wref.sample(d, intr, pose, **kw), wref.loops(d, intr, pose, **kw)
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    return a


def colours(key, h, w):
    return (filler.unit("warp.cpu.rgb/" + key, h * w * 3) * 256.0).astype(np.uint8).reshape(h, w, 3)


# ---- the numpy statement of the contract ----------------------------------------------------------------------------------------------------
def test_identity_pose_returns_the_input():
    d = filler.uniform("warp.cpu.identity", (9, 13), 0.7, 6.0).astype(np.float32)
    for k, bad in enumerate((0.0, -1.0, np.nan, np.inf, 0.25, 7.5)):
        d[k, 2 * k] = bad
    rgb = colours("identity", 9, 13)
    out = both(d, INTR, IDENT, rgb=rgb, min_depth=0.5, max_depth=7.0)
    ok = wref.valid(d, 0.5, 7.0)
    assert ok.sum() == 9 * 13 - 6
    assert out["mask"].tobytes() == ok.astype(np.uint8).tobytes()
    assert out["depth"].tobytes() == np.where(ok, d, np.float32(0)).astype(np.float32).tobytes()
    np.testing.assert_array_equal(out["index"], np.where(ok, np.arange(9 * 13).reshape(9, 13), -1))
    np.testing.assert_array_equal(out["rgb"], np.where(ok[..., None], rgb, 0))
    full = both(np.full((4, 6), 2.0, np.float32), INTR, IDENT)                     # all valid: index == arange
    np.testing.assert_array_equal(full["index"].reshape(-1), np.arange(24))
    assert "rgb" not in full


def test_stereo_plane_shifts_by_the_disparity():
    from md_rdm_amd import warp
    fx, Z, k = 40.0, 2.0, 3                                                        # disparity fx * b / Z = 3 columns: b = 0.15
    b = k * Z / fx
    assert fx * b / Z == k
    d = np.full((5, 11), Z, np.float32)
    rgb = colours("stereo", 5, 11)
    out = both(d, (fx, 44.0, 5.0, 2.0), warp.stereo_pose(b), rgb=rgb)
    idx = np.arange(55).reshape(5, 11)
    # the right camera sees every point k columns to the LEFT; the k columns at the right edge see nothing
    np.testing.assert_array_equal(out["index"][:, :11 - k], idx[:, k:])
    np.testing.assert_array_equal(out["index"][:, 11 - k:], -1)
    np.testing.assert_array_equal(out["mask"][:, :11 - k], 1)
    np.testing.assert_array_equal(out["mask"][:, 11 - k:], 0)
    np.testing.assert_array_equal(out["rgb"][:, :11 - k], rgb[:, k:])
    np.testing.assert_array_equal(out["rgb"][:, 11 - k:], 0)
    assert (out["depth"][:, :11 - k] == np.float32(Z)).all() and (out["depth"][:, 11 - k:] == 0).all()


def test_nearer_surface_occludes_and_equal_depth_takes_the_smaller_index():
    from md_rdm_amd import warp
    # one row, fx = 8, camera moved 0.5 m right: depth 4 moves 1 column left, depth 1 moves 4 columns left
    intr = (8.0, 8.0, 0.0, 0.0)
    d = np.array([[4.0, 4.0, 4.0, 4.0, 4.0, 1.0, 4.0, 4.0]], np.float32)
    out = both(d, intr, warp.stereo_pose(0.5))
    # far pixels x -> x - 1: cells 0..3 from 1..4, cell 5, 6 from 6, 7; the near pixel 5 -> cell 1, where the far pixel 2 lands too: the near one wins
    assert out["index"].tolist() == [[1, 5, 3, 4, -1, 6, 7, -1]]
    assert out["depth"].tolist() == [[4.0, 1.0, 4.0, 4.0, 0.0, 4.0, 4.0, 0.0]]
    assert out["mask"].tolist() == [[1, 1, 1, 1, 0, 1, 1, 0]]
    # equal zf on one cell: a camera pulled back so that a 1x6 row of constant depth lands on 2 cells; the smallest source index of each cell wins
    pose = IDENT.copy()
    pose[2, 3] = 4.0                                                               # Qz = 2 + 4 = 6: u = x / 3
    out = both(np.full((1, 6), 2.0, np.float32), intr, pose)
    # u = 0, 1/3, 2/3, 1, 4/3, 5/3 -> floor(u + 0.5) = 0 0 1 1 1 2
    assert out["index"].tolist() == [[0, 2, 5, -1, -1, -1]] and (out["depth"][0, :3] == np.float32(6.0)).all()


def test_fill_takes_the_farther_side_prefers_left_respects_f_and_never_chains():
    EM = wref.EMPTY

    def K(z, i):
        return np.uint64((int(np.float32(z).view(np.uint32)) << 32) | i)
    keys = np.array([[K(2, 10), EM, EM, K(5, 11), EM, K(5, 12), EM, EM, EM, EM, EM, K(1, 13), EM]], np.uint64)
    out = wref.resolve(keys, None, 2)
    #         cell: 0   1   2   3   4   5   6   7   8   9  10  11  12
    # 1: left 10 (k=1, z 2) and right 11 (k=2, z 5): the farther 11; 2: likewise; 4: 11 and 12, both z 5: the left; 6: left 12, no right within 2;
    # 7: left 12 at k=2; 8: nothing within 2 - although 7 was filled: no chaining; 9: right 13 at k=2; 10: right 13; 12: left 13
    assert out["index"].tolist() == [[10, 11, 11, 11, 11, 12, 12, 12, -1, 13, 13, 13, 13]]
    assert out["mask"].tolist() == [[1, 2, 2, 1, 2, 1, 2, 2, 0, 2, 2, 1, 2]]
    assert out["depth"].tolist() == [[2.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 0.0, 1.0, 1.0, 1.0, 1.0]]
    out = wref.resolve(keys, None, 0)
    assert out["mask"].tolist() == [[1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0]]
    out = wref.resolve(keys, None, 1)
    assert out["index"].tolist() == [[10, 10, 11, 11, 11, 12, 12, -1, -1, -1, 13, 13, 13]]          # cell 4: a tie at k = 1 on both sides: left
    out = wref.resolve(keys, None, 64)
    assert out["index"].tolist() == [[10, 11, 11, 11, 11, 12, 12, 12, 12, 12, 12, 13, 13]]          # 6..10 between z 5 (left) and z 1 (right): the farther
    rgb = colours("fill", 1, 14)
    out = wref.resolve(keys, rgb, 2)
    np.testing.assert_array_equal(out["rgb"][0, 1], rgb[0, 11])
    np.testing.assert_array_equal(out["rgb"][0, 8], 0)
    empty = wref.resolve(np.full((2, 3), EM, np.uint64), None, 64)                  # a frame of holes stays one
    assert not empty["mask"].any() and (empty["index"] == -1).all() and not empty["depth"].any()


@pytest.mark.parametrize("splat", [1, 2, 3, 4])
def test_splat_footprints_are_clipped_at_all_four_borders(splat):
    # one source pixel, projected by the target intrinsics' principal point to a chosen (u, v) of a 5x7 target
    d = np.full((1, 1), 2.0, np.float32)
    src = (10.0, 10.0, 0.0, 0.0)
    for u, v in ((0.0, 0.0), (6.0, 4.0), (0.0, 4.0), (6.0, 0.0), (3.0, 2.0), (-1.0, 2.0), (7.0, 2.0), (3.0, -1.0), (3.0, 5.0), (-4.0, 2.0), (3.0, 9.0), (1e300, 2.0), (3.0, -1e300)):
        out = both(d, src, IDENT, out_hw=(5, 7), intr_dst=(10.0, 10.0, u, v), splat=splat)
        c0, r0 = math.floor(u - (splat - 1) * 0.5 + 0.5), math.floor(v - (splat - 1) * 0.5 + 0.5)
        want = np.zeros((5, 7), np.uint8)
        want[max(r0, 0):max(min(r0 + splat, 5), 0), max(c0, 0):max(min(c0 + splat, 7), 0)] = 1
        np.testing.assert_array_equal(out["mask"], want, err_msg="splat %d at (%r, %r)" % (splat, u, v))
        assert (out["index"][want == 1] == 0).all() and (out["depth"][want == 1] == np.float32(2.0)).all()
    # an even footprint sits on the four cells around a corner, an odd one around the nearest cell
    assert both(d, src, IDENT, out_hw=(5, 7), intr_dst=(10.0, 10.0, 2.5, 1.5), splat=2)["mask"].nonzero()[0].tolist() == [1, 1, 2, 2]


def test_points_behind_the_camera_and_overflowing_depths_are_dropped():
    d = np.array([[1.0, 2.0, 3.0]], np.float32)
    pose = IDENT.copy()
    pose[2, 3] = -2.0                                                              # Qz = -1, 0, 1: only the last is in front
    out = both(d, (4.0, 4.0, 1.0, 0.0), pose, out_hw=(3, 9))
    assert (out["mask"] > 0).sum() == 1 and out["index"].max() == 2 and out["depth"].max() == np.float32(1.0)
    pose[2, 3] = 1e39                                                              # zf overflows float32
    assert not both(d, (4.0, 4.0, 1.0, 0.0), pose)["mask"].any()
    tiny = np.concatenate([1e-46 * np.eye(3), np.zeros((3, 1))], axis=1)           # R as given: Qz = 1e-46 .. 3e-46 > 0, zf rounds to 0
    assert not both(d, (4.0, 4.0, 1.0, 0.0), tiny)["mask"].any()
    out = both(d, (4.0, 4.0, 1.0, 0.0), 1e-45 * tiny / 1e-46)                      # Qz = 1e-45 .. 3e-45: float32 denormals, kept where they were
    assert out["mask"].tolist() == [[1, 1, 1]] and out["depth"].view(np.uint32).tolist() == [[1, 1, 2]]


# ---- the pose helpers ----------------------------------------------------------------------------------------------------------------------------
def test_stereo_pose_and_pose_from_rt():
    from md_rdm_amd import _lib, warp
    p = warp.stereo_pose(0.06)
    assert p.dtype == np.float64 and p.shape == (3, 4) and p.tolist() == [[1, 0, 0, -0.06], [0, 1, 0, 0], [0, 0, 1, 0]]
    assert warp.pose_from_rt((0, 0, 0), (1, 2, 3)).tolist() == [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3]]
    q = warp.pose_from_rt((0, math.pi / 2, 0), (0, 0, 0))                          # a quarter turn about y: z -> x, x -> -z
    np.testing.assert_allclose(q[:, :3] @ np.array([0.0, 0.0, 1.0]), [1.0, 0.0, 0.0], atol=1e-15)
    np.testing.assert_allclose(q[:, :3] @ np.array([1.0, 0.0, 0.0]), [0.0, 0.0, -1.0], atol=1e-15)
    r = np.array([0.3, -0.2, 0.5])
    R = warp.pose_from_rt(r, (0.1, 0.2, 0.3))
    assert R.dtype == np.float64 and R[:, 3].tolist() == [0.1, 0.2, 0.3]
    np.testing.assert_allclose(R[:, :3] @ R[:, :3].T, np.eye(3), atol=1e-15)
    np.testing.assert_allclose(np.linalg.det(R[:, :3]), 1.0, atol=1e-15)
    np.testing.assert_allclose(R[:, :3] @ r, r, atol=1e-15)                        # the axis is fixed
    np.testing.assert_allclose(np.trace(R[:, :3]), 1.0 + 2.0 * math.cos(np.linalg.norm(r)), atol=1e-15)
    np.testing.assert_allclose(warp.pose_from_rt(-r, (0, 0, 0))[:, :3], R[:, :3].T, atol=1e-15)
    for bad in (lambda: warp.stereo_pose(math.nan), lambda: warp.pose_from_rt((0, 0), (0, 0, 0)), lambda: warp.pose_from_rt((0, 0, math.inf), (0, 0, 0))):
        with pytest.raises(_lib.RdmError):
            bad()
    assert warp.pose_rows(np.eye(4), 3).tolist() == [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]
    assert warp.pose_rows(torch.eye(4)[:3], 3).shape == (1, 12) and warp.pose_rows(np.stack([IDENT] * 3), 3).shape == (3, 12)
    for bad in (np.eye(3), np.stack([IDENT] * 2), np.zeros((3, 4, 1, 1)), "abc"):
        with pytest.raises(_lib.RdmError):
            warp.pose_rows(bad, 3)


def test_render_checks_its_arguments_before_the_device():
    """a host tensor is refused as such only after every check that needs no device has passed"""
    from md_rdm_amd import _lib, warp
    d = torch.ones(1, 4, 6)
    for kw, word in ((dict(splat=0), "splat"), (dict(splat=5), "splat"), (dict(splat=1.5), "splat"), (dict(fill=-1), "fill"), (dict(fill=65), "fill"),
                     (dict(want=("depth", "normals")), "want"), (dict(want=()), "want"), (dict(out_hw=(0, 4)), "out_hw"), (dict(out_hw=(4,)), "out_hw"),
                     (dict(intrinsics_out=(1.0, 0.0, 0.0, 0.0)), "intrinsics_out"), (dict(min_depth=-1.0), "min_depth"), (dict(min_depth=2.0, max_depth=1.0), "min_depth"),
                     (dict(max_depth=math.nan), "max_depth")):
        with pytest.raises(_lib.RdmError, match=word):
            warp.render(d, INTR, IDENT, **kw)
    with pytest.raises(_lib.RdmError, match="intrinsics"):
        warp.render(d, (math.inf, 1.0, 0.0, 0.0), IDENT)
    with pytest.raises(_lib.RdmError):
        warp.render(d, "kinect", IDENT)
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        warp.render(d, INTR, IDENT)
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        warp.render(np.ones((1, 4, 6), np.float32), INTR, IDENT, splat=4, fill=64, want="depth")
    assert warp.check_params(1, 0) is None and warp.check_params(4, 64) is None and 1 <= warp.SPLAT <= 4 and 0 <= warp.FILL <= 64


# ---- the command's rules: refused before anything touches a GPU ---------------------------------------------------------------------------
def test_predict_view_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.stereo, a.view_pose, a.view_splat, a.view_fill) == (None, None, None, None)
    predict.check_view_args(a)
    pose = [str(v) for v in IDENT.reshape(-1)]
    for argv in (["--out", "d", "f.npy", "--metric", "--native", "--stereo", "0.06", "--png16", "--view_splat", "2", "--view_fill", "16"],
                 ["--out", "d", "f.npy", "--metric", "--native", "--refine", "--view_pose"] + pose + ["--intrinsics", "500", "500", "320", "240", "--max_depth", "9"],
                 ["--out", "d", "--synthetic", "2", "--metric", "--full_res", "--stereo", "0.06", "--camera", "nyu", "--min_depth", "0.1"]):
        a = P.parse_args(argv)
        for check in (predict.check_metric_args, predict.check_ply_args, predict.check_refine_args, predict.check_mesh_args, predict.check_view_args):
            check(a)
    jobs = predict.view_jobs(P.parse_args(["--out", "d", "f.npy", "--metric", "--native", "--stereo", "0.06", "--view_pose"] + pose))
    assert [s for s, _ in jobs] == ["_right", "_view"] and jobs[0][1][0, 3] == -0.06 and jobs[1][1].tolist() == IDENT.tolist()
    files, syn = ["--out", "d", "f.npy"], ["--out", "d", "--synthetic", "2"]
    for argv, word in ((files + ["--stereo", "0.06"], "need --metric"), (files + ["--native", "--stereo", "0.06"], "need --metric"),
                       (files + ["--view_pose"] + pose, "need --metric"),
                       (files + ["--metric", "--stereo", "0.06"], "need the colours"), (files + ["--metric", "--full_res", "--stereo", "0.06"], "need the colours"),
                       (syn + ["--metric", "--stereo", "0.06"], "need the colours"), (syn + ["--metric", "--view_pose"] + pose, "need the colours"),
                       (files + ["--metric", "--native", "--view_splat", "2"], "need --stereo or --view_pose"), (files + ["--view_fill", "2"], "need --stereo or --view_pose"),
                       (files + ["--metric", "--native", "--stereo", "nan"], "--stereo must be finite"),
                       (files + ["--metric", "--native", "--view_pose"] + pose[:11] + ["inf"], "--view_pose must be"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--view_splat", "5"], "splat must be"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--view_splat", "0"], "splat must be"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--view_fill", "65"], "fill must be"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--view_fill", "-1"], "fill must be"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--ply_step", "2"], "need --ply"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--camera", "kinect"], "--camera kinect"),
                       (files + ["--metric", "--native", "--stereo", "0.06", "--min_depth", "2", "--max_depth", "1"], "--max_depth"),
                       (files + ["--metric", "--native", "--camera", "nyu"], "need --ply")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit):
        P.parse_args(files + ["--view_pose", "1", "2", "3"])                      # twelve values or none
    text = P.format_help()
    for flag in ("--stereo M", "--view_pose", "--view_splat S", "--view_fill F"):
        assert flag in text, flag
    assert all(f in predict.__doc__ for f in ("--stereo", "--view_pose", "--view_splat", "--view_fill")) and "starting points" in predict.__doc__
    steps = predict.depth_steps(np.array([0.0, 0.0004, 0.0016, 1.0, 70.0, np.nan, np.inf], np.float32), 1e-3)
    assert steps.dtype == np.uint16 and steps.tolist() == [0, 0, 2, 1000, 65535, 0, 65535]


# ---- the C ABI of include/rdm_warp.h ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


NAMES = {"rdm_depth_warp", "rdm_depth_warp_workspace_bytes"}


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_warp.h")) == NAMES        # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_depth_warp" not in hip_h and "rdm_warp.h" not in hip_h
    assert "warp.hip" in __import__("md_rdm_amd.build", fromlist=["sources"]).sources()


def test_workspace_bytes(L):
    ws = L.rdm_depth_warp_workspace_bytes
    assert ws(1, 4, 6) == 4 * 6 * 8 and ws(8, 480, 640) == 8 * 480 * 640 * 8 and ws(3, 1, 1) == 24 and ws(65535, 1, 1) == 65535 * 8
    assert ws(4, 46340, 46340) == 4 * 46340 * 46340 * 8                             # beyond 2^32 bytes: a size_t, not an int
    for bad in ((0, 4, 6), (-1, 4, 6), (1, 0, 6), (1, 4, -6), (65536, 4, 6), (1, 65536, 32768)):
        assert ws(*bad) == 0, bad


def test_bad_arguments_are_status_codes_before_any_device_call(L):
    """Made-up pointers only: every refusal comes from the launcher's own checks, which precede the launches (this machine has no device to call)."""
    nan, inf = float("nan"), float("inf")
    P = C.c_void_p(256)
    I4 = lambda *v: (C.c_double * 4)(*v)
    src, dst = I4(500.0, 510.0, 3.25, 2.5), I4(400.0, 410.0, 3.0, 2.0)
    need = L.rdm_depth_warp_workspace_bytes(2, 5, 7)
    assert need == 2 * 5 * 7 * 8
    # positions: 0 depth, 1 rgb, 2 batch, 3 h, 4 w, 5 intr_src, 6 intr_dst, 7 poses, 8 pose_stride, 9 min_depth, 10 max_depth, 11 th, 12 tw, 13 splat, 14 fill,
    # 15 depth_out, 16 rgb_out, 17 index_out, 18 mask_out, 19 workspace, 20 workspace_bytes, 21 stream
    good = [P, P, 2, 4, 6, src, dst, P, 12, 0.0, inf, 5, 7, 1, 0, P, P, P, P, P, need, None]
    bad = [({0: None}, b"depth"), ({5: None}, b"intr_src"), ({6: None}, b"intr_dst"), ({7: None}, b"poses"), ({15: None}, b"depth_out"), ({19: None}, b"workspace"),
           ({1: None}, b"rgb_out needs rgb"), ({2: 0}, b"batch"), ({2: -1}, b"batch"), ({3: 0}, b"h"), ({4: -2}, b"w"), ({11: 0}, b"th"), ({12: -1}, b"tw"),
           ({2: 65536, 20: 65536 * 35 * 8}, b"65535"), ({3: 65536, 4: 32768}, b"h * w"), ({11: 65536, 12: 32768, 20: 2 ** 40}, b"th * tw"),
           ({8: 1}, b"pose_stride"), ({8: 24}, b"pose_stride"), ({8: -12}, b"pose_stride"), ({13: 0}, b"splat"), ({13: 5}, b"splat"), ({14: -1}, b"fill"), ({14: 65}, b"fill"),
           ({20: need - 1}, b"workspace_bytes"), ({20: 0}, b"workspace_bytes"), ({19: C.c_void_p(260)}, b"aligned"),
           ({5: I4(nan, 1, 0, 0)}, b"intr_src"), ({5: I4(1, inf, 0, 0)}, b"intr_src"), ({5: I4(0, 1, 0, 0)}, b"intr_src"), ({5: I4(1, 1, 0, -inf)}, b"intr_src"),
           ({6: I4(1, 0, 0, 0)}, b"intr_dst"), ({6: I4(1, 1, nan, 0)}, b"intr_dst"), ({6: I4(0, 1, 0, 0)}, b"intr_dst"),
           ({9: -1e-9}, b"min_depth"), ({9: nan}, b"min_depth"), ({10: nan}, b"max_depth"), ({9: 2.0, 10: 1.0}, b"max_depth"), ({9: inf, 10: 1.0}, b"max_depth")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_depth_warp(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
