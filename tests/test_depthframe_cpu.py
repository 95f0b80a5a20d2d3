"""Metric depth frames without a GPU: the 16-bit PNG writer, the SID tables against the reference-generated fixture
(tests/golden/sid_tables.npz), the scale formula, the numpy statement of the kernel's contract (tests/depthframe_ref.py), the rules of the
command-line flags, and the C-ABI boundary of include/rdm_depth.h (declared == bound == exported, not in rdm_hip.h)."""
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import depthframe_ref as dref
from conftest import GOLDEN, ROOT
from md_rdm_amd import filler

NAMES = ("nyu", "kitti", "floorplan3d", "Structured3D")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "sid_tables.npz"), allow_pickle=False)


# ---- write_png16 ---------------------------------------------------------------------------------------------------------------------------
def png16_arrays():
    field = (filler.unit("png16.field", 15) * 65536.0).astype(np.uint16).reshape(3, 5)
    fixed = np.array([[0, 1, 255, 256, 65535], [65535, 256, 255, 1, 0], [257, 258, 4660, 52719, 32768]], dtype=np.uint16)
    return [np.array([[v]], dtype=np.uint16) for v in (0, 1, 255, 256, 65535)] + [fixed, field]


def test_write_png16_bytes(tmp_path):
    from md_rdm_amd import viz
    p = str(tmp_path / "d.png")
    viz.write_png16(p, np.array([[0x1234, 0xABCD, 1]], dtype=np.uint16))
    data = open(p, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    assert data[8:16] == struct.pack(">I", 13) + b"IHDR"
    assert data[16:29] == struct.pack(">IIBBBBB", 3, 1, 16, 0, 0, 0, 0)            # width, height, bit depth 16, colour type 0 (greyscale), no interlace
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29])
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    assert zlib.decompress(data[41:41 + n]) == b"\x00\x12\x34\xab\xcd\x00\x01"      # filter 0, big-endian samples
    assert data[41 + n + 4:] == struct.pack(">I", 0) + b"IEND" + struct.pack(">I", zlib.crc32(b"IEND"))


def test_write_png16_round_trip_through_pillow(tmp_path):
    from PIL import Image
    from md_rdm_amd import viz
    for i, a in enumerate(png16_arrays()):
        for src in (a, torch.from_numpy(a.view(np.int16)).view(torch.uint16)):
            p = str(tmp_path / ("a%d.png" % i))
            viz.write_png16(p, src)
            with Image.open(p) as im:
                assert im.mode == "I;16" and im.size == (a.shape[1], a.shape[0]), (im.mode, im.size)
                back = np.asarray(im)
            assert back.dtype == np.uint16
            np.testing.assert_array_equal(back, a)


def test_write_png16_refuses_other_arrays(tmp_path):
    from md_rdm_amd import viz
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.int16), np.zeros((4, 4), np.float32), np.zeros((4, 4, 1), np.uint16), np.zeros((4,), np.uint16),
                np.zeros((0, 4), np.uint16), np.zeros((4, 0), np.uint16), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            viz.write_png16(str(tmp_path / "bad.png"), bad)
    assert not os.listdir(tmp_path)


# ---- the SID tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_sid_tables_bit_for_bit(gold, name):
    from md_rdm_amd import depth, utils
    alpha, beta, K = gold[name + "/params"]
    assert depth.SID[name] == (alpha, beta, K) == dref.SID[name]
    d = utils.get_depth_sid(name, torch.arange(int(K) + 1))
    assert d.dtype == torch.float32
    np.testing.assert_array_equal(d.numpy().view(np.int32), gold[name + "/depth_of_label"].view(np.int32))
    lab = utils.get_labels_sid(name, torch.from_numpy(gold[name + "/grid"]))
    assert lab.dtype == torch.int32
    np.testing.assert_array_equal(lab.numpy(), gold[name + "/label_of_grid"])
    np.testing.assert_array_equal(lab.numpy()[:int(K)], np.arange(int(K)))                       # the grid's bin centres give their own bins


def test_sid_unknown_name():
    from md_rdm_amd import _lib, depth, utils
    for f in (lambda: utils.get_depth_sid("scannet", torch.arange(3)), lambda: utils.get_labels_sid("scannet", torch.ones(3)), lambda: depth.sid_params("scannet")):
        with pytest.raises(_lib.RdmError, match="scannet"):
            f()
    assert depth.sid_params((0.1, 5, 10)) == (0.1, 5.0, 10.0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("offset", [0.0, 0.5])
def test_scale_formula_is_the_mean_log_of_get_depth_sid(name, offset):
    """S = mean over the head of log(get_depth_sid(label + offset)), within the float32 rounding of get_depth_sid: its constants log(alpha) and
    log(beta / alpha) are float32 results of magnitude below 12 (one float32 ulp of the log function: 1.2e-7 * 12 = 1.4e-6 each), alpha and beta
    are rounded to float32 first (6e-8 relative each = 6e-8 in the log) and the depth it returns is rounded to float32 (6e-8 in the log):
    below 3.2e-6 in all; the bound is 4e-6."""
    from md_rdm_amd import depth, utils
    alpha, beta, K = depth.SID[name]
    for n in (1, 63, 64, 418):
        c = (filler.unit("sidscale/%s/%d" % (name, n), n) * (K + 1)).astype(np.int64)
        want = float(torch.log(utils.get_depth_sid(name, torch.from_numpy(c).double() + offset).double()).mean())
        got = depth.sid_log_scale_value(int(c.sum()), n, name, offset)
        assert abs(got - want) <= 4e-6, (name, n, got, want)
        assert got == dref.log_scale(1, c, None, name, offset)[0]                                 # the two statements of the formula, bit for bit
    assert depth.sid_log_scale_value(0, 7, name, 0.0) == math.log(alpha)                           # all counts 0: alpha metres
    assert abs(depth.sid_log_scale_value(int(K) * 7, 7, name, 0.0) - math.log(beta)) < 1e-14      # all counts K: beta metres


# ---- the numpy statement of the contract ----------------------------------------------------------------------------------------------------
def test_reference_full_view_at_map_size_is_exp_of_the_map():
    m = filler.uniform("dframe.cpu.map", (2, 1, 128, 128), -1.5, 1.5, dtype=np.float64)
    ls = np.array([0.25, -1.0])
    r = dref.reference(m, 128, 128, log_scale_in=ls)
    np.testing.assert_array_equal(r["D"], np.exp(m[:, 0] + ls[:, None, None]))
    np.testing.assert_array_equal(r["f32"], np.exp(m[:, 0] + ls[:, None, None]).astype(np.float32))
    assert r["inside"].all() and r["u16"].dtype == np.uint16 and r["f32"].dtype == np.float32
    np.testing.assert_array_equal(r["ls"], ls)


def test_reference_outside_zero_and_quantisation():
    m = filler.uniform("dframe.cpu.map", (2, 1, 128, 128), -1.5, 1.5, dtype=np.float64)
    view = (2.5, -3.25, 30.0, 48.5)                                                  # rows 2.5 .. 32.5, columns -3.25 .. 45.25 of a 37x53 frame
    z, e = dref.reference(m, 37, 53, view=view), dref.reference(m, 37, 53, view=view, outside="edge")
    inside = np.zeros((37, 53), dtype=bool)
    inside[2:32, 0:45] = True                                                        # centres 2.5 (the closed end) .. 31.5 (32.5 is the open end) and 0.5 .. 44.5
    np.testing.assert_array_equal(z["inside"], inside)
    assert (z["f32"][:, ~inside] == 0).all() and (z["u16"][:, ~inside] == 0).all() and (e["u16"][:, ~inside] > 0).all()
    np.testing.assert_array_equal(z["u16"][:, inside], e["u16"][:, inside])
    np.testing.assert_array_equal(z["f32"][:, inside], e["f32"][:, inside])
    u, _ = dref.quantise(np.array([np.nan, np.inf, 65.5349, 70.0, 0.0, 0.0014, 0.0016, 1.2344]), 1e-3)
    np.testing.assert_array_equal(u, [0, 65535, 65535, 65535, 0, 1, 2, 1234])          # NaN, saturation, nearest; ties to even below, on exact quotients
    u, _ = dref.quantise(np.array([0.5, 1.5, 2.5, 65534.4, 65534.5]) / 256.0, 1.0 / 256.0)
    np.testing.assert_array_equal(u, [0, 2, 2, 65534, 65534])


# ---- the commands' rules: refused before anything touches a GPU -----------------------------------------------------------------------------
def test_predict_metric_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.metric, a.sid, a.sid_offset, a.native, a.outside, a.png16, a.depth_unit) == (False, None, None, False, None, False, None)
    predict.check_metric_args(a)
    a = P.parse_args(["--out", "d", "f.npy", "--metric", "--sid", "kitti", "--sid_offset", "0.5", "--native", "--outside", "edge", "--png16", "--depth_unit", "0.00390625"])
    assert (a.metric, a.sid, a.sid_offset, a.native, a.outside, a.png16, a.depth_unit) == (True, "kitti", 0.5, True, "edge", True, 0.00390625)
    predict.check_metric_args(a)
    files, syn = ["--out", "d", "f.npy"], ["--out", "d", "--synthetic", "2"]
    for argv, word in ((files + ["--png16"], "need --metric"), (files + ["--sid", "nyu"], "need --metric"), (files + ["--sid_offset", "0.5"], "need --metric"),
                       (files + ["--outside", "edge"], "need --metric"), (files + ["--depth_unit", "0.01"], "need --metric"), (files + ["--native"], "need --metric"),
                       (files + ["--metric", "--native", "--full_res"], "--native excludes"), (syn + ["--metric", "--native"], "--native excludes"),
                       (files + ["--metric", "--linear"], "--metric excludes --linear"), (syn + ["--metric", "--linear"], "--metric excludes --linear"),
                       (files + ["--metric", "--sid", "scannet"], "--sid scannet"), (files + ["--metric", "--depth_unit", "0"], "--depth_unit"),
                       (files + ["--metric", "--depth_unit", "nan"], "--depth_unit"), (files + ["--metric", "--depth_unit", "inf"], "--depth_unit")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit):
        P.parse_args(files + ["--metric", "--outside", "mirror"])
    text = P.format_help()
    for flag in ("--metric", "--sid NAME", "--sid_offset F", "--native", "--outside {zero,edge}", "--png16", "--depth_unit M"):
        assert flag in text, flag


def test_evaluate_scale_flags():
    from md_rdm_amd import evaluate, harness
    from md_rdm_amd.metrics import StandardMetrics
    P = evaluate.build_parser()
    a = P.parse_args([])
    assert a.scale is None and a.sid is None and a.sid_offset is None
    a = P.parse_args(["--protocol", "standard", "--align", "none", "--scale", "sid", "--sid", "kitti", "--sid_offset", "0.5"])
    assert (a.scale, a.sid, a.sid_offset) == ("sid", "kitti", 0.5)
    assert isinstance(evaluate.make_computer(a), StandardMetrics)
    syn = ["--synthetic", "2"]
    for argv, word in ((syn + ["--scale", "sid"], "--protocol standard"), (syn + ["--protocol", "standard", "--sid", "nyu"], "need --scale sid"),
                       (syn + ["--protocol", "standard", "--sid_offset", "0.5"], "need --scale sid"),
                       (syn + ["--protocol", "standard", "--scale", "sid", "--sid", "scannet"], "--sid scannet")):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        assert word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit):
        P.parse_args(["--scale", "median"])
    with pytest.raises(ValueError, match="standard protocol"):
        harness.evaluate(None, [], ["mse"], scale="sid")                             # the reference protocol compares normalised maps
    with pytest.raises(ValueError, match="scale"):
        harness.evaluate(None, [], StandardMetrics(align="none"), scale="median")


def test_host_tensors_are_refused():
    from md_rdm_amd import _lib, depth
    with pytest.raises(_lib.RdmError):
        depth.metric_frames(torch.zeros(1, 1, 128, 128, dtype=torch.float64), (4, 4))
    with pytest.raises(_lib.RdmError):
        depth.sid_log_scale(torch.zeros(1, 1, 8, 8, dtype=torch.int64))


# ---- the C ABI of include/rdm_depth.h -------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_depth.h")) == {"rdm_depth_frames"}      # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_depth_frames" not in hip_h and "rdm_depth.h" not in hip_h
