"""Depth-map rendering without a GPU: the numpy restatement of the semantics (tests/viz_ref.py) against the reference-generated fixture, the
PNG writer, the C-ABI boundary of include/rdm_viz.h and the command-line flags."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

import viz_ref
from conftest import ROOT
from md_rdm_amd import filler

LU = filler.log_uniform


def rows_input():
    """the fixture's x: (2,3,23,31) float32 holding every k / 255 (tests/golden/make_viz_golden.py)"""
    n = 2 * 3 * 23 * 31
    return ((np.arange(n) * 7 % 256).astype(np.float64) / 255.0).astype(np.float32).reshape(2, 3, 23, 31)


def rows_maps():
    return LU("viz.t", (2, 1, 57, 76), 0.5, 9.5), LU("viz.p", (2, 1, 16, 16), 0.2, 4.0)


def test_fixture_table_is_jet():
    lut = viz_ref.gold()["lut8"]
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [0, 0, 127] and lut[255].tolist() == [127, 0, 0]           # dark blue to dark red
    assert sorted(set(np.round(rows_input().astype(np.float64) * 255).astype(int).ravel())) == list(range(256))    # x holds every k / 255


def test_restatement_equals_every_fixture_array():
    g = viz_ref.gold()
    np.testing.assert_array_equal(viz_ref.colour((np.arange(256) + 0.5) / 256.0, 0.0, 1.0), g["lut8"])
    np.testing.assert_array_equal(viz_ref.colorize(LU("viz.m128", (2, 1, 128, 128), 0.5, 9.5), (37, 53)), g["cd_37x53"])
    np.testing.assert_array_equal(viz_ref.colorize(LU("viz.m8", (2, 1, 8, 8), 0.5, 2.0), (16, 16)), g["cd_16x16"])
    t, p = rows_maps()
    np.testing.assert_array_equal(viz_ref.rows(rows_input(), t, p, (23, 31)), g["rows_23x31"])
    np.testing.assert_array_equal(viz_ref.colorize(p, (23, 31)), g["rows_pred_23x31"])
    two = viz_ref.rows(rows_input(), None, p, (23, 31))
    np.testing.assert_array_equal(two, np.concatenate([g["rows_23x31"][:, :, :31], g["rows_pred_23x31"]], axis=2))


def test_restatement_edge_semantics():
    """bin edges, xa == 256, the clamps, NaN and the constant image, as include/rdm_viz.h states them"""
    lut = viz_ref.gold()["lut8"]
    k = np.arange(257) / 256.0
    np.testing.assert_array_equal(viz_ref.colour(k, 0.0, 1.0), lut[np.minimum(np.arange(257), 255)])
    np.testing.assert_array_equal(viz_ref.colour(np.array([-1.0, 2.0, np.nan]), 0.0, 1.0), np.stack([lut[0], lut[255], np.zeros(3, np.uint8)]))
    assert not viz_ref.colorize(np.full((1, 1, 3, 4), 2.5)).any()                        # 0 / 0
    m = LU("viz.nan", (1, 1, 3, 4), 0.5, 2.0).astype(np.float64)
    m[0, 0, 1, 2] = np.nan
    assert not viz_ref.colorize(m).any()                                                 # np.min propagates it


def _decode(path):
    """(H,W,3) uint8 of an 8-bit RGB PNG: Pillow where importable, else the chunks by hand (filter 0 lines only)"""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB"
            return np.asarray(im).copy()
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    assert (depth, ctype) == (8, 2)
    lines = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not lines[:, 0].any()
    return lines[:, 1:].reshape(h, w, 3).copy()


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (23, 93), (16, 64)])
def test_write_png_round_trips(tmp_path, shape):
    from md_rdm_amd import viz
    a = (filler.unit("viz.png%dx%d" % shape, shape[0] * shape[1] * 3) * 256).astype(np.uint8).reshape(shape + (3,))
    path = str(tmp_path / "a.png")
    viz.write_png(path, a)
    np.testing.assert_array_equal(_decode(path), a)
    raw = open(path, "rb").read()                         # structure, whatever decoded it: signature, IHDR first, 8-bit RGB, filter 0 on every line
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
    assert struct.unpack(">IIBBBBB", raw[16:29]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
    n = struct.unpack(">I", raw[33:37])[0]
    assert raw[37:41] == b"IDAT"
    lines = np.frombuffer(zlib.decompress(raw[41:41 + n]), dtype=np.uint8).reshape(shape[0], 1 + 3 * shape[1])
    assert not lines[:, 0].any()


def test_write_png_refuses_other_arrays(tmp_path):
    from md_rdm_amd import viz
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            viz.write_png(str(tmp_path / "bad.png"), bad)
    assert not os.listdir(tmp_path)


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_viz.h")) == {"rdm_viz_rows_u8"}      # declared == bound == exported, with the header's types: test_abi_cpu.py
    assert "rdm_viz" not in open(os.path.join(ROOT, "include", "rdm_hip.h")).read()


def test_argument_errors_are_status_codes():
    """every refusal happens before the launch: callable without a GPU"""
    import ctypes as C
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    p = C.c_void_p(4096)
    nan = float("nan")
    good = dict(rgb=None, a=None, a64=0, ha=0, wa=0, b=p, b64=1, hb=8, wb=8, batch=1, h=8, w=8, lo=nan, hi=nan, out=p, split=0)
    for change, word in ((dict(b=None), b"NULL"), (dict(out=None), b"NULL"), (dict(batch=0), b"batch"), (dict(h=0), b"batch"), (dict(w=-3), b"batch"),
                         (dict(hb=0), b"map sizes"), (dict(wb=-1), b"map sizes"), (dict(a=p, ha=0, wa=4), b"map sizes"), (dict(split=-1), b"split"),
                         (dict(h=1, w=0x30000000), b"32-bit")):
        kw = dict(good, **change)
        rc = L.rdm_viz_rows_u8(kw["rgb"], kw["a"], kw["a64"], kw["ha"], kw["wa"], kw["b"], kw["b64"], kw["hb"], kw["wb"], kw["batch"], kw["h"], kw["w"], kw["lo"],
                               kw["hi"], kw["out"], kw["split"], None)
        assert rc == -1 and word in L.rdm_last_error_string(), (change, rc, L.rdm_last_error_string())


def test_predict_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "--synthetic", "2"])
    assert a.png is False and a.png_range is None and a.png_with_input is False
    predict.check_png_args(a)
    a = P.parse_args(["--out", "d", "--synthetic", "2", "--png", "--png_range", "-1.5", "2", "--png_with_input"])
    assert a.png and a.png_range == [-1.5, 2.0] and a.png_with_input
    predict.check_png_args(a)
    for argv, word in ((["--png_range", "0", "1"], "need --png"), (["--png_with_input"], "need --png"), (["--png", "--png_range", "1", "1"], "LO < HI"),
                       (["--png", "--png_range", "2", "1"], "LO < HI"), (["--png", "--png_range", "nan", "1"], "LO < HI")):
        with pytest.raises(SystemExit) as e:
            predict.main(["--out", "d", "--synthetic", "2"] + argv)       # refused before anything touches a GPU
        assert word in str(e.value), (argv, e.value)
    with pytest.raises(SystemExit):
        P.parse_args(["--out", "d", "--png_range", "1"])
    text = P.format_help()
    assert "--png_range LO HI" in text and "--png_with_input" in text


def test_evaluate_flags():
    from md_rdm_amd import evaluate
    P = evaluate.build_parser()
    a = P.parse_args([])
    assert a.rows is None and a.rows_max == 16
    a = P.parse_args(["--rows", "out/rows", "--rows_max", "3"])
    assert a.rows == "out/rows" and a.rows_max == 3
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--synthetic", "2", "--rows", "d", "--rows_max", "-1"])
    assert "--rows_max" in str(e.value)
    assert "--rows DIR" in P.format_help()


def test_viz_module_does_not_import_the_oracle_and_refuses_the_cpu():
    import torch
    from md_rdm_amd import _lib, viz
    txt = open(os.path.join(ROOT, "md_rdm_amd", "viz.py")).read()
    assert "oracle" not in txt and re.search(r"^\s*(import|from)\s+(matplotlib|PIL)\b", txt, re.M) is None
    with pytest.raises(_lib.RdmError):
        viz.colorize(torch.zeros(1, 1, 4, 4))
    with pytest.raises(_lib.RdmError):
        viz.comparison_rows(torch.zeros(1, 3, 4, 4), None, torch.zeros(1, 1, 4, 4))
