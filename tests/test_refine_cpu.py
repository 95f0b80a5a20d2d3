"""Guided depth refinement without a GPU: properties of the numpy statement of include/rdm_refine.h (tests/refine_ref.py), the rules of the
command-line flags and of refine.joint_bilateral's arguments, and the C-ABI boundary of include/rdm_refine.h (declared == bound == exported, not
in rdm_hip.h; every bad argument a status code with a message, before any device call)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import refine_ref as rref
from conftest import ROOT
from md_rdm_amd import filler

INF = math.inf


def frame(key, h, w, holes=0.3):
    d = filler.uniform("refine.cpu.depth/" + key, (h, w), 0.5, 9.5).astype(np.float32)
    d[filler.unit("refine.cpu.mask/" + key, h * w).reshape(h, w) < holes] = 0.0
    g = (filler.unit("refine.cpu.rgb/" + key, h * w * 3) * 256.0).astype(np.uint8).reshape(h, w, 3)
    return d, g


# ---- the numpy statement of the contract ----------------------------------------------------------------------------------------------------
def test_tables():
    ws, E = rref.tables(3, 4, 6.0, 12.0)
    assert ws.shape == (4,) and E.shape == (256,) and ws[0] == 1.0 and E[0] == 1.0
    assert abs(ws[2] - math.exp(-64.0 / 72.0)) <= 2e-16 and abs(E[12] - math.exp(-0.5)) <= 2e-16      # numpy's exp may differ from libm's in the last bit
    assert (np.diff(ws) < 0).all() and (np.diff(E[:60]) < 0).all()
    ws, E = rref.tables(8, 3, INF, INF)
    assert (ws == 1.0).all() and (E == 1.0).all()
    ws, E = rref.tables(2, 1, 1e-200, 1e-200)                    # sigma^2 underflows to 0: entry 0 is still 1, the rest 0
    assert ws.tolist() == [1.0, 0.0, 0.0] and E[0] == 1.0 and (E[1:] == 0.0).all()


def test_tiny_sigma_color_is_the_identity_on_valid_pixels():
    h, w = 13, 17
    d, _ = frame("identity", h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.stack([yy * 7 % 256, xx * 11 % 256, (yy * w + xx) % 256], axis=-1).astype(np.uint8)      # (y, x) -> colour is injective here
    assert len({tuple(c) for c in g.reshape(-1, 3).tolist()}) == h * w
    for fill in (False, True):
        r = rref.sample(d, g, 3, 2, 3.0, 1e-3, fill, 1e-3)
        v = rref.valid_mask(d)
        np.testing.assert_array_equal(r["f32"][v], d[v])        # only the pixel's own tap has a weight: D = (1 * d) / 1
        assert (r["f32"][~v] == 0).all() and (r["u16"][~v] == 0).all() and (r["ok"] == v).all()      # and nothing can fill a hole
        np.testing.assert_array_equal(r["u16"][v], np.rint(d[v].astype(np.float64) / 1e-3).astype(np.uint16))


def test_constant_guide_and_infinite_sigmas_give_the_mean_of_the_valid_taps():
    h, w, radius, step = 9, 12, 2, 3
    d = (filler.unit("refine.cpu.mean", h * w).reshape(h, w) * 8.0).astype(np.int64).astype(np.float32)       # small integers: exact sums
    g = np.full((h, w, 3), 77, dtype=np.uint8)
    r = rref.sample(d, g, radius, step, INF, INF, True, 1e-3)
    v = d > 0
    assert (~v).sum() > 5
    for y in range(h):
        for x in range(w):
            taps = [d[y + j * step, x + i * step] for j in range(-radius, radius + 1) for i in range(-radius, radius + 1)
                    if 0 <= y + j * step < h and 0 <= x + i * step < w and v[y + j * step, x + i * step]]       # outside the frame: skipped, not clamped
            if taps:
                assert r["ok"][y, x] and r["den"][y, x] == len(taps) and r["D"][y, x] == np.float64(sum(taps)) / len(taps), (y, x)
            else:
                assert not r["ok"][y, x] and r["f32"][y, x] == 0
    clamped = np.pad(d, radius * step, mode="edge")              # a clamping filter would see the corner value several times
    assert clamped[0, 0] == d[0, 0] and r["den"][0, 0] <= (radius + 1) ** 2


def test_fill_keeps_or_fills_exactly_the_pixels_with_a_valid_tap():
    h, w = 20, 23
    d, g = frame("fill", h, w, holes=0.0)
    d[3:15, 4:19] = 0.0                                          # a hole wider than the reach of the filter: its middle has no valid tap
    d[0, 0], d[1, 1], d[2, 2] = np.nan, np.inf, -1.0
    v = rref.valid_mask(d)
    keep = rref.sample(d, g, 1, 2, INF, INF, False, 1e-3)
    assert (keep["ok"] == v).all() and (keep["f32"][~v] == 0).all() and (keep["u16"][~v] == 0).all()
    full = rref.sample(d, g, 1, 2, INF, INF, True, 1e-3)
    reach = np.zeros((h, w), dtype=bool)
    pv = np.pad(v, 2)
    for j in (-2, 0, 2):
        for i in (-2, 0, 2):
            reach |= pv[2 + j:2 + j + h, 2 + i:2 + i + w]
    assert (full["ok"] == (v | reach)).all() and (~full["ok"]).sum() == 8 * 11 and full["ok"][0, 0] and full["ok"][2, 2]
    np.testing.assert_array_equal(full["f32"][v], keep["f32"][v])            # fill changes nothing at valid pixels
    assert (full["f32"][full["ok"]] > 0).all() and np.isfinite(full["f32"]).all()


def test_taps_outside_the_frame_are_skipped():
    d = np.array([[4.0, 1.0, 1.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    g = np.zeros((2, 3, 3), dtype=np.uint8)
    r = rref.sample(d, g, 1, 1, INF, INF, False, 1e-3)
    assert r["den"].tolist() == [[4.0, 6.0, 4.0], [4.0, 6.0, 4.0]]
    assert r["D"][0, 0] == 7.0 / 4.0 and r["D"][0, 2] == 1.0                  # clamped taps would weigh the corner's 4.0 four times
    r = rref.sample(d, g, 1, 2, INF, INF, False, 1e-3)                       # step 2: only (y, x +- 2) is in the frame
    assert r["den"].tolist() == [[2.0, 1.0, 2.0], [2.0, 1.0, 2.0]] and r["D"][0, 0] == 2.5


def test_quantisation_rule():
    u, q = rref.quantise(np.array([0.0012, 65.5349, 65.5351, 70.0, np.nan, 1.0]), 1e-3, np.array([True] * 5 + [False]))
    assert u.tolist() == [1, 65535, 65535, 65535, 0, 0] and q[3] == 70.0 / 1e-3                  # a pixel that is not ok is 0 whatever its D
    u, _ = rref.quantise(np.array([0.5, 1.5, 2.5, 65534.5, 65535.0, 1e9]), 1.0, np.ones(6, bool))
    assert u.tolist() == [0, 2, 2, 65534, 65535, 65535]                      # ties to even; saturation


# ---- joint_bilateral's arguments and the command's rules: refused before anything touches a GPU ---------------------------------------------
def test_host_tensors_and_bad_parameters_are_refused():
    from md_rdm_amd import _lib, refine
    with pytest.raises(_lib.RdmError, match="no CPU fallback"):
        refine.joint_bilateral(torch.ones(1, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(_lib.RdmError):
        refine.joint_bilateral(np.ones((1, 4, 4), np.float32), np.zeros((1, 4, 4, 3), np.uint8))
    assert refine.DEFAULTS == dict(radius=3, step=4, sigma_space=None, sigma_color=12.0, fill=False)
    assert refine.check_params(3, 4, None, 12.0) is None and refine.check_params(8, 3, INF, INF) is None and refine.check_params(2, 12, 0.1, 1e-3) is None
    assert refine.check_params(1, 16, None, 1.0) is None
    for bad, word in (((0, 4, None, 12.0), "radius"), ((9, 1, None, 12.0), "radius"), ((3, 0, None, 12.0), "step"), ((1, 17, None, 12.0), "step"),
                      ((5, 5, None, 12.0), "radius * step"), ((3, 4, 0.0, 12.0), "sigma_space"), ((3, 4, -1.0, 12.0), "sigma_space"),
                      ((3, 4, math.nan, 12.0), "sigma_space"), ((3, 4, None, 0.0), "sigma_color"), ((3, 4, None, math.nan), "sigma_color")):
        assert word in refine.check_params(*bad), bad
    text = refine.__doc__ + refine.joint_bilateral.__doc__
    assert "not been measured" in refine.joint_bilateral.__doc__ and "NOT been measured" in refine.__doc__, text


def test_predict_refine_flags():
    from md_rdm_amd import predict
    P = predict.build_parser()
    a = P.parse_args(["--out", "d", "f.npy"])
    assert (a.refine, a.refine_radius, a.refine_step, a.refine_sigma_space, a.refine_sigma_color, a.refine_fill) == (False, None, None, None, None, False)
    predict.check_refine_args(a)
    assert predict.refine_options(a) is None
    a = P.parse_args(["--out", "d", "f.npy", "--metric", "--native", "--refine"])
    predict.check_refine_args(a)
    assert predict.refine_options(a) == {"fill": False}
    a = P.parse_args(["--out", "d", "f.npy", "--metric", "--native", "--refine", "--refine_radius", "8", "--refine_step", "3", "--refine_sigma_space", "inf",
                      "--refine_sigma_color", "7.5", "--refine_fill"])
    predict.check_refine_args(a)
    assert predict.refine_options(a) == {"radius": 8, "step": 3, "sigma_space": INF, "sigma_color": 7.5, "fill": True}
    files, syn = ["--out", "d", "f.npy"], ["--out", "d", "--synthetic", "2"]
    on = files + ["--metric", "--native", "--refine"]
    for argv, word in ((files + ["--refine"], "--refine needs --metric --native"), (files + ["--metric", "--refine"], "--refine needs --metric --native"),
                       (syn + ["--metric", "--refine"], "--refine needs --metric --native"), (files + ["--metric", "--native", "--refine_radius", "2"], "need --refine"),
                       (files + ["--metric", "--native", "--refine_step", "2"], "need --refine"), (files + ["--metric", "--native", "--refine_sigma_space", "2"], "need --refine"),
                       (files + ["--metric", "--native", "--refine_sigma_color", "2"], "need --refine"), (files + ["--metric", "--native", "--refine_fill"], "need --refine"),
                       (on + ["--refine_radius", "0"], "radius"), (on + ["--refine_radius", "9", "--refine_step", "1"], "radius"), (on + ["--refine_step", "0"], "step"),
                       (on + ["--refine_step", "17", "--refine_radius", "1"], "step"), (on + ["--refine_step", "9"], "radius * step"),
                       (on + ["--refine_radius", "7"], "radius * step"), (on + ["--refine_sigma_space", "0"], "sigma_space"), (on + ["--refine_sigma_space", "nan"], "sigma_space"),
                       (on + ["--refine_sigma_color", "-1"], "sigma_color"), (on + ["--refine_sigma_color", "nan"], "sigma_color")):
        with pytest.raises(SystemExit) as e:
            predict.main(argv)
        assert word in str(e.value), (argv, e.value)
    text = P.format_help()
    for flag in ("--refine", "--refine_radius R", "--refine_step S", "--refine_sigma_space F", "--refine_sigma_color F", "--refine_fill"):
        assert flag in text, flag
    assert "filled from inside it" in " ".join(text.split())
    assert "--refine" in predict.__doc__ and "--metric --native --refine --png16 --ply" in predict.__doc__


# ---- the C ABI of include/rdm_refine.h ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_refine.h")) == {"rdm_depth_refine"}     # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    assert "rdm_depth_refine" not in hip_h and "rdm_refine.h" not in hip_h


def test_bad_arguments_are_status_codes_before_any_device_call(L):
    """Made-up pointers only: every refusal comes from the launcher's own checks, which precede the launch (this machine has no device to call)."""
    nan, inf = float("nan"), float("inf")
    P, Q, R = C.c_void_p(256), C.c_void_p(512), C.c_void_p(1024)
    # positions: 0 depth, 1 guide, 2 batch, 3 h, 4 w, 5 radius, 6 step, 7 sigma_space, 8 sigma_color, 9 fill, 10 unit, 11 out_f32, 12 out_u16, 13 stream
    good = [P, Q, 1, 4, 6, 3, 4, 6.0, 12.0, 0, 1e-3, R, None, None]
    bad = [({0: None}, b"depth"), ({1: None}, b"guide"), ({11: None}, b"both be NULL"), ({11: P}, b"in place"), ({11: P, 12: R}, b"in place"),
           ({2: 0}, b"batch"), ({2: -1}, b"batch"), ({3: 0}, b"h"), ({4: -2}, b"w"), ({2: 65536}, b"65535"), ({3: 65536, 4: 32768}, b"h * w"),
           ({5: 0}, b"radius"), ({5: -1}, b"radius"), ({5: 9, 6: 1}, b"radius"), ({6: 0}, b"step"), ({6: 17, 5: 1}, b"step"), ({5: 5, 6: 5}, b"radius * step"),
           ({5: 8, 6: 4}, b"radius * step"), ({5: 2, 6: 13}, b"radius * step"), ({7: 0.0}, b"sigma_space"), ({7: -1.0}, b"sigma_space"), ({7: nan}, b"sigma_space"),
           ({7: -inf}, b"sigma_space"), ({8: 0.0}, b"sigma_color"), ({8: -2.0}, b"sigma_color"), ({8: nan}, b"sigma_color"), ({9: 2}, b"fill"), ({9: -1}, b"fill"),
           ({10: 0.0}, b"unit"), ({10: -1e-3}, b"unit"), ({10: nan}, b"unit"), ({10: inf}, b"unit")]
    for argv, word in bad:
        args = list(good)
        for pos, val in argv.items():
            args[pos] = val
        rc = L.rdm_depth_refine(*args)
        assert rc == -1 and word in L.rdm_last_error_string(), (argv, rc, L.rdm_last_error_string())
