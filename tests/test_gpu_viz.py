"""rdm_viz_rows_u8 (include/rdm_viz.h) and md_rdm_amd.viz on the MI355X, byte for byte against the reference-generated fixture
(tests/golden/viz_goldens.npz) and its numpy restatement (tests/viz_ref.py).  Every comparison is assert_array_equal on uint8: the resize is
bit-exact already, and what follows is two subtractions, one division and a product with a power of two in IEEE float64."""
import os

import numpy as np
import pytest
import torch

import stream_probe as sp
import viz_ref
from md_rdm_amd import filler
from test_viz_cpu import _decode, rows_input, rows_maps

pytestmark = pytest.mark.gpu
LU = filler.log_uniform
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return viz_ref.gold()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def eq(got, want):
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


def raw(dev, b, h, w, lo=NAN, hi=NAN, rgb=None, a=None, split=0, out=None):
    """the entry point itself -> (status, out)"""
    from md_rdm_amd import _lib
    panels = (rgb is not None) + (a is not None) + 1
    if out is None:
        out = torch.full((b.shape[0], h, panels * w, 3), 0xEE, dtype=torch.uint8, device=dev)
    ha, wa = (a.shape[2], a.shape[3]) if a is not None else (0, 0)
    rc = _lib.lib().rdm_viz_rows_u8(_lib.ptr(rgb), _lib.ptr(a), int(a is not None and a.dtype == torch.float64), ha, wa, _lib.ptr(b), int(b.dtype == torch.float64),
                                    b.shape[2], b.shape[3], b.shape[0], h, w, lo, hi, _lib.ptr(out), split, _lib.stream())
    return rc, out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_no_resize_automatic_range_per_image(dev, gold, dtype):
    from md_rdm_amd import viz
    m = LU("viz.own", (3, 1, 5, 7), 0.5, 9.5).astype(dtype)
    m[1] *= 3.0                                                      # the images have different ranges
    m[2] -= 4.0
    got = viz.colorize(T(m, dev)).cpu().numpy()
    eq(torch.from_numpy(got), viz_ref.colorize(m))
    for i in range(3):
        y, x = np.unravel_index(np.argmax(m[i, 0]), (5, 7))
        assert got[i, y, x].tolist() == gold["lut8"][255].tolist()  # the maximum maps to index 255
        y, x = np.unravel_index(np.argmin(m[i, 0]), (5, 7))
        assert got[i, y, x].tolist() == gold["lut8"][0].tolist()
    assert not np.array_equal(got[0], viz_ref.colorize(m[:1], d_min=float(m[1].min()), d_max=float(m[1].max()))[0])   # image 1's range is not image 0's


def test_fixed_range_bin_edges(dev, gold):
    from md_rdm_amd import viz
    k = (np.arange(257) / 256.0).reshape(1, 1, 1, 257)
    eq(viz.colorize(T(k, dev), 0.0, 1.0), gold["lut8"][np.minimum(np.arange(257), 255)].reshape(1, 1, 257, 3))


def test_fixed_range_clamps_and_nan_pixel(dev, gold):
    from md_rdm_amd import viz
    m = LU("viz.clamp", (2, 1, 6, 9), 0.5, 9.5).astype(np.float64)
    m[0, 0, 0, 0], m[0, 0, 5, 8], m[1, 0, 2, 3] = -3.0, 1e9, 2.0 - 1e-12
    want = viz_ref.colorize(m, d_min=2.0, d_max=7.0)
    assert want[0, 0, 0].tolist() == gold["lut8"][0].tolist() and want[0, 5, 8].tolist() == gold["lut8"][255].tolist()
    eq(viz.colorize(T(m, dev), 2.0, 7.0), want)
    m[1, 0, 4, 4] = np.nan                                           # black there, nothing else changes (the map is read as it is: no resize taps)
    want[1, 4, 4] = 0
    eq(viz.colorize(T(m, dev), 2.0, 7.0), want)


def test_nan_pixel_under_an_automatic_range_blackens_that_image(dev):
    from md_rdm_amd import viz
    m = LU("viz.nanauto", (2, 1, 6, 8), 0.5, 9.5)
    want = viz_ref.colorize(m)
    m[1, 0, 3, 3] = np.nan
    want[1] = 0
    assert want[0].any()
    eq(viz.colorize(T(m, dev)), want)
    half = viz_ref.colorize(m, d_max=5.0)                            # one end fixed: the other is still NaN for image 1
    assert not half[1].any()
    eq(viz.colorize(T(m, dev), None, 5.0), half)


def test_constant_image_is_black(dev):
    from md_rdm_amd import viz
    m = np.full((2, 1, 4, 8), 2.5, dtype=np.float32)
    m[1, 0, 0, 0] = 3.0
    want = viz_ref.colorize(m)
    assert not want[0].any() and want[1].any()
    eq(viz.colorize(T(m, dev)), want)


@pytest.mark.parametrize("key,shape,lo,hi,size,name", [("viz.m128", (2, 1, 128, 128), 0.5, 9.5, (37, 53), "cd_37x53"), ("viz.m8", (2, 1, 8, 8), 0.5, 2.0, (16, 16), "cd_16x16")])
def test_resize_against_the_reference_fixture(dev, gold, key, shape, lo, hi, size, name):
    from md_rdm_amd import viz
    m = LU(key, shape, lo, hi)
    eq(viz.colorize(T(m, dev), size=size), gold[name])
    eq(viz.colorize(T(m.astype(np.float64), dev), size=size), gold[name])


def test_resize_to_full_resolution(dev):
    from md_rdm_amd import viz
    m = LU("viz.m128", (2, 1, 128, 128), 0.5, 9.5)
    eq(viz.colorize(T(m, dev), size=(480, 640)), viz_ref.colorize(m, (480, 640)))


def test_rows_share_one_range(dev, gold):
    from md_rdm_amd import viz
    t, p = rows_maps()
    x = rows_input()
    eq(viz.comparison_rows(T(x, dev), T(t, dev), T(p, dev)), gold["rows_23x31"])
    eq(viz.comparison_rows(T(x, dev), T(t.astype(np.float64), dev), T(p, dev)), gold["rows_23x31"])
    two = np.concatenate([gold["rows_23x31"][:, :, :31], gold["rows_pred_23x31"]], axis=2)
    eq(viz.comparison_rows(T(x, dev), None, T(p, dev)), two)
    assert not np.array_equal(gold["rows_23x31"][:, :, 62:], gold["rows_pred_23x31"])          # the shared range differs from the prediction's own
    eq(viz.comparison_rows(T(x, dev), T(t, dev), T(p, dev), 1.0, 3.0), viz_ref.rows(x, t, p, (23, 31), 1.0, 3.0))


def test_split_does_not_change_the_bytes_and_nothing_lands_outside(dev):
    t, p = rows_maps()
    x, t, p = T(rows_input(), dev), T(t, dev), T(p, dev)
    n = 2 * 23 * 93 * 3
    want = None
    for split in (0, 1, 2, 4, 23, 500):
        for off in (0, 1, 3):                                        # every alignment of out; canaries on both sides
            buf = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device=dev)
            out = buf[32 + off:32 + off + n].view(2, 23, 93, 3)
            rc, _ = raw(dev, p, 23, 31, rgb=x, a=t, split=split, out=out)
            assert rc == 0
            got = buf.cpu().numpy()
            assert (got[:32 + off] == 0xEE).all() and (got[32 + off + n:] == 0xEE).all(), (split, off)
            if want is None:
                want = got[32:32 + n].copy()
                np.testing.assert_array_equal(want.reshape(2, 23, 93, 3), viz_ref.gold()["rows_23x31"])
            np.testing.assert_array_equal(got[32 + off:32 + off + n], want, err_msg="split %d, offset %d" % (split, off))


def test_wide_rows_cross_tiles(dev):
    """more than one 256-column tile per row, a ragged last tile, rows that start at every byte alignment"""
    from md_rdm_amd import viz
    m = LU("viz.wide", (1, 1, 9, 40), 0.5, 9.5)
    eq(viz.colorize(T(m, dev), size=(11, 601)), viz_ref.colorize(m, (11, 601)))


def test_bad_arguments_write_nothing(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    b = T(LU("viz.bad", (1, 1, 8, 8), 0.5, 2.0), dev)
    out = torch.full((1, 8, 8, 3), 0xEE, dtype=torch.uint8, device=dev)
    P, st = _lib.ptr, _lib.stream()
    calls = [
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, None, 0, 8, 8, 1, 8, 8, NAN, NAN, P(out), 0, st), b"NULL"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 8, 8, 1, 8, 8, NAN, NAN, None, 0, st), b"NULL"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 8, 8, 0, 8, 8, NAN, NAN, P(out), 0, st), b"batch"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 8, 8, 1, 0, 8, NAN, NAN, P(out), 0, st), b"batch"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 8, 8, 1, 8, -8, NAN, NAN, P(out), 0, st), b"batch"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 0, 8, 1, 8, 8, NAN, NAN, P(out), 0, st), b"map sizes"),
        (lambda: L.rdm_viz_rows_u8(None, P(b), 0, 8, 0, P(b), 0, 8, 8, 1, 8, 8, NAN, NAN, P(out), 0, st), b"map sizes"),
        (lambda: L.rdm_viz_rows_u8(None, None, 0, 0, 0, P(b), 0, 8, 8, 1, 8, 8, NAN, NAN, P(out), -2, st), b"split"),
    ]
    for call, word in calls:
        assert call() == -1
        assert word in L.rdm_last_error_string(), L.rdm_last_error_string()
    torch.cuda.synchronize()
    assert bool((out == 0xEE).all())
    with pytest.raises(_lib.RdmError):
        from md_rdm_amd import viz
        viz.colorize(b.cpu())


# ---- the stream argument: tests/stream_probe.py's late producer, with the null-stream control -----------------------------------------------
def stream_inputs():
    """the rows case, with the 17 input values 238 / 255 moved to 237 / 255: stream_probe's poison for uint8 is the byte 0xEE (238), and its control
    only counts an output as poisoned where the reference holds no such byte.  The jet table has none, so the input panel is the only source."""
    x = rows_input()
    x[x == np.float32(238.0 / 255.0)] = np.float32(237.0 / 255.0)
    t, p = rows_maps()
    return x, t, p


@pytest.fixture(scope="module")
def stream_want(gold):
    want = viz_ref.rows(*stream_inputs(), (23, 31))
    assert not (want == 0xEE).any() and not (gold["lut8"] == 0xEE).any()
    differs = want != gold["rows_23x31"]
    assert differs.sum() == 17 and (gold["rows_23x31"][differs] == 238).all() and (want[differs] == 237).all()    # every other byte is the reference-generated fixture's
    return want


def stream_case(dev):
    from md_rdm_amd import viz
    x, t, p = stream_inputs()
    ins = dict(x=T(x, dev), t=T(t, dev), p=T(p, dev))
    out = torch.empty(2, 23, 93, 3, dtype=torch.uint8, device=dev)

    def call(b, st):
        from md_rdm_amd import _lib
        _lib.check(_lib.lib().rdm_viz_rows_u8(_lib.ptr(b["x"]), _lib.ptr(b["t"]), 0, 57, 76, _lib.ptr(b["p"]), 0, 16, 16, 2, 23, 31, NAN, NAN, _lib.ptr(b["out"]), 0, st))
        return dict(wrapped=viz.comparison_rows(b["x"], b["t"], b["p"]))           # the product wrapper resolves the caller's stream itself
    return sp.Case(ins, call, outs=("out",), scratch=dict(out=out))


@pytest.fixture(scope="module")
def delay(dev):
    return sp.Delay(dev)


def test_call_on_a_late_non_default_stream(dev, delay, stream_want):
    ref = sp.check(stream_case(dev), delay)
    eq(ref["out"], stream_want)
    eq(ref["wrapped"], stream_want)


def test_control_call_on_the_null_stream_is_detected(dev, delay, stream_want):
    sp.control(stream_case(dev), delay)


# ---- the commands -----------------------------------------------------------------------------------------------------------------------------
def test_predict_png(dev, tmp_path):
    from md_rdm_amd import predict, viz
    out = tmp_path / "maps"
    assert predict.main(["--synthetic", "2", "--batch_size", "2", "--out", str(out), "--png"]) == 0
    assert sorted(os.listdir(out)) == ["synthetic_0000.npy", "synthetic_0000.png", "synthetic_0001.npy", "synthetic_0001.png"]
    maps = np.stack([np.load(out / ("synthetic_%04d.npy" % i)) for i in range(2)])
    want = viz.colorize(T(maps, dev)).cpu().numpy()
    assert want.shape == (2, 128, 128, 3) and want.any()
    for i in range(2):
        np.testing.assert_array_equal(_decode(str(out / ("synthetic_%04d.png" % i))), want[i])
    np.testing.assert_array_equal(want, viz_ref.colorize(maps))
    # fixed range, linear map, the input beside it
    out2 = tmp_path / "maps2"
    assert predict.main(["--synthetic", "2", "--batch_size", "2", "--out", str(out2), "--linear", "--png", "--png_range", "0.5", "2", "--png_with_input"]) == 0
    lin = np.stack([np.load(out2 / ("synthetic_%04d.npy" % i)) for i in range(2)])
    assert lin.dtype == np.float32
    x = filler.synthetic_batch(2, 226, 226)[0]
    want = viz.comparison_rows(T(x, dev), None, T(lin, dev), 0.5, 2.0).cpu().numpy()
    assert want.shape == (2, 226, 452, 3)
    for i in range(2):
        np.testing.assert_array_equal(_decode(str(out2 / ("synthetic_%04d.png" % i))), want[i])


def test_evaluate_rows(dev, tmp_path, monkeypatch):
    from md_rdm_amd import evaluate, harness, viz
    from md_rdm_amd.metrics import MetricComputation
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rows_dir = tmp_path / "rows"
    assert evaluate.main(["--synthetic", "3", "--batch_size", "2", "--rows", str(rows_dir), "--rows_max", "3", "--metrics", "delta1", "rmse"]) == 0
    assert sorted(os.listdir(rows_dir)) == ["row_%05d.png" % i for i in range(3)]
    model = DepthEstimationNet()
    filler.fill_state_dict(model.state_dict())
    model = model.to(dev).eval()
    xs, ys = evaluate.synthetic_samples(3, 226, 226)
    x, y = T(xs, dev), T(ys, dev)
    mc = MetricComputation(["delta1", "rmse"])
    got = []
    res, maps = harness.evaluate(model, [(x[:2], y[:2]), (x[2:], y[2:])], mc, return_maps=True, rows_out=got, rows_max=3)
    assert res["n"] == 3 and len(got) == 3
    for lo in (0, 2):                                                # batch by batch, as the maps were made
        tgt = torch.empty_like(maps[lo:lo + 2])
        mc.compute_rows(maps[lo:lo + 2], y[lo:lo + 2], target_out=tgt)
        want = viz.comparison_rows(x[lo:lo + 2], tgt, maps[lo:lo + 2]).cpu().numpy()
        for i in range(want.shape[0]):
            assert want[i].shape == (226, 678, 3)
            np.testing.assert_array_equal(got[lo + i], want[i])
            np.testing.assert_array_equal(_decode(str(rows_dir / ("row_%05d.png" % (lo + i)))), want[i])
    capped = []
    harness.evaluate(model, [(x[:2], y[:2]), (x[2:], y[2:])], mc, exp_pred=True, rows_out=capped, rows_max=1)
    assert len(capped) == 1
    tgt = torch.empty_like(maps[:2])
    mc.compute_rows(maps[:2], y[:2], target_out=tgt)
    np.testing.assert_array_equal(capped[0], viz.comparison_rows(x[:1], tgt[:1], maps[:1].exp()).cpu().numpy()[0])
