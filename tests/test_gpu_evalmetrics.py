"""-m gpu: rdm_eval_target_metrics_f64 (csrc/evalmetrics.hip) through the C ABI - raw depth + predicted map -> one row of metric sums per
sample in one launch - against the composed path it fuses (harness.prepare_target -> harness.normalize -> rdm_depth_metrics_f64 per sample,
on the GPU) and against the CPU oracle (oracle.computations_cpu.resize / quick_gm / depth_metrics).

Which bound holds where (each comparison prints its observed figure before it asserts):
* geometric mean and normalised target vs the GPU composed path: EQUAL outright.  The kernel keeps k_gm_normalize's order of additions
  (csrc/evalmetrics.hip: four threads continue one column's sum in sequence, then the reduction of a four-wavefront workgroup), the resize
  and the mask are bit-exact, and the division is the same operation;
* the same two vs the CPU oracle: rtol 1e-13.  numpy sums the 16384 logarithms pairwise, in another order; the relative error of
  exp(e * S) is about eps * mean|log t| < 1e-14, 1e-13 leaves a decade.  target * gm (the resized and masked target the kernel formed, which
  does not depend on the prediction) is held to the oracle's at 2^-51: one rounding of the division and one of the product;
* the CPU-side masked target equals harness.prepare_target's bit for bit (the float32 `(y <= 0) + 1e-4` of module.py:75-78);
* metric sums vs rdm_depth_metrics_f64 per sample on the composed target, and vs oracle depth_metrics: rtol 1e-11, the project's bound for
  these sums in another order (tests/test_gpu_ops.py); the four counts EQUAL, under the precondition (asserted on the CPU first) that no
  pixel's max-ratio lies within 1e-9 relative of 1.25, 1.25^2, 1.25^3 - otherwise the next seed is taken, eight at the most.

Every case whose resize is a real resize asserts that the oracle's resize overshoots below zero next to the punched hole.  The identity case
(128x128 input) cannot: bicubic taps at scale 1 are (0, 1, 0, 0), the resize returns its input and a depth map with a hole of zeros has no
negative pixel; that case asserts the identity and the presence of zero (non-positive) pixels instead."""
import functools

import numpy as np
import pytest
import torch

from md_rdm_amd import filler
from oracle import computations_cpu as ocp

pytestmark = pytest.mark.gpu
NAMES = ("delta1", "delta2", "delta3", "mse", "mae", "log10", "absrel", "sqrel", "rmse")
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)
SHAPES = [(1, 226, 226), (3, 228, 304), (2, 128, 128), (2, 5, 7)]
CASES = [(B, H, W, dt, False) for (B, H, W) in SHAPES for dt in ("float32", "float64")] + [(1, 226, 226, "float32", True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_inputs(B, H, W, dtype, seed):
    """depth: filler.synthetic_batch with a rectangular hole of zeros punched into every sample; pred: a hash map over [-1, 2)."""
    y = filler.synthetic_batch(B, H, W, seed=seed)[1]
    r0, c0 = H // 4, W // 3
    y[:, :, r0:r0 + max(2, H // 5), c0:c0 + max(2, W // 4)] = 0.0
    if dtype == "float64":                                            # genuinely float64 data: bits below float32's last place
        y = y.astype(np.float64) * (1.0 + 2.0 ** -30)
    pred = filler.uniform("evalmetrics-pred/%d/%dx%dx%d" % (seed, B, H, W), (B, 1, 128, 128), -1.0, 2.0, dtype=np.float64)
    return np.ascontiguousarray(y), pred


def cpu_reference(depth, pred_eff):
    """Oracle side: resized map, masked target (module.py:75-78 with torch's dtypes), geometric mean, normalised target, max-ratio."""
    B = depth.shape[0]
    y = ocp.resize(depth.astype(np.float64), 128)
    m2 = (y <= 0).astype(np.float32) + np.float32(1e-4)              # a float32 tensor in torch: bool + Python scalar
    t = y * (y > 0) + m2.astype(np.float64)
    gm = ocp.quick_gm(t.reshape(B, -1, 1), 128).reshape(B)
    tn = t / gm.reshape(B, 1, 1, 1)
    p = np.maximum(pred_eff, 1e-7)
    ratio = np.maximum(p / tn, tn / p)
    return y, t, gm, tn, ratio


@functools.lru_cache(maxsize=None)
def case_data(B, H, W, dtype, exp_pred):
    """Inputs and the CPU reference of one case, computed once; the seed is the first of eight that satisfies the threshold precondition."""
    for seed in range(31, 39):
        depth, pred = make_inputs(B, H, W, dtype, seed)
        pred_eff = np.exp(pred) if exp_pred else pred
        y, t, gm, tn, ratio = cpu_reference(depth, pred_eff)
        near = min(float(np.abs(ratio / thr - 1.0).min()) for thr in THRESHOLDS)
        print("seed %d: closest max-ratio to a delta threshold, relative: %.3e" % (seed, near))
        if near > 1e-9:
            break
    else:
        raise AssertionError("no seed in 31..38 keeps every max-ratio 1e-9 away from the delta thresholds")
    assert (tn > 0).all() and float((pred < 1e-7).mean()) > 0.2       # the 1e-7 clamp is exercised on the log-domain map
    if (H, W) == (128, 128):
        assert np.array_equal(y, depth.astype(np.float64)) and (y == 0).any() and not (y < 0).any()
    else:
        print("resized map: %d negative pixels, minimum %.4f" % (int((y < 0).sum()), float(y.min())))
        assert (y < 0).any(), "no bicubic overshoot below zero next to the hole"
    return dict(depth=depth, pred=pred, pred_eff=pred_eff, y=y, t=t, gm=gm, tn=tn, ratio=ratio)


def fused(dev, depth, pred, exp_pred=False, want_target=True, want_gm=True):
    """rdm_eval_target_metrics_f64 -> (rc, rows, target or None, gm or None); outputs pre-filled with sentinels."""
    from md_rdm_amd import _lib
    d = depth if torch.is_tensor(depth) else torch.from_numpy(depth).to(dev)
    p = pred if torch.is_tensor(pred) else torch.from_numpy(pred).to(dev)
    B, _, H, W = d.shape
    rows = torch.full((B, 10), -777.0, dtype=torch.float64, device=dev)
    tgt = torch.full((B, 1, 128, 128), -777.0, dtype=torch.float64, device=dev) if want_target else None
    gm = torch.full((B,), -777.0, dtype=torch.float64, device=dev) if want_gm else None
    rc = _lib.lib().rdm_eval_target_metrics_f64(_lib.ptr(p), _lib.ptr(d), int(d.dtype == torch.float64), B, H, W, _lib.ptr(rows), _lib.ptr(tgt), _lib.ptr(gm),
                                                1 if exp_pred else 0, _lib.stream())
    torch.cuda.synchronize()
    return rc, rows, tgt, gm


def composed(dev, depth, pred_eff):
    """The path the kernel fuses, on the GPU: prepare_target -> quick_gm / normalize -> rdm_depth_metrics_f64 per sample."""
    from md_rdm_amd import _lib, harness
    from md_rdm_amd.network import computations as cp
    d, p = torch.from_numpy(depth).to(dev), torch.from_numpy(pred_eff).to(dev)
    B = d.shape[0]
    t = harness.prepare_target(d)
    gm = cp.quick_gm(t.reshape(B, -1, 1), 128).reshape(B)
    tn = harness.normalize(t)
    rows = torch.empty(B, 10, dtype=torch.float64, device=dev)
    for b in range(B):
        _lib.check(_lib.lib().rdm_depth_metrics_f64(_lib.ptr(p[b].contiguous()), _lib.ptr(tn[b].contiguous()), 128 * 128, _lib.ptr(rows[b]), _lib.stream()))
    torch.cuda.synchronize()
    return t, gm, tn, rows


@pytest.mark.parametrize("B,H,W,dtype,exp_pred", CASES)
def test_fused_vs_composed_and_oracle(dev, B, H, W, dtype, exp_pred):
    c = case_data(B, H, W, dtype, exp_pred)
    rc, rows, tgt, gm = fused(dev, c["depth"], c["pred"], exp_pred=exp_pred)
    assert rc == 0
    rows, tgt, gm = rows.cpu().numpy(), tgt.cpu().numpy(), gm.cpu().numpy()
    assert not (rows == -777.0).any() and not (tgt == -777.0).any() and not (gm == -777.0).any()
    t_c, gm_c, tn_c, rows_c = composed(dev, c["depth"], c["pred_eff"])
    t_c, gm_c, tn_c, rows_c = t_c.cpu().numpy(), gm_c.cpu().numpy(), tn_c.cpu().numpy(), rows_c.cpu().numpy()

    # target side: EQUAL to the composed GPU path (the kernel keeps k_gm_normalize's summation order)
    print("gm: fused %s, composed %s, oracle %s" % (gm, gm_c, c["gm"]))
    print("target vs composed: max |diff| = %.3e" % np.abs(tgt - tn_c).max())
    np.testing.assert_array_equal(gm, gm_c)
    np.testing.assert_array_equal(tgt, tn_c)
    np.testing.assert_array_equal(c["t"], t_c)                       # oracle-side mask == prepare_target, bit for bit
    # ... and the CPU oracle (pairwise numpy sum: another order)
    print("gm vs oracle: max rel = %.3e; target vs oracle: max rel = %.3e; target * gm vs oracle masked target: max rel = %.3e"
          % (np.abs(gm / c["gm"] - 1).max(), np.abs(tgt / c["tn"] - 1).max(), np.abs(tgt * gm.reshape(B, 1, 1, 1) / c["t"] - 1).max()))
    np.testing.assert_allclose(gm, c["gm"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(tgt, c["tn"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(tgt * gm.reshape(B, 1, 1, 1), c["t"], rtol=2.0 ** -51, atol=0)

    # rows: counts equal, sums at the project's 1e-11
    print("rows vs rdm_depth_metrics_f64 per sample: max rel = %.3e" % np.abs(rows[:, 4:] / rows_c[:, 4:] - 1).max())
    np.testing.assert_array_equal(rows[:, :4], rows_c[:, :4])
    np.testing.assert_allclose(rows[:, 4:], rows_c[:, 4:], rtol=1e-11, atol=0)
    for b in range(B):
        assert rows[b, 0] == 128 * 128
        for k, thr in enumerate(THRESHOLDS):
            assert rows[b, 1 + k] == int((c["ratio"][b] < thr).sum()), (b, k)
        ref = np.array(ocp.depth_metrics(c["pred_eff"][b], c["tn"][b], NAMES))
        got = np.array([float(np.float32(rows[b, 1 + k]) / np.float32(rows[b, 0])) for k in range(3)] + [rows[b, 4 + k] / rows[b, 0] for k in range(6)])
        print("sample %d values vs oracle depth_metrics: max rel = %.3e" % (b, np.abs(got / ref - 1).max()))
        np.testing.assert_array_equal(got[:3], ref[:3])
        np.testing.assert_allclose(got[3:], ref[3:], rtol=1e-11, atol=0)


def test_repeated_call_is_bit_identical_and_optional_outputs_may_be_null(dev):
    c = case_data(3, 228, 304, "float32", False)
    rc, rows, tgt, gm = fused(dev, c["depth"], c["pred"])
    rc2, rows2, tgt2, gm2 = fused(dev, c["depth"], c["pred"])
    assert rc == 0 and rc2 == 0
    assert torch.equal(rows, rows2) and torch.equal(tgt, tgt2) and torch.equal(gm, gm2)
    rc3, rows3, tgt3, gm3 = fused(dev, c["depth"], c["pred"], want_target=False, want_gm=False)
    assert rc3 == 0 and tgt3 is None and gm3 is None and torch.equal(rows3, rows)


def test_a_sample_scores_the_same_alone_as_in_a_batch(dev):
    c = case_data(3, 228, 304, "float32", False)
    d, p = torch.from_numpy(c["depth"]).to(dev), torch.from_numpy(c["pred"]).to(dev)
    rc, rows, tgt, gm = fused(dev, d, p)
    assert rc == 0
    for b in range(3):
        rc1, r1, t1, g1 = fused(dev, d[b:b + 1].contiguous(), p[b:b + 1].contiguous())
        assert rc1 == 0
        assert torch.equal(r1[0], rows[b]) and torch.equal(t1[0], tgt[b]) and torch.equal(g1[0], gm[b]), b


def test_bad_arguments_are_status_codes(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    p = torch.zeros(1, 1, 128, 128, dtype=torch.float64, device=dev)
    d = torch.ones(1, 1, 8, 8, dtype=torch.float32, device=dev)
    rows = torch.full((1, 10), -777.0, dtype=torch.float64, device=dev)
    assert L.rdm_eval_target_metrics_f64(_lib.ptr(p), _lib.ptr(d), 0, 1, 8, 8, None, None, None, 0, _lib.stream()) == -1
    assert b"eval_target_metrics" in L.rdm_last_error_string() and b"NULL" in L.rdm_last_error_string()
    assert L.rdm_eval_target_metrics_f64(_lib.ptr(p), _lib.ptr(d), 0, 1, 0, 8, _lib.ptr(rows), None, None, 0, _lib.stream()) == -1
    assert b"eval_target_metrics" in L.rdm_last_error_string() and b"h, w > 0" in L.rdm_last_error_string()
    assert L.rdm_eval_target_metrics_f64(_lib.ptr(p), _lib.ptr(d), 0, 1, 8, 8, _lib.ptr(rows), None, None, 2, _lib.stream()) == -1      # unknown flag
    torch.cuda.synchronize()
    assert bool((rows == -777.0).all())
