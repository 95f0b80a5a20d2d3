"""-m gpu: the predict path - rdm_predict_tail_f32 (csrc/predict.hip: d_1 logits -> log depth map in one launch), DepthEstimationNet.predict
and `python -m md_rdm_amd.predict`.

Criterion everywhere a map is compared: the project's 1e-4, element-wise on every element, atol = 1e-4 * max|ref| (as tests/test_gpu_net.py
asserts it); DORN counts are compared exactly.  Each comparison prints its observed maximum difference before it asserts."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from md_rdm_amd import filler
from oracle import computations_cpu as ocp

pytestmark = pytest.mark.gpu
REL = 1e-4
SEED = filler.MARGIN_SEEDS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def make_model(dev, relative_decoders=(), deterministic=True):
    """As tests/test_gpu_net.py builds it (hash-filled), eval mode; ordered reductions so that two forwards of one input give the same logits."""
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=relative_decoders)
    m.deterministic = deterministic
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model(dev):
    return make_model(dev)


def level_weights(m, n):
    return torch.cat([m.weight_layer.get(k).detach().reshape(-1)[:1].float() for k in range(n + 1)]).contiguous()


def tail(logits, wv, n_out=7, split=0, want_decode=True, want_linear=True):
    """rdm_predict_tail_f32 -> (rc, log map, decode or None, linear map or None); the outputs are pre-filled with sentinels."""
    from md_rdm_amd import _lib
    B, C2, h, w = logits.shape
    S = 1 << n_out
    out = torch.full((B, 1, S, S), -777.0, dtype=torch.float64, device=logits.device)
    dec = torch.full((B, 1, h, w), -777, dtype=torch.int64, device=logits.device) if want_decode else None
    lin = torch.full((B, 1, S, S), -777.0, dtype=torch.float32, device=logits.device) if want_linear else None
    rc = _lib.lib().rdm_predict_tail_f32(_lib.ptr(logits.contiguous()), _lib.ptr(wv), _lib.ptr(out), _lib.ptr(dec), _lib.ptr(lin), B, C2 // 2, h, w, n_out, split,
                                         _lib.stream())
    torch.cuda.synchronize()
    return rc, out, dec, lin


def composed(logits, wv):
    """The operators DepthEstimationNet.forward + recombination launch, from the logits on: dorn -> gm_normalize -> decompose ->
    fine_detail_pred -> recombine."""
    from md_rdm_amd.network import computations as cp
    B, _, s, _ = logits.shape
    n = int(math.log2(s))
    dec, _ = cp.dorn_ordinal_regression(logits)
    norm = cp.gm_normalize(dec, 1.0 / (s * s)).float()
    levels = cp.decompose_depth_map([], norm, n)[::-1]
    A = cp.relative_fine_detail_matrix([levels], True)
    yh = cp.make_pred([wv[k].reshape(1, 1) for k in range(n + 1)], A, True, False)
    return cp.recombination(list(yh)), dec


def assert_map(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(ref).all(), what
    print("%s: max |diff| = %.3e, max |ref| = %.3e" % (what, np.abs(got - ref).max(), np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=0, atol=REL * np.abs(ref).max(), err_msg=what)


def stats3(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([a.mean(), np.abs(a).mean(), np.abs(a).max()])


def random_logits(B, side, seed):
    """(B,180,side,side) float32 in [0.01, 6): inside the DORN clamp, no pair (2k, 2k+1) tied (checked on the host)."""
    x = filler.uniform("predict-logits/%d/%d/%d" % (seed, B, side), (B, 180, side, side), 0.01, 6.0)
    a, b = np.clip(x[:, 0::2], np.float32(1e-8), np.float32(1e4)), np.clip(x[:, 1::2], np.float32(1e-8), np.float32(1e4))
    assert not (a == b).any(), "a tied ordinal pair in the drawn logits"
    return x


# ---- 1. the operator against the reference's recorded results -----------------------------------
@pytest.mark.parametrize("case", ["train228", "eval226"])
def test_tail_vs_reference_fixtures(dev, model, net_gold, case):
    logits = net_gold[case + "_logits"]
    rc, out, dec, lin = tail(torch.from_numpy(logits).to(dev), level_weights(model, 3))
    assert rc == 0
    ref = ocp.recombination([net_gold["%s_yhat%d" % (case, i)] for i in range(4)])
    assert_map(out.cpu().numpy(), ref, case + " log map vs recombination(reference yhat)")
    ref_dec, _ = ocp.dorn_ordinal_regression(logits)
    np.testing.assert_array_equal(dec.cpu().numpy(), ref_dec)
    np.testing.assert_array_equal(dec.cpu().numpy(), net_gold[case + "_decode_c"])
    if case == "train228":
        o = out.cpu().numpy()
        assert_map(o[:, :, :4, :4], net_gold["train228_final_depth_corner"], "train228 final_depth corner")
        assert_map(stats3(o), net_gold["train228_final_depth_stats"], "train228 final_depth statistics")


# ---- 2. the operator against the composed operators ---------------------------------------------
@pytest.mark.parametrize("B,side", [(1, 8), (2, 8), (16, 8), (13, 8), (1, 16), (2, 16), (16, 16), (13, 16)])
def test_tail_vs_composed_operators(dev, B, side):
    n = int(math.log2(side))
    logits = torch.from_numpy(random_logits(B, side, seed=5)).to(dev)
    wv = torch.from_numpy(filler.uniform("predict-w/%d" % side, (n + 1,), 0.2, 1.5)).to(dev)
    ref, ref_dec = composed(logits, wv)
    rc, out, dec, _ = tail(logits, wv)
    assert rc == 0
    assert torch.equal(dec, ref_dec)
    assert_map(out.cpu().numpy(), ref.cpu().numpy(), "B=%d side=%d fused vs composed" % (B, side))
    for split in (1, 2, 32, 128):                                   # the result does not depend on the row split
        rc, o2, d2, _ = tail(logits, wv, split=split)
        assert rc == 0 and torch.equal(o2, out) and torch.equal(d2, dec), split


def test_count_shortcut_equals_the_probability_form_on_neighbouring_floats(dev):
    """The fused kernel counts `clamp(b) > clamp(a)` where rdm_dorn_fwd counts `P > 0.5` (postproc_dev.h argues they are the same integer):
    pairs of NEIGHBOURING floats across and beyond the clamp range [1e-8, 1e4], in both orders, plus exact ties."""
    from md_rdm_amd.network import computations as cp
    B, K, side = 4, 90, 8
    n = B * K * side * side
    mag = np.exp(np.linspace(np.log(1e-10), np.log(5e4), n)).astype(np.float32)
    mag[::97] *= -1                                                   # some negative logits (clamped to 1e-8: ties)
    kind = np.arange(n) % 3
    other = np.where(kind == 0, np.nextafter(mag, np.float32(np.inf)), np.where(kind == 1, np.nextafter(mag, np.float32(-np.inf)), mag)).astype(np.float32)
    perm = np.argsort(filler.unit("predict-neighbours", n))          # spread the magnitudes over pixels and pairs
    x = np.empty((B, 2 * K, side, side), dtype=np.float32)
    x[:, 0::2] = mag[perm].reshape(B, K, side, side)
    x[:, 1::2] = other[perm].reshape(B, K, side, side)
    logits = torch.from_numpy(x).to(dev)
    ref_dec, _ = cp.dorn_ordinal_regression(logits)
    rc, _, dec, _ = tail(logits, torch.ones(4, device=dev), want_linear=False)
    assert rc == 0
    assert 0 < int(ref_dec.min()) and int(ref_dec.max()) < K          # both outcomes occur at every pixel
    assert torch.equal(dec, ref_dec)
    np.testing.assert_array_equal(dec.cpu().numpy(), ocp.dorn_ordinal_regression(x)[0])


# ---- 3. optional outputs, 4. determinism ----------------------------------------------------------
def test_optional_outputs_and_determinism(dev):
    logits = torch.from_numpy(random_logits(3, 8, seed=9)).to(dev)
    wv = torch.from_numpy(filler.uniform("predict-w/8", (4,), 0.2, 1.5)).to(dev)
    rc, out, dec, lin = tail(logits, wv)
    assert rc == 0
    rc2, out2, dec2, lin2 = tail(logits, wv)
    assert rc2 == 0 and torch.equal(out, out2) and torch.equal(dec, dec2) and torch.equal(lin, lin2)          # bit-identical launches
    rc3, out3, dec3, lin3 = tail(logits, wv, want_decode=False, want_linear=False)
    assert rc3 == 0 and dec3 is None and lin3 is None and torch.equal(out3, out)
    rc4, out4, _, lin4 = tail(logits, wv, want_decode=False)
    assert rc4 == 0 and torch.equal(out4, out) and torch.equal(lin4, lin)
    want = torch.exp(out).float()
    err = ((lin.double() - want.double()).abs() / want.double()).max().item()
    print("linear map vs float32(exp(log map)): max relative difference %.3e" % err)
    assert err <= 2.0 ** -23                                            # one float32 rounding (2^-24) + the f64 exp's own last bit


# ---- 5. argument checks -------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(8, 10), (6, 6), (10, 8), (32, 32)])
def test_bad_heads_return_an_error_and_write_nothing(dev, hw):
    from md_rdm_amd import _lib
    logits = torch.ones(2, 180, hw[0], hw[1], dtype=torch.float32, device=dev)
    rc, out, dec, lin = tail(logits, torch.ones(6, device=dev))
    assert rc == -1 and b"predict_tail" in _lib.lib().rdm_last_error_string()
    assert bool((out == -777.0).all()) and bool((dec == -777).all()) and bool((lin == -777.0).all())


def test_null_required_pointers_are_errors(dev):
    from md_rdm_amd import _lib
    L = _lib.lib()
    assert L.rdm_predict_tail_f32(None, None, None, None, None, 1, 90, 8, 8, 7, 0, None) == -1
    x = torch.ones(1, 180, 8, 8, device=dev)
    o = torch.zeros(1, 1, 128, 128, dtype=torch.float64, device=dev)
    w = torch.ones(4, device=dev)
    assert L.rdm_predict_tail_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(o), None, None, 1, 90, 8, 8, 7, 3, None) == -1      # split not a power of two
    assert L.rdm_predict_tail_f32(_lib.ptr(x), _lib.ptr(w), _lib.ptr(o), None, None, 1, 90, 8, 8, 2, 0, None) == -1      # n_out below the head
    torch.cuda.synchronize()
    assert bool((o == 0).all())


# ---- 6. the model route -------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_predict_equals_forward_plus_recombination(dev, model, precision):
    from md_rdm_amd.network import computations as cp
    model.set_precision(precision)
    try:
        x = torch.from_numpy(filler.synthetic_batch(2, 226, 226, seed=SEED["eval226"])[0]).to(dev)
        with torch.no_grad():
            yh, counts, _ = model(x)
            ref = cp.recombination(list(yh))
        got, got_counts = model.predict(x, return_counts=True)
        assert got.shape == (2, 1, 128, 128) and got.dtype == torch.float64
        assert torch.equal(got_counts, counts)
        assert_map(got.cpu().numpy(), ref.cpu().numpy(), "predict vs forward + recombination (%s)" % precision)
        assert torch.equal(model.predict(x), got)
        lin = model.predict(x, linear=True)
        assert lin.dtype == torch.float32
        assert_map(lin.cpu().numpy(), torch.exp(ref).cpu().numpy(), "linear map (%s)" % precision)
        sized = model.predict(x, size=(226, 226))
        assert sized.shape == (2, 1, 226, 226) and torch.equal(sized, cp.resize(got, (226, 226)))
        lin_sized = model.predict(x, size=(226, 226), linear=True)
        assert_map(lin_sized.cpu().numpy(), torch.exp(cp.resize(ref, (226, 226))).cpu().numpy(), "linear resized map (%s)" % precision)
    finally:
        model.set_precision("f32")


def test_predict_uses_the_fused_kernel_for_the_default_model(dev, model):
    """One librdm launch after the forward (the tail), against the composed path's five."""
    from md_rdm_amd import _lib
    L = _lib.lib()
    x = torch.from_numpy(filler.synthetic_batch(1, 226, 226, seed=SEED["eval226"])[0]).to(dev)
    model.predict(x)
    with torch.no_grad():
        a = L.rdm_launch_count()
        model._native_forward(x)
        fwd = L.rdm_launch_count() - a
        a = L.rdm_launch_count()
        model.predict(x)
        assert L.rdm_launch_count() - a == fwd + 1


def test_predict_rectangular_head_falls_back_to_the_composed_operators(dev, model):
    from md_rdm_amd.network import computations as cp
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 304, seed=SEED["train228x304"])[0]).to(dev)
    with torch.no_grad():
        yh, counts, _ = model(x)
        ref = cp.recombination(list(yh))
    got, got_counts = model.predict(x, return_counts=True)
    assert got_counts.shape == (2, 1, 8, 10) and torch.equal(got_counts, counts)
    assert_map(got.cpu().numpy(), ref.cpu().numpy(), "predict vs forward + recombination (8x10 head)")


def test_predict_with_a_relative_decoder_falls_back_to_the_composed_operators(dev):
    from md_rdm_amd.network import computations as cp
    m = make_model(dev, relative_decoders=(6,))
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 228, seed=SEED["train228"])[0]).to(dev)
    with torch.no_grad():
        yh, counts, _ = m(x)
        ref = cp.recombination(list(yh))
    got, got_counts = m.predict(x, return_counts=True)
    assert torch.equal(got_counts, counts)
    assert_map(got.cpu().numpy(), ref.cpu().numpy(), "predict vs forward + recombination (relative_decoders=(6,))")


def test_predict_raises_in_train_mode(dev, model):
    from md_rdm_amd import _lib
    x = torch.zeros(1, 3, 226, 226, device=dev)
    model.train()
    try:
        with pytest.raises(_lib.RdmError):
            model.predict(x)
    finally:
        model.eval()


# ---- 7. the command ------------------------------------------------------------------------------
def test_cli_writes_the_maps_predict_gives(dev, tmp_path):
    out = tmp_path / "maps"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.predict", "--synthetic", "3", "--batch_size", "2", "--out", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    files = sorted(os.listdir(out))
    assert files == ["synthetic_%04d.npy" % i for i in range(3)]
    maps = [np.load(out / f) for f in files]
    assert all(m.shape in ((1, 128, 128), (128, 128)) and m.dtype == np.float64 for m in maps)
    assert "warning" in r.stdout and r.stdout.count("images/s") == 2          # batches of 2 and 1
    m = make_model(dev, deterministic=False)                                  # the command's model and its first batch: the same launches
    x = torch.from_numpy(filler.synthetic_batch(3, 226, 226)[0][:2]).to(dev)
    ref = m.predict(x)[0].cpu().numpy()
    assert_map(maps[0].reshape(ref.shape), ref, "CLI map 0 vs in-process predict")
