"""-m gpu: the TRAINING-mode forward of the relative decoders d_6..d_10 on the bf16 path (rdm_rel_forward_bf16_train, csrc/wsm_bf16.hip;
the dense block through dense_block_bf16_train, csrc/net.hip): BatchNorm from the batch statistics, running statistics updated like
nn.BatchNorm2d (momentum 0.1, unbiased variance) - the reference's `--precision 16` treatment of these forward-only decoders.

Tolerances:
  * operators (the statistics epilogues of the bf16 1x1 GEMM and 3x3 conv, the column statistics of the encoder output), against float64
    on the SAME bf16-rounded operands: the stored output within the bound of tests/test_gpu_relative_bf16.py (2e-3 of the max on top of
    the one rounding of the stored value); the sums against float64 sums of the STORED values within 1e-5 of sum |x| per channel (a
    cancelling sum has no relative scale of its own), the sums of squares within 1e-5 relative; two launches give the same bits;
  * decoders (train mode, state from the filler, input tests/test_rel_restatement_cpu.py::decoder_input), bf16 map against the float64
    training-mode restatement and against the product's f32 train-mode path: RMS(d) relative to the spread of the reference map (as
    tests/test_gpu_relative_bf16.py).  Measured on MI355X (d_6 .. d_10): 0.74 / 0.69 / 0.98 / 1.05 / 1.08 % against the restatement,
    the same to 0.01 % against the f32 path; bounds 1.2 / 1.3 / 1.8 / 1.9 / 2.0 % (<= 1.85x the measurement, at most the 2 % ceiling);
  * running statistics: every updated running_mean / running_var against the f32 path and the float64 reference (helper below), as the
    implied batch statistic ((new - 0.9 old) / 0.1), max |d| relative to the max |batch statistic| of that BatchNorm.  Measured <= 0.25 %
    (means) and <= 0.51 % (variances); bound 1 %.  num_batches_tracked exactly +1;
  * model (B=2 228x228, relative_decoders=(6..10), train mode, deterministic models: the same bits every run), bf16 mode against f32
    mode, one step from the same state for each of STEP_SEEDS: loss within 0.5 % (measured <= 0.064 % over those 16 seeds), weight_layer
    gradient cosine >= 0.99 (measured >= 0.9978)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from md_rdm_amd import filler
from test_rel_restatement_cpu import decoder_input, decoder_state, rel_decoder_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
DEC_BOUND = {6: 0.012, 7: 0.013, 8: 0.018, 9: 0.019, 10: 0.02}
STAT_BOUND = 0.01
LOSS_TOL = 0.005
COS_MIN = 0.99
# synthetic_batch seeds 0..23 whose f32 training step is finite in BOTH modes (deterministic models; measured on MI355X).  The step of this
# hash-filled, untrained model is NaN on 7 of those 24 seeds on the default f32 path too: d_7's head gives a map whose pyramid has negative
# fine-detail values, and the fine-detail matrix takes their log.  On seeds 3 and 7 the two modes fall on opposite sides of that singularity
# (f32 NaN / bf16 finite, and the reverse); the decoder maps themselves are finite and within DEC_BOUND there.
STEP_SEEDS = (2, 4, 6, 8, 9, 10, 11, 13, 14, 15, 17, 18, 19, 20, 22, 23)
REL = (6, 7, 8, 9, 10)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def _L():
    from md_rdm_amd import _lib
    return _lib


def bfr(t):
    return t.to(torch.bfloat16).double()


def rnd(key, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(filler.uniform(key, shape, lo, hi)).double()


def same_bits(a, b):
    """bit equality (the unwritten NaN columns included)"""
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(it), b.view(it))


def _half_ulp(want):
    return torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 8)


def _check_out(got, want):
    excess = ((got - want).abs() - _half_ulp(want)).max().item()
    assert excess <= 2e-3 * want.abs().max().item(), (excess, want.abs().max().item())


def _check_stats(stored, s, q):
    """s / q (device f64) against float64 sums of the stored bf16 values (rows x channels)"""
    ref_s, ref_q, mag = stored.sum(0), stored.pow(2).sum(0), stored.abs().sum(0)
    s, q = s.cpu(), q.cpu()
    assert ((s - ref_s).abs() <= 1e-5 * mag + 1e-30).all(), (s - ref_s).abs().max().item()
    assert ((q - ref_q).abs() <= 1e-5 * ref_q + 1e-30).all(), ((q - ref_q).abs() / ref_q.clamp_min(1e-30)).max().item()


def _act(x, scale, shift):
    """the kernels' prologue: relu(x * scale + shift) in f32, rounded to bf16"""
    return torch.relu(x.float() * scale + shift).to(torch.bfloat16).double()


def _ws(dev, m, n, extra_floats):
    nb = int(_L().lib().rdm_bf16_stats_workspace_bytes(m, n)) + 4 * extra_floats
    return torch.empty(nb, dtype=torch.uint8, device=dev), nb


# ---- operators -----------------------------------------------------------------------------------------------------------------
# (M, N, K): the decoders' 1x1 of layer 23 (K = 2160) at B = 1, 2, 16, and a ragged case whose M and N divide no tile (the epilogue's tails)
GEMM_GEOMS = [(64, 384, 2160), (128, 384, 2160), (1024, 384, 2160), (100, 200, 1056)]


@pytest.mark.parametrize("split", [False, True], ids=["nosplit", "splitK"])
@pytest.mark.parametrize("geom", GEMM_GEOMS, ids=lambda g: "M%d_N%d" % g[:2])
def test_gemm_bf16_stats_epilogue(dev, geom, split):
    """the dense layer's 1x1 in training form: norm1 BN-ReLU prologue, raw bf16 output + its statistics"""
    _lib = _L()
    L = _lib.lib()
    M, N, K = geom
    ldx = K + 48
    key = "rtrain.gemm.%d.%d" % (M, N)
    X = bfr(rnd(key + ".x", (M, ldx)))
    W = bfr(rnd(key + ".w", (N, K), -1 / np.sqrt(K), 1 / np.sqrt(K)))
    sc = rnd(key + ".s", (K,), 0.5, 1.5).float()
    sh = rnd(key + ".t", (K,), -0.3, 0.3).float()
    Xd, Wd, scd, shd = X.to(torch.bfloat16).to(dev), W.to(torch.bfloat16).to(dev), sc.to(dev), sh.to(dev)
    ws, nb = _ws(dev, M, N, 8 * M * N if split else 0)
    res = []
    L.rdm_census_reset()
    L.rdm_census_enable(1)
    try:
        for _ in range(2):
            out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
            s = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
            q = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
            _lib.check(L.rdm_gemm_bf16_stats(_lib.ptr(Xd), ldx, K, _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(Wd), K, _lib.ptr(out), N, M, N,
                                             _lib.ptr(s), _lib.ptr(q), _lib.ptr(ws), nb, _lib.stream()))
            res.append((out, s, q))
        census = _lib.census()
    finally:
        L.rdm_census_enable(0)
    assert any(k.endswith("/splitK") for k in census) == split, census
    want = _act(X[:, :K], sc, sh) @ W.t()
    stored = res[0][0].cpu().double()
    _check_out(stored, want)
    _check_stats(stored, res[0][1], res[0][2])
    for a, b in zip(res[0], res[1]):
        assert same_bits(a, b)


# (B, H, W): the decoders' 8x8 maps at B = 1, 2, 16, and two whose pixel count is no multiple of the 64-pixel tile (the epilogue's tails)
CONV_GEOMS = [(1, 8, 8), (2, 8, 8), (16, 8, 8), (1, 10, 10), (2, 6, 7)]


@pytest.mark.parametrize("split", [False, True], ids=["nosplit", "splitK"])
@pytest.mark.parametrize("geom", CONV_GEOMS, ids=lambda g: "B%d_%dx%d" % g)
def test_conv3x3_bf16_stats_epilogue(dev, geom, split):
    """the dense layer's 3x3 in training form: norm2 BN-ReLU prologue over the 384-channel bottleneck, 48 channels written into a slice
    of a wider buffer + their statistics (norm1 of every later layer)"""
    _lib = _L()
    L = _lib.lib()
    B, H, W = geom
    M, C, ldc, coff = B * H * W, 384, 112, 48
    key = "rtrain.c3.%d.%d.%d" % geom
    Y = bfr(rnd(key + ".y", (M, C)))
    w = bfr(rnd(key + ".w", (48, C, 3, 3), -1 / np.sqrt(9 * C), 1 / np.sqrt(9 * C)))
    sc = rnd(key + ".s", (C,), 0.5, 1.5).float()
    sh = rnd(key + ".t", (C,), -0.3, 0.3).float()
    wp = w.permute(2, 3, 0, 1).reshape(9, 48, C).contiguous().to(torch.bfloat16).to(dev)
    Yd, scd, shd = Y.to(torch.bfloat16).to(dev), sc.to(dev), sh.to(dev)
    ws, nb = _ws(dev, M, 48, 16 * M * 48 if split else 0)
    res = []
    import ctypes
    L.rdm_census_reset()
    L.rdm_census_enable(1)
    try:
        for _ in range(2):
            out = torch.full((M, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
            s = torch.full((48,), float("nan"), dtype=torch.float64, device=dev)
            q = torch.full((48,), float("nan"), dtype=torch.float64, device=dev)
            _lib.check(L.rdm_conv3x3_bf16_stats(_lib.ptr(Yd), C, C, _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(wp), ctypes.c_void_p(out.data_ptr() + 2 * coff), ldc,
                                                B, H, W, _lib.ptr(s), _lib.ptr(q), _lib.ptr(ws), nb, _lib.stream()))
            res.append((out, s, q))
        census = _lib.census()
    finally:
        L.rdm_census_enable(0)
    assert any("/stats" in k for k in census) and any(k.endswith("/stats/splitK") for k in census) == split, census
    a = _act(Y, sc, sh).reshape(B, H, W, C).permute(0, 3, 1, 2)
    want = F.conv2d(a, w, padding=1).permute(0, 2, 3, 1).reshape(M, 48)
    got = res[0][0].cpu().double()
    assert torch.isnan(got[:, :coff]).all() and torch.isnan(got[:, coff + 48:]).all()
    stored = got[:, coff:coff + 48]
    _check_out(stored, want)
    _check_stats(stored, res[0][1], res[0][2])
    for x, y in zip(res[0], res[1]):
        assert same_bits(x, y)


@pytest.mark.parametrize("B", [1, 2, 16])
def test_colstats_bf16(dev, B):
    _lib = _L()
    M, C, ld = B * 64, 1056, 1064
    X = bfr(rnd("rtrain.cs.%d" % B, (M, ld), -2.0, 3.0))
    Xd = X.to(torch.bfloat16).to(dev)
    out = []
    for _ in range(2):
        s = torch.empty(C, dtype=torch.float64, device=dev)
        q = torch.empty(C, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().rdm_colstats_bf16(_lib.ptr(Xd), ld, M, C, _lib.ptr(s), _lib.ptr(q), _lib.stream()))
        out.append((s, q))
    _check_stats(X[:, :C], *out[0])
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_train_entry_argument_errors(dev):
    _lib = _L()
    L = _lib.lib()
    x = torch.zeros(64, 1056, dtype=torch.bfloat16, device=dev)
    import ctypes
    table = (ctypes.c_void_p * 300)()
    assert L.rdm_rel_forward_bf16_train(5, _lib.ptr(x), 1056, None, 1, table, _lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), _lib.stream()) == -1
    assert L.rdm_rel_bf16_train_workspace_bytes(11, 1) == 0 and L.rdm_rel_bf16_train_workspace_bytes(6, 0) == 0
    assert L.rdm_rel_bf16_train_workspace_bytes(6, 2) > L.rdm_rel_bf16_workspace_bytes(6, 2)


# ---- decoders --------------------------------------------------------------------------------------------------------------------
def _decoder(did, dev):
    from md_rdm_amd.network import RDM_Net
    dec = RDM_Net.Decoder(in_channels=1056, num_wsm_layers=did - 6, DORN=False, id=did, quant=RDM_Net.Quantization())
    sd = decoder_state(did)
    with torch.no_grad():
        for key, t in dec.state_dict().items():
            if key in sd:
                t.copy_(sd[key].float())
    return dec.to(dev).train()


def _spread_rms(got, ref):
    ref = ref.double()
    return (got.double() - ref).pow(2).mean().sqrt().item() / (ref - ref.mean()).pow(2).mean().sqrt().item()


def running_stats_f64(sd, x):
    """float64 reference of the running statistics after one training forward of the dense block: {prefix: (running_mean, running_var)}"""
    out = {}
    with torch.no_grad():
        x = x.double()
        n = x.shape[0] * x.shape[2] * x.shape[3]

        def bn(v, pre):
            mean, var = v.mean((0, 2, 3)), v.var((0, 2, 3), unbiased=False)
            out[pre] = (0.9 * sd[pre + "running_mean"] + 0.1 * mean, 0.9 * sd[pre + "running_var"] + 0.1 * var * n / (n - 1))
            sh = (1, -1, 1, 1)
            return F.relu((v - mean.view(sh)) / torch.sqrt(var.view(sh) + EPS) * sd[pre + "weight"].view(sh) + sd[pre + "bias"].view(sh))

        for i in range(1, 25):
            p = f"dense_layer.denselayer{i}."
            y = F.conv2d(bn(x, p + "norm1."), sd[p + "conv1.weight"])
            y = F.conv2d(bn(y, p + "norm2."), sd[p + "conv2.weight"], padding=1)
            x = torch.cat((x, y), 1)
    return out


def _enc16(dev, x):
    _lib = _L()
    B = x.shape[0]
    enc = torch.empty(B * 64, 1056, dtype=torch.bfloat16, device=dev)
    _lib.check(_lib.lib().rdm_rel_bf16_input_nchw(_lib.ptr(x.contiguous()), B, _lib.ptr(enc), 1056, _lib.stream()))
    return enc


def _stat_err(new, old, ref_batch):
    """max |implied batch statistic - reference| / max |reference|"""
    implied = (new.double().cpu() - 0.9 * old.double()) / 0.1
    return (implied - ref_batch).abs().max().item() / ref_batch.abs().max().item()


@pytest.mark.parametrize("did", [6, 7, 8, 9, 10])
def test_decoder_bf16_train_vs_restatement_and_f32_path(dev, did):
    x = decoder_input()
    xd = x.float().to(dev)
    sd = decoder_state(did)
    d32 = _decoder(did, dev)
    f32 = d32.features(xd)
    dec = _decoder(did, dev)
    sd0 = {k: v.clone() for k, v in dec.state_dict().items()}
    enc = _enc16(dev, xd)
    b16 = dec.features_bf16_train(enc, 1056, 2)
    ref = rel_decoder_f64(did, sd, x, training=True)
    assert b16.shape == ref.shape == f32.shape and torch.isfinite(b16).all()
    e_ref, e_f32 = _spread_rms(b16.cpu(), ref), _spread_rms(b16.cpu(), f32.cpu())
    print("d_%d bf16 train rms/spread vs restatement %.5f vs f32 path %.5f" % (did, e_ref, e_f32))
    assert e_ref <= DEC_BOUND[did] and e_f32 <= DEC_BOUND[did], (e_ref, e_f32)
    # running statistics
    rs = running_stats_f64(sd, x)
    st16, st32 = dec.state_dict(), d32.state_dict()
    worst = [0.0, 0.0]
    for pre, (rm_ref, rv_ref) in rs.items():
        for j, (name, r) in enumerate((("running_mean", rm_ref), ("running_var", rv_ref))):
            old = sd[pre + name]
            batch_ref = (r - 0.9 * old) / 0.1
            e1 = _stat_err(st16[pre + name], old, batch_ref)
            e2 = _stat_err(st16[pre + name], old, (st32[pre + name].double().cpu() - 0.9 * old) / 0.1)
            worst[j] = max(worst[j], e1, e2)
        assert int(st16[pre + "num_batches_tracked"]) == int(sd0[pre + "num_batches_tracked"]) + 1
    print("d_%d running statistics: worst mean %.5f var %.5f" % (did, worst[0], worst[1]))
    assert max(worst) <= STAT_BOUND, worst
    # the same state again: the same bits, maps and buffers
    after = {k: v.clone() for k, v in dec.state_dict().items()}
    dec.load_state_dict(sd0)
    again = dec.features_bf16_train(enc, 1056, 2)
    assert torch.equal(again, b16)
    for k, v in dec.state_dict().items():
        assert torch.equal(v, after[k]), k
    # standalone stats given by the caller: the same bits as computed inside
    dec.load_state_dict(sd0)
    stats = torch.empty(2 * 1056, dtype=torch.float64, device=dev)
    _lib = _L()
    _lib.check(_lib.lib().rdm_colstats_bf16(_lib.ptr(enc), 1056, 128, 1056, _lib.ptr(stats[:1056]), _lib.ptr(stats[1056:]), _lib.stream()))
    assert torch.equal(dec.features_bf16_train(enc, 1056, 2, stats), b16)
    dec.eval()
    with pytest.raises(Exception):
        dec.features_bf16_train(enc, 1056, 2)                                    # the training form needs train mode


# ---- model -----------------------------------------------------------------------------------------------------------------------
def _model(dev):
    """deterministic (RDM_NET_OPT_DETERMINISTIC, as tests/test_gpu_net.py::make_model): the encoder output the decoders read, and so the
    discontinuous Lloyd / ALS head behind them, are the same bits every run"""
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=REL)
    m.deterministic = True
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).train()


def test_set_relative_train_precision_rejects_other_values(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=(6,))
    assert m.relative_train_precision == "f32"
    with pytest.raises(ValueError):
        m.set_relative_train_precision("bf32")


def test_model_training_step_bf16_vs_f32(dev):
    """one training step from the same state and batch in both modes, for each of STEP_SEEDS; the bounds hold for every seed"""
    from md_rdm_amd import harness
    models = {mode: _model(dev).set_relative_train_precision(mode) for mode in ("f32", "bf16")}
    sd0 = {k: v.clone() for k, v in models["f32"].state_dict().items()}
    worst = [0.0, 1.0]
    for seed in STEP_SEEDS:
        x, y = filler.synthetic_batch(2, 228, 228, seed=seed)
        x, y = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
        out = {}
        for mode, m in models.items():
            m.load_state_dict(sd0)
            m.zero_grad(set_to_none=True)
            loss, _ = harness.training_step(m, x, y)
            loss.backward()
            g = torch.cat([p.grad.reshape(-1) for p in m.weight_layer.parameters() if p.grad is not None]).double()
            out[mode] = (float(loss.detach()), g)
        (l32, g32), (l16, g16) = out["f32"], out["bf16"]
        cos = (torch.dot(g16, g32) / (g16.norm() * g32.norm())).item()
        rel = abs(l16 - l32) / abs(l32)
        print("training step seed %d: loss f32 %.6f bf16 %.6f (rel %.5f), weight_layer gradient cosine %.6f" % (seed, l32, l16, rel, cos))
        assert np.isfinite(l32) and np.isfinite(l16), (seed, l32, l16)
        worst = [max(worst[0], rel), min(worst[1], cos)]
    assert worst[0] <= LOSS_TOL and worst[1] >= COS_MIN, worst
    xb = torch.from_numpy(filler.synthetic_batch(2, 260, 260, seed=5)[0]).to(dev)
    with pytest.raises(Exception, match="8x8"):
        models["bf16"](xb)                                                       # a non-8x8 encoder output still raises


def test_model_bf16_mode_takes_the_bf16_training_forward(dev):
    """set_relative_train_precision("bf16") routes the model's train-mode forward to features_bf16_train: every decoder's updated BatchNorm
    buffers equal those of a direct features_bf16_train call on the same encoder output bit for bit, and differ from the f32 path's"""
    m = _model(dev).set_relative_train_precision("bf16")
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 228, seed=3)[0]).to(dev)
    decs = {did: getattr(m, "d_%d" % did) for did in REL}
    sd0 = {did: {k: v.clone() for k, v in d.state_dict().items()} for did, d in decs.items()}
    with torch.no_grad():
        m(x)
        enc = m.encoder_output()
        enc16 = _enc16(dev, enc)
        for did, d in decs.items():
            after = {k: v.clone() for k, v in d.state_dict().items()}
            assert any(not torch.equal(after[k], sd0[did][k]) for k in after if "running_mean" in k)
            d.load_state_dict(sd0[did])
            d.features_bf16_train(enc16, 1056, 2)
            for k, v in d.state_dict().items():
                assert torch.equal(v, after[k]), (did, k)
            d.load_state_dict(sd0[did])
            d.features(enc)                                                      # the f32 training forward
            assert any(not torch.equal(v, after[k]) for k, v in d.state_dict().items() if "running_var" in k), did


def test_eval_maps_after_a_bf16_training_forward_equal_a_fresh_model(dev):
    """The bf16 training forward moves the running statistics: the eval-folded affines are rebuilt, so the bf16 eval maps afterwards equal
    those of a freshly loaded model bit for bit."""
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 228, seed=3)[0]).to(dev)
    m = _model(dev).eval().set_precision("bf16")
    with torch.no_grad():
        before = [t.clone() for t in m(x)[0]]
        m.train().set_precision("f32").set_relative_train_precision("bf16")
        m(x)
        m.eval().set_precision("bf16")
        after = m(x)[0]
    fresh = DepthEstimationNet(relative_decoders=REL)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).eval().set_precision("bf16")
    with torch.no_grad():
        ref = fresh(x)[0]
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    for a, b in zip(after, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["32", "16"])
def test_train_cli_relative_bf16(precision):
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.train", "--synthetic", "--dev", "--precision", precision, "--relative_decoders", "6", "7", "8", "9", "10",
                        "--relative_bf16", "--batch_size", "2", "--size", "228", "228"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if "val_delta1" in l]
    assert line, r.stdout[-2000:]
    v = float(line[-1].split("val_delta1")[1].split(",")[0])
    assert np.isfinite(v)
