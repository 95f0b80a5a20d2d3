"""-m gpu: the relative decoders d_6..d_10 on the bf16 inference path (reference network/RDM_Net.py:57-61,106-125 with Decoder :137-162
and WSMLayer :163-236; csrc/wsm_bf16.hip, rdm_rel_forward_bf16).

Tolerances (bf16 cannot meet the f32 path's 1e-4: 8 significant bits per stored activation and weight, f32 accumulation):
  * operator level, against float64 convolutions of the SAME bf16-rounded operands: 2e-3 of the output's max for bf16 outputs on top
    of the one rounding of the stored result (half a bf16 ulp of each value: near the maximum that alone is up to 3.9e-3 of it),
    1e-5 of the max for the f32 single-channel output;
  * decoder level (eval mode, running statistics from the filler), bf16 feature map against the float64 restatement
    (tests/test_rel_restatement_cpu.py) and against the product's f32 eval path, RMS(d) relative to the SPREAD of the reference map
    (RMS(ref - mean): the fixtures' conv1 bias of 2.0 would hide the error in a magnitude-relative bound).  Measured on MI355X
    (d_6 .. d_10): 0.68 / 0.59 / 0.84 / 0.97 / 1.01 % against the restatement, the same to 0.01 % against the f32 path; bounds
    1.2 / 1.05 / 1.5 / 1.75 / 1.8 % (<= 1.8x the measurement, under the 2 % ceiling);
  * model level (B=2 228x228, eval, relative_decoders=(6..10)), bf16 against f32: the d_1 head within the bounds of
    tests/test_gpu_bf16.py (logits max |d| <= 4 % / RMS <= 1 %, probabilities mean |dP| <= 5e-3 / max <= 0.15, counts within +-3 and
    mean <= 0.5); every level of y_hat (8 with d_10: 1x1 .. 128x128) finite with identical shapes; each relative map on its path's own
    encoder output within 4 % of its spread (measured 1.0 - 2.0 %); the levels of y_hat (Lloyd bins flip where a ratio sits near a
    threshold, as in tests/test_gpu_relative.py, and a flipped bin moves a whole page) agree to rtol 5 % / atol 5 % of the level's RMS
    on >= 75 % of their entries with RMS(d) <= 30 % of the level's RMS (measured: agreement 0.83 - 1.0, RMS(d) 3 - 16 %)."""
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
WSM = [(2208, 1664, 16), (1664, 832, 32), (832, 416, 64), (416, 208, 128)]     # (raw, C, S) of WSM_1..WSM_4
AGREE = 0.75
LEVEL_RMS = 0.3
MAP_BOUND = 0.04
DEC_BOUND = {6: 0.012, 7: 0.0105, 8: 0.015, 9: 0.0175, 10: 0.018}


def p32(c):
    return (c + 31) // 32 * 32


def p64(c):
    return (c + 63) // 64 * 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def _L():
    from md_rdm_amd import _lib
    return _lib


def bfr(t):
    """round to bf16 and back (float64): the operand the kernel sees"""
    return t.to(torch.bfloat16).double()


def rnd(key, shape, scale=1.0):
    return torch.from_numpy(filler.uniform(key, shape, -scale, scale)).double()


def _rows(w2d):
    return F.pad(w2d, (0, 0, 0, p64(w2d.shape[0]) - w2d.shape[0]))


def pack_conv(w):
    """(n, cin, k, k) -> bf16 [p64(n)][k*k*p32(cin)], k = tap * p32(cin) + ci"""
    n, cin, k, _ = w.shape
    return _rows(F.pad(w.permute(0, 2, 3, 1), (0, p32(cin) - cin)).reshape(n, -1)).to(torch.bfloat16)


def _nhwc_buffer(key, B, H, W, ld):
    return bfr(rnd(key, (B * H * W, ld)))


def _half_ulp(want):
    """half an ulp of bf16 at each value: the one rounding of the stored result (2^-9 of the value's power of two)"""
    return torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(1e-30))) - 8)


def _check(out_bf16, want, coff, n, ldc):
    got = out_bf16.double()
    d = (got[:, coff:coff + n] - want).abs()
    excess = (d - _half_ulp(want)).max().item()
    assert excess <= 2e-3 * want.abs().max().item(), (excess, d.max().item(), want.abs().max().item())
    assert torch.isnan(got[:, :coff]).all() and torch.isnan(got[:, coff + n:]).all()             # nothing outside the slot


def _to_nhwc(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def run_conv(dev, B, H, W, cin, n, k, ldx, xoff, ldc, coff, key):
    _lib = _L()
    X = _nhwc_buffer(key + ".x", B, H, W, ldx)
    w = bfr(rnd(key + ".w", (n, cin, k, k), 1.0 / np.sqrt(cin * k * k)))
    b = rnd(key + ".b", (n,), 0.5).float()
    out = torch.full((B * H * W, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    wp = pack_conv(w).to(dev)
    Xd = X.to(torch.bfloat16).to(dev)
    bd = b.to(dev)
    _lib.check(_lib.lib().rdm_wsm_conv_bf16(_lib.ptr(Xd), ldx, xoff, cin, _lib.ptr(wp), _lib.ptr(bd), n, _lib.ptr(out), ldc, coff, B, H, W, k, _lib.stream()))
    xin = X[:, xoff:xoff + cin].reshape(B, H, W, cin).permute(0, 3, 1, 2)
    want = _to_nhwc(F.conv2d(xin, w, b.double(), padding=k // 2))
    _check(out.cpu(), want, coff, n, ldc)


def run_deconv(dev, B, h, cin, c, key):
    _lib = _L()
    ldx, cp = p32(cin), p32(c)
    X = _nhwc_buffer(key + ".x", B, h, h, ldx)
    w = bfr(rnd(key + ".w", (cin, c, 2, 2), 1.0 / np.sqrt(cin)))
    b = rnd(key + ".b", (c,), 0.5).float()
    wr = torch.zeros(4 * cp, p32(cin), dtype=torch.float64)
    br = torch.zeros(4 * cp, dtype=torch.float32)
    for r in range(2):
        for s in range(2):
            ph = 2 * r + s
            wr[ph * cp:ph * cp + c, :cin] = w[:, :, r, s].t()
            br[ph * cp:ph * cp + c] = b
    ldc = c + 8
    out = torch.full((B * 4 * h * h, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    Xd, wd, bd = X.to(torch.bfloat16).to(dev), _rows(wr).to(torch.bfloat16).to(dev), br.to(dev)
    _lib.check(_lib.lib().rdm_wsm_deconv_bf16(_lib.ptr(Xd), ldx, cin, _lib.ptr(wd), _lib.ptr(bd), c, _lib.ptr(out), ldc, B, h, h, _lib.stream()))
    xin = X[:, :cin].reshape(B, h, h, cin).permute(0, 3, 1, 2)
    want = _to_nhwc(F.conv_transpose2d(xin, w, b.double(), stride=2))
    _check(out.cpu(), want, 0, c, ldc)


def run_strip(dev, B, S, wi, columns, ldx, xoff, ldc, coff, key):
    """wsm_wx3 (columns=0: (3,S)/(1,S) after ZeroPad2d((0,0,1,1)), repeated along W) or wsm_3xh (columns=1: (S,3)/(S,1) after
    ZeroPad2d((1,1,0,0)), repeated along H) on channels [xoff, xoff+wi) of a (B,S,S,ldx) map (pad channels up to p32(wi): finite)."""
    _lib = _L()
    cw = p32(wi)
    X = _nhwc_buffer(key + ".x", B, S, S, ldx)
    shape = (wi, wi, S, 3) if columns else (wi, wi, 3, S)
    w = bfr(rnd(key + ".w", shape, 1.0 / np.sqrt(3 * S * wi)))
    b = rnd(key + ".b", (wi,), 0.5).float()
    wt = w.permute(0, 3, 2, 1) if columns else w.permute(0, 2, 3, 1)             # (n, tap, position, ci)
    wp = _rows(F.pad(wt, (0, cw - wi)).reshape(wi, -1)).to(torch.bfloat16)
    out = torch.full((B * S * S, ldc), float("nan"), dtype=torch.bfloat16, device=dev)
    Xd, wd, bd = X.to(torch.bfloat16).to(dev), wp.to(dev), b.to(dev)
    _lib.check(_lib.lib().rdm_wsm_strip_bf16(_lib.ptr(Xd), ldx, xoff, cw, _lib.ptr(wd), _lib.ptr(bd), wi, _lib.ptr(out), ldc, coff, B, S, int(columns), _lib.stream()))
    xin = X[:, xoff:xoff + wi].reshape(B, S, S, wi).permute(0, 3, 1, 2)
    if columns:
        r = F.conv2d(F.pad(xin, (1, 1, 0, 0)), w, b.double(), stride=(S, 1))
        want = r.repeat(1, 1, r.shape[3], 1)
    else:
        r = F.conv2d(F.pad(xin, (0, 0, 1, 1)), w, b.double(), stride=(1, S))
        want = r.repeat(1, 1, 1, r.shape[2])
    _check(out.cpu(), _to_nhwc(want), coff, wi, ldc)


def run_conv1(dev, B, S, cin, key):
    _lib = _L()
    X = _nhwc_buffer(key + ".x", B, S, S, cin)
    w = bfr(rnd(key + ".w", (1, cin, 1, 1), 1.0 / np.sqrt(cin)))
    b = torch.tensor([2.0], dtype=torch.float32)
    out = torch.full((B * S * S,), float("nan"), dtype=torch.float32, device=dev)
    Xd, wd, bd = X.to(torch.bfloat16).to(dev), pack_conv(w).to(dev), b.to(dev)
    _lib.check(_lib.lib().rdm_wsm_conv1x1_f32(_lib.ptr(Xd), cin, cin, _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(out), B, S, S, _lib.stream()))
    want = F.conv2d(X.reshape(B, S, S, cin).permute(0, 3, 1, 2), w, b.double()).reshape(-1)
    err = (out.cpu().double() - want).abs().max().item()
    assert err <= 1e-5 * want.abs().max().item(), (err, want.abs().max().item())


# ---- operator level: the real WSM geometries at B = 1, 2 and two small odd widths -----------------------------------------------
GEOMS = [(raw, C, S) for raw, C, S in WSM] + [(80, 40, 8), (208, 104, 4)]


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "C%d_S%d" % (g[1], g[2]))
def test_wsm_operators_each_epilogue_mode(dev, geom, B):
    raw, C, S = geom
    h, ki, wi = S // 2, C // 4, C // 8
    kip, wip = p32(ki), p32(wi)
    ldT = 2 * kip + 2 * wip                                                      # the decoder's scratch of the four 1x1 branches
    key = "wsmop.%d.%d.%d" % (C, S, B)
    run_conv(dev, B, h, h, raw, C, 1, raw, 0, p32(C), 0, key + ".ia")            # input_adjustment_layer (plain store)
    run_deconv(dev, B, h, p32(C), C, key + ".dc")                                # deconv1 (pixel shuffle)
    run_conv(dev, B, S, S, p32(C), C, 1, p32(C), 0, C, 0, key + ".f5")           # conv1_1..conv1_5 as one N = C GEMM
    run_conv(dev, B, S, S, kip, ki, 3, ldT, 0, C, ki, key + ".c3")               # conv2_1 3x3 -> slot 1
    run_conv(dev, B, S, S, kip, ki, 5, ldT, kip, C, 2 * ki, key + ".c5")         # conv2_2 5x5 -> slot 2
    run_strip(dev, B, S, wi, True, ldT, 2 * kip + wip, C, 3 * ki, key + ".sh")   # wsm_3xh -> completion_vertical, slot 3
    run_strip(dev, B, S, wi, False, ldT, 2 * kip, C, 3 * ki + wi, key + ".sv")   # wsm_wx3 -> completion_horizontal, slot 4
    run_conv1(dev, B, S, C, key + ".c1")                                         # Decoder.conv1 (f32, one channel)


def test_wsm_operator_argument_errors(dev):
    _lib = _L()
    L = _lib.lib()
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    assert L.rdm_wsm_conv_bf16(_lib.ptr(x), 64, 0, 32, _lib.ptr(x), None, 32, _lib.ptr(x), 64, 0, 1, 8, 8, 7, _lib.stream()) == -1     # kernel size 7
    assert L.rdm_wsm_conv_bf16(_lib.ptr(x), 64, 4, 32, _lib.ptr(x), None, 32, _lib.ptr(x), 64, 0, 1, 8, 8, 1, _lib.stream()) == -1     # xoff not a multiple of 8
    assert L.rdm_wsm_strip_bf16(_lib.ptr(x), 64, 0, 20, _lib.ptr(x), None, 8, _lib.ptr(x), 64, 0, 1, 8, 0, _lib.stream()) == -1       # cin not padded
    assert L.rdm_rel_forward_bf16(5, _lib.ptr(x), 1056, 1, _lib.ptr(x), _lib.ptr(x), 0, _lib.ptr(x), _lib.stream()) == -1
    assert L.rdm_rel_bf16_weight_bytes(11) == 0 and L.rdm_rel_bf16_workspace_bytes(6, 0) == 0


# ---- decoder level ------------------------------------------------------------------------------------------------------------------
def _decoder(did, dev):
    """tests/test_gpu_relative.py::_decoder, eval mode: every float state tensor (running statistics included) from the filler."""
    from md_rdm_amd.network import RDM_Net
    dec = RDM_Net.Decoder(in_channels=1056, num_wsm_layers=did - 6, DORN=False, id=did, quant=RDM_Net.Quantization())
    sd = decoder_state(did)
    with torch.no_grad():
        for key, t in dec.state_dict().items():
            if key in sd:
                t.copy_(sd[key].float())
    return dec.to(dev).eval()


def _spread_rms(got, ref):
    ref = ref.double()
    return (got.double() - ref).pow(2).mean().sqrt().item() / (ref - ref.mean()).pow(2).mean().sqrt().item()


@pytest.mark.parametrize("did", [6, 7, 8, 9, 10])
def test_decoder_bf16_vs_restatement_and_f32_path(dev, did):
    dec = _decoder(did, dev)
    x = decoder_input()
    xd = x.float().to(dev)
    f32 = dec.features(xd)
    dec.set_precision("bf16")
    b16 = dec.features(xd)
    ref = rel_decoder_f64(did, decoder_state(did), x, training=False)
    assert b16.shape == ref.shape == f32.shape and b16.dtype == torch.float32
    assert torch.isfinite(b16).all()
    e_ref = _spread_rms(b16.cpu(), ref)
    e_f32 = _spread_rms(b16.cpu(), f32.cpu())
    print("d_%d bf16 rms/spread vs restatement %.5f vs f32 path %.5f" % (did, e_ref, e_f32))
    assert e_ref <= DEC_BOUND[did] and e_f32 <= DEC_BOUND[did], (e_ref, e_f32)
    again = dec.features(xd)
    assert torch.equal(again, b16)                                               # deterministic: same launch, same bits
    one = dec.features(xd[1:2])                                                  # batch independence (tile choice may differ with M)
    assert _spread_rms(one.cpu(), b16[1:2].cpu()) <= 0.2 * DEC_BOUND[did]
    dec.train()
    with pytest.raises(Exception):
        dec.features(xd)                                                         # bf16 stays inference only


# ---- model level ------------------------------------------------------------------------------------------------------------------
REL = (6, 7, 8, 9, 10)


def _model(dev):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=REL)
    filler.fill_state_dict(m.state_dict())
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def model_io(dev):
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 228, seed=filler.MARGIN_SEEDS["train228"])[0]).to(dev)
    m = _model(dev)
    with torch.no_grad():
        lg32 = m._native_forward(x)
        y32, c32, P32 = m(x)
        m.set_precision("bf16")
        lg16 = m._native_forward_bf16(x)
        y16, c16, P16 = m(x)
    return m, x, (lg32, y32, c32, P32), (lg16, y16, c16, P16)


def test_model_bf16_with_relative_decoders_vs_f32(model_io):
    m, x, (lg32, y32, c32, P32), (lg16, y16, c16, P16) = model_io
    assert len(y16) == len(y32) == 8
    for a, b in zip(y16, y32):
        assert a.shape == b.shape and torch.isfinite(a).all()
    d = (lg16 - lg32).double()
    assert d.abs().max().item() <= 0.04 * lg32.abs().max().item()
    assert d.pow(2).mean().sqrt().item() <= 0.01 * lg32.double().pow(2).mean().sqrt().item()
    dP = (P16.double() - P32.double()).abs()
    assert dP.mean().item() <= 5e-3 and dP.max().item() <= 0.15, (dP.mean().item(), dP.max().item())
    dc = (c16.double() - c32.double()).abs()
    assert dc.max().item() <= 3 and dc.mean().item() <= 0.5, (dc.max().item(), dc.mean().item())
    with torch.no_grad():                                                        # the relative maps themselves, on each path's own encoder output
        m.set_precision("f32")
        m._native_forward(x)
        enc32 = m.encoder_output()
        m.set_precision("bf16")
        m._native_forward_bf16(x)
        enc16 = m.encoder_output_bf16()
        for did in REL:
            dec = getattr(m, "d_%d" % did)
            e = _spread_rms(dec.features_bf16(enc16, 1056, 2).cpu(), dec.features(enc32).cpu())
            print("d_%d map in the model: rms(d)/spread %.4f" % (did, e))
            assert e <= MAP_BOUND, (did, e)
    res = []
    for i, (a, b) in enumerate(zip(y16, y32)):
        a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
        scale = np.sqrt((b ** 2).mean())
        close = np.isclose(a, b, rtol=5e-2, atol=5e-2 * scale).mean()
        rel = np.sqrt(((a - b) ** 2).mean()) / scale
        print("level %d agreement %.4f rms(d)/rms %.4f" % (i, close, rel))
        res.append((i, close, rel))
    for i, close, rel in res:
        assert close >= AGREE and rel <= LEVEL_RMS, (i, close, rel)


def test_model_bf16_deterministic(model_io):
    m, x, _, (lg16, y16, c16, P16) = model_io
    with torch.no_grad():
        y, c, P = m(x)
    for a, b in zip(y, y16):
        assert torch.equal(a, b)
    assert torch.equal(P, P16) and torch.equal(c, c16)


def _d7_map(m):
    enc = m.encoder_output_bf16()
    return m.d_7.features_bf16(enc, 1056, m._last_bf16[2])


def test_prepared_weights_follow_load_state_dict(dev, model_io):
    m, x, _, _ = model_io
    m.set_precision("bf16")
    with torch.no_grad():
        m(x)
        a = _d7_map(m).clone()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd["d_7.conv1.bias"] += 1.0
        m.load_state_dict(sd)
        m(x)
        b = _d7_map(m)
        np.testing.assert_allclose((b - a).cpu().numpy(), 1.0, atol=1e-5)
        sd["d_7.conv1.bias"] -= 1.0
        m.load_state_dict(sd)


def test_prepared_weights_follow_a_training_forward(dev):
    """A train-mode forward updates the relative decoders' running statistics in place (by a kernel: no _version bump); the bf16 eval
    maps afterwards equal those of a freshly prepared model bit for bit."""
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    x = torch.from_numpy(filler.synthetic_batch(2, 228, 228, seed=3)[0]).to(dev)
    m = _model(dev)
    m.set_precision("bf16")
    with torch.no_grad():
        before = [t.clone() for t in m(x)[0]]
        m.train()
        m.set_precision("f32")
        m(x)                                                                     # training forward: running statistics move
        m.eval()
        m.set_precision("bf16")
        after = m(x)[0]
    fresh = DepthEstimationNet(relative_decoders=REL)
    fresh.load_state_dict(m.state_dict())
    fresh = fresh.to(dev).eval().set_precision("bf16")
    with torch.no_grad():
        ref = fresh(x)[0]
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    for a, b in zip(after, ref):
        assert torch.equal(a, b)


def test_train_cli_precision16_with_all_relative_decoders():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-m", "md_rdm_amd.train", "--synthetic", "--dev", "--precision", "16", "--relative_decoders", "6", "7", "8", "9", "10",
                        "--batch_size", "2", "--size", "228", "228"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [l for l in r.stdout.splitlines() if "val_delta1" in l]
    assert line, r.stdout[-2000:]
    v = float(line[-1].split("val_delta1")[1].split(",")[0])
    assert np.isfinite(v)
