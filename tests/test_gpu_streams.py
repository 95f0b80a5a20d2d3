"""-m gpu: every entry point of include/rdm_hip.h that takes an rdm_stream_t, called on a NON-DEFAULT stream (one per module, proven to run beside the null stream) behind a late producer
(tests/stream_probe.py: poisoned buffers, a measured delay, the real inputs copied in on the caller's stream only after it) and compared with the
same call on the null stream - whose value the parity modules tie to float64 oracles and reference goldens.  ROWS is the table: one row per
exported function (tests/test_streams_table_cpu.py holds it against the header); operator rows carry a builder of the smallest case that still
launches several workgroups and takes the kernel's main loop more than once, plan rows (rdm_net_*, rdm_rel_*) name the whole-plan test below that
drives them at B=2 228x228 in deterministic mode.

Comparison: bit for bit, except outputs summed with float / double atomics, which take the tolerance of their own parity test (named at the row).
Delay: calibrated per module (stream_probe.Delay): 1 ms = ~2.4e6 `torch.cuda._sleep` cycles on the MI355X, each case sleeps
max(5 ms, 20 x its null-stream time); the control of each family (CONTROLS) shows that this is enough to catch a call made on the null stream."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import stream_probe as sp
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu

f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16


def _l():
    from md_rdm_amd import _lib
    return _lib


def P(t):
    return _l().ptr(t)


def off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


def chk(rc):
    _l().check(rc)


def desc(*a):
    return _l().ConvDesc(*a)


class Gen:
    """seeded host draws, moved to the device by the builders (on the null stream, before any case runs)"""

    def __init__(self, name, dev):
        self.g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31))
        self.dev = dev

    def n(self, *shape, scale=1.0, dtype=f32):
        return (torch.randn(*shape, generator=self.g) * scale).to(dtype).to(self.dev)

    def u(self, *shape, lo=0.0, hi=1.0, dtype=f32):
        return (torch.rand(*shape, generator=self.g, dtype=f64) * (hi - lo) + lo).to(dtype).to(self.dev)

    def z(self, *shape, dtype=f32):
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    def e(self, *shape, dtype=f32):
        return torch.empty(*shape, dtype=dtype, device=self.dev)


# tolerances of the outputs that are summed with float / double atomics, each from the parity test of its entry point
TOL_CONV = 2e-5         # tests/test_gpu_conv.py::test_conv_family (TOL): K-split partial sums added with f32 atomics
TOL_STAT_FWD = 1e-6     # tests/test_gpu_conv.py::test_conv_family: the statistics epilogue's f64 atomics
TOL_STAT_BWD = 1e-5     # tests/test_gpu_conv.py::test_conv_family / tests/test_gpu_xsplit.py::test_xs_dgrad1x1_vs_float64: gate sums
TOL_BN = 2e-5           # tests/test_gpu_bnpool.py::test_bn_relu_forward_backward (TOL): column sums with f64 atomics
TOL_LOSS = 2e-6         # tests/test_gpu_ops.py::test_ordinal_loss
TOL_METRICS = 1e-11     # tests/test_gpu_ops.py::test_validation_metrics_vs_reference

CB, CH, CW, CIN, COUT = 2, 9, 11, 96, 48          # (2, 9, 11, 96, ...): the small case of the xsplit / deferred-norm1 operator tests; 198 pixels = two 128-pixel tiles
CM = CB * CH * CW


def _conv_common(g, kh=3):
    x = g.n(CB, CH, CW, CIN)
    w = g.n(kh * kh, COUT, CIN, scale=1.0 / math.sqrt(CIN * kh * kh))
    sc, sh = g.u(CIN, lo=0.5, hi=1.5), g.n(CIN, scale=0.3)
    d = desc(CB, CH, CW, CIN, CIN, COUT, COUT, kh, kh, 1, 1, kh // 2, kh // 2)
    return x, w, sc, sh, d


def row_conv2d_fwd(dev):
    g = Gen("fwd", dev)
    x, w, sc, sh, d = _conv_common(g)
    L = _l().lib()
    return sp.Case(dict(x=x, w=w, sc=sc, sh=sh, s=g.z(COUT, dtype=f64), q=g.z(COUT, dtype=f64)),
                   lambda b, st: chk(L.rdm_conv2d_fwd(C.byref(d), P(b["x"]), P(b["w"]), None, P(b["sc"]), P(b["sh"]), P(b["y"]), P(b["s"]), P(b["q"]), st)),
                   outs=("y", "s", "q"), scratch=dict(y=g.e(CM, COUT)), tol=dict(y=TOL_CONV, s=TOL_STAT_FWD, q=TOL_STAT_FWD))


def row_conv2d_fwd_ex(dev):
    g = Gen("fwd_ex", dev)
    x, w, sc, sh, d = _conv_common(g, 1)
    L = _l().lib()
    bias = g.n(COUT)
    return sp.Case(dict(x=x, w=w, bias=bias),
                   lambda b, st: chk(L.rdm_conv2d_fwd_ex(C.byref(d), P(b["x"]), P(b["w"]), P(b["bias"]), None, None, P(b["y"]), None, None, 1, st)),
                   outs=("y",), scratch=dict(y=g.e(CM, COUT)))                       # split_k = 1: one workgroup per element, bit-reproducible


def _dgrad(dev, name, ex):
    g = Gen(name, dev)
    x, w, sc, sh, d = _conv_common(g)
    dy = g.n(CM, COUT)
    L = _l().lib()
    ins = dict(x=x, w=w, sc=sc, sh=sh, dy=dy, s0=g.z(CIN, dtype=f64), s1=g.z(CIN, dtype=f64))
    if ex:      # split_k = 3: the ATOMIC / MASK_STATS_ATOMIC epilogues (the launcher zero-fills dx on the caller's stream first)
        call = lambda b, st: chk(L.rdm_conv2d_dgrad_ex(C.byref(d), P(b["dy"]), P(b["w"]), P(b["dx"]), CIN, P(b["x"]), CIN, P(b["sc"]), P(b["sh"]), P(b["s0"]), P(b["s1"]), 3, st))
    else:
        call = lambda b, st: chk(L.rdm_conv2d_dgrad(C.byref(d), P(b["dy"]), P(b["w"]), P(b["dx"]), CIN, P(b["x"]), CIN, P(b["sc"]), P(b["sh"]), P(b["s0"]), P(b["s1"]), st))
    return sp.Case(ins, call, outs=("dx", "s0", "s1"), scratch=dict(dx=g.e(CM, CIN)), tol=dict(dx=TOL_CONV, s0=TOL_STAT_BWD, s1=TOL_STAT_BWD))


def row_conv2d_dgrad(dev):
    return _dgrad(dev, "dgrad", False)


def row_conv2d_dgrad_ex(dev):
    return _dgrad(dev, "dgrad_ex", True)


def _wgrad(dev, name, ex):
    g = Gen(name, dev)
    x, w, sc, sh, d = _conv_common(g)
    dy = g.n(CM, COUT)
    L = _l().lib()
    ins = dict(x=x, sc=sc, sh=sh, dy=dy, dw=g.z(9, COUT, CIN))                       # dw: pre-zeroed by the caller, accumulated with f32 atomics
    if ex:
        call = lambda b, st: chk(L.rdm_conv2d_wgrad_ex(C.byref(d), P(b["dy"]), P(b["x"]), P(b["sc"]), P(b["sh"]), P(b["dw"]), 3, st))
    else:
        call = lambda b, st: chk(L.rdm_conv2d_wgrad(C.byref(d), P(b["dy"]), P(b["x"]), P(b["sc"]), P(b["sh"]), P(b["dw"]), st))
    return sp.Case(ins, call, outs=("dw",), tol=dict(dw=TOL_CONV))


def row_conv2d_wgrad(dev):
    return _wgrad(dev, "wgrad", False)


def row_conv2d_wgrad_ex(dev):
    return _wgrad(dev, "wgrad_ex", True)


def _bnsums(g, x):
    xs = x.double().reshape(-1, x.shape[-1])
    return xs.sum(0).contiguous(), (xs * xs).sum(0).contiguous(), g.u(x.shape[-1], lo=0.5, hi=1.5), g.n(x.shape[-1], scale=0.3)


def row_conv2d_fwd_bnsums(dev):
    g = Gen("bnsums", dev)
    x, w, _, _, d = _conv_common(g)
    s, q, gamma, beta = _bnsums(g, x)
    L = _l().lib()
    return sp.Case(dict(x=x, w=w, s=s, q=q, gamma=gamma, beta=beta),
                   lambda b, st: chk(L.rdm_conv2d_fwd_bnsums(C.byref(d), P(b["x"]), P(b["w"]), P(b["s"]), P(b["q"]), float(CM), P(b["gamma"]), P(b["beta"]), P(b["y"]),
                                                             None, None, 1, st)),
                   outs=("y",), scratch=dict(y=g.e(CM, COUT)))


def row_conv3x3_fwd_bnsums_acc(dev):
    g = Gen("bnsums_acc", dev)
    x, w, _, _, d = _conv_common(g)
    s, q, gamma, beta = _bnsums(g, x)
    L = _l().lib()
    ins = dict(x=x, w=w, s=s, q=q, gamma=gamma, beta=beta, y=g.z(CM, COUT), s0=g.z(COUT, dtype=f64), s1=g.z(COUT, dtype=f64),
               tickets=g.z((CM + 127) // 128, dtype=torch.int32))
    return sp.Case(ins, lambda b, st: chk(L.rdm_conv3x3_fwd_bnsums_acc(C.byref(d), P(b["x"]), P(b["w"]), P(b["s"]), P(b["q"]), float(CM), P(b["gamma"]), P(b["beta"]),
                                                                       P(b["y"]), P(b["s0"]), P(b["s1"]), P(b["tickets"]), 3, st)),
                   outs=("y", "s0", "s1", "tickets"), tol=dict(y=TOL_CONV, s0=TOL_STAT_BWD, s1=TOL_STAT_BWD))   # tests/test_gpu_conv.py::test_conv_fwd_with_raw_batchnorm_sums


def row_frame_split_rows_f32(dev):
    g = Gen("frame", dev)
    L = _l().lib()
    B, H, W, N = 2, 9, 7, 48                                                          # the tiny frame of tests/test_gpu_xsplit.py WGRAD3_CASES
    dy = g.n(B, H, W, N)
    fb = int(L.rdm_frame_split_rows_bytes(B, H, W))
    return sp.Case(dict(dy=dy), lambda b, st: chk(L.rdm_frame_split_rows_f32(P(b["dy"]), N, N, B, H, W, P(b["dst"]), st)), outs=("dst",), scratch=dict(dst=g.e(fb // 4)))


def row_split_rows_f32(dev):
    g = Gen("split_rows", dev)
    L = _l().lib()
    M, Cc, ld, ldd = 1037, 144, 160, 148                                              # tests/test_gpu_xsplit.py::test_split_rows_producers_are_bit_exact
    return sp.Case(dict(x=g.n(M, ld), sc=g.u(Cc, lo=0.5, hi=1.5), sh=g.n(Cc, scale=0.3)),
                   lambda b, st: chk(L.rdm_split_rows_f32(P(b["x"]), ld, P(b["sc"]), P(b["sh"]), P(b["dst"]), ldd, M, Cc, st)), outs=("dst",), scratch=dict(dst=g.e(M, ldd)))


def row_conv2d_wgrad_x3(dev):
    g = Gen("wgrad_x3", dev)
    L = _l().lib()
    Cc, N = 144, 96
    d = desc(CB, CH, CW, Cc, Cc, N, N, 1, 1, 1, 1, 0, 0)
    ins = dict(x=g.n(CM, Cc), dy=g.n(CM, N), sc=g.u(Cc, lo=0.5, hi=1.5), sh=g.n(Cc, scale=0.3), dw=g.z(N, Cc))
    return sp.Case(ins, lambda b, st: chk(L.rdm_conv2d_wgrad_x3(C.byref(d), P(b["dy"]), P(b["x"]), P(b["sc"]), P(b["sh"]), P(b["dw"]), 3, 0, st)),
                   outs=("dw",), tol=dict(dw=TOL_CONV))                               # tests/test_gpu_xsplit.py::test_xs_wgrad1x1_vs_float64 (TOL 2e-5), K split of 3


def row_conv1x1_fwd_x6(dev):
    g = Gen("fwd_x6", dev)
    L = _l().lib()
    K, N = 96, 208
    d = desc(CB, CH, CW, K, K, N, N, 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_fwd_x6_workspace_bytes(K, N))
    return sp.Case(dict(x=g.n(CM, K), w=g.n(N, K, scale=K ** -0.5), sc=g.u(K, lo=0.5, hi=1.5), sh=g.n(K, scale=0.3)),
                   lambda b, st: chk(L.rdm_conv1x1_fwd_x6(C.byref(d), P(b["x"]), P(b["w"]), P(b["sc"]), P(b["sh"]), P(b["y"]), None, None, P(b["ws"]), wsb, 0, st)),
                   outs=("y",), scratch=dict(y=g.e(CM, N), ws=g.e(wsb, dtype=torch.uint8)))


def row_conv1x1_dgrad_x3(dev):
    g = Gen("dgrad1_x3", dev)
    L = _l().lib()
    K, N = 144, 96                                                                    # K contracted (bottleneck), N outputs: DGRAD1_CASES' short-K case
    d = desc(CB, CH, CW, N, N, K, K, 1, 1, 1, 1, 0, 0)
    wsb = int(L.rdm_conv1x1_dgrad_x3_workspace_bytes(K, N))
    ins = dict(dy=g.n(CM, K), w=g.n(K, N, scale=K ** -0.5), x=g.n(CM, N), sc=g.u(N, lo=0.5, hi=1.5), sh=g.n(N, scale=0.3), s0=g.z(N, dtype=f64), s1=g.z(N, dtype=f64))
    return sp.Case(ins, lambda b, st: chk(L.rdm_conv1x1_dgrad_x3(C.byref(d), P(b["dy"]), P(b["w"]), P(b["dz"]), N, P(b["x"]), N, P(b["sc"]), P(b["sh"]), P(b["s0"]), P(b["s1"]),
                                                                  P(b["ws"]), wsb, 0, st)),
                   outs=("dz", "s0", "s1"), scratch=dict(dz=g.e(CM, N), ws=g.e(wsb, dtype=torch.uint8)), tol=dict(s0=TOL_STAT_BWD, s1=TOL_STAT_BWD))


def row_conv3x3_dgrad_x3(dev):
    g = Gen("dgrad3_x3", dev)
    L = _l().lib()
    B, H, W, Cb, N = 3, 9, 7, 96, 48                                                  # tests/test_gpu_xsplit.py DGRAD3_CASES[2]
    M = B * H * W
    d = desc(B, H, W, Cb, Cb, N, N, 3, 3, 1, 1, 1, 1)
    wsb = int(L.rdm_conv3x3_dgrad_x3_workspace_bytes(Cb))
    return sp.Case(dict(dy=g.n(M, N), w=g.n(9, N, Cb, scale=(9 * N) ** -0.5)),
                   lambda b, st: chk(L.rdm_conv3x3_dgrad_x3(C.byref(d), P(b["dy"]), P(b["w"]), P(b["dx"]), Cb, None, 0, None, None, None, None, P(b["ws"]), wsb, 0, st)),
                   outs=("dx",), scratch=dict(dx=g.e(M, Cb), ws=g.e(wsb, dtype=torch.uint8)))


def _wino_fwd(dev, x6):
    g = Gen("wino" + str(x6), dev)
    L = _l().lib()
    B, H, W, Cb, ld, N = 3, 8, 10, 384, 400, 48                                       # tests/test_gpu_wino.py CASES[2]
    M = B * H * W
    d = desc(B, H, W, Cb, ld, N, 64, 3, 3, 1, 1, 1, 1)
    nb = int((L.rdm_conv3x3_wino_x6_workspace_bytes if x6 else L.rdm_conv3x3_wino_workspace_bytes)(Cb, B, H, W, 3))
    fn = L.rdm_conv3x3_wino_fwd_x6 if x6 else L.rdm_conv3x3_wino_fwd
    ins = dict(x=g.n(B, H, W, ld), w=g.n(9, N, Cb, scale=(9 * Cb) ** -0.5), sc=g.u(Cb, lo=0.5, hi=1.5), sh=g.n(Cb, scale=0.3))
    return sp.Case(ins, lambda b, st: chk(fn(C.byref(d), P(b["x"]), P(b["w"]), P(b["sc"]), P(b["sh"]), P(b["y"]), None, None, P(b["ws"]), nb, 3, st)),
                   outs=("y",), scratch=dict(y=g.e(M, 64), ws=g.e(max(nb, 256), dtype=torch.uint8)))   # K split of 3, partials summed in a fixed order: bits


def row_conv3x3_wino_fwd(dev):
    return _wino_fwd(dev, False)


def row_conv3x3_wino_fwd_x6(dev):
    return _wino_fwd(dev, True)


def row_conv3x3_wino_wgrad(dev):
    g = Gen("wino_wgrad", dev)
    L = _l().lib()
    B, H, W, Cb, N = 2, 9, 9, 64, 48                                                  # tests/test_gpu_wino.py WGRAD_CASES[4]
    d = desc(B, H, W, Cb, Cb, N, N, 3, 3, 1, 1, 1, 1)
    nb = int(L.rdm_conv3x3_wino_wgrad_workspace_bytes(Cb, B, H, W))
    ins = dict(x=g.n(B, H, W, Cb), dy=g.n(B, H, W, N), sc=g.u(Cb, lo=0.5, hi=1.5), sh=g.n(Cb, scale=0.3))
    return sp.Case(ins, lambda b, st: chk(L.rdm_conv3x3_wino_wgrad(C.byref(d), P(b["dy"]), P(b["x"]), P(b["sc"]), P(b["sh"]), P(b["dw"]), P(b["ws"]), nb, st)),
                   outs=("dw",), scratch=dict(dw=g.e(9, N, Cb), ws=g.e(nb, dtype=torch.uint8)))


def row_pack_conv_weight(dev):
    g = Gen("pack", dev)
    L = _l().lib()
    return sp.Case(dict(w=g.n(COUT, CIN, 3, 3)), lambda b, st: chk(L.rdm_pack_conv_weight(P(b["w"]), P(b["wp"]), COUT, CIN, 3, 3, 64, st)), outs=("wp",),
                   scratch=dict(wp=g.e(9, 64, CIN)))                                  # rows 48..63 zero-filled by the kernel


def row_unpack_conv_weight(dev):
    g = Gen("unpack", dev)
    L = _l().lib()
    return sp.Case(dict(wp=g.n(9, COUT, CIN)), lambda b, st: chk(L.rdm_unpack_conv_weight(P(b["wp"]), P(b["w"]), COUT, CIN, 3, 3, COUT, st)), outs=("w",),
                   scratch=dict(w=g.e(COUT, CIN, 3, 3)))


# ---- bf16 ----------------------------------------------------------------------------------------------------------------------------
def row_gemm_bf16(dev):
    g = Gen("gemm_bf16", dev)
    L = _l().lib()
    M, K, N = 77, 160, 96                                                             # tests/test_gpu_bf16.py::test_gemm_bf16_operator, with the few-row K split
    nb = 8 * M * N * 4
    ins = dict(x=g.u(M, K, lo=-2, hi=2, dtype=bf16), w=g.u(N, K, lo=-0.1, hi=0.1, dtype=bf16), sc=g.u(K, lo=0.5, hi=1.5), sh=g.n(K, scale=0.3), bias=g.n(N))
    return sp.Case(ins, lambda b, st: chk(L.rdm_gemm_bf16(P(b["x"]), K, K, P(b["sc"]), P(b["sh"]), P(b["w"]), K, P(b["bias"]), P(b["out"]), N + 12, M, N, 0, P(b["ws"]), nb, st)),
                   outs=("out",), scratch=dict(out=g.e(M, N + 12, dtype=bf16), ws=g.e(nb, dtype=torch.uint8)))


def row_gemm_bf16_act(dev):
    g = Gen("gemm_bf16_act", dev)
    L = _l().lib()
    M, K, N = 285, 208, 96
    nb = 8 * M * N * 4
    ins = dict(x=g.u(M, K, lo=-2, hi=2, dtype=bf16), w=g.u(N, K, lo=-0.1, hi=0.1, dtype=bf16), sc=g.u(K, lo=0.5, hi=1.5), sh=g.n(K, scale=0.3),
               osc=g.u(N, lo=-1.5, hi=1.5), osh=g.n(N, scale=0.3))
    return sp.Case(ins, lambda b, st: chk(L.rdm_gemm_bf16_act(P(b["x"]), K, K, P(b["sc"]), P(b["sh"]), P(b["w"]), K, P(b["osc"]), P(b["osh"]), P(b["out"]), N + 8, M, N,
                                                               P(b["ws"]), nb, st)),
                   outs=("out",), scratch=dict(out=g.e(M, N + 8, dtype=bf16), ws=g.e(nb, dtype=torch.uint8)))


def _c3_bf16(dev, stats):
    g = Gen("c3_bf16" + str(stats), dev)
    L = _l().lib()
    B, H, W, Cc, ldc, coff = 2, 6, 7, 384, 112, 48                                    # tests/test_gpu_relative_bf16_train.py CONV_GEOMS[-1]
    M = B * H * W
    ins = dict(y=g.u(M, Cc, lo=-2, hi=2, dtype=bf16), w=g.u(9, 48, Cc, lo=-0.05, hi=0.05, dtype=bf16), sc=g.u(Cc, lo=0.5, hi=1.5), sh=g.n(Cc, scale=0.3))
    if stats:
        nb = int(L.rdm_bf16_stats_workspace_bytes(M, 48)) + 4 * 16 * M * 48          # + room for the K split's partial sums
        call = lambda b, st: chk(L.rdm_conv3x3_bf16_stats(P(b["y"]), Cc, Cc, P(b["sc"]), P(b["sh"]), P(b["w"]), off(b["out"], 2 * coff), ldc, B, H, W, P(b["s"]), P(b["q"]),
                                                          P(b["ws"]), nb, st))
        return sp.Case(ins, call, outs=("out", "s", "q"), scratch=dict(out=g.e(M, ldc, dtype=bf16), s=g.e(48, dtype=f64), q=g.e(48, dtype=f64), ws=g.e(nb, dtype=torch.uint8)))
    nb = 3 * M * 48 * 4                                                               # a K split squeezed into 3 slabs (tests/test_gpu_bf16.py::test_conv3x3_bf16_operator)
    call = lambda b, st: chk(L.rdm_conv3x3_bf16(P(b["y"]), Cc, Cc, P(b["sc"]), P(b["sh"]), P(b["w"]), off(b["out"], 2 * coff), ldc, B, H, W, P(b["ws"]), nb, st))
    return sp.Case(ins, call, outs=("out",), scratch=dict(out=g.e(M, ldc, dtype=bf16), ws=g.e(nb, dtype=torch.uint8)))


def row_conv3x3_bf16(dev):
    return _c3_bf16(dev, False)


def row_conv3x3_bf16_stats(dev):
    return _c3_bf16(dev, True)


def row_gemm_bf16_stats(dev):
    g = Gen("gemm_stats", dev)
    L = _l().lib()
    M, N, K = 100, 200, 1056                                                          # tests/test_gpu_relative_bf16_train.py GEMM_GEOMS[-1], K split
    ldx = K + 48
    nb = int(L.rdm_bf16_stats_workspace_bytes(M, N)) + 4 * 8 * M * N
    ins = dict(x=g.u(M, ldx, lo=-1, hi=1, dtype=bf16), w=g.u(N, K, lo=-K ** -0.5, hi=K ** -0.5, dtype=bf16), sc=g.u(K, lo=0.5, hi=1.5), sh=g.n(K, scale=0.3))
    return sp.Case(ins, lambda b, st: chk(L.rdm_gemm_bf16_stats(P(b["x"]), ldx, K, P(b["sc"]), P(b["sh"]), P(b["w"]), K, P(b["out"]), N, M, N, P(b["s"]), P(b["q"]),
                                                                 P(b["ws"]), nb, st)),
                   outs=("out", "s", "q"), scratch=dict(out=g.e(M, N, dtype=bf16), s=g.e(N, dtype=f64), q=g.e(N, dtype=f64), ws=g.e(nb, dtype=torch.uint8)))


ACT_B, ACT_H, ACT_W, ACT_C = 5, 9, 13, 64                                             # tests/test_gpu_bf16.py::test_conv3x3_act_bf16_operator


def row_conv3x3_act_bf16_pack(dev):
    g = Gen("act_pack", dev)
    L = _l().lib()
    nb = int(L.rdm_conv3x3_act_bf16_weight_bytes(ACT_C))
    return sp.Case(dict(w=g.u(48, ACT_C, 3, 3, lo=-0.05, hi=0.05)), lambda b, st: chk(L.rdm_conv3x3_act_bf16_pack(P(b["w"]), ACT_C, P(b["img"]), st)), outs=("img",),
                   scratch=dict(img=g.e(nb, dtype=torch.uint8)))


def row_conv3x3_act_bf16(dev):
    g = Gen("act", dev)
    L = _l().lib()
    B, H, W, Cp = ACT_B, ACT_H, ACT_W, ACT_C
    M, ldy, ldc = B * H * W, Cp + 8, 96
    w = g.u(48, ACT_C, 3, 3, lo=-0.05, hi=0.05)
    img = g.e(int(L.rdm_conv3x3_act_bf16_weight_bytes(ACT_C)), dtype=torch.uint8)
    chk(L.rdm_conv3x3_act_bf16_pack(P(w), ACT_C, P(img), None))                      # the weight image is an INPUT of this row (null stream, before any case runs)
    torch.cuda.synchronize()
    nb = 16384 + 2 * 512 * 48 * 4 * B * ((H * W + 127) // 128)                        # a tight K-split scratch: tile counters (zeroed by the entry point) + partial sums
    ins = dict(y=torch.relu(g.u(B, H, W, ldy, lo=-2, hi=2)).to(bf16), img=img)
    return sp.Case(ins, lambda b, st: chk(L.rdm_conv3x3_act_bf16(P(b["y"]), ldy, Cp, P(b["img"]), off(b["out"], 2 * 16), ldc, B, H, W, P(b["ws"]), nb, st)),
                   outs=("out",), scratch=dict(out=g.e(M, ldc, dtype=bf16), ws=g.e(nb, dtype=torch.uint8)))


def row_colstats_bf16(dev):
    g = Gen("colstats", dev)
    L = _l().lib()
    M, Cc, ld = 128, 1056, 1064                                                       # tests/test_gpu_relative_bf16_train.py::test_colstats_bf16, B = 2
    return sp.Case(dict(x=g.u(M, ld, lo=-2, hi=3, dtype=bf16)), lambda b, st: chk(L.rdm_colstats_bf16(P(b["x"]), ld, M, Cc, P(b["s"]), P(b["q"]), st)), outs=("s", "q"),
                   scratch=dict(s=g.e(Cc, dtype=f64), q=g.e(Cc, dtype=f64)))


# the helper kernels of the bf16 forward (tests/test_gpu_bf16_exact.py holds their values to float64 references)
def row_stem_patches_bf16(dev):
    g = Gen("stem_patches", dev)
    L = _l().lib()
    B, H, W = 2, 31, 30                                                                # 16 x 15 output pixels x 80 threads each: 150 workgroups
    M = B * 16 * 15
    return sp.Case(dict(x=g.n(B, 3, H, W)), lambda b, st: chk(L.rdm_stem_patches_bf16(P(b["x"]), P(b["p"]), B, H, W, st)), outs=("p",), scratch=dict(p=g.e(M, 160, dtype=bf16)))


def row_maxpool3s2_bf16(dev):
    g = Gen("maxpool_bf16", dev)
    L = _l().lib()
    B, H, W, Cc, ldy = 2, 15, 14, 96, 104
    M = B * 8 * 7
    return sp.Case(dict(x=g.n(B, H, W, Cc, dtype=bf16)), lambda b, st: chk(L.rdm_maxpool3s2_bf16(P(b["x"]), P(b["y"]), ldy, B, H, W, Cc, st)), outs=("y",),
                   scratch=dict(y=g.e(M, ldy, dtype=bf16)))


def row_padavgpool2_bf16(dev):
    g = Gen("padavgpool_bf16", dev)
    L = _l().lib()
    B, H, W, Cc, ldx = 2, 15, 13, 96, 104
    M = B * 8 * 7
    ins = dict(x=g.n(B, H, W, ldx, dtype=bf16), sc=g.u(Cc, lo=0.5, hi=1.5), sh=g.n(Cc, scale=0.3))
    return sp.Case(ins, lambda b, st: chk(L.rdm_padavgpool2_bf16(P(b["x"]), ldx, P(b["sc"]), P(b["sh"]), P(b["out"]), B, H, W, Cc, st)), outs=("out",),
                   scratch=dict(out=g.e(M, Cc, dtype=bf16)))


def row_f32_to_bf16_rows(dev):
    g = Gen("rows_bf16", dev)
    L = _l().lib()
    rows, cols, cols_pad, lds, ldd = 96, 147, 160, 152, 168                            # the stem weight's conversion, in wider buffers
    return sp.Case(dict(src=g.n(rows, lds)), lambda b, st: chk(L.rdm_f32_to_bf16_rows(P(b["src"]), lds, P(b["dst"]), ldd, rows, cols, cols_pad, st)), outs=("dst",),
                   scratch=dict(dst=g.e(rows, ldd, dtype=bf16)))


def row_pack_conv_weight_bf16(dev):
    g = Gen("pack_bf16", dev)
    L = _l().lib()
    O, I, ld = 48, 136, 160
    return sp.Case(dict(w=g.n(O, I, 3, 3)), lambda b, st: chk(L.rdm_pack_conv_weight_bf16(P(b["w"]), P(b["wp"]), O, I, ld, 9, st)), outs=("wp",),
                   scratch=dict(wp=g.e(9, O, ld, dtype=bf16)))


def _p32(c):
    return (c + 31) // 32 * 32


def _rows64(w2d):
    return F.pad(w2d, (0, 0, 0, (w2d.shape[0] + 63) // 64 * 64 - w2d.shape[0]))


def row_wsm_conv_bf16(dev):
    g = Gen("wsm_conv", dev)
    L = _l().lib()
    B, S, cin, n, k, ldx, xoff, ldc, coff = 2, 8, 32, 24, 3, 64, 32, 40, 8           # the conv2_1 form of tests/test_gpu_relative_bf16.py (slot of a wider scratch)
    w = torch.randn(n, cin, k, k, generator=g.g) / math.sqrt(cin * k * k)
    wp = _rows64(F.pad(w.permute(0, 2, 3, 1), (0, _p32(cin) - cin)).reshape(n, -1)).to(bf16).to(dev)
    ins = dict(x=g.u(B * S * S, ldx, lo=-1, hi=1, dtype=bf16), w=wp, bias=g.n(n, scale=0.5))
    return sp.Case(ins, lambda b, st: chk(L.rdm_wsm_conv_bf16(P(b["x"]), ldx, xoff, cin, P(b["w"]), P(b["bias"]), n, P(b["out"]), ldc, coff, B, S, S, k, st)), outs=("out",),
                   scratch=dict(out=g.e(B * S * S, ldc, dtype=bf16)))


def row_wsm_deconv_bf16(dev):
    g = Gen("wsm_deconv", dev)
    L = _l().lib()
    B, h, cin, c = 2, 4, 32, 24
    cp, ldc = _p32(c), c + 8
    w = torch.randn(cin, c, 2, 2, generator=g.g) / math.sqrt(cin)
    bv = torch.randn(c, generator=g.g) * 0.5
    wr, br = torch.zeros(4 * cp, _p32(cin)), torch.zeros(4 * cp)
    for r in range(2):
        for s in range(2):
            ph = 2 * r + s
            wr[ph * cp:ph * cp + c, :cin] = w[:, :, r, s].t()
            br[ph * cp:ph * cp + c] = bv
    ins = dict(x=g.u(B * h * h, _p32(cin), lo=-1, hi=1, dtype=bf16), w=_rows64(wr).to(bf16).to(dev), bias=br.to(dev))
    return sp.Case(ins, lambda b, st: chk(L.rdm_wsm_deconv_bf16(P(b["x"]), _p32(cin), cin, P(b["w"]), P(b["bias"]), c, P(b["out"]), ldc, B, h, h, st)), outs=("out",),
                   scratch=dict(out=g.e(B * 4 * h * h, ldc, dtype=bf16)))


def row_wsm_strip_bf16(dev):
    g = Gen("wsm_strip", dev)
    L = _l().lib()
    B, S, wi, ldx, xoff, ldc, coff = 2, 8, 13, 64, 32, 24, 8
    cw = _p32(wi)
    w = torch.randn(wi, wi, S, 3, generator=g.g) / math.sqrt(3 * S * wi)              # wsm_3xh (columns = 1)
    wp = _rows64(F.pad(w.permute(0, 3, 2, 1), (0, cw - wi)).reshape(wi, -1)).to(bf16).to(dev)
    ins = dict(x=g.u(B * S * S, ldx, lo=-1, hi=1, dtype=bf16), w=wp, bias=g.n(wi, scale=0.5))
    return sp.Case(ins, lambda b, st: chk(L.rdm_wsm_strip_bf16(P(b["x"]), ldx, xoff, cw, P(b["w"]), P(b["bias"]), wi, P(b["out"]), ldc, coff, B, S, 1, st)), outs=("out",),
                   scratch=dict(out=g.e(B * S * S, ldc, dtype=bf16)))


def row_wsm_conv1x1_f32(dev):
    g = Gen("wsm_c1", dev)
    L = _l().lib()
    B, S, cin = 2, 8, 64
    wp = _rows64(torch.randn(1, cin, generator=g.g) / math.sqrt(cin)).to(bf16).to(dev)
    ins = dict(x=g.u(B * S * S, cin, lo=-1, hi=1, dtype=bf16), w=wp, bias=torch.tensor([2.0], device=dev))
    return sp.Case(ins, lambda b, st: chk(L.rdm_wsm_conv1x1_f32(P(b["x"]), cin, cin, P(b["w"]), P(b["bias"]), P(b["out"]), B, S, S, st)), outs=("out",),
                   scratch=dict(out=g.e(B * S * S)))


# ---- BatchNorm / pools / layout --------------------------------------------------------------------------------------------------------
NB, NH, NW, NC, NLD = 3, 8, 10, 100, 100                                              # (3, 8, 10, 100, 100) of tests/test_gpu_bnpool.py
NM = NB * NH * NW


def row_bn_stats(dev):
    g = Gen("bn_stats", dev)
    L = _l().lib()
    return sp.Case(dict(x=g.u(NM, NLD, lo=-2, hi=2), s=g.z(NC, dtype=f64), q=g.z(NC, dtype=f64)),
                   lambda b, st: chk(L.rdm_bn_stats(P(b["x"]), NLD, NM, NC, P(b["s"]), P(b["q"]), st)), outs=("s", "q"), tol=dict(s=TOL_BN, q=TOL_BN))


def _bn_moments(x):
    xs = x.double()
    mean, var = xs.mean(0), xs.var(0, unbiased=False)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def row_bn_finalize(dev):
    g = Gen("bn_finalize", dev)
    L = _l().lib()
    x = g.u(NM, NC, lo=-2, hi=2).double()
    ins = dict(s=x.sum(0), q=(x * x).sum(0), gamma=g.u(NC, lo=0.5, hi=1.5), beta=g.n(NC, scale=0.3), rm=g.n(NC, scale=0.2), rv=g.u(NC, lo=0.5, hi=1.5),
               nbt=torch.full((1,), 3, dtype=torch.int64, device=dev))
    row = lambda t, i: off(t, i * NC * 4)
    return sp.Case(ins, lambda b, st: chk(L.rdm_bn_finalize(P(b["s"]), P(b["q"]), float(NM), P(b["gamma"]), P(b["beta"]), P(b["rm"]), P(b["rv"]), P(b["nbt"]),
                                                             row(b["coef"], 0), row(b["coef"], 1), row(b["coef"], 2), row(b["coef"], 3), NC, 1, st)),
                   outs=("rm", "rv", "nbt", "coef"), scratch=dict(coef=g.e(4, NC)))


def row_bn_bwd_reduce(dev):
    g = Gen("bn_bwd_reduce", dev)
    L = _l().lib()
    ins = dict(dz=g.n(NM, NLD), x=g.u(NM, NLD, lo=-2, hi=2), sc=g.u(NC, lo=0.5, hi=1.5), sh=g.n(NC, scale=0.3), r0=g.z(NC, dtype=f64), r1=g.z(NC, dtype=f64))
    return sp.Case(ins, lambda b, st: chk(L.rdm_bn_bwd_reduce(P(b["dz"]), NLD, P(b["x"]), NLD, P(b["sc"]), P(b["sh"]), NM, NC, P(b["r0"]), P(b["r1"]), st)),
                   outs=("dz", "r0", "r1"), tol=dict(r0=TOL_BN, r1=TOL_BN))


def row_bn_bwd(dev):
    g = Gen("bn_bwd", dev)
    L = _l().lib()
    x, dz = g.u(NM, NLD, lo=-2, hi=2), g.n(NM, NLD)
    mean, rstd = _bn_moments(x)
    ins = dict(x=x, dz=dz, r0=dz.double().sum(0), r1=(dz.double() * x.double()).sum(0), gamma=g.u(NC, lo=0.5, hi=1.5), mean=mean.float(), rstd=rstd.float())
    return sp.Case(ins, lambda b, st: chk(L.rdm_bn_bwd(P(b["dx"]), NLD, P(b["dz"]), NLD, P(b["x"]), NLD, P(b["r0"]), P(b["r1"]), float(NM), P(b["gamma"]), P(b["mean"]),
                                                        P(b["rstd"]), P(b["dg"]), P(b["db"]), NM, NC, 0, 1, st)),
                   outs=("dx", "dg", "db"), scratch=dict(dx=g.e(NM, NLD), dg=g.e(NC), db=g.e(NC)))


def row_bn_bwd_defer(dev):
    g = Gen("bn_bwd_defer", dev)
    L = _l().lib()
    cin, ctot = 96, 144                                                               # "small" of tests/test_gpu_xsplit.py::test_deferred_norm1_backward_operator_level
    x = g.n(CM, ctot)
    mean, rstd = _bn_moments(x[:, :cin])
    ins = dict(G=g.n(CM, ctot), x=x, s0=g.n(cin, dtype=f64), s1=g.n(cin, dtype=f64), gamma=g.u(cin, lo=0.5, hi=1.5), mean=mean.float().contiguous(),
               rstd=rstd.float().contiguous(), b_in=g.n(cin, scale=0.01), c_in=g.n(cin, scale=0.01))
    return sp.Case(ins, lambda b, st: chk(L.rdm_bn_bwd_defer(P(b["G"]), ctot, P(b["x"]), ctot, P(b["s0"]), P(b["s1"]), float(CM), P(b["gamma"]), P(b["mean"]), P(b["rstd"]),
                                                              P(b["dg"]), P(b["db"]), P(b["b_in"]), P(b["c_in"]), P(b["b_out"]), P(b["c_out"]), CM, cin, cin - 48, 48, 1, st)),
                   outs=("G", "dg", "db", "b_out", "c_out"), scratch=dict(dg=g.e(cin), db=g.e(cin), b_out=g.e(cin), c_out=g.e(cin)))


PB, PH, PW, PC, PLD = 3, 16, 16, 20, 32                                               # (3, 16, 16, 20, 32) of tests/test_gpu_bnpool.py::test_maxpool3s2_forward_backward
PHO, PWO = 8, 8


def row_maxpool3s2_fwd(dev):
    g = Gen("maxpool", dev)
    L = _l().lib()
    return sp.Case(dict(x=g.u(PB, PH, PW, PC, lo=-2, hi=2)), lambda b, st: chk(L.rdm_maxpool3s2_fwd(P(b["x"]), P(b["y"]), PLD, P(b["arg"]), PB, PH, PW, PC, st)),
                   outs=("y", "arg"), scratch=dict(y=g.e(PB, PHO, PWO, PLD), arg=g.e(PB, PHO, PWO, PC, dtype=torch.uint8)))


def row_maxpool3s2_bwd(dev):
    g = Gen("maxpool_bwd", dev)
    L = _l().lib()
    x = g.u(PB, PH, PW, PC, lo=-2, hi=2)
    y, arg = g.e(PB, PHO, PWO, PLD), g.e(PB, PHO, PWO, PC, dtype=torch.uint8)
    chk(L.rdm_maxpool3s2_fwd(P(x), P(y), PLD, P(arg), PB, PH, PW, PC, None))        # a valid argmax map is an INPUT of this row
    torch.cuda.synchronize()
    return sp.Case(dict(dy=g.n(PB, PHO, PWO, PLD), arg=arg), lambda b, st: chk(L.rdm_maxpool3s2_bwd(P(b["dy"]), PLD, P(b["arg"]), P(b["dx"]), PB, PH, PW, PC, st)),
                   outs=("dx",), scratch=dict(dx=g.e(PB, PH, PW, PC)))


AB, AH, AW, AC, ALD = 2, 15, 19, 48, 64                                               # (2, 15, 19, 48, 64) of tests/test_gpu_bnpool.py::test_padavgpool2_transition_front_end


def row_padavgpool2_fwd(dev):
    g = Gen("padavg", dev)
    L = _l().lib()
    return sp.Case(dict(x=g.u(AB, AH, AW, ALD, lo=-2, hi=2), sc=g.u(AC, lo=0.5, hi=1.5), sh=g.n(AC, scale=0.3)),
                   lambda b, st: chk(L.rdm_padavgpool2_fwd(P(b["x"]), ALD, P(b["sc"]), P(b["sh"]), P(b["p"]), AB, AH, AW, AC, st)), outs=("p",),
                   scratch=dict(p=g.e(AB, 8, 10, AC)))


def row_padavgpool2_bwd(dev):
    g = Gen("padavg_bwd", dev)
    L = _l().lib()
    x = g.u(AB, AH, AW, ALD, lo=-2, hi=2)
    mean, rstd = _bn_moments(x.reshape(-1, ALD)[:, :AC])
    gamma, beta = g.u(AC, lo=0.5, hi=1.5), g.n(AC, scale=0.3)
    sc = (gamma.double() * rstd).float()
    sh = (beta.double() - mean * gamma.double() * rstd).float()
    wsb = int(L.rdm_padavgpool2_bwd_workspace_bytes(AC))
    ins = dict(dp=g.n(AB, 8, 10, AC), x=x, sc=sc, sh=sh, gamma=gamma, mean=mean.float(), rstd=rstd.float())
    return sp.Case(ins, lambda b, st: chk(L.rdm_padavgpool2_bwd(P(b["dp"]), P(b["x"]), ALD, P(b["sc"]), P(b["sh"]), P(b["gamma"]), P(b["mean"]), P(b["rstd"]), P(b["dx"]), AC,
                                                                 P(b["dg"]), P(b["db"]), AB, AH, AW, AC, 1, P(b["ws"]), wsb, st)),
                   outs=("dx", "dg", "db"), scratch=dict(dx=g.e(AB, AH, AW, AC), dg=g.e(AC), db=g.e(AC), ws=g.e(wsb, dtype=torch.uint8)),
                   tol=dict(dx=TOL_BN, dg=TOL_BN, db=TOL_BN))   # tests/test_gpu_bnpool.py (TOL): the reductions in the workspace are summed with f64 atomics


def row_layout_nchw_to_nhwc_f32(dev):
    g = Gen("to_nhwc", dev)
    L = _l().lib()
    B, Cc, HW, ld = 2, 20, 63, 24
    return sp.Case(dict(x=g.n(B, Cc, HW)), lambda b, st: chk(L.rdm_layout_nchw_to_nhwc_f32(P(b["x"]), P(b["y"]), ld, B, Cc, HW, st)), outs=("y",),
                   scratch=dict(y=g.e(B, HW, ld)))


def row_layout_nhwc_to_nchw_f32(dev):
    g = Gen("to_nchw", dev)
    L = _l().lib()
    B, Cc, HW, ld = 2, 20, 63, 24
    return sp.Case(dict(x=g.n(B, HW, ld)), lambda b, st: chk(L.rdm_layout_nhwc_to_nchw_f32(P(b["x"]), ld, P(b["y"]), B, Cc, HW, st)), outs=("y",),
                   scratch=dict(y=g.e(B, Cc, HW)))


# ---- loss head (through the product's wrappers where one call maps to one entry point) ---------------------------------------------------------
def row_dorn_fwd(dev):
    from md_rdm_amd.network import computations as cp
    g = Gen("dorn", dev)

    def call(b, st):
        dec, lab = cp.dorn_ordinal_regression(b["x"])
        return dict(decode=dec, ord=lab)
    return sp.Case(dict(x=g.u(2, 180, 8, 10, lo=-2, hi=3)), call)


def row_dorn_bwd(dev):
    g = Gen("dorn_bwd", dev)
    L = _l().lib()
    return sp.Case(dict(x=g.u(2, 180, 8, 10, lo=-2, hi=3), dord=g.n(2, 90, 8, 10, dtype=f64)),
                   lambda b, st: chk(L.rdm_dorn_bwd(P(b["x"]), P(b["dord"]), P(b["dx"]), 2, 90, 80, st)), outs=("dx",), scratch=dict(dx=g.e(2, 180, 8, 10)))


def _loss_inputs(g):
    return g.u(2, 90, 8, 8, lo=0.01, hi=0.99, dtype=f64), torch.floor(g.u(2, 1, 8, 8, lo=0, hi=95)).to(torch.int32)


def row_ordinal_loss_fwd(dev):
    g = Gen("loss", dev)
    L = _l().lib()
    Pm, T = _loss_inputs(g)
    return sp.Case(dict(P=Pm, T=T), lambda b, st: chk(L.rdm_ordinal_loss_fwd(P(b["P"]), P(b["T"]), P(b["loss"]), 2, 90, 64, st)), outs=("loss",),
                   scratch=dict(loss=g.e(1)), tol=dict(loss=TOL_LOSS))                 # the entry point zeroes `loss` itself (poisoned on S just before the call)


def row_ordinal_loss_bwd(dev):
    g = Gen("loss_bwd", dev)
    L = _l().lib()
    Pm, T = _loss_inputs(g)
    return sp.Case(dict(P=Pm, T=T, dl=torch.full((1,), 0.75, device=dev)), lambda b, st: chk(L.rdm_ordinal_loss_bwd(P(b["P"]), P(b["T"]), P(b["dl"]), P(b["dP"]), 2, 90, 64, st)),
                   outs=("dP",), scratch=dict(dP=g.e(2, 90, 8, 8, dtype=f64)))


def row_depth2label_sid(dev):
    g = Gen("sid", dev)
    L = _l().lib()
    n = 2 * 64 * 64
    return sp.Case(dict(d=g.u(n, lo=0.01, hi=12.0, dtype=f64)), lambda b, st: chk(L.rdm_depth2label_sid(P(b["d"]), P(b["lab"]), n, st)), outs=("lab",),
                   scratch=dict(lab=g.e(n, dtype=torch.int32)))


def row_depth2label_sid_ex(dev):
    from md_rdm_amd import utils
    g = Gen("sid_ex", dev)
    return sp.Case(dict(d=g.u(2, 1, 64, 64, lo=0.01, hi=12.0, dtype=f64)), lambda b, st: dict(lab=utils.depth2label_sid(b["d"], cuda=True)))


# ---- post-processing -------------------------------------------------------------------------------------------------------------------
def row_resize_bicubic_f64(dev):
    from md_rdm_amd.network import computations as cp
    g = Gen("resize", dev)
    return sp.Case(dict(x=g.u(2, 1, 23, 31, lo=0.5, hi=9.5, dtype=f64)), lambda b, st: dict(y=cp.resize(b["x"], (13, 17))))


def row_gm_normalize_f64(dev):
    g = Gen("gm", dev)
    L = _l().lib()
    B, n = 3, 64 * 64
    return sp.Case(dict(x=g.u(B, n, lo=0.5, hi=9.0, dtype=f64)), lambda b, st: chk(L.rdm_gm_normalize_f64(P(b["x"]), P(b["y"]), P(b["gm"]), B, n, 1.0 / n, st)),
                   outs=("y", "gm"), scratch=dict(y=g.e(B, n, dtype=f64), gm=g.e(B, dtype=f64)))


def _levels(g, B, n_levels):
    return g.u(B, ((1 << (2 * n_levels)) - 1) // 3, lo=0.5, hi=2.0, dtype=f64)


def row_decompose_f64(dev):
    g = Gen("decompose", dev)
    L = _l().lib()
    B, n = 3, 5
    return sp.Case(dict(dn=g.u(B, 32, 32, lo=0.5, hi=2.0, dtype=f64)), lambda b, st: chk(L.rdm_decompose_f64(P(b["dn"]), P(b["lv"]), B, n, st)), outs=("lv",),
                   scratch=dict(lv=g.e(B, ((1 << (2 * (n + 1))) - 1) // 3, dtype=f64)))


def row_fine_detail_pred_f32(dev):
    g = Gen("fdp", dev)
    L = _l().lib()
    B, nl = 3, 6
    lv = _levels(g, B, nl)
    return sp.Case(dict(lv=lv, w=g.u(nl, lo=0.5, hi=1.5)), lambda b, st: chk(L.rdm_fine_detail_pred_f32(P(b["lv"]), P(b["w"]), P(b["yh"]), B, nl, st)), outs=("yh",),
                   scratch=dict(yh=g.e(B, lv.shape[1])))


def row_fine_detail_pred_bwd(dev):
    g = Gen("fdp_bwd", dev)
    L = _l().lib()
    B, nl = 3, 6
    lv = _levels(g, B, nl)
    return sp.Case(dict(lv=lv, dy=g.n(B, lv.shape[1])), lambda b, st: chk(L.rdm_fine_detail_pred_bwd(P(b["lv"]), P(b["dy"]), P(b["dw"]), B, nl, st)), outs=("dw",),
                   scratch=dict(dw=g.e(nl)))


def row_candidates_matvec_f32(dev):
    g = Gen("matvec", dev)
    L = _l().lib()
    B, K, M = 2, 3, 1024
    return sp.Case(dict(a=g.n(B, K, M, dtype=f64), w=g.u(K, lo=0.2, hi=0.8)), lambda b, st: chk(L.rdm_candidates_matvec_f32(P(b["a"]), P(b["w"]), P(b["o"]), B, K, M, st)),
                   outs=("o",), scratch=dict(o=g.e(B, M)))


def row_candidates_matvec_bwd(dev):
    g = Gen("matvec_bwd", dev)
    L = _l().lib()
    B, K, M = 2, 3, 1024
    return sp.Case(dict(a=g.n(B, K, M, dtype=f64), do=g.n(B, M)), lambda b, st: chk(L.rdm_candidates_matvec_bwd(P(b["a"]), P(b["do"]), P(b["dw"]), B, K, M, st)),
                   outs=("dw",), scratch=dict(dw=g.e(K)))


def row_recombine_f64(dev):
    g = Gen("recombine", dev)
    L = _l().lib()
    B, nl = 3, 4
    return sp.Case(dict(yh=g.n(B, 85)), lambda b, st: chk(L.rdm_recombine_f64(P(b["yh"]), P(b["o"]), B, nl, 7, 0, st)), outs=("o",), scratch=dict(o=g.e(B, 1, 128, 128, dtype=f64)))


def row_recombine_bwd(dev):
    g = Gen("recombine_bwd", dev)
    L = _l().lib()
    B, nl = 3, 4
    return sp.Case(dict(do=g.n(B, 1, 128, 128, dtype=f64)), lambda b, st: chk(L.rdm_recombine_bwd(P(b["do"]), P(b["dy"]), B, nl, 7, 0, st)), outs=("dy",),
                   scratch=dict(dy=g.e(B, 85)))


# ---- relative path -----------------------------------------------------------------------------------------------------------------------
def _tables(tid, dev):
    from md_rdm_amd.network import RDM_Net
    q, inv = RDM_Net.Quantization().device_tables(tid, dev)
    return dict(q=q, inv=inv)


def row_ratio_grid_lloyd_dense(dev):
    from md_rdm_amd.network import computations as cp
    g = Gen("lloyd_dense", dev)
    return sp.Case(dict(d=g.u(2, 1, 8, 8, lo=0.5, hi=2.0)), lambda b, st: dict(R=cp.ratio_grid_lloyd_dense(b["d"], b["q"], b["inv"])), const=_tables(3, dev))


def row_ratio_grid_lloyd_paged(dev):
    from md_rdm_amd.network import computations as cp
    g = Gen("lloyd_paged", dev)
    return sp.Case(dict(dn=g.u(2, 1, 32, 32, lo=0.5, hi=2.0), dn1=g.u(2, 1, 16, 16, lo=0.5, hi=2.0, dtype=f64)),
                   lambda b, st: dict(R=cp.ratio_grid_lloyd_paged(b["dn"], b["dn1"], b["q"], b["inv"])), const=_tables(5, dev))


def row_als_rank1(dev):
    g = Gen("als", dev)
    L = _l().lib()
    G, B, lim = 4, 2, 30                                                              # four pages x two samples
    nb = int(L.rdm_als_workspace_bytes(G, B, 256, 64, lim))
    return sp.Case(dict(R=g.u(G, B, 256, 64, lo=0.5, hi=2.0)), lambda b, st: chk(L.rdm_als_rank1(P(b["R"]), 0, P(b["p"]), G, B, 256, 64, lim, P(b["ws"]), nb, st)),
                   outs=("p",), scratch=dict(p=g.e(G, B, 256), ws=g.e(nb, dtype=torch.uint8)))


def row_als_rank1_paged(dev):
    g = Gen("als_paged", dev)
    L = _l().lib()
    B, S, lim = 2, 32, 30
    nb = int(L.rdm_als_workspace_bytes((S // 16) ** 2, B, 256, 64, lim))
    return sp.Case(dict(dn=g.u(B, 1, S, S, lo=0.5, hi=2.0), dn1=g.u(B, 1, S // 2, S // 2, lo=0.5, hi=2.0, dtype=f64)),
                   lambda b, st: chk(L.rdm_als_rank1_paged(P(b["dn"]), P(b["dn1"]), P(b["p"]), B, S, P(b["q"]), P(b["inv"]), lim, P(b["ws"]), nb, st)),
                   outs=("p",), scratch=dict(p=g.e((S // 16) ** 2, B, 256), ws=g.e(nb, dtype=torch.uint8)), const=_tables(5, dev))


def row_page_split_f32(dev):
    g = Gen("page_split", dev)
    L = _l().lib()
    return sp.Case(dict(x=g.n(2, 32, 32)), lambda b, st: chk(L.rdm_page_split_f32(P(b["x"]), P(b["pg"]), 2, 32, 16, st)), outs=("pg",), scratch=dict(pg=g.e(4, 2, 16, 16)))


def row_page_reconstruct_f32(dev):
    g = Gen("page_rec", dev)
    L = _l().lib()
    return sp.Case(dict(pg=g.n(4, 2, 16, 16)), lambda b, st: chk(L.rdm_page_reconstruct_f32(P(b["pg"]), P(b["o"]), 2, 32, 16, st)), outs=("o",), scratch=dict(o=g.e(2, 32, 32)))


# ---- tails and data ----------------------------------------------------------------------------------------------------------------------
def row_predict_tail_f32(dev):
    g = Gen("tail", dev)
    L = _l().lib()
    B, K, s = 2, 90, 8
    return sp.Case(dict(x=g.u(B, 2 * K, s, s, lo=0.01, hi=6.0), w=g.u(4, lo=0.5, hi=1.5)),
                   lambda b, st: chk(L.rdm_predict_tail_f32(P(b["x"]), P(b["w"]), P(b["o"]), P(b["dec"]), P(b["lin"]), B, K, s, s, 7, 0, st)), outs=("o", "dec", "lin"),
                   scratch=dict(o=g.e(B, 1, 128, 128, dtype=f64), dec=g.e(B, 1, s, s, dtype=torch.int64), lin=g.e(B, 1, 128, 128)))


def _depth(g, *shape):
    d = g.u(*shape, lo=0.5, hi=9.5)
    d[..., 3:9, 4:11] = 0.0
    return d


def row_eval_target_metrics_f64(dev):
    from md_rdm_amd.metrics import MetricComputation
    g = Gen("evalmetrics", dev)
    mc = MetricComputation(["delta1"])

    def call(b, st):
        return dict(rows=mc.compute_rows(b["pred"], b["depth"], target_out=b["tgt"], gm_out=b["gm"]))
    return sp.Case(dict(pred=g.u(2, 1, 128, 128, lo=-1, hi=2, dtype=f64), depth=_depth(g, 2, 1, 57, 76)), call, outs=("tgt", "gm"),
                   scratch=dict(tgt=g.e(2, 1, 128, 128, dtype=f64), gm=g.e(2, dtype=f64)))


def row_depth_metrics_f64(dev):
    g = Gen("metrics", dev)
    L = _l().lib()
    n = 2 * 64 * 64
    t = g.u(n, lo=0.2, hi=4.0, dtype=f64)
    t[::7] = 0.0
    return sp.Case(dict(p=g.u(n, lo=-0.5, hi=3.0, dtype=f64), t=t), lambda b, st: chk(L.rdm_depth_metrics_f64(P(b["p"]), P(b["t"]), n, P(b["o"]), st)), outs=("o",),
                   scratch=dict(o=g.e(10, dtype=f64)), tol=dict(o=("each", TOL_METRICS)))       # the entry point zeroes out10 itself


def row_nyu_preprocess(dev):
    """through the C ABI (the product wrapper stages the augmentation table with a pageable host-to-device copy, which would make the host wait
    for the late producer): the table is pre-staged, the workspace poisoned on S just before the call (the entry point zeroes its luma sums itself)"""
    from md_rdm_amd.dataloaders import nyu
    g = Gen("nyu", dev)
    L = _l().lib()
    B, H, W, resize, (oh, ow) = 2, 120, 160, 64, (57, 76)                             # a quarter of the NYU geometry (480 x 640, Resize(250), 228 x 304)
    h1, w1 = nyu.resized_hw(H, W, resize)
    params = [nyu.make_params(1.2, 3.0, True, [("contrast", 1.3), ("saturation", 0.7)], (H, W), resize, (oh, ow)),
              nyu.make_params(1.0, -4.0, False, [("brightness", 0.8)], (H, W), resize, (oh, ow))]
    aug = torch.frombuffer(bytearray(bytes((nyu.NyuAug * B)(*params))), dtype=torch.uint8).to(dev)
    nb = int(L.rdm_nyu_preprocess_workspace_bytes(B, H, W, h1, w1, ow))
    rgb = (g.u(B, H, W, 3, lo=0, hi=255.99)).to(torch.uint8)
    return sp.Case(dict(rgb=rgb, depth=_depth(g, B, H, W)),
                   lambda b, st: chk(L.rdm_nyu_preprocess(P(b["rgb"]), P(b["depth"]), P(b["aug"]), B, H, W, h1, w1, oh, ow, P(b["x"]), P(b["y"]), P(b["ws"]), nb, st)),
                   outs=("x", "y"), scratch=dict(x=g.e(B, 3, oh, ow), y=g.e(B, 1, oh, ow), ws=g.e(nb, dtype=torch.uint8)), const=dict(aug=aug))


def row_adamw_fused(dev):
    g = Gen("adamw", dev)
    L = _l().lib()
    n = 100_003
    return sp.Case(dict(p=g.n(n), gr=g.n(n), m=g.n(n, scale=0.1), v=g.u(n, lo=0.0, hi=0.1)),
                   lambda b, st: chk(L.rdm_adamw_fused(P(b["p"]), P(b["gr"]), P(b["m"]), P(b["v"]), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, st)), outs=("p", "m", "v"))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
# name -> (family, builder of the operator case | name of the whole-plan test in this module that drives the entry point)
ROWS = {
    "rdm_conv2d_fwd": ("conv", row_conv2d_fwd),
    "rdm_conv2d_dgrad": ("conv", row_conv2d_dgrad),
    "rdm_conv2d_wgrad": ("conv", row_conv2d_wgrad),
    "rdm_conv2d_fwd_ex": ("conv", row_conv2d_fwd_ex),
    "rdm_conv2d_dgrad_ex": ("conv", row_conv2d_dgrad_ex),
    "rdm_conv2d_wgrad_ex": ("conv", row_conv2d_wgrad_ex),
    "rdm_conv2d_fwd_bnsums": ("conv", row_conv2d_fwd_bnsums),
    "rdm_conv3x3_fwd_bnsums_acc": ("conv", row_conv3x3_fwd_bnsums_acc),
    "rdm_conv2d_wgrad_x3": ("conv", row_conv2d_wgrad_x3),
    "rdm_conv1x1_fwd_x6": ("conv", row_conv1x1_fwd_x6),
    "rdm_conv1x1_dgrad_x3": ("conv", row_conv1x1_dgrad_x3),
    "rdm_conv3x3_dgrad_x3": ("conv", row_conv3x3_dgrad_x3),
    "rdm_conv3x3_wino_fwd": ("conv", row_conv3x3_wino_fwd),
    "rdm_conv3x3_wino_fwd_x6": ("conv", row_conv3x3_wino_fwd_x6),
    "rdm_conv3x3_wino_wgrad": ("conv", row_conv3x3_wino_wgrad),
    "rdm_frame_split_rows_f32": ("split_rows", row_frame_split_rows_f32),
    "rdm_split_rows_f32": ("split_rows", row_split_rows_f32),
    "rdm_pack_conv_weight": ("pack", row_pack_conv_weight),
    "rdm_unpack_conv_weight": ("pack", row_unpack_conv_weight),
    "rdm_gemm_bf16": ("bf16", row_gemm_bf16),
    "rdm_gemm_bf16_act": ("bf16", row_gemm_bf16_act),
    "rdm_conv3x3_bf16": ("bf16", row_conv3x3_bf16),
    "rdm_gemm_bf16_stats": ("bf16", row_gemm_bf16_stats),
    "rdm_conv3x3_bf16_stats": ("bf16", row_conv3x3_bf16_stats),
    "rdm_conv3x3_act_bf16_pack": ("bf16", row_conv3x3_act_bf16_pack),
    "rdm_conv3x3_act_bf16": ("bf16", row_conv3x3_act_bf16),
    "rdm_colstats_bf16": ("bf16", row_colstats_bf16),
    "rdm_stem_patches_bf16": ("bf16", row_stem_patches_bf16),
    "rdm_maxpool3s2_bf16": ("bf16", row_maxpool3s2_bf16),
    "rdm_padavgpool2_bf16": ("bf16", row_padavgpool2_bf16),
    "rdm_f32_to_bf16_rows": ("bf16", row_f32_to_bf16_rows),
    "rdm_pack_conv_weight_bf16": ("bf16", row_pack_conv_weight_bf16),
    "rdm_wsm_conv_bf16": ("bf16", row_wsm_conv_bf16),
    "rdm_wsm_deconv_bf16": ("bf16", row_wsm_deconv_bf16),
    "rdm_wsm_strip_bf16": ("bf16", row_wsm_strip_bf16),
    "rdm_wsm_conv1x1_f32": ("bf16", row_wsm_conv1x1_f32),
    "rdm_bn_stats": ("bn", row_bn_stats),
    "rdm_bn_finalize": ("bn", row_bn_finalize),
    "rdm_bn_bwd_reduce": ("bn", row_bn_bwd_reduce),
    "rdm_bn_bwd": ("bn", row_bn_bwd),
    "rdm_bn_bwd_defer": ("bn", row_bn_bwd_defer),
    "rdm_maxpool3s2_fwd": ("pool", row_maxpool3s2_fwd),
    "rdm_maxpool3s2_bwd": ("pool", row_maxpool3s2_bwd),
    "rdm_padavgpool2_fwd": ("pool", row_padavgpool2_fwd),
    "rdm_padavgpool2_bwd": ("pool", row_padavgpool2_bwd),
    "rdm_layout_nchw_to_nhwc_f32": ("layout", row_layout_nchw_to_nhwc_f32),
    "rdm_layout_nhwc_to_nchw_f32": ("layout", row_layout_nhwc_to_nchw_f32),
    "rdm_dorn_fwd": ("loss", row_dorn_fwd),
    "rdm_dorn_bwd": ("loss", row_dorn_bwd),
    "rdm_ordinal_loss_fwd": ("loss", row_ordinal_loss_fwd),
    "rdm_ordinal_loss_bwd": ("loss", row_ordinal_loss_bwd),
    "rdm_depth2label_sid": ("loss", row_depth2label_sid),
    "rdm_depth2label_sid_ex": ("loss", row_depth2label_sid_ex),
    "rdm_resize_bicubic_f64": ("postproc", row_resize_bicubic_f64),
    "rdm_gm_normalize_f64": ("postproc", row_gm_normalize_f64),
    "rdm_decompose_f64": ("postproc", row_decompose_f64),
    "rdm_fine_detail_pred_f32": ("postproc", row_fine_detail_pred_f32),
    "rdm_fine_detail_pred_bwd": ("postproc", row_fine_detail_pred_bwd),
    "rdm_candidates_matvec_f32": ("postproc", row_candidates_matvec_f32),
    "rdm_candidates_matvec_bwd": ("postproc", row_candidates_matvec_bwd),
    "rdm_recombine_f64": ("postproc", row_recombine_f64),
    "rdm_recombine_bwd": ("postproc", row_recombine_bwd),
    "rdm_ratio_grid_lloyd_dense": ("relative", row_ratio_grid_lloyd_dense),
    "rdm_ratio_grid_lloyd_paged": ("relative", row_ratio_grid_lloyd_paged),
    "rdm_als_rank1": ("relative", row_als_rank1),
    "rdm_als_rank1_paged": ("relative", row_als_rank1_paged),
    "rdm_page_split_f32": ("relative", row_page_split_f32),
    "rdm_page_reconstruct_f32": ("relative", row_page_reconstruct_f32),
    "rdm_predict_tail_f32": ("tails", row_predict_tail_f32),
    "rdm_eval_target_metrics_f64": ("tails", row_eval_target_metrics_f64),
    "rdm_depth_metrics_f64": ("tails", row_depth_metrics_f64),
    "rdm_nyu_preprocess": ("tails", row_nyu_preprocess),
    "rdm_adamw_fused": ("tails", row_adamw_fused),
    "rdm_net_forward": ("plan", "test_plan_training_steps_back_to_back"),
    "rdm_net_backward_stage": ("plan", "test_plan_staged_backward_gradients_are_final_per_stage"),
    "rdm_net_backward": ("plan", "test_plan_segment_backward"),
    "rdm_net_encoder_output": ("plan", "test_plan_inference_paths"),
    "rdm_net_bf16_prepare": ("plan", "test_plan_inference_paths"),
    "rdm_net_forward_bf16": ("plan", "test_plan_inference_paths"),
    "rdm_net_encoder_output_bf16": ("plan", "test_plan_inference_paths"),
    "rdm_rel_bf16_prepare": ("plan", "test_plan_inference_paths"),
    "rdm_rel_forward_bf16": ("plan", "test_plan_inference_paths"),
    "rdm_rel_bf16_input_nchw": ("plan", "test_plan_relative_training_forward_bf16"),
    "rdm_rel_forward_bf16_train": ("plan", "test_plan_relative_training_forward_bf16"),
}

# rows that reach their entry point through a product wrapper: "module:attribute path" of the wrapper whose source makes the call
# (tests/test_streams_table_cpu.py checks that it does, and that every other row's builder names its entry point itself)
VIA = {
    "rdm_dorn_fwd": "md_rdm_amd.network.computations:_Dorn.forward",
    "rdm_depth2label_sid_ex": "md_rdm_amd.utils:depth2label_sid",
    "rdm_resize_bicubic_f64": "md_rdm_amd.network.computations:resize",
    "rdm_ratio_grid_lloyd_dense": "md_rdm_amd.network.computations:ratio_grid_lloyd_dense",
    "rdm_ratio_grid_lloyd_paged": "md_rdm_amd.network.computations:ratio_grid_lloyd_paged",
    "rdm_eval_target_metrics_f64": "md_rdm_amd.metrics:MetricComputation.compute_rows",
    "rdm_net_forward": "md_rdm_amd.network.RDM_Net:DepthEstimationNet._native_forward",
    "rdm_net_backward_stage": "md_rdm_amd.network.RDM_Net:DepthEstimationNet._native_backward",
    "rdm_net_encoder_output": "md_rdm_amd.network.RDM_Net:DepthEstimationNet.encoder_output",
    "rdm_net_bf16_prepare": "md_rdm_amd.network.RDM_Net:DepthEstimationNet.prepare_bf16",
    "rdm_net_forward_bf16": "md_rdm_amd.network.RDM_Net:DepthEstimationNet._native_forward_bf16",
    "rdm_net_encoder_output_bf16": "md_rdm_amd.network.RDM_Net:DepthEstimationNet.encoder_output_bf16",
    "rdm_rel_bf16_prepare": "md_rdm_amd.network.RDM_Net:Decoder._prepare_bf16",
    "rdm_rel_forward_bf16": "md_rdm_amd.network.RDM_Net:Decoder.features_bf16",
    "rdm_rel_bf16_input_nchw": "md_rdm_amd.network.RDM_Net:DepthEstimationNet.forward",
    "rdm_rel_forward_bf16_train": "md_rdm_amd.network.RDM_Net:Decoder.features_bf16_train",
}

# stream-taking declarations that enqueue no device work (none today: every rdm_stream_t function launches or copies)
EXEMPT = {}

# one control per family: a row whose inputs are all floating point (poison read on the wrong stream cannot become an address) and whose outputs
# are written in full (no poisoned padding survives in the reference)
CONTROLS = {"conv": "rdm_conv2d_fwd_ex", "split_rows": "rdm_frame_split_rows_f32", "pack": "rdm_unpack_conv_weight", "bf16": "rdm_colstats_bf16", "bn": "rdm_bn_bwd",
            "pool": "rdm_padavgpool2_fwd", "layout": "rdm_layout_nhwc_to_nchw_f32", "loss": "rdm_dorn_bwd", "postproc": "rdm_recombine_f64",
            "relative": "rdm_page_split_f32", "tails": "rdm_predict_tail_f32"}

OPERATOR_ROWS = sorted(k for k, v in ROWS.items() if callable(v[1]))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    _l().lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def delay(dev):
    d = sp.Delay(dev)
    print("delay calibration: %.3e units per ms (%s)" % (d.units_per_ms, "torch.cuda._sleep" if d.sleep is not None else "matmul chain"))
    return d


@pytest.mark.parametrize("name", OPERATOR_ROWS)
def test_operator_on_a_late_non_default_stream(dev, delay, name):
    case = ROWS[name][1](dev)
    torch.cuda.synchronize()
    sp.check(case, delay)


@pytest.mark.parametrize("family", sorted(CONTROLS))
def test_control_a_call_on_the_null_stream_is_detected(dev, delay, family):
    name = CONTROLS[family]
    assert ROWS[name][0] == family
    case = ROWS[name][1](dev)
    torch.cuda.synchronize()
    ms = sp.control(case, delay)
    print("control %s (%s): detected with a delay of %.1f ms" % (family, name, ms))


# ---- two streams at once: caller-supplied workspaces only, no hidden device-side state shared between calls ----------------------------------------
@pytest.mark.parametrize("name", ["rdm_conv3x3_wino_fwd", "rdm_gemm_bf16", "rdm_als_rank1_paged"])
def test_two_streams_at_once_equal_the_solo_results(dev, delay, name):
    a, b = ROWS[name][1](dev), ROWS[name][1](dev)
    for k in b.staged:                                       # an independent second case: other values in the same shapes
        if b.staged[k].dtype.is_floating_point:
            b.staged[k] = (b.staged[k].double() * 0.75).to(b.staged[k].dtype)
    torch.cuda.synchronize()
    ra, rb = sp.reference_run(a), sp.reference_run(b)
    assert not all(sp.same_bits(ra[k], rb[k]) for k in ra)
    for c in (a, b):
        for t in c.bufs.values():
            sp.poison_(t)
    torch.cuda.synchronize()
    S1, S2 = delay.S, delay.second_stream()                 # S2 proven to run beside S1 and beside the null stream
    snaps = []
    for _ in range(3):                                       # several calls in flight on each stream, interleaved from the host
        for c, S in ((a, S1), (b, S2)):
            snaps.append((c, _enqueue(c, S, delay)))
    S1.synchronize()
    S2.synchronize()
    for c, snap in snaps:
        ref = ra if c is a else rb
        assert not sp.mismatches(c, snap, ref)


def _enqueue(case, S, delay):
    """late_run without the up-front poison + synchronise: the case's buffers are reused by the next call on the same stream, in stream order"""
    with torch.cuda.stream(S):
        delay.enqueue(1.0)
        for k, v in case.staged.items():
            case.bufs[k].copy_(v, non_blocking=True)
        for t in case.scratch.values():
            sp.poison_(t)
        extra = case.call(case.all_bufs(), _l().stream()) or {}
        snap = {k: case.bufs[k].clone() for k in case.outs}
        snap.update({k: v.detach().clone() for k, v in extra.items()})
    return snap


# ---- whole-plan coverage: B = 2, 228 x 228, deterministic mode, bit for bit against the null-stream run ------------------------------------------
# Two identical models (hash-filled, RDM_NET_OPT_DETERMINISTIC: tests/test_gpu_net.py shows two instances agree bit for bit): one runs on the null
# stream, the other behind the late producer on the module's non-default stream.  Allocated on the null stream and poisoned beforehand: the input
# buffers, the flat gradient buffer and the plan's WORKSPACE (bytes of 0xFF: NaN as f32, f64 and bf16) - all activations, dZ buffers and packed
# weight images live there, and they are what the side-stream forks read and the plan's event joins protect - and, for the bf16 paths, the
# prepared-weight buffer and the bf16 workspace.  Weights, running statistics and optimiser moments are state a step reads AND writes: they keep
# their values.  (The relative decoders allocate their own prepared weights / workspace inside the stream context on first use.)
PLAN_B, PLAN_HW = 2, 228


def make_model(dev, relative_decoders=(), train=True):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet(relative_decoders=relative_decoders)
    m.deterministic = True
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev)
    return m.train() if train else m.eval()


@pytest.fixture(scope="module")
def batch(dev):
    x, y = filler.synthetic_batch(PLAN_B, PLAN_HW, PLAN_HW, seed=9)
    return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


def prealloc_poisoned(m, x, bf16_too=False):
    """the model's plan workspace(s) for this input geometry, allocated here (null stream) and filled with 0xFF; the model then uses them as they are"""
    L = _l().lib()
    B, _, H, W = x.shape
    m._ensure_flat(x.device)
    h, ws_bytes, _, _ = m._plan(B, H, W)
    m._ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=x.device)
    if bf16_too:
        m._bf16_w = torch.full((int(L.rdm_net_bf16_weight_bytes(h)),), 0xFF, dtype=torch.uint8, device=x.device)
        m._bf16_ws = torch.full((int(L.rdm_net_bf16_workspace_bytes(h)),), 0xFF, dtype=torch.uint8, device=x.device)
        m._bf16_stale = True


def _time_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class Trainer:
    def __init__(self, dev, batch, hook=None):
        from md_rdm_amd import harness
        self.h = harness
        self.m = make_model(dev)
        self.m.flatten_parameters()
        self.m.direct_grads = True
        self.m.grad_ready_hook = hook
        self.opt = harness.FusedAdamW(self.m, lr=1e-4)
        self.x_real, self.y_real = batch
        self.x, self.y = torch.empty_like(self.x_real), torch.empty_like(self.y_real)

    def load_inputs(self):
        self.x.copy_(self.x_real, non_blocking=True)
        self.y.copy_(self.y_real, non_blocking=True)

    def poison(self):
        for t in (self.x, self.y, self.m._flat[1]):
            sp.poison_(t)
        prealloc_poisoned(self.m, self.x_real)

    def step(self, snaps, update=True):
        """one training step on the current stream; its results are cloned in stream order"""
        self.opt.zero_grad()
        loss, parts = self.h.training_step(self.m, self.x, self.y)
        loss.backward()
        snap = dict(logits=parts["ord_label_pred"].detach().clone(), loss=loss.detach().clone(), grads=self.m._flat[1].clone())
        if update:
            self.opt.step()
            snap["weights"] = self.m._flat[0].clone()
        snaps.append(snap)


def _assert_steps_equal(got, ref):
    assert len(got) == len(ref)
    for i, (a, b) in enumerate(zip(got, ref)):
        for k in b:
            if k == "loss":         # its ordinal term is summed with f32 atomics (rdm_ordinal_loss_fwd): tests/test_gpu_ops.py::test_ordinal_loss, 2e-6
                assert bool(torch.isfinite(a[k])) and abs(float(a[k]) - float(b[k])) <= TOL_LOSS * abs(float(b[k])), "step %d: loss" % i
                continue
            assert sp.same_bits(a[k], b[k]), "step %d: %s differs from the null-stream run" % (i, k)
        assert bool(torch.isfinite(a["grads"]).all()) and float(a["grads"].abs().max()) > 0


def test_plan_training_steps_back_to_back(dev, delay, batch):
    """Forward, backward and FusedAdamW.step on S behind the late producer, a second step on S with no synchronisation in between (reuse of the plan's
    events - ev_dz / dz_busy, ev_pkf, ev_pkb - across calls), then a third on the null stream (reuse across streams).  Logits, loss, all gradients and
    the post-step weights of the three steps equal those of three null-stream steps of an identical model, bit for bit."""
    r = Trainer(dev, batch)
    r.load_inputs()
    ref = []
    r.step(ref)
    r.step(ref)
    torch.cuda.synchronize()
    null_ms = _time_ms(lambda: r.step(ref))
    t = Trainer(dev, batch)
    t.poison()
    torch.cuda.synchronize()
    got = []
    S = delay.S
    with torch.cuda.stream(S):
        delay.enqueue(delay.ms_for(null_ms))
        t.load_inputs()
        t.step(got)
        t.step(got)
    torch.cuda.current_stream().wait_stream(S)              # the caller's own ordering between its two streams
    t.step(got)
    S.synchronize()
    torch.cuda.synchronize()
    print("training step: null-stream time %.1f ms, delay %.1f ms" % (null_ms, delay.ms_for(null_ms)))
    _assert_steps_equal(got, ref)


def test_control_plan_forward_on_the_null_stream_is_detected(dev, delay, batch):
    """the control of the plan family: the late-producer forward with the caller's stream context left out (rdm_net_forward lands on the null
    stream) reads the poisoned input.  A ReLU network launders NaN (fmaxf(NaN, 0) = 0, and the DORN head clamps), so "contains poison" is shown
    the only way it can be here: the escaped forward's logits equal, bit for bit, the logits an identical model computes from an all-poison input."""
    r = Trainer(dev, batch)
    r.load_inputs()
    with torch.no_grad():
        ref = r.m._native_forward(r.x).clone()
        torch.cuda.synchronize()
        null_ms = _time_ms(lambda: r.m._native_forward(r.x))
        t = Trainer(dev, batch)
        t.poison()
        torch.cuda.synchronize()
        S = delay.S
        with torch.cuda.stream(S):
            delay.enqueue(delay.ms_for(null_ms))
            t.load_inputs()
        wrong = t.m._native_forward(t.x)                        # WRONG: on the null stream, not ordered after the producer on S
        with torch.cuda.stream(S):
            late = wrong.clone()
    S.synchronize()
    torch.cuda.synchronize()
    print("control plan: detected with a delay of %.1f ms (null-stream time of the forward %.1f ms)" % (delay.ms_for(null_ms), null_ms))
    p = Trainer(dev, batch)
    p.poison()
    with torch.no_grad():
        from_poison = p.m._native_forward(p.x).clone()
    torch.cuda.synchronize()
    assert not sp.same_bits(late, ref) and sp.same_bits(late, from_poison)


def test_plan_staged_backward_gradients_are_final_per_stage(dev, delay, batch):
    """rdm_net_backward_stage driven as md_rdm_amd/parallel.py drives it: after each stage an event is recorded on S, a second stream C waits on it and
    copies that stage's gradient range; each snapshot equals the monolithic backward's gradients of the range - once the stage call has returned
    and its event is recorded, the stage's gradients are final with respect to S, the library's weight-gradient side stream included."""
    r = Trainer(dev, batch)
    r.load_inputs()
    ref = []
    r.step(ref, update=False)
    torch.cuda.synchronize()
    null_ms = _time_ms(lambda: r.step([], update=False))
    Cs = torch.cuda.Stream()
    snaps = {}
    t = Trainer(dev, batch)
    slices = t.m.stage_slices()

    def hook(stage):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        Cs.wait_event(ev)
        a, b = slices[stage]
        with torch.cuda.stream(Cs):
            snaps[stage] = t.m._flat[1][a:b].clone()
    t.m.grad_ready_hook = hook
    t.poison()
    torch.cuda.synchronize()
    got = []
    S = delay.S
    with torch.cuda.stream(S):
        delay.enqueue(delay.ms_for(null_ms))
        t.load_inputs()
        t.step(got, update=False)
    S.synchronize()
    Cs.synchronize()
    torch.cuda.synchronize()
    assert sorted(snaps) == list(range(len(slices))) and len(slices) > 4
    for stage, (a, b) in enumerate(slices):
        assert sp.same_bits(snaps[stage], ref[0]["grads"][a:b]), "stage %d: the gradient range was not final when the stage's event fired" % stage
    _assert_steps_equal(got, ref)


def _segment_backward(m, x, dlogits, gbuf):
    """rdm_net_forward through the model, then rdm_net_backward (segments 0..3) through the C ABI into `gbuf`, on the current stream"""
    _lib = _l()
    L = _lib.lib()
    logits = m._native_forward(x)
    h, ws_bytes, table, tensors = m._last
    flat, gflat, entries = m._flat
    goff = {k: o for k, p, o, n, g in entries if p.requires_grad}
    gt = [gbuf.data_ptr() + 4 * goff[k] if (is_p and k in goff) else None for k, is_p in zip(m._names, m._is_param)]
    gtable = (C.c_void_p * len(gt))(*gt)
    gbuf.zero_()                                            # RDM_NET_OPT_GRADS_PREZEROED: the caller's one fill
    chk(L.rdm_net_backward(h, P(dlogits), table, gtable, C.c_void_p(m._ws.data_ptr()), ws_bytes, 0, 3, _lib.stream()))
    return logits.clone(), gbuf.clone()


def test_plan_segment_backward(dev, delay, batch):
    """rdm_net_backward (the four coarse segments in one call; no Python wrapper) after a forward, both on S behind the late producer"""
    g = Gen("dlogits", dev)
    dl = g.n(PLAN_B, 180, 8, 8, scale=1e-3)
    r = Trainer(dev, batch)
    r.load_inputs()
    rl, rg = _segment_backward(r.m, r.x, dl, torch.empty_like(r.m._flat[1]))
    torch.cuda.synchronize()
    r2 = Trainer(dev, batch)
    r2.load_inputs()
    gb = torch.empty_like(r2.m._flat[1])
    null_ms = _time_ms(lambda: _segment_backward(r2.m, r2.x, dl, gb))
    t = Trainer(dev, batch)
    gbuf, dlb = torch.empty_like(t.m._flat[1]), torch.empty_like(dl)
    t.poison()
    sp.poison_(gbuf)
    sp.poison_(dlb)
    torch.cuda.synchronize()
    S = delay.S
    with torch.cuda.stream(S):
        delay.enqueue(delay.ms_for(null_ms))
        t.load_inputs()
        dlb.copy_(dl, non_blocking=True)
        sl, sg = _segment_backward(t.m, t.x, dlb, gbuf)
    S.synchronize()
    torch.cuda.synchronize()
    assert sp.same_bits(sl, rl) and sp.same_bits(sg, rg)
    assert bool(torch.isfinite(sg).all()) and float(sg.abs().max()) > 0


def _late_model_call(dev, delay, batch, build, run, names):
    """`run(model, x)` -> tuple of tensors, on the null stream with one model and behind the late producer with an identical one"""
    xr = batch[0]
    r = build()
    ref = [v.clone() for v in run(r, xr)]
    torch.cuda.synchronize()
    null_ms = _time_ms(lambda: run(r, xr))
    t = build()
    x = torch.empty_like(xr)
    sp.poison_(x)
    prealloc_poisoned(t, xr, bf16_too=True)
    ws_ptrs = (t._ws.data_ptr(), t._bf16_w.data_ptr(), t._bf16_ws.data_ptr())
    torch.cuda.synchronize()
    S = delay.S
    with torch.cuda.stream(S):
        delay.enqueue(delay.ms_for(null_ms))
        x.copy_(xr, non_blocking=True)
        got = [v.clone() for v in run(t, x)]
    assert ws_ptrs == (t._ws.data_ptr(), t._bf16_w.data_ptr(), t._bf16_ws.data_ptr())        # the model ran in the poisoned buffers
    S.synchronize()
    torch.cuda.synchronize()
    for n, a, b in zip(names, got, ref):
        assert sp.same_bits(a, b), "%s differs from the null-stream run" % n
        assert not sp.has_poison(a), n


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("relative", [(), (7,)], ids=["ordinal_only", "with_d7"])
def test_plan_inference_paths(dev, delay, batch, precision, relative):
    """model.eval().predict(x) on S at both precisions.  bf16: rdm_net_bf16_prepare (the weights are stale on the first call, so it runs on S too),
    rdm_net_forward_bf16 and, with a relative decoder, rdm_net_encoder_output_bf16 -> rdm_rel_bf16_prepare -> rdm_rel_forward_bf16; f32 with a
    relative decoder: rdm_net_encoder_output into the f32 decoder path; ordinal-only: the fused rdm_predict_tail_f32 behind either forward."""
    def build():
        return make_model(dev, relative_decoders=relative, train=False).set_precision(precision)

    def run(m, x):
        out, counts = m.predict(x, return_counts=True)
        return out, counts
    _late_model_call(dev, delay, batch, build, run, ("map", "counts"))


def test_plan_relative_training_forward_bf16(dev, delay, batch):
    """the training-mode forward with a relative decoder on the bf16 path on S: rdm_net_forward, rdm_net_encoder_output, rdm_rel_bf16_input_nchw,
    rdm_colstats_bf16, rdm_rel_bf16_prepare (weights only) and rdm_rel_forward_bf16_train, whose running statistics are compared too"""
    def build():
        return make_model(dev, relative_decoders=(7,), train=True).set_relative_train_precision("bf16")

    def run(m, x):
        with torch.no_grad():
            y_hat, x_d1, ord_labels = m(x)
        sd = m.state_dict()
        stats = torch.cat([v.detach().double().reshape(-1) for k, v in sd.items() if k.startswith("d_7.") and ("running_" in k or "num_batches" in k)])
        return tuple(y_hat) + (x_d1, ord_labels, stats)
    xr = batch[0]
    r = build()
    ref = [v.clone() for v in run(r, xr)]
    torch.cuda.synchronize()
    t = build()
    x = torch.empty_like(xr)
    sp.poison_(x)
    prealloc_poisoned(t, xr)
    torch.cuda.synchronize()
    S = delay.S
    with torch.cuda.stream(S):
        delay.enqueue(delay.ms_for(50.0 / sp.MULTIPLE))     # a second forward of `r` would move its running statistics: a fixed 50 ms instead of a measured multiple
        x.copy_(xr, non_blocking=True)
        got = [v.clone() for v in run(t, x)]
    S.synchronize()
    torch.cuda.synchronize()
    assert len(got) == len(ref) >= 4
    names = ["y_hat[%d]" % i for i in range(len(ref) - 3)] + ["x_d1", "ord_labels", "d_7 running statistics"]
    for n, a, b in zip(names, got, ref):
        assert sp.same_bits(a, b), "%s differs from the null-stream run" % n
