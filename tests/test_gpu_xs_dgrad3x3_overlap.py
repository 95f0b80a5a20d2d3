"""-m gpu: xs_dgrad3x3_kernel's chunked epilogue (gate values fetched ahead of their use, the first chunk under the last k-step) through the
C ABI (rdm_conv3x3_dgrad_x3) against a float64 shifted-slice matmul on the CPU.

Gates, both the project's own (tests/test_gpu_xsplit.py): dZ within 2e-5 of the tensor's maximum, the two BatchNorm-backward sums within 2e-5 of
their own maximum.  With products = 1 the operator is DEFINED on operands rounded to bf16, so those cases feed operands that are bf16 values
already and the float64 product of them is the reference, at the same gate.

Shapes: the smallest at which the chunking can go wrong - a pixel count that ends inside the first 96 pixels of a tile, inside a 32-pixel
epilogue chunk of the second tile, at exactly one tile; channel counts with a tail inside the wave's second 16-channel tile, inside a
128-channel column tile, and none; W = 3 and H = 1 (every tap leaves the image somewhere); one shape with more work items than resident
workgroups (834 items for 512 slots)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-5
N = 48

SHAPES = [
    # B, H, W, Cb
    (1, 5, 19, 48),        # 95 pixels: ends inside the first 96 of the tile, inside chunk 2; 48 = 3 tiles: wave 1 has a dead second tile
    (1, 12, 16, 112),      # 192 pixels: exactly one tile; 112 = 7 tiles: wave 3 has a dead second tile
    (1, 7, 29, 128),       # 203 pixels: the second tile ends inside its first chunk; one full column tile
    (2, 11, 3, 176),       # W = 3: every pixel is next to a border; 176 = 128 + 48
    (3, 1, 37, 176),       # H = 1: the taps of rows -1 / +1 never land
    (8, 100, 100, 176),    # 417 pixel tiles x 2 column tiles = 834 items: every persistent workgroup walks more than one
]
IDS = [f"{b}x{h}x{w}_c{c}" for b, h, w, c in SHAPES]


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def _ref3x3_dgrad(gy, w9):
    """gy (B,H,W,N) f64, w9 (9,N,C) f64 -> (B*H*W, C): the definition (shifted-slice matmuls, zero padding 1)"""
    import torch.nn.functional as F
    B, H, W, n = gy.shape
    gp = F.pad(gy, (0, 0, 1, 1, 1, 1))
    dx = torch.zeros(B * H * W, w9.shape[2], dtype=torch.float64)
    for r in range(3):
        for q in range(3):
            dx += gp[:, 2 - r:2 - r + H, 2 - q:2 - q + W, :].reshape(-1, n) @ w9[r * 3 + q]
    return dx


_CACHE = {}


def _problem(shape, products):
    """inputs and the float64 reference, computed once per (shape, products) and never modified"""
    key = (shape, products)
    if key not in _CACHE:
        B, H, W, Cb = shape
        M = B * H * W
        g = torch.Generator().manual_seed(7000 + 13 * Cb + M)
        gy = torch.randn(B, H, W, N, generator=g)
        w9 = torch.randn(9, N, Cb, generator=g) / (9 * N) ** 0.5
        if products == 1:
            gy, w9 = gy.bfloat16().float(), w9.bfloat16().float()
        ldx = Cb + 16                                           # the gate tensor's rows are wider than Cb: NaN behind the channels
        y = torch.randn(M, ldx, generator=g)
        y[:, Cb:] = float("nan")
        sc = torch.rand(Cb, generator=g) + 0.5
        sh = torch.randn(Cb, generator=g) * 0.3
        want = _ref3x3_dgrad(gy.double(), w9.double())
        gate = (y[:, :Cb] * sc + sh) > 0
        wantz = want * gate
        _CACHE[key] = dict(gy=gy, w9=w9, y=y, sc=sc, sh=sh, ldx=ldx, want=want, wantz=wantz,
                           s0=wantz.sum(0), s1=(wantz * y[:, :Cb].double()).sum(0))
    return _CACHE[key]


def _run(shape, products, masked, P, launches=1):
    """-> list of (dz with its 16 guard columns, s0, s1) per launch"""
    from md_rdm_amd import _lib
    from md_rdm_amd._lib import ConvDesc, check, ptr, stream
    L = _lib.lib()
    dev = torch.device("cuda:0")
    B, H, W, Cb = shape
    M, ldc = B * H * W, Cb + 16
    d = ConvDesc(B, H, W, Cb, Cb, N, N, 3, 3, 1, 1, 1, 1)
    gyg, wg, yg, scg, shg = P["gy"].to(dev), P["w9"].to(dev), P["y"].to(dev), P["sc"].to(dev), P["sh"].to(dev)
    wsb = L.rdm_conv3x3_dgrad_x3_workspace_bytes(Cb)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(launches):
        dz = torch.full((M, ldc), -7.0, device=dev)             # the guard columns behind Cb must come back untouched
        s0 = torch.zeros(Cb, dtype=torch.float64, device=dev)
        s1 = torch.zeros_like(s0)
        if masked:
            check(L.rdm_conv3x3_dgrad_x3(C.byref(d), ptr(gyg), ptr(wg), ptr(dz), ldc, ptr(yg), P["ldx"], ptr(scg), ptr(shg), ptr(s0), ptr(s1), ptr(ws), wsb, products, stream()))
        else:
            check(L.rdm_conv3x3_dgrad_x3(C.byref(d), ptr(gyg), ptr(wg), ptr(dz), ldc, None, 0, None, None, None, None, ptr(ws), wsb, products, stream()))
        outs.append((dz, s0, s1))
    torch.cuda.synchronize()
    return outs


def _check(shape, products, masked, out, P):
    Cb = shape[3]
    dz, s0, s1 = out
    dzc = dz.cpu()
    assert torch.all(dzc[:, Cb:] == -7.0), "a store landed behind the Cb channels"
    got = dzc[:, :Cb].double()
    assert torch.isfinite(got).all()
    err = _rel(got, P["wantz"] if masked else P["want"])
    print(f"{shape} products={products} masked={masked}: dZ {err:.2e}", end="")
    assert err < TOL, err
    if masked:
        e0, e1 = _rel(s0.cpu(), P["s0"]), _rel(s1.cpu(), P["s1"])
        print(f" sums {e0:.2e} {e1:.2e}", end="")
        assert torch.isfinite(s0).all() and torch.isfinite(s1).all()
        assert e0 < TOL and e1 < TOL, (e0, e1)
    print()


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gate_and_sums_vs_float64(shape, products):
    """EPI_MASK_STATS: the gated dZ and both sums; NaN behind the gate tensor's Cb columns reaches neither; two launches store the same dZ bit for
    bit (the sums go through atomics and are left out of that comparison)."""
    P = _problem(shape, products)
    a, b = _run(shape, products, True, P, launches=2)
    _check(shape, products, True, a, P)
    assert torch.equal(a[0], b[0])


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plain_store_vs_float64(shape, products):
    """EPI_STORE: no atomics anywhere, so two launches are bit-identical."""
    P = _problem(shape, products)
    a, b = _run(shape, products, False, P, launches=2)
    _check(shape, products, False, a, P)
    assert torch.equal(a[0], b[0])


def test_non_default_stream():
    shape = SHAPES[2]
    P = _problem(shape, 3)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        (out,) = _run(shape, 3, True, P)
    _check(shape, 3, True, out, P)
