"""-m gpu: the persistent walk of conv3x3_wino_fwd_kernel (csrc/wino.hip) at the shapes where a walk can go wrong - through the C ABI entry of
tests/test_gpu_wino.py (rdm_conv3x3_wino_fwd; its split_k argument forces the workgroup count G of the walk), against the same float64 torch-CPU
evaluation and at the same tolerances: 2e-5 of the output's maximum, 1e-5 for the channel statistics.

The U = tile blocks x slabs (tile block, slab) units are dealt to G workgroups as contiguous ranges [floor(b U / G), floor((b + 1) U / G)); a tile
block (64 tiles, nslab = C / 16 slabs) is cut wherever a range ends inside it.  With 3 tile blocks (B=2, 13x21: 154 tiles = 64 + 64 + 26):
  C = 48 (U = 9):  G = 2 cuts block 1 after its FIRST slab;  G = 3 cuts nothing (one piece per block, still through the reduction);
                   G = 5 gives ranges that span two blocks and cuts block 1 before its LAST slab;  G = 7 cuts block 0 into 3 pieces
  C = 80 (U = 15): G = 2 cuts block 1 in the middle;  G = 7 ranges of 2-3 slabs, 3 pieces per block
  G = 1: the whole problem in one workgroup (three blocks back to back, stored directly);  G = 0: the launcher's choice (one workgroup per 4 slabs here)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 2e-5                 # tests/test_gpu_wino.py: this operator against float64, relative to the output's maximum
STAT_TOL = 1e-5            # tests/test_gpu_wino.py: sum and sum of squares per channel


def rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def ref3x3(a, w9):
    """the definition in float64: nine shifted-slice matmuls, no library convolution (as tests/test_gpu_wino.py)"""
    B, H, W, Cc = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B * H * W, w9.shape[1], dtype=torch.float64)
    for r in range(3):
        for q in range(3):
            y += ap[:, r:r + H, q:q + W, :].reshape(-1, Cc) @ w9[r * 3 + q].t()
    return y


SHAPES = {
    # name: (B, H, W, Cb, N)
    "one_slab": (2, 13, 21, 16, 48),          # U = 3 tile blocks, one slab each: a forced G = 7 leaves four workgroups without work
    "tiny3x3": (1, 3, 3, 48, 48),             # 4 tiles: a single ragged tile block, odd extents
    "tiny5x7": (1, 5, 7, 48, 40),             # 12 tiles, N < 48
    "tt_plus_1": (1, 9, 25, 48, 48),          # 5 x 13 = 65 tiles: the last tile block holds one tile
    "c48": (2, 13, 21, 48, 48),
    "c80": (2, 13, 21, 80, 48),
}
GROUPS = {
    "one_slab": (0, 1, 2, 7),
    "tiny3x3": (0, 1, 2, 5),
    "tiny5x7": (0, 1, 3),
    "tt_plus_1": (0, 1, 2, 5),
    "c48": (0, 1, 2, 3, 5, 7),
    "c80": (0, 1, 2, 3, 5, 7),
}
_REF = {}


def problem(name, bn):
    """inputs on the CPU and the float64 reference, computed once per (shape, prologue) and never modified"""
    if (name, bn) not in _REF:
        B, H, W, Cb, N = SHAPES[name]
        g = torch.Generator().manual_seed(9100 + 7 * Cb + W)
        y = torch.randn(B, H, W, Cb, generator=g)
        w = torch.randn(9, N, Cb, generator=g) / (9 * Cb) ** 0.5
        sc = torch.rand(Cb, generator=g) + 0.5
        sh = torch.randn(Cb, generator=g) * 0.3
        a = (torch.relu(y * sc + sh) if bn else y).double()
        _REF[(name, bn)] = (y, w, sc, sh, ref3x3(a, w.double()))
    return _REF[(name, bn)]


def run(name, bn, G, stats, ws=None, dev=None):
    from md_rdm_amd import _lib
    from md_rdm_amd._lib import ConvDesc, check, ptr, stream
    L = _lib.lib()
    dev = dev or torch.device("cuda:0")
    B, H, W, Cb, N = SHAPES[name]
    y, w, sc, sh, _ = problem(name, bn)
    d = ConvDesc(B, H, W, Cb, Cb, N, 64, 3, 3, 1, 1, 1, 1)               # output: a channel slice of a 64-wide buffer
    yg, wg, scg, shg = y.to(dev), w.to(dev), sc.to(dev), sh.to(dev)
    if ws is None:
        nb = int(L.rdm_conv3x3_wino_workspace_bytes(Cb, B, H, W, G))
        ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
    out = torch.full((B * H * W, 64), float("nan"), device=dev)
    ssum = torch.zeros(N, dtype=torch.float64, device=dev)
    ssq = torch.zeros_like(ssum)
    check(L.rdm_conv3x3_wino_fwd(C.byref(d), ptr(yg), ptr(wg), ptr(scg) if bn else None, ptr(shg) if bn else None, ptr(out),
                                 ptr(ssum) if stats else None, ptr(ssq) if stats else None, ptr(ws), ws.numel(), G, stream()))
    return out.cpu(), ssum.cpu(), ssq.cpu()


def verify(name, bn, G, stats, got, ssum, ssq):
    N = SHAPES[name][4]
    want = problem(name, bn)[4]
    assert torch.isnan(got[:, N:]).all()                                  # nothing outside the N-channel slice is written
    e = rel(got[:, :N].double(), want)
    print(f"{name} bn={bn} G={G}: rel {e:.2e}")
    assert e < TOL, (name, bn, G, e)
    if stats:
        e0, e1 = rel(ssum, want.sum(0)), rel(ssq, (want ** 2).sum(0))
        print(f"    statistics: sum {e0:.2e}  sum of squares {e1:.2e}")
        assert e0 < STAT_TOL and e1 < STAT_TOL, (name, bn, G, e0, e1)


@pytest.mark.parametrize("bn", [True, False], ids=["bn1", "bn0"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_walk_vs_float64(name, bn):
    """every forced G of the shape, with the channel statistics requested and once without"""
    for G in GROUPS[name]:
        verify(name, bn, G, True, *run(name, bn, G, True))
    G = GROUPS[name][-1]
    verify(name, bn, G, False, *run(name, bn, G, False))


@pytest.mark.parametrize("name", ["c48", "c80"])
def test_same_partial_buffer_other_partition(name):
    """two launches on ONE workspace with different G: the second partition's pieces lie in other slots than the first's - a reduction that read
    a slot of the earlier launch (a stale piece) would miss the tolerance; and the same G again is bit-identical (no atomics in the sum)"""
    from md_rdm_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    B, H, W, Cb, N = SHAPES[name]
    nb = max(int(L.rdm_conv3x3_wino_workspace_bytes(Cb, B, H, W, G)) for G in (7, 2, 5))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    first = None
    for G in (7, 2, 5, 7):
        got, ssum, ssq = run(name, True, G, True, ws=ws)
        verify(name, True, G, True, got, ssum, ssq)
        if G == 7 and first is None:
            first = got
    assert torch.equal(got[:, :N], first[:, :N])
