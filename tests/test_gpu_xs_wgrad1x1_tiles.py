"""-m gpu: the tile edges of xs_wgrad1x1_kernel (csrc/xsplit.hip) through rdm_conv2d_wgrad_x3 vs float64, at the 2e-5 of the tensor's maximum
that tests/test_gpu_xsplit.py holds the kernel to.  One body serves every shape (256-row tiles, four 64-row waves by two column halves), so no
case depends on a selection rule; the shapes sit on both sides of every edge: row tiles (N below one tile, across 128 and 256 with ragged
remainders), column tiles (96 / 144 / 192 / 144 + 96 / 192 + 144: NT = 6 / 9 / 12, the 5 + 4 wave split of NT = 9), slab counts (one ragged slab,
two, four ragged - both image sets of the 256-row body - and 33 full ones), the K split (auto, 1, and explicit values up to and above the slab
count), the BatchNorm + ReLU prologue, and both split-row operand forms."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 2e-5

CASES = [
    # N, C, ld, (B, H, W), bn
    (4, 96, 96, (1, 4, 5), False),          # below one row tile; one 96-channel tile; one ragged slab (20 pixels)
    (132, 144, 160, (1, 5, 7), True),       # across 128; one 144-channel tile (NT = 9: 5 + 4); two slabs (35 pixels); ld > C
    (260, 192, 192, (1, 1, 97), True),      # across 256; one 192-channel tile; four slabs, the last ragged (97 pixels)
    (388, 240, 272, (1, 32, 33), False),    # 256 + 132; tiles 144 + 96; 33 full slabs; ld > C
    (260, 336, 352, (1, 1, 97), True),      # tiles 192 + 144; ld > C
    (132, 240, 240, (1, 32, 33), True),     # tiles 144 + 96 with the prologue, 33 slabs
    (388, 144, 144, (1, 1, 97), False),     # NT = 9 over two 256-row tiles
    (388, 96, 128, (1, 5, 7), True),        # NT = 6 (3 + 3), two slabs; ld > C
]
SPLITS = (0, 1, 2, 5, 7)


def rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-30)


def _total(_lib):
    return sum(v for k, v in _lib.census().items() if k.startswith("xs_wgrad1x1_kernel/"))


@pytest.fixture(scope="module", autouse=True)
def _census_on():
    from md_rdm_amd import _lib
    L = _lib.lib()
    L.rdm_census_reset()
    L.rdm_census_enable(1)
    yield
    L.rdm_census_enable(0)


_REF = {}


def _operands(case):
    """Seeded operands and the float64 product of a case: computed once, shared by the tests, never modified."""
    if case not in _REF:
        N, Cc, ld, (B, H, W), bn = case
        M = B * H * W
        g = torch.Generator().manual_seed(5000 + 7 * N + Cc + M)
        x = torch.randn(M, ld, generator=g)
        x[:, Cc:] = float("nan")                                                    # nothing behind column C may reach a product
        gy = torch.randn(M, N, generator=g)
        sc = torch.rand(Cc, generator=g) + 0.5
        sh = torch.randn(Cc, generator=g) * 0.3
        a = (torch.relu(x[:, :Cc] * sc + sh) if bn else x[:, :Cc]).double()
        want = gy.double().t() @ a
        dev = torch.device("cuda:0")
        _REF[case] = (x.to(dev), gy.to(dev), sc.to(dev), sh.to(dev), want)
    return _REF[case]


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_c{c[1]}_m{c[3][0] * c[3][1] * c[3][2]}_bn{int(c[4])}" for c in CASES])
def test_tiles_vs_float64(case):
    from md_rdm_amd import _lib
    from md_rdm_amd._lib import ConvDesc, check, ptr, stream
    L = _lib.lib()
    N, Cc, ld, (B, H, W), bn = case
    xg, gyg, scg, shg, want = _operands(case)
    d = ConvDesc(B, H, W, Cc, ld, N, N, 1, 1, 1, 1, 0, 0)
    for split in SPLITS:
        before = _total(_lib)
        dw = torch.zeros(N, Cc, device=xg.device)
        check(L.rdm_conv2d_wgrad_x3(C.byref(d), ptr(gyg), ptr(xg), ptr(scg) if bn else None, ptr(shg) if bn else None, ptr(dw), split, 0, stream()))
        err = rel(dw.cpu().double(), want)
        print(f"N={N} C={Cc} M={B * H * W} bn={bn} split_k={split}: {err:.2e}")
        assert err < TOL, (split, err)
        assert _total(_lib) == before + 1, split                                   # one launch, one census hit


@pytest.mark.parametrize("case", CASES, ids=[f"n{c[0]}_c{c[1]}_m{c[3][0] * c[3][1] * c[3][2]}_bn{int(c[4])}" for c in CASES])
def test_tiles_on_split_rows(case):
    """Split-row operands (0x10: dY; 0x30: dY and the activated input): 2e-5 against float64 at every split; at split_k = 1 the same bits as the
    float32-operand launch (same operand bits, one workgroup per output, one accumulation order) and the same bits from one launch to the next."""
    from md_rdm_amd import _lib
    from md_rdm_amd._lib import ConvDesc, check, ptr, stream
    L = _lib.lib()
    N, Cc, ld, (B, H, W), bn = case
    M = B * H * W
    xg, gyg, scg, shg, want = _operands(case)
    dev = xg.device
    gy_rows = torch.empty(M, N, device=dev)
    check(L.rdm_split_rows_f32(ptr(gyg), N, None, None, ptr(gy_rows), N, M, N, stream()))
    x_rows = torch.empty(M, Cc, device=dev)
    check(L.rdm_split_rows_f32(ptr(xg), ld, ptr(scg) if bn else None, ptr(shg) if bn else None, ptr(x_rows), Cc, M, Cc, stream()))
    d_f32 = ConvDesc(B, H, W, Cc, ld, N, N, 1, 1, 1, 1, 0, 0)
    d_rows = ConvDesc(B, H, W, Cc, Cc, N, N, 1, 1, 1, 1, 0, 0)
    refs = []
    for _ in range(2):
        ref = torch.zeros(N, Cc, device=dev)
        check(L.rdm_conv2d_wgrad_x3(C.byref(d_f32), ptr(gyg), ptr(xg), ptr(scg) if bn else None, ptr(shg) if bn else None, ptr(ref), 1, 0, stream()))
        refs.append(ref)
    assert torch.equal(refs[0], refs[1])
    for flags, desc, xop, bnp in ((0x10, d_f32, xg, bn), (0x30, d_rows, x_rows, False)):
        for split in SPLITS:
            before = _total(_lib)
            dw = torch.zeros(N, Cc, device=dev)
            check(L.rdm_conv2d_wgrad_x3(C.byref(desc), ptr(gy_rows), ptr(xop), ptr(scg) if bnp else None, ptr(shg) if bnp else None, ptr(dw), split, flags, stream()))
            err = rel(dw.cpu().double(), want)
            assert err < TOL, (hex(flags), split, err)
            assert _total(_lib) == before + 1, (hex(flags), split)
            if split == 1:
                assert torch.equal(dw, refs[0]), hex(flags)
