"""tests/xsplit_ref.py without a GPU: every planted case of tests/test_gpu_xsplit_exact.py against the conditions under which the split-precision
kernels' f32 arithmetic is exact, and the teeth of the retained-terms reference.
  (a) every retained plane product is a multiple of one quantum q and sum |product| < 2^24 q per output, in the case's arithmetic (x3 / x6) and in
      the one-product mode;
  (b) both operands have non-zero lo planes (the x6 cases non-zero third planes), zero elements and elements with a zero lo part, and no value
      that is split sits on a bf16 tie;
  (c) gated cases: exact ties (gated off), elements on either side, and statistics (sum dz, sum dz y) whose addends are multiples of a quantum with
      sum |addend| < 2^24 quanta; the accumulating epilogue's result is an f32 number; the mirrored x6 cases: the same for sum y and sum y^2;
  (d) teeth: the reference differs from the full float64 product (a kernel that added lo x lo would be noticed), from itself with one cross term
      dropped in one k-step of one tile, and from itself with one lo value moved to the neighbouring row.
These are conditions on the inputs (the reference alone), not measurements of a kernel."""
import functools

import numpy as np
import pytest
import torch

import xsplit_ref as X

torch.set_num_threads(min(16, torch.get_num_threads()))
ALL = [(op, name) for op, (cases, _, _) in X.BUILDERS.items() for name in cases]
IDS = ["%s-%s" % c for c in ALL]


@functools.lru_cache(maxsize=2)
def built(op, name):
    _, build, np_ = X.BUILDERS[op]
    c = build(name)
    return (c, np_) + X.reference(c, np_)


@pytest.mark.parametrize("op,name", ALL, ids=IDS)
def test_case_is_exactly_summable(op, name):
    c, np_, ref, mag, ap, bp = built(op, name)
    assert X.exact_ok(ap, bp, X.PAIRS[np_], mag).all(), (mag.max(), X.quantum(ap, bp, X.PAIRS[np_]))                         # (a)
    assert X.exact_ok(ap[:1], bp[:1], X.X1, c["mm"](np.abs(ap[0]), np.abs(bp[0]))).all()
    assert X.is_f32(ref)
    assert X.no_ties(c["A"]) and X.no_ties(c["Bop"])                                                                            # (b): the values that are split
    for p in (ap, bp):
        assert (p[1] != 0).sum() >= 10 and ((p[0] == 0) & (p[1] == 0)).any() and ((p[0] != 0) & (p[1] == 0)).any()
        assert np_ != 6 or (p[2] != 0).sum() >= 10
    if "gate" in c:                                                                                                             # (c)
        q = X.quantum(ap, bp, X.PAIRS[np_])
        y, gate, ties = np.nan_to_num(c["y"][:, :ref.shape[1]], nan=0.0), c["gate"], c["ties"]
        assert ties.sum() >= 10 and gate.mean() > 0.2 and (~gate & ~ties).mean() > 0.2 and not (gate & ties).any()
        dz = ref * gate
        assert X.stats_ok(dz, q).all() and X.stats_ok(dz * y, q / 2).all()
        r1 = X.reference(c, 1)                                                                                                   # and in the one-product mode
        q1 = X.quantum(r1[2], r1[3], X.X1)
        assert X.stats_ok(r1[0] * gate, q1).all() and X.stats_ok(r1[0] * gate * y, q1 / 2).all()
        if "G0" in c:
            assert X.is_f32(c["G0"] + c["sc"] * dz)
    if c.get("mirror"):
        assert X.stats_ok(ref, 0.25).all() and X.stats_ok(ref * ref, 1.0 / 16).all() and (ref != 0).mean() > 0.2


@pytest.mark.parametrize("op,name", ALL, ids=IDS)
def test_reference_has_teeth(op, name):
    c, np_, ref, mag, ap, bp = built(op, name)
    A, mm = c["A"], c["mm"]
    if not c.get("mirror"):
        assert (mm(A, c["Bop"]) != ref).any()                 # the dropped products are visible: a kernel that added lo x lo would not match
    lo2 = ap[1].reshape(-1, A.shape[-1])
    nz = np.argwhere(lo2 != 0)
    r, k = nz[len(nz) // 2]
    # one cross term (a_lo b_hi) dropped for one k-step (32 of the contracted index) of one 16-row tile
    mask = np.zeros_like(lo2)
    if c["kaxis"] == 1:
        mask[r // 16 * 16:r // 16 * 16 + 16, k // 32 * 32:k // 32 * 32 + 32] = 1.0
    else:
        mask[r // 32 * 32:r // 32 * 32 + 32, k // 16 * 16:k // 16 * 16 + 16] = 1.0
    assert mm((lo2 * mask).reshape(A.shape), bp[0]).any()
    # one lo value moved to the neighbouring row
    r = min(r, lo2.shape[0] - 2)
    d = np.zeros_like(lo2)
    for (rr, kk) in nz[len(nz) // 2:len(nz) // 2 + 8]:
        rr = min(rr, lo2.shape[0] - 2)
        if lo2[rr, kk] != lo2[rr + 1, kk]:
            d[rr, kk], d[rr + 1, kk] = lo2[rr + 1, kk] - lo2[rr, kk], lo2[rr, kk] - lo2[rr + 1, kk]      # the two rows' values swapped
            break
    assert d.any() and mm(d.reshape(A.shape), bp[0]).any()


def test_split_restatement():
    """planes() and split_rows_bits() against _split_rows_ref of tests/test_gpu_xsplit.py on the values of test_split_rows_producers_are_bit_exact"""
    from test_gpu_xsplit import _split_rows_ref
    g = torch.Generator().manual_seed(77)
    M, Cc, ld = 1037, 144, 160
    x = torch.randn(M, ld, generator=g) * torch.logspace(-3, 3, ld)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    act = torch.relu((x[:, :Cc].double() * sc.double() + sh.double()).float())
    for v in (x[:, :Cc].contiguous(), act):
        want = _split_rows_ref(v)
        assert torch.equal(X.split_rows_bits(v), want)
        p = X.planes(v.double().numpy(), 3)
        w16 = want.view(torch.bfloat16).double().numpy()
        assert np.array_equal(p[0], w16[:, :, :4].reshape(M, Cc)) and np.array_equal(p[1], w16[:, :, 4:].reshape(M, Cc))
        assert np.array_equal(p[0] + p[1] + p[2], v.double().numpy())          # three planes hold all 24 bits
    v = X.plant("restate", (64, 48), 3, 0.6, 0.5, 0.3)
    p = X.planes(v, 3)
    H = np.round(v)
    assert np.array_equal(p[0][H != 0], H[H != 0]) and (p[2] != 0).any() and np.array_equal(p[0] + p[1] + p[2], v)


def test_shapes_reach_the_intended_paths():
    """the launchers' rules restated (xsplit_ref) give what the case tables claim"""
    for name, (Bn, H, W, C, N, bn) in X.WGRAD1_CASES.items():
        assert X.wgrad1_auto_split(Bn * H * W, C, N) == (2 if "split" in name else 1) and (Bn * H * W) % 32 != 0
    items, slots, lds = X.dgrad3_grid(*X.DGRAD3_CASES["walk"][:4])
    assert items > slots == 256 and items < 2 * slots
    assert X.dgrad3_grid(1, 2, 318, 48)[2] <= 156 * 1024 < X.dgrad3_grid(1, 2, 319, 48)[2]
    assert X.dgrad3_grid(*X.DGRAD3_CASES["cb48_tiny"][:4])[:2] == (1, 512)
    for Bn, H, W, C, ld, N, ldg, bn in X.WGRAD3_CASES.values():
        assert X.cdiv(Bn * (H + 2) * (W + 2), 32) // 8 >= 3 and W <= 93
    for Bn, H, W, K, N, dg, dw in X.DGRAD1_CASES.values():
        assert (Bn * H * W) % 16 != 0 and K >= 32
    assert 3 * 2731 == 8193
