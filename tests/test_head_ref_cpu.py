"""tests/head_ref.py (the float64 references tests/test_gpu_head_grads.py holds the kernels to) is itself checked here, without a GPU: its
gradients against torch float64 autograd of the plain composition, its values against the fixtures the reference wrote, and its clamp-gate
conventions against torch's own clamp / log backward on the edge inputs the GPU tests plant."""
import numpy as np
import pytest
import torch

import head_ref as hr
from md_rdm_amd import filler
from oracle import computations_cpu as ocp

U, LU = filler.uniform, filler.log_uniform
T64 = torch.float64


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _torch_dorn(x32, gP):
    """RDM_Net.py:313-345 with the float32 clamp restated on the exactly widened logits, so the gradient stays float64: the comparisons and
    the clamped values are the float32 ones (widening is exact, the bounds are the float32 bounds)."""
    x = t64(x32).requires_grad_(True)
    c = torch.clamp(x, min=float(hr.F32_LO), max=float(hr.F32_HI))
    P = torch.softmax(torch.stack((c[:, 0::2], c[:, 1::2]), dim=0), dim=0)[1]
    (P * t64(gP)).sum().backward()
    return P.detach().numpy(), x.grad.numpy()


def _torch_ordinal_loss(P, T, dloss=1.0):
    """loss.py:8-59 on the CPU, as the reference writes it (float32 logs and sums)"""
    Pt = t64(P).requires_grad_(True)
    N, C, H, W = Pt.shape
    K = torch.arange(C, dtype=torch.int64).view(1, C, 1, 1).expand(N, C, H, W)
    tt = torch.from_numpy(np.asarray(T).astype(np.int64))
    m0, m1 = K <= tt, K > tt
    loss = torch.sum(torch.log(torch.clamp(Pt[m0], min=1e-8, max=1e8).float())) + torch.sum(torch.log(torch.clamp(1.0 - Pt[m1], min=1e-8, max=1e8).float()))
    loss = loss / (-(N * H * W))
    (loss * dloss).backward()
    return float(loss.detach()), Pt.grad.numpy()


# ----------------------------------------------------------------------------------
# gradients == torch float64 autograd of the plain composition
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 7, 5, 7), (2, 90, 8, 10)])
def test_dorn_backward_is_torch_autograd(shape):
    B, K, H, W = shape
    for x in hr.dorn_inputs(filler, *shape):
        gP = U("hg.dorn.g", (B, K, H, W), -1, 1).astype(np.float64)
        P, dx = _torch_dorn(x, gP)
        np.testing.assert_allclose(hr.dorn(x)[1], P, rtol=1e-13, atol=0)
        want, gate = hr.dorn_backward64(x, gP)
        np.testing.assert_allclose(want, dx, rtol=1e-13, atol=0)
        assert np.array_equal(dx != 0, gate & (want != 0)) and not dx[~gate].any()
        got32, gate32 = hr.dorn_backward(x, gP)
        assert got32.dtype == np.float32 and np.array_equal(gate32, gate)
        assert np.all(np.abs(got32 - want) <= 2.0 ** -24 * np.abs(want) + 1e-45)           # one rounding to float32


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 7, 5, 7), (2, 90, 8, 8)])
def test_ordinal_loss_and_grad_are_torch_autograd(shape):
    for P, T in hr.ordinal_inputs(filler, *shape):
        loss, dP = _torch_ordinal_loss(P, T, dloss=0.75)
        want, gate = hr.ordinal_loss_grad(P, T, 0.75)
        # NOT 1e-13: the reference's backward of this node is float32.  torch rounds dloss / -(N*H*W) to float32 and divides it by float32(q)
        # (two float32 roundings); the restatement (oracle and kernel alike) scales the float32 reciprocal 1 / float32(q) in float64 (one).
        # Each rounding is within 2^-24 relative, so the two differ by at most 3 * 2^-24 (cross terms included); the gate is exact.
        assert np.all(np.abs(want - dP) <= 3 * 2.0 ** -24 * np.abs(want))
        np.testing.assert_array_equal(dP != 0, gate)
        assert not want[~gate].any() and np.all(want[gate] != 0)
        ref = hr.ordinal_loss(P, T)
        n = P.size
        assert abs(loss - ref) <= (np.log2(n) + 4) * 2.0 ** -24 * abs(ref)             # torch's float32 logs and pairwise float32 sums
        assert abs(float(ocp.ordinal_loss(P, T)) - ref) <= (np.log2(n) + 4) * 2.0 ** -24 * abs(ref)


@pytest.mark.parametrize("n_levels,B", [(1, 1), (2, 3), (4, 3), (8, 2)])
def test_fine_detail_pred_grad_is_torch_autograd(n_levels, B):
    per = hr.level_off(n_levels)
    levels = hr.split_levels(LU(f"hg.fd.{n_levels}.{B}", (B, per), 0.5, 2.0, dtype=np.float64), n_levels)
    dy = hr.split_levels(U(f"hg.fd.dy.{n_levels}.{B}", (B, per), -1, 1), n_levels)
    w = [torch.tensor(float(v), dtype=T64, requires_grad=True) for v in U("hg.fd.w", (n_levels,), 0.5, 1.5)]
    l32 = [torch.log(t64(l)).float().double() for l in levels]
    yh = [l * wk for l, wk in zip(l32, w)]
    for a, b in zip(hr.fine_detail_pred(levels, [wk.item() for wk in w]), yh):
        np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-15, atol=0)
    sum((y * t64(d)).sum() for y, d in zip(yh, dy)).backward()
    dw, s_abs = hr.fine_detail_pred_grad(levels, dy)
    for k in range(n_levels):
        assert abs(dw[k] - w[k].grad.item()) <= 1e-13 * s_abs[k]


@pytest.mark.parametrize("B,K,M", [(1, 1, 1), (3, 8, 4), (2, 2, 257), (2, 9, 16), (4, 6, 4096)])
def test_candidates_matvec_grad_is_torch_autograd(B, K, M):
    A = np.log(LU(f"hg.mv.a.{B}.{K}.{M}", (B, K, M), 0.5, 2.0, dtype=np.float64))
    w32 = U(f"hg.mv.w.{K}", (K,), 0.2, 0.8)
    dout = U(f"hg.mv.d.{B}.{M}", (B, M), -1, 1)
    w = t64(w32).requires_grad_(True)
    out = torch.matmul(t64(A).float().double().transpose(1, 2), w)
    got, s_abs = hr.candidates_matvec(A, w32)
    assert np.all(np.abs(got - out.detach().numpy()) <= 1e-13 * s_abs)
    (out * t64(dout)).sum().backward()
    dw, sw = hr.candidates_matvec_grad(A, dout)
    assert np.all(np.abs(dw - w.grad.numpy()) <= 1e-13 * sw)


@pytest.mark.parametrize("n_levels,n_out,first", [(1, 0, 0), (4, 3, 0), (4, 7, 0), (5, 7, 1), (8, 7, 0), (8, 7, 1), (2, 9, 0)])
def test_recombine_and_grad(n_levels, n_out, first):
    """the forward is the oracle's recombination; the autograd gradient is the sum of dout over each element's square footprint"""
    B = 2
    lv = [U(f"hg.rc.{n_levels}.{k}", (B, 1, 1 << k, 1 << k), -1, 1).astype(np.float64) for k in range(first, n_levels)]
    out, s_abs = hr.recombine(lv, n_out, first)
    if len(lv) > 1:                                              # the reference (and the oracle with it) pops two components: no single-level form
        np.testing.assert_array_equal(out, ocp.recombination(list(lv), n_out))
    else:
        np.testing.assert_array_equal(out, ocp.multi_upsample(lv[0], n_out - first))
    assert out.shape == (B, 1, 1 << n_out, 1 << n_out) and np.all(s_abs >= np.abs(out))
    dout = U(f"hg.rc.d.{n_out}", out.shape, -1, 1).astype(np.float64)
    g, gs = hr.recombine_grad([l.shape for l in lv], dout, n_out, first)
    for k, a, s in zip(range(first, n_levels), g, gs):
        assert np.all(np.abs(a - hr.block_sums(dout, k)) <= 1e-13 * s)
        assert s.shape == a.shape


# ----------------------------------------------------------------------------------
# values == the fixtures written by the reference, at the tolerances tests/test_oracle_ops.py holds the oracle to
# ----------------------------------------------------------------------------------
def test_fixtures_dorn(op_gold):
    xl = U("op.dorn", (2, 180, 8, 10), -2.0, 3.0)
    xl.flat[::53] = 2e4
    xl.flat[7::59] = -5.0
    xl[0, 10, 0, 0] = xl[0, 11, 0, 0]
    dec, P = hr.dorn(xl)
    np.testing.assert_array_equal(dec, op_gold["dorn_decode"])
    np.testing.assert_allclose(P, op_gold["dorn_labels"], rtol=1e-14, atol=1e-300)
    g = U("op.dorn_g", (2, 90, 8, 10), -1, 1).astype(np.float64)
    np.testing.assert_allclose(hr.dorn_backward(xl, g)[0], op_gold["dorn_dx"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hr.dorn_backward64(xl, g)[0], op_gold["dorn_dx"], rtol=1e-6, atol=1e-9)


def test_fixtures_ordinal_loss(op_gold):
    P = U("op.ol_p", (2, 90, 8, 8), 0.0, 1.0).astype(np.float64)
    P.flat[::97] = 0.0
    P.flat[5::101] = 1.0
    T = np.floor(U("op.ol_t", (2, 1, 8, 8), 0, 95)).astype(np.int32)
    assert abs(hr.ordinal_loss(P, T) - float(op_gold["ordinal_loss"])) < 2e-5 * abs(float(op_gold["ordinal_loss"]))
    np.testing.assert_allclose(hr.ordinal_loss_grad(P, T)[0], op_gold["ordinal_loss_dP"], rtol=1e-6, atol=1e-12)


def test_fixtures_make_pred_and_recombination(op_gold):
    f1 = [LU(f"op.fd1_{i}", (2, 1, 2 ** i, 2 ** i), 0.5, 2.0).astype(np.float64) for i in range(4)]
    f2 = [LU(f"op.fd2_{i}", (2, 1, 2 ** i, 2 ** i), 0.5, 2.0).astype(np.float64) for i in range(1, 4)]
    mats = ocp.relative_fine_detail_matrix([f1, f2])
    w = [U("op.w0", (1, 1), 0.5, 1.5), U("op.w1", (2, 1), 0.2, 0.8), U("op.w2", (2, 1), 0.2, 0.8), U("op.w3", (2, 1), 0.2, 0.8)]
    for i, (A, wi) in enumerate(zip(mats, w)):
        got = hr.candidates_matvec(A, wi)[0].reshape(2, 1, 2 ** i, 2 ** i)
        np.testing.assert_allclose(got, op_gold[f"make_pred_{i}"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(hr.fine_detail_pred([f1[0]], [w[0]])[0], op_gold["make_pred_0"], rtol=1e-5, atol=1e-6)   # one candidate: the fused form
    comps = [U(f"op.rc{i}", (2, 1, 2 ** i, 2 ** i), -1.0, 1.0).astype(np.float64) for i in range(4)]
    np.testing.assert_allclose(hr.recombine(comps, 3, 0)[0], op_gold["recombination_n3"], rtol=1e-14)
    np.testing.assert_allclose(hr.recombine(comps[1:], 4, 1)[0], op_gold["recombination_n4_rel"], rtol=1e-14)


# ----------------------------------------------------------------------------------
# clamp-gate conventions == torch's clamp / log backward on the planted edges
# ----------------------------------------------------------------------------------
def test_dorn_gate_is_torchs_float32_clamp_backward():
    """the reference clamps the float32 logits (RDM_Net.py:334): torch passes the gradient where lo <= x <= hi, equality included, with the
    bounds taken as float32"""
    pairs = np.array(hr.dorn_planted_pairs(), dtype=np.float32)
    x = torch.from_numpy(pairs.copy()).requires_grad_(True)
    c = torch.clamp(x, min=1e-8, max=1e4)
    c.sum().backward()
    passed = x.grad.numpy() != 0
    np.testing.assert_array_equal(passed, hr.dorn_gate(pairs))
    np.testing.assert_array_equal(c.detach().numpy(), np.clip(pairs, hr.F32_LO, hr.F32_HI))
    lo, hi = hr.F32_LO, hr.F32_HI
    for v, want in [(lo, True), (hi, True), (np.nextafter(lo, np.float32(-1)), False), (np.nextafter(lo, np.float32(1)), True),
                    (np.nextafter(hi, np.float32(0)), True), (np.nextafter(hi, np.float32(np.inf)), False), (np.float32(-3), False), (np.float32(2e4), False)]:
        assert v in pairs and bool(hr.dorn_gate(v)) == want, v
    # and through the whole head: the float32 autograd of the reference's expression is zero exactly where the gate is closed
    xs = pairs.reshape(1, len(pairs), 2).transpose(0, 2, 1).reshape(1, 2, len(pairs), 1)       # (B=1, 2K=2, H=n, W=1): every pixel one pair
    xt = torch.from_numpy(np.ascontiguousarray(xs)).requires_grad_(True)
    cc = torch.clamp(torch.cat((xt[:, ::2].reshape(1, 1, -1), xt[:, 1::2].reshape(1, 1, -1)), dim=1), min=1e-8, max=1e4).double()
    torch.softmax(cc, dim=1)[:, 1].sum().backward()
    want, gate = hr.dorn_backward(xs, np.ones((1, 1, len(pairs), 1)))
    assert not xt.grad.numpy()[~gate].any()
    np.testing.assert_allclose(xt.grad.numpy(), want, rtol=2.0 ** -23, atol=0)


def test_ordinal_gate_is_torchs_clamp_and_log_backward():
    """every planted probability under every planted label, K = 3: q = P on the k <= label side, 1 - P on the other; the gradient passes
    where 1e-8 <= q <= 1e8 (q == 1e-8 passes and so does 1 - (1 - 1e-8), which rounds to just above 1e-8; 5e-9 and 0 do not) and is the float32 reciprocal there"""
    K = 3
    tv, pv = hr.ordinal_targets(K), hr.ORDINAL_P
    P = np.empty((len(tv), K, len(pv), 1))
    P[:] = np.array(pv).reshape(1, 1, -1, 1)
    T = np.empty((len(tv), 1, len(pv), 1), dtype=np.int32)
    T[:] = np.array(tv, dtype=np.int64).astype(np.int32).reshape(-1, 1, 1, 1)
    _, dP = _torch_ordinal_loss(P, T)
    want, gate = hr.ordinal_loss_grad(P, T)
    np.testing.assert_array_equal(dP != 0, gate)
    assert np.all(np.abs(want - dP) <= 3 * 2.0 ** -24 * np.abs(want))       # float32 scale and division in torch: see the autograd test above
    n = P.shape[0] * P.shape[2]
    for j, p in enumerate(pv):
        lo_side, hi_side = dP[0, 0, j, 0], dP[4, 0, j, 0]          # label 0 -> k = 0 is on the P side; label -1 -> on the 1 - P side
        assert (lo_side != 0) == (1e-8 <= p <= 1e8) and (hi_side != 0) == (1e-8 <= 1.0 - p <= 1e8)
        if lo_side != 0:
            assert want[0, 0, j, 0] == (-1.0 / n) * float(np.float32(1) / np.float32(p))
    assert dP[0, 0, 2, 0] != 0 and dP[0, 0, 3, 0] == 0 and dP[4, 0, 4, 0] != 0 and dP[4, 0, 1, 0] == 0 and dP[0, 0, 0, 0] == 0
    # labels outside [0, K): K, 95 put every k on the P side, -1 and -2**31 every k on the 1 - P side
    lower = np.arange(K).reshape(1, K, 1, 1) <= T.astype(np.int64)
    assert lower[2].all() and lower[3].all() and not lower[4].any() and not lower[5].any()
    assert np.all(dP[lower] <= 0) and np.all(dP[~lower] >= 0)
