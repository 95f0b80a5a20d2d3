"""-m gpu: the head's backward kernels (csrc/dorn.hip), the pyramid kernels (csrc/postproc.hip) and the routing of network/computations.py
against the float64 references of tests/head_ref.py (themselves checked in tests/test_head_ref_cpu.py).  Each kernel is reached through the
Python wrapper AND through the C ABI; a buffer handed to the C ABI is NaN-filled first, so an element the kernel does not write shows.
The tolerances come from the float32 / float64 roundings of each kernel and are written at the asserts; S_abs is the sum of the absolute
values of the terms behind an output."""
import functools

import numpy as np
import pytest
import torch

import head_ref as hr
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
U, LU = filler.uniform, filler.log_uniform
E23, E24 = 2.0 ** -23, 2.0 ** -24
DEV = "cuda:0"


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from md_rdm_amd import _lib, loss
    from md_rdm_amd.network import computations as cp
    return dict(cp=cp, loss=loss, L=_lib.lib(), lib=_lib)


def g(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nans(shape, dtype):
    if dtype == torch.int64:
        return torch.full(shape, -(2 ** 62), dtype=dtype, device=DEV)            # no NaN in an integer buffer: a value no count can take
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def c(t):
    return t.detach().cpu().numpy()


def close(got, want, rel, s_abs=None, abs_rel=0.0, what=""):
    """|got - want| <= rel * |want| + abs_rel * S_abs element-wise, NaN never passes; prints the worst ratio before asserting"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    tol = rel * np.abs(want) + (abs_rel * np.asarray(s_abs) if s_abs is not None else 0.0)
    err = np.abs(got - want)
    bad = ~(err <= tol)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))) if got.size else 0.0
    print(f"{what}: worst error / tolerance = {worst:.3g}")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the tolerance, first at {np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r} want {want[bad][0]!r}"


# ------------------------------------------------------------------------------------------
# DORN head
# ------------------------------------------------------------------------------------------
DORN_SHAPES = [(1, 1, 1, 1), (3, 7, 5, 7), (2, 90, 8, 10), (16, 90, 19, 20)]       # the last: 547 200 pairs > 2048 x 256, a second grid-stride pass


@functools.lru_cache(maxsize=None)
def dorn_ref(shape):
    B, K, H, W = shape
    gP = U(f"hg.dorn.g.{B}x{K}x{H}x{W}", (B, K, H, W), -1, 1).astype(np.float64)
    out = []
    for x in hr.dorn_inputs(filler, *shape):
        dec, P = hr.dorn(x)
        dx, gate = hr.dorn_backward(x, gP)
        out.append((x, gP, dec, P, dx, gate))
    return out


def check_dorn(ref, dec, P, dx):
    x, gP, wdec, wP, wdx, gate = ref
    np.testing.assert_array_equal(c(dec), wdec)                                   # bit-exact ordinal indices
    np.testing.assert_allclose(c(P), wP, rtol=1e-14, atol=0)
    dx = c(dx)
    assert dx.dtype == np.float32
    close(dx, wdx, E23, what="dorn dx")                                           # one float32 rounding of a float64 value (observed: equal bit for bit)
    assert not dx[~gate].any() and not np.isnan(dx).any()                         # a closed clamp gate passes exactly nothing


@pytest.mark.parametrize("shape", DORN_SHAPES)
def test_dorn_through_the_wrapper(env, shape):
    for ref in dorn_ref(shape):
        xt = g(ref[0]).requires_grad_(True)
        dec, P = env["cp"].dorn_ordinal_regression(xt)
        assert dec.dtype == torch.int64 and P.dtype == torch.float64
        (P * g(ref[1])).sum().backward()
        check_dorn(ref, dec, P, xt.grad)


@pytest.mark.parametrize("shape", DORN_SHAPES)
def test_dorn_through_the_c_abi(env, shape):
    B, K, H, W = shape
    L, lib = env["L"], env["lib"]
    for ref in dorn_ref(shape):
        xt, gt = g(ref[0]), g(ref[1])
        P, dec, dx = nans((B, K, H, W), torch.float64), nans((B, 1, H, W), torch.int64), nans((B, 2 * K, H, W), torch.float32)
        lib.check(L.rdm_dorn_fwd(lib.ptr(xt), lib.ptr(P), lib.ptr(dec), B, K, H * W, lib.stream()))
        lib.check(L.rdm_dorn_bwd(lib.ptr(xt), lib.ptr(gt), lib.ptr(dx), B, K, H * W, lib.stream()))
        check_dorn(ref, dec, P, dx)


# ------------------------------------------------------------------------------------------
# ordinal loss
# ------------------------------------------------------------------------------------------
OL_SHAPES = [(1, 1, 1, 1), (3, 7, 5, 7), (2, 90, 8, 8), (16, 90, 8, 10)]          # the last: 450 blocks' worth > the 256-block cap, a second pass
DLOSS = 0.75


@functools.lru_cache(maxsize=None)
def ol_ref(shape):
    out = []
    for P, T in hr.ordinal_inputs(filler, *shape):
        dP, gate = hr.ordinal_loss_grad(P, T, DLOSS)
        out.append((P, T, hr.ordinal_loss(P, T), dP, gate))
    return out


def check_ol(ref, loss, dP, loss_rel=None):
    P, T, wloss, wdP, gate = ref
    nblocks = min(-(-P.size // 256), 256)
    # every term has one sign (q <= 1), so nothing cancels: each block's partial is rounded to float32 once and each of the atomic additions
    # rounds a running sum no larger than the total - nblocks * 2^-24 together; 6 * 2^-24 covers 2 ulp of logf per term and the final rounding
    rel = (nblocks + 6) * E24 if loss_rel is None else loss_rel              # observed: at most 0.11 of it
    print(f"ordinal loss: got {loss!r} want {wloss!r} error / tolerance = {abs(loss - wloss) / (rel * abs(wloss)) if wloss else abs(loss - wloss):.3g}")
    assert abs(loss - wloss) <= rel * abs(wloss)
    dP = c(dP)
    close(dP, wdP, E23, what="ordinal dP")                                        # the float32 reciprocal the kernel restates, scaled in float64 (observed 3e-9 of it)
    assert not dP[~gate].any() and not np.isnan(dP).any()
    np.testing.assert_array_equal(dP != 0, wdP != 0)


def ol_wrapper(env, ref):
    Pt = g(ref[0]).requires_grad_(True)
    lo = env["loss"].Ordinal_Loss().calc(Pt, g(ref[1]), cuda=True)
    assert lo.dtype == torch.float32
    (lo * DLOSS).backward()
    return float(lo.detach()), Pt.grad


def ol_abi(env, ref):
    L, lib = env["L"], env["lib"]
    B, K, H, W = ref[0].shape
    Pt, Tt = g(ref[0]), g(ref[1])
    lo, dP = nans((1,), torch.float32), nans((B, K, H, W), torch.float64)
    dl = torch.full((1,), DLOSS, dtype=torch.float32, device=DEV)
    lib.check(L.rdm_ordinal_loss_fwd(lib.ptr(Pt), lib.ptr(Tt), lib.ptr(lo), B, K, H * W, lib.stream()))
    lib.check(L.rdm_ordinal_loss_bwd(lib.ptr(Pt), lib.ptr(Tt), lib.ptr(dl), lib.ptr(dP), B, K, H * W, lib.stream()))
    return float(lo[0]), dP


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("shape", OL_SHAPES)
def test_ordinal_loss(env, shape, via):
    """probabilities 0, 1, 1e-8, 5e-9, 1 - 1e-8, 0.5 under labels 0, K-1, K, 95, -1 and -2**31 (what depth2label_sid gives a non-positive depth)"""
    for ref in ol_ref(shape):
        check_ol(ref, *(ol_wrapper if via == "wrapper" else ol_abi)(env, ref))


@functools.lru_cache(maxsize=None)
def spike_ref(at):
    B, K, H, W = OL_SHAPES[-1]
    T = np.floor(U("hg.ol.spike.t", (B, 1, H, W), 0, K)).astype(np.int32)
    T.flat[::17] = np.resize(np.array(hr.ordinal_targets(K), dtype=np.int64).astype(np.int32), len(T.flat[::17]))
    P = (np.arange(K).reshape(1, K, 1, 1) <= T.astype(np.int64)).astype(np.float64)           # q == 1 everywhere: every log is 0 ...
    P.flat[at if at >= 0 else P.size + at] = 0.5                                                # ... but one: q = 0.5 on either side
    dP, gate = hr.ordinal_loss_grad(P, T, DLOSS)
    wloss = hr.ordinal_loss(P, T)
    assert abs(wloss - np.log(2.0) / (B * H * W)) <= 4 * E24 * wloss and gate.all()
    return P, T, np.log(2.0) / (B * H * W), dP, gate


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("at", [0, 65536, -1])
def test_ordinal_loss_sees_one_element(env, at, via):
    """one term among 115 200 (the first, the first of the capped grid's second pass, the last): the loss must be log(2) / (B*HW) to 2^-22 -
    logf(0.5f), the block's float32 partial and the division are one rounding each, the other partials are exact zeros"""
    ref = spike_ref(at)
    check_ol(ref, *(ol_wrapper if via == "wrapper" else ol_abi)(env, ref), loss_rel=2.0 ** -22)


# ------------------------------------------------------------------------------------------
# pyramid nodes
# ------------------------------------------------------------------------------------------
def dw_close(got, want, s_abs, what):
    # a float64 sum of exact products rounded once to float32: 2^-23 |want| holds the rounding twice over, 1e-12 S_abs the float64 summation
    # order (at most 1024 sequential additions per thread, 2^-53 each)
    close(got, want, E23, s_abs, 1e-12, what)                                  # observed: at most 0.42 of it (the float32 rounding)


@functools.lru_cache(maxsize=None)
def fd_ref(n_levels, B):
    per = hr.level_off(n_levels)
    packed = LU(f"hg.fd.{n_levels}.{B}", (B, per), 0.5, 2.0, dtype=np.float64)
    levels = hr.split_levels(packed, n_levels)
    w = U(f"hg.fd.w.{n_levels}", (n_levels,), 0.5, 1.5)
    dy = U(f"hg.fd.dy.{n_levels}.{B}", (B, per), -1, 1)
    # a second dyhat, orthogonal per level to float32(log L): the gradient nearly cancels, so what is left shows the float32 rounding of the log
    l32 = hr.pack_levels(hr.log32(levels), n_levels)
    dyc = dy.astype(np.float64).copy()
    for k in range(n_levels):
        s = slice(hr.level_off(k), hr.level_off(k + 1))
        dyc[:, s] -= (dyc[:, s] * l32[:, s]).sum() / (l32[:, s] ** 2).sum() * l32[:, s]
    dyc = dyc.astype(np.float32)
    grads = [hr.fine_detail_pred_grad(levels, hr.split_levels(d, n_levels)) for d in (dy, dyc)]
    return packed, w, hr.pack_levels(hr.fine_detail_pred(levels, w), n_levels), (dy, dyc), grads


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("n_levels", [1, 2, 4, 8])
def test_fine_detail_pred(env, n_levels, B, via):
    packed, w, want, dys, grads = fd_ref(n_levels, B)
    L, lib, cp = env["L"], env["lib"], env["cp"]
    pt = g(packed)
    if via == "wrapper":
        wt = [torch.nn.Parameter(g(np.array([[v]], dtype=np.float32))) for v in w]
        yhat = cp._FineDetailPred.apply(pt, n_levels, *wt)
        dws = [torch.stack([x.reshape(()) for x in torch.autograd.grad(yhat, wt, g(dy), retain_graph=True)]) for dy in dys]
    else:
        yhat = nans(packed.shape, torch.float32)
        lib.check(L.rdm_fine_detail_pred_f32(lib.ptr(pt), lib.ptr(g(w)), lib.ptr(yhat), B, n_levels, lib.stream()))
        dws = []
        for dy in dys:
            dws.append(nans((n_levels,), torch.float32))
            lib.check(L.rdm_fine_detail_pred_bwd(lib.ptr(pt), lib.ptr(g(dy)), lib.ptr(dws[-1]), B, n_levels, lib.stream()))
    assert yhat.dtype == torch.float32
    np.testing.assert_allclose(c(yhat), want, rtol=1e-6, atol=1e-8)
    for dw, (wdw, s_abs), name in zip(dws, grads, ("dw", "dw, cancelling dyhat")):
        dw_close(c(dw), wdw, s_abs, f"fine_detail_pred {name}")


MV_SHAPES = [(1, 1, 1), (3, 8, 4), (2, 2, 257), (2, 3, 1024), (16, 6, 16384)]


@functools.lru_cache(maxsize=None)
def mv_ref(B, K, M):
    A = np.log(LU(f"hg.mv.a.{B}.{K}.{M}", (B, K, M), 0.5, 2.0, dtype=np.float64))          # not float32 values: the (float) cast of A counts
    w = U(f"hg.mv.w.{K}", (K, 1), 0.2, 0.8)
    dout = U(f"hg.mv.d.{B}.{M}", (B, M), -1, 1)
    return A, w, dout, hr.candidates_matvec(A, w), hr.candidates_matvec_grad(A, dout)


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("B,K,M", MV_SHAPES)
def test_candidates_matvec(env, B, K, M, via):
    A, w, dout, (want, s_abs), (wdw, sw) = mv_ref(B, K, M)
    L, lib, cp = env["L"], env["lib"], env["cp"]
    At = g(A)
    if via == "wrapper":
        wt = g(w).requires_grad_(True)
        out = cp._CandidatesMatvec.apply(At, wt)
        (dw,) = torch.autograd.grad(out, wt, g(dout))
        assert dw.shape == wt.shape
    else:
        out, dw = nans((B, M), torch.float32), nans((K,), torch.float32)
        lib.check(L.rdm_candidates_matvec_f32(lib.ptr(At), lib.ptr(g(w)), lib.ptr(out), B, K, M, lib.stream()))
        lib.check(L.rdm_candidates_matvec_bwd(lib.ptr(At), lib.ptr(g(dout)), lib.ptr(dw), B, K, M, lib.stream()))
    close(c(out), want, 0.0, s_abs, K * E23, "candidates_matvec out")          # K float32 fmas, each within 2^-24 S_abs (observed 0.33 of it)
    dw_close(c(dw).reshape(-1), wdw, sw, "candidates_matvec dw")


def test_nine_candidates_take_the_matmul_branch(env):
    """make_pred hands more than 8 candidates to torch.matmul: no library launch, and the same reference"""
    B, K, M = 3, 9, 16
    A, w, dout, (want, s_abs), (wdw, sw) = mv_ref(B, K, M)
    wt = g(w).requires_grad_(True)
    before = env["L"].rdm_launch_count()
    (out,) = env["cp"].make_pred([wt], [g(A)], True, False)
    assert env["L"].rdm_launch_count() == before and out.shape == (B, 1, 4, 4) and out.dtype == torch.float32
    close(c(out).reshape(B, M), want, 0.0, s_abs, K * E23, "matmul out")
    (dw,) = torch.autograd.grad(out, wt, g(dout).view(B, 1, 4, 4))
    # torch's float32 matmul backward: B*M float32 products summed in float32, each addition within 2^-24 of a partial sum <= S_abs
    close(c(dw).reshape(-1), wdw, 0.0, sw, (B * M + 1) * E24, "matmul dw")


RC_SHAPES = [(1, 0, 0), (4, 3, 0), (4, 7, 0), (5, 7, 1), (8, 7, 0), (8, 7, 1), (2, 9, 0)]      # (n_levels, n_out, first_level)


@functools.lru_cache(maxsize=None)
def rc_ref(n_levels, n_out, first, B):
    per, S = hr.level_off(n_levels), 1 << n_out
    yhat = U(f"hg.rc.y.{n_levels}.{B}", (B, per), -1, 1)
    if first:
        yhat[:, :hr.level_off(first)] = np.nan                                  # a relative pyramid has no level below the first: never read
    dout = U(f"hg.rc.d.{n_out}.{B}", (B, 1, S, S), -1, 1).astype(np.float64)
    lv = hr.split_levels(yhat, n_levels, first)
    gr, gs = hr.recombine_grad([l.shape for l in lv], dout, n_out, first)
    return yhat, dout, hr.recombine(lv, n_out, first), hr.pack_levels(gr, n_levels, first), hr.pack_levels(gs, n_levels, first)


def rc_run(env, via, yhat, dout, n_levels, n_out, first):
    L, lib, cp = env["L"], env["lib"], env["cp"]
    B, S = yhat.shape[0], 1 << n_out
    if via == "wrapper":
        yt = g(yhat).requires_grad_(True)
        out = cp._Recombine.apply(yt, n_levels, n_out, first)
        (dy,) = torch.autograd.grad(out, yt, g(dout))
    else:
        out, dy = nans((B, 1, S, S), torch.float64), nans(yhat.shape, torch.float32)
        lib.check(L.rdm_recombine_f64(lib.ptr(g(yhat)), lib.ptr(out), B, n_levels, n_out, first, lib.stream()))
        lib.check(L.rdm_recombine_bwd(lib.ptr(g(dout)), lib.ptr(dy), B, n_levels, n_out, first, lib.stream()))
    assert out.dtype == torch.float64 and dy.dtype == torch.float32 and out.shape == (B, 1, S, S)
    return c(out), c(dy)


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_levels,n_out,first", RC_SHAPES)
def test_recombine(env, n_levels, n_out, first, B, via):
    yhat, dout, (want, s_abs), wdy, sdy = rc_ref(n_levels, n_out, first, B)
    out, dy = rc_run(env, via, yhat, dout, n_levels, n_out, first)
    close(out, want, 0.0, s_abs, 1e-14, "recombine out")                        # the same float64 additions in the same order (observed: equal)
    # the float64 sum of a footprint (up to 4096 sequential additions per lane) rounded once to float32
    close(dy, wdy, E23, sdy, 1e-13, "recombine dyhat")                          # observed 0.5 of it: the rounding to float32 itself
    if first:
        lead = dy[:, :hr.level_off(first)]
        assert not np.isnan(lead).any() and not lead.any()                      # below the first level: exactly 0


@pytest.mark.parametrize("via", ["wrapper", "c_abi"])
@pytest.mark.parametrize("n_levels,n_out,first", [(4, 7, 0), (8, 7, 1)])
def test_recombine_bwd_one_hot(env, n_levels, n_out, first, via):
    """a single 1.0 in dout: every level from the first on holds exactly one 1.0, at (y >> sh, x >> sh) of the same sample, and zeros elsewhere -
    a transposed or shifted footprint has nowhere to hide"""
    B, S = 2, 1 << n_out
    yhat = np.zeros((B, hr.level_off(n_levels)), dtype=np.float32)
    for (y, x) in [(0, 0), (S - 1, S - 1), (S - 1, 0), (5, S - 2)]:
        dout = np.zeros((B, 1, S, S))
        dout[1, 0, y, x] = 1.0
        _, dy = rc_run(env, via, yhat, dout, n_levels, n_out, first)
        want = np.zeros_like(dy)
        for k in range(first, n_levels):
            sh = n_out - k
            want[1, hr.level_off(k) + (y >> sh) * (1 << k) + (x >> sh)] = 1.0
        np.testing.assert_array_equal(dy, want)


# ------------------------------------------------------------------------------------------
# routing: the packed-pyramid registry of network/computations.py
# ------------------------------------------------------------------------------------------
ROUTES = [(8, 3), (128, 7)]                                                       # (side of the map, n): 4 and 8 scalar weights


class Route:
    """decompose -> relative_fine_detail_matrix -> make_pred -> recombination(., 7) -> backward, with the library launches of the forward counted"""

    def __init__(self, env, S, n):
        self.env, self.S, self.n, self.B = env, S, n, 3
        self.src = g(LU(f"hg.route.{S}", (self.B, 1, S, S), 0.5, 2.0).astype(np.float64))
        self.w = [torch.nn.Parameter(g(U(f"hg.route.w{i}", (1, 1), 0.5, 1.5))) for i in range(n + 1)]
        self.dout = U("hg.route.dout", (self.B, 1, 128, 128), -1, 1).astype(np.float64)

    def rows(self, relative_map=False):
        return self.env["cp"].decompose_depth_map([], self.src, self.n, relative_map)[::-1]

    def run(self, rows, weights=None, relative_only=False):
        cp, L = self.env["cp"], self.env["L"]
        before = L.rdm_launch_count()
        yh = cp.make_pred(list(self.w if weights is None else weights), cp.relative_fine_detail_matrix([rows], True), True, relative_only)
        final = cp.recombination(list(yh), 7)
        launches = L.rdm_launch_count() - before
        return [c(t) for t in yh], final, launches

    def check(self, rows_np, yh, final, first=0, launches=None, want_launches=None):
        """against head_ref on the data the rows hold"""
        n_levels = self.n + 1
        w = [float(p.detach().cpu()) for p in self.w]
        want = hr.fine_detail_pred(rows_np, w[first:])
        assert len(yh) == len(want)
        for a, b in zip(yh, want):
            assert a.dtype == np.float32 and a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-8)
        wfin, s_abs = hr.recombine(yh, 7, first)                                   # of the float32 predictions the kernel was handed
        close(c(final), wfin, 0.0, s_abs, 1e-14, "route final")
        grads = torch.autograd.grad(final, self.w[first:], g(self.dout))
        dy32 = [hr.block_sums(self.dout, k).astype(np.float32) for k in range(first, n_levels)]      # the node boundary is float32
        wdw, sw = hr.fine_detail_pred_grad(rows_np, dy32)
        dw = np.array([float(x.cpu()) for x in grads])
        dw_close(dw, wdw, sw, "route dw")
        if want_launches is not None:
            assert launches == want_launches, (launches, want_launches)
        return dw, sw


@pytest.fixture(scope="module", params=ROUTES, ids=lambda p: f"{p[0]}x{p[0]}")
def route(request, env):
    return Route(env, *request.param)


def test_route_fused_and_general_agree(route):
    cp = route.env["cp"]
    rows = route.rows()
    data = [c(r) for r in rows]
    assert cp._pyramid_of(rows) is not None
    yh_f, fin_f, n_f = route.run(rows)
    dw_f, sw = route.check(data, yh_f, fin_f, launches=n_f, want_launches=2)               # one fused log * w launch, one recombine launch
    clones = [r.clone() for r in rows]
    assert cp._pyramid_of(clones) is None
    yh_g, fin_g, n_g = route.run(clones)
    dw_g, _ = route.check(data, yh_g, fin_g, launches=n_g, want_launches=route.n + 1)      # one mat-vec launch per level, torch ops after
    for a, b in zip(yh_f, yh_g):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(c(fin_f), c(fin_g), rtol=0, atol=1e-14 * float(np.abs(hr.recombine(yh_f, 7)[1]).max()))
    dw_close(dw_f, dw_g, sw, "fused dw against general dw")


def test_route_in_place_write_falls_back(route):
    cp = route.env["cp"]
    rows = route.rows()
    rows[0].mul_(2.0)
    assert cp._pyramid_of(rows) is None                                           # the packed buffer's version moved on
    yh, fin, n = route.run(rows)
    route.check([c(r) for r in rows], yh, fin, launches=n, want_launches=route.n + 1)


def test_route_evicted_entry_still_computes_right(route):
    cp = route.env["cp"]
    rows = route.rows()
    data = [c(r) for r in rows]
    later = [route.rows() for _ in range(9)]                                      # more pyramids than the registry keeps
    assert cp._pyramid_of(rows) is None and cp._pyramid_of(later[-1]) is not None
    yh, fin, n = route.run(rows)
    route.check(data, yh, fin, launches=n, want_launches=route.n + 1)


def test_route_reassembled_and_detached_lists_stay_fused(route):
    rows = route.rows()
    data = [c(r) for r in rows]
    for again in (list(rows), [r.detach() for r in rows], rows[:]):
        yh, fin, n = route.run(again)
        route.check(data, yh, fin, launches=n, want_launches=2)


def test_route_single_row_outside_the_fused_branch_sees_logs(route):
    """a single row that came from decompose_depth_map reaches make_pred as views of the RAW levels (the log is taken by the fused launch); when
    the fused launch is not taken - a relative row with relative_only=True, or a level with more than one weight - the general branch must
    still work on the logs, as the reference's make_matrix hands them over: float32(log L) * w, not L * w."""
    cp = route.env["cp"]
    rel = route.rows(relative_map=True)
    assert len(rel) == route.n and rel[0].shape[2] == 2
    data = [c(r) for r in rel]
    yh, fin, n = route.run(rel, relative_only=True)
    route.check(data, yh, fin, first=1, launches=n, want_launches=route.n)
    # a full row kept out of the fused branch by one weight of two elements (a shape the reference's matmul refuses for one candidate, so
    # that level is not compared): every level with a scalar weight must come out as float32(log L) * w
    rows = route.rows()
    data = [c(r) for r in rows]
    odd = 2
    weights = [p.detach() for p in route.w]
    weights[odd] = torch.cat([weights[odd], weights[odd]])
    with torch.no_grad():
        yh = cp.make_pred(weights, cp.relative_fine_detail_matrix([rows], True), True, False)
    want = hr.fine_detail_pred(data, [float(p.detach().cpu()) for p in route.w])
    for k, (a, b) in enumerate(zip(yh, want)):
        if k != odd:
            np.testing.assert_allclose(c(a), b, rtol=1e-6, atol=1e-8)
