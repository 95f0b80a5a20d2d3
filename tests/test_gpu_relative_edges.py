"""-m gpu: the relative-decoder kernels of csrc/als.hip (dense and paged ratio grids, Lloyd quantisation, rank-1 ALS with its record /
select / finish / replay passes, page split / reconstruct) and the two pyramid kernels of csrc/postproc.hip their tail uses
(k_gm_normalize, k_decompose), against oracle/computations_cpu.py at the edges the one-shape-per-golden tests leave out.  The inputs are
built by tests/als_ref.py; tests/test_als_ref_cpu.py shows, on the oracle alone, that each has the arg-min, the margin (>= 1e-4 between the
best and the runner-up rmse) and the threshold hits this file relies on.

Every kernel is reached through its network/computations.py wrapper; the C ABI is used in addition where a test needs what the wrapper hides:
the ALS workspace (the k* the select kernel chose), both outputs of rdm_gm_normalize_f64 at once, and NaN-filled output buffers (every
buffer handed to the C ABI here is NaN-filled first, so an element no thread wrote shows).  No wrapper refused a shape.

Tolerances.  Levels, raw grids, pages and k* are bit-exact.  ALS outputs with k* <= 7 use the project's rtol 3e-5 (tests/test_gpu_ops.py:
the float32 geometric mean with its 256 pow roundings).  For a late arg-min the float32 oracle's own distance from the float64 recurrence
(als_ref.als_f64) at the same k* was measured on the CPU - 7.8e-7 after 8 iterations, 2.2e-6 after 30 (late_grid), 7.0e-6 after 100
(late_page) - and the GPU is allowed max(3e-5, 4 x that distance) from the oracle (als_ref.late_rtol), which is 3e-5 in every case here.

Mutations of als.hip, each of which makes the named test fail:
  * the replay ignoring kstar[group] (running to `limit`, or to another group's k*): test_replay_pass_serves_the_late_pages_of_a_mixed_call
    (pages 1 and 2 would be overwritten with iterate 100 instead of iterate 1; with limit = k* everywhere, as in
    test_replay_pass_every_instantiation, the two coincide, which is why the mixed call exists);
  * `>=` turned into `>` in lloyd_index_f64 (or in k_ratio_dense): test_thresholds_paged_and_fused, test_thresholds_dense;
  * `group * batch + b` swapped for `b * groups + group`: test_indexing (every B > 1 with more than one page), test_replay_pass_serves_...;
  * the window clamp at 5 changed to 6: test_indexing (all sides), test_indexing_marked_page_edges;
  * a dropped grid-stride step (`for` turned into `if`): test_grid_stride_* (the NaN-filled tail is never written);
  * als_keep off by one: test_keep_boundary (the workspace layout the test derives from keep = min(limit, 7) no longer matches
    rdm_als_workspace_bytes; with the replay gate `limit > keep` moved instead, limit 8 loses its replay launch and returns the NaN fill).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import als_ref as A
from md_rdm_amd import _lib
from oracle import computations_cpu as ocp

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from md_rdm_amd.network import RDM_Net, computations as cp
    return dict(cp=cp, quant=RDM_Net.Quantization(), dev=torch.device("cuda:0"))


def g(a, env):
    return torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def nans(env, shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=env["dev"])


def dev_tables(env, table):
    q, inv = A.tables()[table]
    if table == "008":
        return env["quant"].device_tables(3, env["dev"])
    qd, invd = env["quant"].device_tables({"016": 4, "032": 5, "064": 6, "128": 7}[table], env["dev"])
    np.testing.assert_array_equal(qd.cpu().numpy(), q)                         # the library's tables are the oracle's
    np.testing.assert_array_equal(invd.cpu().numpy(), inv)
    return qd, invd


# ----------------------------------------------------------------------------------------------------------------------------------------
# C ABI with NaN-filled outputs and a readable workspace
# ----------------------------------------------------------------------------------------------------------------------------------------
def _workspace(env, groups, batch, rows, limit):
    """The workspace of rdm_als_rank1 / rdm_als_rank1_paged: [iterates 0..keep | squared errors | k* per group | rmse record], each part
    rounded up to 256 bytes, keep = min(limit, 7).  Filled with 0xFF bytes (NaN as float, -1 as int).  Returns (buffer, bytes, k* offset,
    rmse offset)."""
    up = lambda n: (n + 255) & ~255
    keep = min(limit, 7)
    hist, sse, ks, rm = up(groups * batch * (keep + 1) * rows * 4), up(groups * (limit + 1) * batch * 8), up(groups * 4), up(groups * (limit + 1) * 4)
    nbytes = int(_lib.lib().rdm_als_workspace_bytes(groups, batch, rows, 64, limit))
    assert nbytes == hist + sse + ks + rm, "the ALS workspace layout changed: keep = min(limit, 7) iterates + 1 are recorded"
    ws = torch.full((nbytes,), 255, dtype=torch.uint8, device=env["dev"])
    assert ws.data_ptr() % 256 == 0
    return ws, nbytes, hist + sse, hist + sse + ks


def _read_ws(ws, off_k, off_r, groups, limit):
    kstar = ws[off_k:off_k + 4 * groups].view(torch.int32).cpu().numpy()
    rmse = ws[off_r:off_r + 4 * groups * (limit + 1)].view(torch.float32).cpu().numpy().reshape(groups, limit + 1)
    return kstar, rmse


def abi_als(env, R, groups, batch, rows, limit):
    """rdm_als_rank1 -> (p (groups, batch, rows), k* per group, rmse record per group)"""
    R = R.contiguous()
    ws, nbytes, off_k, off_r = _workspace(env, groups, batch, rows, limit)
    p = nans(env, (groups, batch, rows), torch.float32)
    _lib.check(_lib.lib().rdm_als_rank1(_lib.ptr(R), int(R.dtype == torch.float64), _lib.ptr(p), groups, batch, rows, 64, limit, C.c_void_p(ws.data_ptr()), nbytes,
                                        _lib.stream()))
    return (p,) + _read_ws(ws, off_k, off_r, groups, limit)


def abi_als_paged(env, dn, dn1, qd, invd, limit):
    """rdm_als_rank1_paged -> (p (P, B, 256), k* per page, rmse record per page)"""
    B, _, S, _ = dn.shape
    P = (S // 16) ** 2
    ws, nbytes, off_k, off_r = _workspace(env, P, B, 256, limit)
    p = nans(env, (P, B, 256), torch.float32)
    _lib.check(_lib.lib().rdm_als_rank1_paged(_lib.ptr(dn.contiguous()), _lib.ptr(dn1.contiguous()), _lib.ptr(p), B, S, _lib.ptr(qd), _lib.ptr(invd), limit,
                                              C.c_void_p(ws.data_ptr()), nbytes, _lib.stream()))
    return (p,) + _read_ws(ws, off_k, off_r, P, limit)


def abi_grid(env, dn, dn1, qd, invd, quantize):
    B, _, S, _ = dn.shape
    R = nans(env, ((S // 16) ** 2, B, 256, 64), torch.float64)
    _lib.check(_lib.lib().rdm_ratio_grid_lloyd_paged(_lib.ptr(dn.contiguous()), _lib.ptr(dn1.contiguous()), _lib.ptr(R), B, S, _lib.ptr(qd), _lib.ptr(invd),
                                                     int(quantize), _lib.stream()))
    return R


def check_paged(env, dn, dn1, table, limit, res, pages=None, late=()):
    """One map through every paged path against the per-page oracle ``res``: the raw and the quantised grid bit for bit (wrapper and C ABI),
    the fused and the unfused ALS against the oracle's ALS on the oracle's grid, their k* against the oracle's, and fused == unfused bit
    for bit.  ``late`` pages take als_ref.late_rtol, the others 3e-5."""
    cp = env["cp"]
    qd, invd = dev_tables(env, table)
    d, d1 = g(dn, env), g(dn1, env)
    raw = cp.ratio_grid_lloyd_paged(d, d1, qd, invd, quantize=False)
    Rq = cp.ratio_grid_lloyd_paged(d, d1, qd, invd)
    raw_abi, Rq_abi = abi_grid(env, d, d1, qd, invd, 0), abi_grid(env, d, d1, qd, invd, 1)
    P, B = Rq.shape[0], dn.shape[0]
    assert Rq.shape == raw.shape == (P, B, 256, 64) and Rq.dtype == torch.float64
    fused = cp.als_pages_fused(d, d1, qd, invd, limit=limit).view(P, B, 256)
    unfused = cp.als_pages(Rq, limit=limit).view(P, B, 256)
    f_abi, f_k, _ = abi_als_paged(env, d, d1, qd, invd, limit)
    u_abi, u_k, _ = abi_als(env, Rq_abi, P, B, 256, limit)
    raw, Rq, raw_abi, Rq_abi = raw.cpu().numpy(), Rq.cpu().numpy(), raw_abi.cpu().numpy(), Rq_abi.cpu().numpy()
    fused, unfused, f_abi, u_abi = fused.cpu().numpy(), unfused.cpu().numpy(), f_abi.cpu().numpy(), u_abi.cpu().numpy()
    for p in (range(P) if pages is None else pages):
        o = res[p]
        for got in (raw[p], raw_abi[p]):
            np.testing.assert_array_equal(got, o["raw"], err_msg=f"raw grid, page {p}")          # NaN == NaN, inf == inf here
        for got in (Rq[p], Rq_abi[p]):
            np.testing.assert_array_equal(got, o["R"], err_msg=f"quantised grid, page {p}")
        assert f_k[p] == u_k[p] == o["kstar"], (p, f_k[p], u_k[p], o["kstar"])
        rtol = A.late_rtol(o["R"], limit) if p in late else A.ALS_RTOL
        for got in (fused[p], unfused[p], f_abi[p], u_abi[p]):
            np.testing.assert_allclose(got, o["out"], rtol=rtol, equal_nan=True, err_msg=f"ALS, page {p}, k* {o['kstar']}")
    np.testing.assert_array_equal(fused, unfused)                                                 # bit-identical, every page (both pinned above
    np.testing.assert_array_equal(f_abi, fused)                                                   # by the oracle on the pages compared)
    np.testing.assert_array_equal(u_abi, unfused)
    assert not np.isnan(Rq_abi).any() and not np.isnan(f_abi).any() and not np.isnan(u_abi).any()    # no element of the NaN fill is left


# ----------------------------------------------------------------------------------------------------------------------------------------
# 1. the replay pass, every instantiation
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dt,limit", A.REPLAY_CASES)
def test_replay_pass_every_instantiation(env, rows, dt, limit):
    """k_als<256, 0, true>, <256, 1, true>, <64, 1, true> and <64, 0, true> (the fused <256, 2, true> is the next test): late_grid, B = 3, the
    oracle's arg-min is the last iterate (k* = limit > 7), so the output is written by the replay pass - the walk to kstar[group], the
    Q = 4 shuffle of the q-update at 256 rows, the in-kernel geometric mean and the store."""
    cp = env["cp"]
    R = A.replay_grid(rows)
    want, _, kstar, _ = A.oracle_als(R, limit)
    assert kstar == limit > 7
    Rd = g(R.astype(np.float64) if dt == "f64" else R, env)                                       # the same values either way: float32 numbers
    got = cp.alternating_least_squares(Rd, n=4, cuda=True, limit=limit) if rows == 256 else cp.quadratic_als(Rd, cuda=True, n=3, limit=limit)
    p, k, rmse = abi_als(env, Rd, 1, 3, rows, limit)
    assert k[0] == kstar, (k[0], kstar)
    rtol = A.late_rtol(R, limit)          # max(3e-5, 4 x d), d = oracle vs float64 at k*: 7.8e-7 (limit 8), 2.2e-6 (256x64, limit 30), 1.4e-6 (64x64)
    np.testing.assert_allclose(got.cpu().numpy().reshape(3, rows), want, rtol=rtol)
    np.testing.assert_allclose(p.cpu().numpy()[0], want, rtol=rtol)
    assert np.isfinite(rmse).all()


@pytest.mark.parametrize("limit", A.MIXED_LIMITS)
def test_replay_pass_serves_the_late_pages_of_a_mixed_call(env, limit):
    """k_als<256, 2, true> (fused) and <256, 1, true> (unfused) in ONE call whose pages disagree: pages 0 and 3 are late_page under
    dn_1 == 1 (k* = limit, served by the replay), pages 1 and 2 are log-uniform (k* = 1, served by the finish kernel from the recorded
    iterates, and left alone by the replay).  k* is read back from the workspace and equals the oracle's page by page."""
    dn, dn1, res = A.mixed_case(limit)
    assert [res[p]["kstar"] for p in range(4)] == [limit, 1, 1, limit]
    # oracle vs float64 at k*: 7.4e-7 / 8.8e-7 (limit 8), 4.6e-6 / 7.0e-6 (limit 100) on pages 0 / 3
    check_paged(env, dn, dn1, "032", limit, res, late=(0, 3))


# ----------------------------------------------------------------------------------------------------------------------------------------
# 2. the keep boundary
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("limit", A.KEEP_LIMITS)
def test_keep_boundary(env, limit):
    """limit 0, 1, 7: keep == limit, no replay launch, the finish kernel serves every k*; limit 8: the first value with a replay launch,
    which the log-uniform grid (k* = 1) must pass through untouched and the late grid (k* = 8) needs."""
    cp = env["cp"]
    for R in A.keep_grids():
        want, _, kstar, _ = A.oracle_als(R, limit)
        got = cp.alternating_least_squares(g(R, env), n=4, cuda=True, limit=limit)
        p, k, _ = abi_als(env, g(R, env), 1, 2, 256, limit)
        assert k[0] == kstar, (k[0], kstar)
        rtol = A.late_rtol(R, limit) if kstar > 7 else A.ALS_RTOL                                # late grid at limit 8: oracle vs float64 8.2e-7
        np.testing.assert_allclose(got.cpu().numpy().reshape(2, 256), want, rtol=rtol)
        np.testing.assert_allclose(p.cpu().numpy()[0], want, rtol=rtol)
        if limit == 0:                                                                            # the normalised all-ones start, exactly
            np.testing.assert_array_equal(want, 1.0)
            np.testing.assert_array_equal(p.cpu().numpy(), 1.0)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 3. thresholds
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["016", "032", "064", "128"])
def test_thresholds_paged_and_fused(env, table):
    """float64 products dn * (1 / area) that land exactly ON a threshold and one ulp below it, in each of the nine window slots, and
    float32 neighbours of every threshold in the base slots: k_ratio_paged (raw and quantised, bit-exact) and the fused row builder of
    k_als<256, 2, .> (its ALS against the oracle's ALS on the oracle's grid, and bit-identical with the unfused path)."""
    dn, dn1, plan, res = A.threshold_case(table)
    check_paged(env, dn, dn1, table, A.LIMIT, res)
    # the planted probes themselves, named: level inv[bin] at [page, sample, fine pixel, coarse slot]
    qd, invd = dev_tables(env, table)
    R = env["cp"].ratio_grid_lloyd_paged(g(dn, env), g(dn1, env), qd, invd).cpu().numpy()
    inv = A.tables()[table][1]
    for page, b, pix, slot, bin_ in plan:
        if slot is not None:
            np.testing.assert_array_equal(R[page, b, pix, slot], inv[bin_])


def test_thresholds_dense(env):
    """k_ratio_dense compares in float32 against thresholds rounded to float32: d_i * (1 / 1) equal to float32(q[k]) (bin k + 1) and to the
    float32 number below it (bin k), for all 40 thresholds of the derived 008 table, in a 81 x 81 grid."""
    d, rows = A.dense_threshold_depths()
    q, inv = A.tables()["008"]
    qd, invd = dev_tables(env, "008")
    want = ocp.lloyd_quantization(ocp.sparse_comparison_v1_raw(d), q, inv)[0]
    got = env["cp"].ratio_grid_lloyd_dense(g(d, env), qd, invd)
    assert got.dtype == torch.float32 and want.dtype == np.float32
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    for i, bin_ in rows:
        assert got[0, i, 0].item() == np.float32(inv[bin_])


# ----------------------------------------------------------------------------------------------------------------------------------------
# 4. indexing
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,B", A.INDEX_CASES)
def test_indexing(env, side, B):
    """mat = group * batch + b, pi = p / ratio and the window origin clamp(r / 2, 0, 5) at sides 16, 48 (9 pages, ratio 3) and 80 (25 pages)
    with batch 1, 3 and 5, through the fused and the unfused path; dn_1 is the library's own resize, itself bit-exact."""
    dn, dn1, res = A.index_case(side, B)
    got1 = env["cp"].resize(g(dn, env), side // 2)
    np.testing.assert_array_equal(got1.cpu().numpy(), dn1)
    check_paged(env, dn, dn1, A.INDEX_TABLE[side], A.LIMIT, res)


def test_indexing_marked_page_edges(env):
    """a coarse map whose page corners and page edge rows / columns hold values of their own: a window origin off by one at a page edge
    reads a value that no correct window of that pixel holds"""
    side, B = A.MARKED_CASE
    dn, dn1, res = A.index_case(side, B, True)
    check_paged(env, dn, dn1, A.INDEX_TABLE[side], A.LIMIT, res)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 5. non-finite inputs
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_inputs_match_the_oracle(env):
    """a coarse pixel equal to 0.0 (infinite ratio: bin 40) and a NaN dn pixel (NaN compares false: bin 0) in page 1 of a 4-page call:
    raw grids (with their inf and NaN) and levels bit-exact, ALS of the page that holds them and of its clean neighbours against the
    oracle, k* taken from the oracle"""
    dn, dn1, res = A.nonfinite_case()
    assert np.isinf(res[1]["raw"]).any() and np.isnan(res[1]["raw"]).any()
    check_paged(env, dn, dn1, "032", A.LIMIT, res)


# ----------------------------------------------------------------------------------------------------------------------------------------
# 6. grid-stride second passes
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_grid_stride_paged_grid(env):
    """k_ratio_paged at side 128, B = 3: 64 x 3 x 256 x 64 = 3.1 M elements on 8192 x 256 threads, so every thread takes a second step.
    The first page, an interior page and the last page against the oracle (its Python loop is slow), raw and quantised."""
    dn = A.log_uniform(31, (3, 1, 128, 128), 0.5, 2.0).astype(np.float32)
    dn1 = ocp.resize(dn, 64)
    pages = (0, 27, 63)
    res = A.paged_oracle(dn, dn1, "128", None, pages=pages)
    qd, invd = dev_tables(env, "128")
    d, d1 = g(dn, env), g(dn1, env)
    assert 64 * 3 * 256 * 64 > 8192 * 256
    for quantize, key in ((0, "raw"), (1, "R")):
        for R in (abi_grid(env, d, d1, qd, invd, quantize), env["cp"].ratio_grid_lloyd_paged(d, d1, qd, invd, quantize=bool(quantize))):
            assert not torch.isnan(R).any()                                                       # every element written
            for p in pages:
                np.testing.assert_array_equal(R[p].cpu().numpy(), res[p][key])


@pytest.mark.parametrize("B,h,w", [(257, 8, 8), (1, 1, 1), (1, 1, 7)])
def test_grid_stride_dense_grid(env, B, h, w):
    """k_ratio_dense at n = 64, B = 257 (1 052 672 elements on 4096 x 256 threads: a second step for the first 4096 of them), and at the
    smallest grids, n = 1 and n = 7, where most of the one workgroup is idle"""
    n = h * w
    d = A.log_uniform(41 + n, (B, 1, h, w), 0.5, 2.0).astype(np.float32)
    q, inv = A.tables()["008"]
    qd, invd = dev_tables(env, "008")
    want = ocp.lloyd_quantization(ocp.sparse_comparison_v1_raw(d), q, inv)[0]
    dd = g(d, env)
    got = env["cp"].ratio_grid_lloyd_dense(dd, qd, invd)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    R = nans(env, (B, n, n), torch.float32)
    _lib.check(_lib.lib().rdm_ratio_grid_lloyd_dense(_lib.ptr(dd), _lib.ptr(R), B, n, _lib.ptr(qd), _lib.ptr(invd), _lib.stream()))
    np.testing.assert_array_equal(R.cpu().numpy(), want)
    if B == 257:
        assert B * n * n > 4096 * 256


@pytest.mark.parametrize("side,B", [(512, 5), (16, 2), (48, 2)])
def test_grid_stride_page_split_and_reconstruct(env, side, B):
    """k_page_split / k_page_reconstruct at side 512, B = 5 (1.3 M elements on 4096 x 256 threads), and at ratio 1 and ratio 3, against
    ocp.split_matrix / ocp.reconstruct (which keeps the reference's column-block reuse: only pages 0 .. ratio - 1 are read)."""
    cp = env["cp"]
    ratio = side // 16
    dn = A.uniform(51 + side, (B, 1, side, side), 0.0, 1.0).astype(np.float32)
    dn1 = A.uniform(52 + side, (B, 1, side // 2, side // 2), 0.0, 1.0).astype(np.float32)
    wa, wb = ocp.split_matrix(dn, dn1)
    dnd = g(dn, env)
    ga, gb = cp.split_matrix(dnd, g(dn1, env))
    assert len(ga) == len(gb) == ratio * ratio
    np.testing.assert_array_equal(torch.stack(ga).cpu().numpy(), np.stack(wa))
    np.testing.assert_array_equal(torch.stack(gb).cpu().numpy(), np.stack(wb))
    pages = nans(env, (ratio * ratio, B, 1, 16, 16), torch.float32)
    _lib.check(_lib.lib().rdm_page_split_f32(_lib.ptr(dnd),_lib.ptr(pages), B, side, 16, _lib.stream()))
    np.testing.assert_array_equal(pages.cpu().numpy(), np.stack(wa))
    want = ocp.reconstruct(wa)
    assert want.shape == (B, 1, side, side)
    np.testing.assert_array_equal(cp.reconstruct(ga).cpu().numpy(), want)
    out = nans(env, (B, 1, side, side), torch.float32)
    _lib.check(_lib.lib().rdm_page_reconstruct_f32(_lib.ptr(pages), _lib.ptr(out), B, side, 16, _lib.stream()))
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    if side == 512:
        assert B * side * side > 4096 * 256


# ----------------------------------------------------------------------------------------------------------------------------------------
# 7. rdm_gm_normalize_f64 and rdm_decompose_f64
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 16384])
def test_gm_normalize_shapes_and_outputs(env, n, B):
    """k_gm_normalize with fewer samples than threads, one short of / exactly / one past the workgroup, and 64 strides; dst only and gm_out
    only through the wrappers, both at once through the C ABI.  Reference exp(e * fsum(log x)) in float64, 1e-13 relative as the existing
    wrapper test (the float64 log sum of <= 16384 terms of magnitude <= 2.2 carries ~1e-12 absolute error before the factor e = 1 / n)."""
    cp = env["cp"]
    x = A.log_uniform(61 + n + B, (B, n), 0.5, 9.0)
    rc = math.sqrt(n)
    e = 1.0 / (rc * rc)                                                                           # the exponent quick_gm forms from rc
    gm, y = A.gm_reference(x, e)
    xd = g(x, env)
    np.testing.assert_allclose(cp.gm_normalize(xd.view(B, 1, 1, n), e).cpu().numpy().reshape(B, n), y, rtol=1e-13)       # dst only
    got = cp.quick_gm(xd.view(B, n, 1), rc)                                                                                  # gm_out only
    assert got.dtype == torch.float64 and got.shape == (B, 1)
    np.testing.assert_allclose(got.cpu().numpy().reshape(B), gm, rtol=1e-13)
    dst, out = nans(env, (B, n), torch.float64), nans(env, (B,), torch.float64)                                              # both
    _lib.check(_lib.lib().rdm_gm_normalize_f64(_lib.ptr(xd), _lib.ptr(dst), _lib.ptr(out), B, n, e, _lib.stream()))
    np.testing.assert_allclose(dst.cpu().numpy(), y, rtol=1e-13)
    np.testing.assert_allclose(out.cpu().numpy(), gm, rtol=1e-13)
    dst2, out2 = nans(env, (B, n), torch.float64), nans(env, (B,), torch.float64)                                            # each alone, NaN-filled
    _lib.check(_lib.lib().rdm_gm_normalize_f64(_lib.ptr(xd), _lib.ptr(dst2), None, B, n, e, _lib.stream()))
    _lib.check(_lib.lib().rdm_gm_normalize_f64(_lib.ptr(xd), None, _lib.ptr(out2), B, n, e, _lib.stream()))
    np.testing.assert_allclose(dst2.cpu().numpy(), y, rtol=1e-13)
    np.testing.assert_allclose(out2.cpu().numpy(), gm, rtol=1e-13)


@pytest.mark.parametrize("B", [1, 16])
@pytest.mark.parametrize("depth", [0, 1, 2, 5, 6])
def test_decompose_depths(env, depth, B):
    """k_decompose at the pyramid depths the goldens leave out, bit-exact against ocp.decompose_depth_map (exact resize, IEEE division),
    into a NaN-filled packed buffer [d_0 | F_1 (2x2) | ... | F_n] so that an unwritten slot shows."""
    cp = env["cp"]
    S = 1 << depth
    src = A.log_uniform(71 + depth + B, (B, 1, S, S), 0.5, 9.5)
    want = ocp.decompose_depth_map(src, depth)[::-1]                                              # [d_0, F_1, ..., F_n]
    assert [w.shape[2] for w in want] == [1 << k for k in range(depth + 1)]
    srcd = g(src, env)
    got = cp.decompose_depth_map([], srcd, depth)[::-1]
    assert len(got) == depth + 1
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    off = lambda k: ((1 << (2 * k)) - 1) // 3
    levels = nans(env, (B, off(depth + 1)), torch.float64)
    _lib.check(_lib.lib().rdm_decompose_f64(_lib.ptr(srcd),_lib.ptr(levels), B, depth, _lib.stream()))
    levels = levels.cpu().numpy()
    for k, w in enumerate(want):
        np.testing.assert_array_equal(levels[:, off(k):off(k + 1)], np.asarray(w).reshape(B, -1))
    if depth >= 1:
        rel = cp.decompose_depth_map([], srcd, depth, relative_map=True)[::-1]          # the relative decoders' form: no d_0
        assert len(rel) == depth
        for a, b in zip(rel, want[1:]):
            np.testing.assert_array_equal(a.cpu().numpy(), b)
