"""tests/als_ref.py without a GPU: every property of its inputs that tests/test_gpu_relative_edges.py relies on, shown on the oracle alone.
  (a) ``als_f64`` is the oracle's recurrence (it meets the float32 oracle to float32 accuracy at every k), and the oracle's own distance
      from it after 8 .. 100 float32 iterations - the figure the late-arg-min tolerances are derived from - is printed;
  (b) every input that runs ALS has the k* the GPU test expects and a margin of at least 1e-4 between the best and the runner-up rmse;
  (c) ``threshold_window`` covers at least 30 of the 40 thresholds of every table both ways, reaches bins 0 and 40, no threshold is a
      float32 number, and the oracle quantises every planted probe of ``threshold_map`` / ``dense_threshold_depths`` into its bin.
Run with -s to see the margins, distances and coverage."""
import math

import numpy as np
import pytest

import als_ref as A
from oracle import computations_cpu as ocp

TABLES = ("016", "032", "064", "128")


def test_als_f64_is_the_oracles_recurrence():
    for rows, seed in ((256, 3), (64, 4)):
        R = A.log_uniform(seed, (2, rows, 64), 0.5, 2.0).astype(np.float32)
        np.testing.assert_array_equal(A.als_f64(R, 5, 0), 1.0)                     # the normalised all-ones start
        out, _, k, _ = A.oracle_als(R, 30)
        assert k == 1
        np.testing.assert_allclose(out, A.als_f64(R, 30, k), rtol=2e-6)
    for rows in (256, 64):                                                          # and deep into the iteration, on the late grids
        R = A.replay_grid(rows)
        out, _, k, _ = A.oracle_als(R, 30)
        assert k == 30
        np.testing.assert_allclose(out, A.als_f64(R, 30, 30), rtol=2e-5)
        assert not np.allclose(out, A.als_f64(R, 30, 29), rtol=2e-5)                # one iteration less is another vector: k matters


@pytest.mark.parametrize("rows,dt,limit", A.REPLAY_CASES)
def test_late_grid_argmin_is_the_last_iterate(rows, dt, limit):
    R = A.replay_grid(rows)
    assert R.dtype == np.float32 and R.shape == (3, rows, 64)
    _, rec, k, m = A.oracle_als(R, limit)
    dist = A.oracle_distance(R, limit)
    print(f"late_grid {rows}x64 limit {limit}: k* = {k}, margin {m:.2e}, oracle-vs-float64 distance {dist:.2e}, rtol {A.late_rtol(R, limit):.2e}")
    assert k == limit > 7 and m >= A.MARGIN
    assert dist < 1e-5                                                              # measured 7.8e-7 (limit 8) .. 2.2e-6 (limit 30)


def test_late_grid_at_64_rows_needs_limit_30():
    """the docstring's caveat: at 64x64 the grid is late only from limit 30 on, which is the one 64-row limit the GPU test uses"""
    assert A.oracle_als(A.replay_grid(64), 8)[2] == 1


@pytest.mark.parametrize("limit", A.KEEP_LIMITS)
def test_keep_boundary_inputs(limit):
    plain, late = A.keep_grids()
    _, _, k, m = A.oracle_als(plain, limit)
    _, _, kl, ml = A.oracle_als(late, limit)
    print(f"limit {limit}: log-uniform k* = {k} margin {m:.2e}; late_grid k* = {kl} margin {ml:.2e}, distance {A.oracle_distance(late, limit):.2e}")
    assert k == min(limit, 1) and m >= A.MARGIN
    assert kl == limit and ml >= A.MARGIN


@pytest.mark.parametrize("limit", A.MIXED_LIMITS)
def test_mixed_map_pages(limit):
    dn, dn1, res = A.mixed_case(limit)
    q, inv = A.tables()["032"]
    for page, levels in A.MIXED_LATE.items():
        d = res[page]
        for b, lv in enumerate(levels):                                             # the level survives float32 inside its own bin
            assert ocp.lloyd_quantization(np.float64(np.float32(inv[lv])), q, inv)[1] == lv
            np.testing.assert_array_equal(d["R"][b], inv[lv])
        dist = A.oracle_distance(d["R"], limit)
        print(f"mixed page {page} limit {limit}: k* = {d['kstar']}, margin {d['margin']:.2e}, distance {dist:.2e}")
        assert d["kstar"] == limit > 7 and d["margin"] >= A.MARGIN
        assert dist < 2e-5                                                          # measured 7e-6 at limit 100
    for page in (1, 2):
        assert res[page]["kstar"] == 1 and res[page]["margin"] >= A.MARGIN


def test_a_spread_of_levels_is_not_late():
    """why late_page uses one level per sample: two neighbouring levels, or 8 stray pixels, already give k* = 1"""
    _, inv = A.tables()["032"]
    rng = np.random.default_rng(0)
    for c in (12, 34, 37):
        lv = rng.integers(c, c + 2, (2, 256))
        assert A.oracle_als(np.repeat(inv[lv].astype(np.float32)[:, :, None], 64, axis=2), 100)[2] == 1
        lv = np.full((2, 256), c)
        lv[:, rng.integers(0, 256, 8)] = c + 1
        assert A.oracle_als(np.repeat(inv[lv].astype(np.float32)[:, :, None], 64, axis=2), 100)[2] == 1


@pytest.mark.parametrize("table", TABLES)
def test_threshold_window_coverage(table):
    q, inv = A.tables()[table]
    assert (q.astype(np.float32).astype(np.float64) == q).sum() == 0                # nothing to plant in a float32 dn directly
    on, under, both, bins = A.threshold_cover(table)
    print(f"table {table}: {len(on)} thresholds hit exactly, {len(under)} one ulp below, {len(both)} both ways")
    assert len(both) >= 30 and 0 in bins and 40 in bins
    for k, below, dn, area, bin_ in A.threshold_window(table):
        assert dn.dtype == np.float32 and area.dtype == np.float64
        val = np.float64(dn) * (1.0 / area)
        assert val == (np.nextafter(q[k], 0.0) if below else q[k])
        assert ocp.lloyd_quantization(val, q, inv)[1] == bin_ == (k if below else k + 1)


@pytest.mark.parametrize("table", TABLES)
def test_threshold_map_carries_every_probe(table):
    q, inv = A.tables()[table]
    dn, dn1, plan, res = A.threshold_case(table)
    assert dn.shape[2] % 16 == 0 and dn1.shape[2] * 2 == dn.shape[2]
    assert len(plan) == len(A.threshold_window(table)) + len(A.base_probes(table))
    window_slots = set()
    for page, b, pix, slot, bin_ in plan:
        R = res[page]["R"][b]
        for f in pix:
            rs, cs = min(f // 16 // 2, 5), min(f % 16 // 2, 5)
            win = [(rs + i) * 8 + cs + j for i in range(3) for j in range(3)]
            if slot is None:                                                        # a base probe: all 55 slots outside the window
                base = [j for j in range(64) if j not in win]
                np.testing.assert_array_equal(R[f, base], inv[bin_])
            else:
                assert slot in win
                window_slots.add(win.index(slot))
                assert R[f, slot] == inv[bin_]
    assert window_slots == set(range(9))                                            # every one of the nine window slots meets a probe
    for page, d in res.items():
        print(f"threshold map {table} page {page}: k* = {d['kstar']}, margin {d['margin']:.2e}")
        assert d["kstar"] <= 7 and d["margin"] >= A.MARGIN


def test_dense_threshold_depths():
    q, inv = A.tables()["008"]
    d, rows = A.dense_threshold_depths()
    raw = ocp.sparse_comparison_v1_raw(d)
    assert raw.dtype == np.float32 and raw.shape == (1, 81, 81)
    R, idx = ocp.lloyd_quantization(raw, q, inv)
    q32 = q.astype(np.float32)
    for i, bin_ in rows:
        k = (i - 1) // 2
        assert raw[0, i, 0] == (q32[k] if bin_ == k + 1 else np.nextafter(q32[k], np.float32(0)))
        assert idx[0, i, 0] == bin_
    assert {b for _, b in rows} == set(range(41))


@pytest.mark.parametrize("side,B,marked", [c + (False,) for c in A.INDEX_CASES] + [A.MARKED_CASE + (True,)])
def test_index_maps_have_a_clear_argmin(side, B, marked):
    dn, dn1, res = A.index_case(side, B, marked)
    assert len(res) == (side // 16) ** 2
    ks = sorted({d["kstar"] for d in res.values()})
    m = min(d["margin"] for d in res.values())
    print(f"side {side} B {B} marked {marked}: k* in {ks}, least margin {m:.2e}")
    assert max(ks) <= 7 and m >= A.MARGIN
    if marked:                                                                      # the corners of every page hold values nothing else does
        for pi in range(side // 16):
            for pj in range(side // 16):
                pg = dn1[0, 0, 8 * pi:8 * pi + 8, 8 * pj:8 * pj + 8]
                corners = [pg[0, 0], pg[0, 7], pg[7, 0], pg[7, 7]]
                assert len(set(corners)) == 4 and all((dn1[0, 0] == c).sum() == 1 for c in corners)


def test_nonfinite_map():
    dn, dn1, res = A.nonfinite_case()
    q, inv = A.tables()["032"]
    d = res[1]
    assert np.isinf(d["raw"][0]).sum() > 0 and np.isnan(d["raw"][1]).sum() == 64
    assert (d["R"][0][np.isinf(d["raw"][0])] == inv[40]).all()                      # an infinite ratio: at or above every threshold
    assert (d["R"][1][np.isnan(d["raw"][1])] == inv[0]).all()                       # NaN compares false: bin 0
    for page, r in res.items():
        print(f"non-finite map page {page}: k* = {r['kstar']}, margin {r['margin']:.2e}")
        assert np.isfinite(r["R"]).all() and np.isfinite(r["out"]).all()
        assert r["kstar"] <= 7 and r["margin"] >= A.MARGIN


def test_teeth_of_the_planted_inputs():
    """the mutations the GPU test names, applied to the ORACLE: each changes what the planted inputs give by far more than a tolerance"""
    # `>` for `>=`: every probe that sits exactly on a threshold falls one bin lower
    q, inv = A.tables()["016"]
    on = [p for p in A.threshold_window("016") if not p[1]]
    vals = np.array([np.float64(p[2]) * (1.0 / p[3]) for p in on])
    assert (np.sum(vals[:, None] > q, axis=1) == np.array([p[4] for p in on]) - 1).all()
    d, rows = A.dense_threshold_depths()
    raw = ocp.sparse_comparison_v1_raw(d)[0, :, 0]
    q8 = A.tables()["008"][0].astype(np.float32)
    assert sum(int(np.sum(raw[i] > q8)) != b for i, b in rows) == 40
    # a replay that runs pages 1 and 2 of the mixed call to `limit` instead of their k* = 1: another vector, 1e3 tolerances away
    for limit in A.MIXED_LIMITS:
        _, _, res = A.mixed_case(limit)
        for page in (1, 2):
            R = res[page]["R"]
            assert np.max(np.abs(A.als_f64(R, limit, limit) / A.als_f64(R, limit, 1) - 1.0)) > 1000 * A.ALS_RTOL
    # the iterate before k* on a late grid: outside the tolerance at every limit used, so a replay that stops one short is seen
    for rows_, _, limit in A.REPLAY_CASES:
        R = A.replay_grid(rows_)
        assert np.max(np.abs(A.als_f64(R, limit, limit - 1) / A.als_f64(R, limit, limit) - 1.0)) > 2 * A.late_rtol(R, limit)
    # the window origin clamped at 6 instead of 5, on a re-implemented window: coarse slot (jr, jc) of the 8x8 page holds a coarse depth
    # iff rs <= jr <= rs + 2 and cs <= jc <= cs + 2, so fine rows / columns 12..15 (origin 6) lose coarse row / column 5 and every
    # page of the marked map gives another raw grid, at exactly those pixels
    dn, dn1, res = A.index_case(*A.MARKED_CASE, True)
    a, b = ocp.split_matrix(dn, dn1)

    def grid(fine, coarse, clamp):
        out = np.empty((fine.shape[0], 256, 64))
        for r in range(16):
            for c in range(16):
                rs, cs = min(r // 2, clamp), min(c // 2, clamp)
                area = np.ones((fine.shape[0], 8, 8))
                area[:, rs:rs + 3, cs:cs + 3] = coarse[:, 0, rs:rs + 3, cs:cs + 3]
                out[:, r * 16 + c] = fine[:, 0, r, c].astype(np.float64)[:, None] * (1.0 / area.reshape(-1, 64))
        return out

    hit = np.array([r >= 12 or c >= 12 for r in range(16) for c in range(16)])
    for p in res:
        np.testing.assert_array_equal(grid(a[p], b[p], 5), res[p]["raw"])                   # the re-implementation is the oracle's window
        diff = (grid(a[p], b[p], 6) != res[p]["raw"]).any(axis=2)
        assert (diff == hit).all()


def test_gm_reference():
    x = A.log_uniform(5, (3, 257), 0.5, 9.0)
    gm, y = A.gm_reference(x, 1.0 / 257)
    np.testing.assert_allclose(gm, np.prod(x ** (1.0 / 257), axis=1), rtol=1e-13)
    np.testing.assert_allclose(np.exp(np.log(y).sum(axis=1) / 257), 1.0, rtol=1e-13)
    assert math.isclose(A.gm_reference(np.full((1, 1), 4.0), 0.5)[0][0], 2.0, rel_tol=1e-15)
