"""Input builders and float64 references for the edge-case tests of the relative-decoder kernels (csrc/als.hip: dense and paged ratio
grids, Lloyd quantisation, rank-1 ALS with its record / select / finish / replay passes, paging) and of the two pyramid kernels their
tail uses (csrc/postproc.hip: k_gm_normalize, k_decompose).  tests/test_als_ref_cpu.py checks every claim made here without a GPU;
tests/test_gpu_relative_edges.py runs the kernels on what is built here.

The reference of every GPU comparison is oracle/computations_cpu.py.  What this file adds is
  * inputs on which the oracle's batch-global rmse arg-min lands LATE (k* > 7, past the iterates the record pass keeps) with a margin far
    above float32 summation-order noise - ``late_grid`` and ``late_page``;
  * inputs that sit exactly ON a Lloyd threshold, or one ulp below it, AFTER the kernel's own arithmetic - ``threshold_window`` (float64
    product dn * (1 / area) of the paged grid) and ``dense_threshold_depths`` (float32 product of the dense grid);
  * ``als_f64``: the recurrence of ``ocp.als_rank1`` in float64, stopped at a given k, used ONLY to measure how far the float32 oracle
    itself has drifted after k iterations (the tolerance of the late cases is derived from that distance, never from a GPU result);
  * whole maps (``mixed_map``, ``threshold_map``, ``index_map``, ``nonfinite_map``) and ``paged_oracle``, the per-page oracle chain
    split_matrix -> ratio_grid_raw -> lloyd_quantization -> als_rank1.
The case lists at the end are shared by the CPU test (which proves the margins) and the GPU test (which relies on them).
"""
import functools
import math

import numpy as np

from oracle import computations_cpu as ocp

MARGIN = 1e-4            # least relative gap between the best and the runner-up rmse of any input whose arg-min is data-dependent
ALS_RTOL = 3e-5          # the project's ALS tolerance (tests/test_gpu_ops.py: the float32 geometric mean with its 256 pow roundings)


@functools.lru_cache(maxsize=1)
def tables():
    return ocp.load_quant_tables()


def uniform(seed, shape, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, shape)


def log_uniform(seed, shape, lo, hi):
    return np.exp(np.random.default_rng(seed).uniform(math.log(lo), math.log(hi), shape))


def argmin_margin(rec):
    """(k*, relative gap between rmse[k*] and the smallest other recorded rmse).  One record (limit 0): no choice to make, gap inf."""
    rec = np.asarray(rec, dtype=np.float64)
    k = int(np.argmin(rec))
    if len(rec) == 1:
        return k, math.inf
    rest = np.delete(rec, k).min()
    return k, (math.inf if rec[k] == 0 else (rest - rec[k]) / rec[k])


# ------------------------------------------------------------------------------------------------------------------------------------
# float64 ALS (measures the oracle's own rounding)
# ------------------------------------------------------------------------------------------------------------------------------------
def als_f64(R, limit, k):
    """p_k / gm(p_k) of ``ocp.als_rank1`` (computations.py:95-155 / :38-85) in float64: p = (R q) / (q.q + 0.05), then
    q = (R' p) / (p.p + 0.05) with R' = R.view(B, W, H) - the reference's reinterpretation of the same buffer, not a transpose - and
    the output divided by exp(sum(log p) / H^2), the reference's squared geometric-mean exponent.  Stops after the k-th p-update
    (k = 0: the all-ones start).  R: (B, H, W), returns (B, H) float64."""
    assert 0 <= k <= limit
    R = np.ascontiguousarray(R, dtype=np.float64)
    B, H, W = R.shape
    Rv = R.reshape(B, W, H)
    p, q = np.ones((B, H)), np.ones((B, W))
    for it in range(1, k + 1):
        p = np.einsum("bhw,bw->bh", R, q) / (np.sum(q * q, axis=1, keepdims=True) + 0.05)
        if it < k:
            q = np.einsum("bwh,bh->bw", Rv, p) / (np.sum(p * p, axis=1, keepdims=True) + 0.05)
    return p / np.exp(np.sum(np.log(p), axis=1, keepdims=True) / (H * H))


def oracle_als(R, limit):
    """ocp.als_rank1 on a (B, 256, 64) or (B, 64, 64) grid: (out (B, rows) float32, rmse record, k*, margin)."""
    R = np.asarray(R)
    rows = R.shape[1]
    out, rec = ocp.als_rank1(R, 4 if rows == 256 else 3, limit, q_size=64)
    k, m = argmin_margin(rec)
    return out.reshape(R.shape[0], rows), rec, k, m


def oracle_distance(R, limit):
    """max relative distance between the float32 oracle's output and ``als_f64`` at the oracle's own k*."""
    out, _, k, _ = oracle_als(R, limit)
    ref = als_f64(np.asarray(R, dtype=np.float32), limit, k)
    return float(np.max(np.abs(out.astype(np.float64) - ref) / np.abs(ref)))


def late_rtol(R, limit):
    """Tolerance of a late-arg-min comparison: max(3e-5, 4 x the oracle's own distance from float64).  The factor 4 covers a different
    float32 summation order on each side."""
    return max(ALS_RTOL, 4.0 * oracle_distance(R, limit))


# ------------------------------------------------------------------------------------------------------------------------------------
# late arg-min inputs
# ------------------------------------------------------------------------------------------------------------------------------------
def late_grid(B, rows, seed):
    """2 * (1 + 0.002 u), u uniform in [-1, 1], float32 (B, rows, 64).  A nearly constant grid: the reinterpreted q-update is then
    close to a true ALS step, the rmse keeps falling, and the oracle's arg-min is the LAST iterate - at 256x64 for limit 7, 8, 30 and
    100, at 64x64 for limit 30 and 100 (at 64x64 and limit <= 8 it is k* = 1) - leading every other record by 3e-4 to 5e-4."""
    assert rows in (64, 256)
    return (2.0 * (1.0 + 0.002 * uniform(seed, (B, rows, 64), -1.0, 1.0))).astype(np.float32)


def late_page(table, levels):
    """A (B, 1, 16, 16) float32 ``dn`` page: sample b is CONSTANT at the Lloyd level ``levels[b]`` of ``table`` (a level lies in its own
    bin and survives the cast to float32 there).  With dn_1 == 1.0 the quantised 256x64 grid of sample b is constant at that level, the
    rmse falls with every iteration and the oracle's arg-min is the last iterate, with a margin of about 1e-3 at limit 8, 30 and 100
    (test_als_ref_cpu.py::test_mixed_map_pages).  One level per sample, not a spread: measured on the CPU, a page whose pixels are drawn
    from two or three neighbouring levels - even 8 pixels of 256 moved to the next level - has k* = 1 at every level of table 032 (the
    levels are ~3 % apart, and rows that differ by that much make the reinterpreted q-update overshoot at once), so the samples of the
    batch differ instead of the rows.  Level 20 is 1.0 (rmse 0 from the start) and must not be used."""
    _, inv = tables()[table]
    assert 20 not in levels
    return np.stack([np.full((1, 16, 16), np.float32(inv[k]), dtype=np.float32) for k in levels])


# ------------------------------------------------------------------------------------------------------------------------------------
# values exactly on a threshold after the kernel's arithmetic
# ------------------------------------------------------------------------------------------------------------------------------------
def _ulps(x, d):
    return (np.float64(x).view(np.int64) + np.int64(d)).view(np.float64)


_DN_CANDIDATES = (1.0, 0.5, 2.0, 0.75, 1.5, 1.25, 1.75, 0.625, 0.875, 3.0)


@functools.lru_cache(maxsize=None)
def threshold_window(table):
    """Probes (k, below, dn float32, area float64, bin) with float64(dn) * (1.0 / area) == q[k] exactly (``below`` False, bin k + 1:
    ``r >= q[k]`` holds) or == nextafter(q[k], 0) (``below`` True, bin k).  Search: dn = 1.0, area = 1 / target nudged by ulps; if the
    rounding of 1 / area steps over the target for every such area, the next float32 ``dn`` of a short list is tried with
    area = dn / target.  No threshold of any table is a float32 number, so these values cannot be planted in ``dn`` itself."""
    q, _ = tables()[table]
    out = []
    for k in range(40):
        for below in (False, True):
            target = np.nextafter(q[k], 0.0) if below else q[k]
            hit = None
            for dn in _DN_CANDIDATES:
                a0 = np.float64(dn) / target
                for d in sorted(range(-40, 41), key=abs):
                    area = _ulps(a0, d)
                    if np.float64(np.float32(dn)) * (1.0 / area) == target:
                        hit = (k, below, np.float32(dn), area, k if below else k + 1)
                        break
                if hit:
                    break
            if hit:
                out.append(hit)
    return tuple(out)


def threshold_cover(table):
    """(thresholds hit exactly, thresholds hit one ulp below, thresholds hit both ways, bins reached)"""
    pr = threshold_window(table)
    on = {p[0] for p in pr if not p[1]}
    under = {p[0] for p in pr if p[1]}
    return on, under, on & under, {p[4] for p in pr}


def base_probes(table):
    """float32 ``dn`` values for the 55 base slots (area 1): the float32 neighbours of every threshold, and values far outside the
    table on either side (bins 0 and 40).  (value float32, bin)"""
    q, _ = tables()[table]
    vals = []
    for k in range(40):
        f = np.float32(q[k])
        lo = f if np.float64(f) < q[k] else np.nextafter(f, np.float32(0))
        hi = np.nextafter(lo, np.float32(np.inf))
        assert np.float64(lo) < q[k] < np.float64(hi)
        vals += [(lo, k), (hi, k + 1)]
    vals += [(np.float32(v), 0) for v in (1e-30, 1e-3, 0.5 * q[0])] + [(np.float32(v), 40) for v in (2.0 * q[39], 1e3, 1e30)]
    return vals


_ORIGINS = ((0, 0), (0, 3), (3, 0), (3, 3))      # four window origins of a page whose 3x3 windows are disjoint


def threshold_map(table, B=2):
    """A whole map that carries ``threshold_window(table)`` and ``base_probes(table)``: ``dn`` (B, 1, S, S) float32 and an explicit
    ``dn_1`` (B, 1, S/2, S/2) float64, log-uniform wherever no probe sits, so that the ALS of every page keeps an early, well separated
    arg-min.  One CELL is one (page, sample).  Probes are grouped by their ``dn`` value, nine to a WINDOW: the window with origin (a, b)
    puts its nine areas into the coarse pixels (a..a+2, b..b+2) - one probe in each of the nine window slots - and its ``dn`` value into
    the four fine pixels (2a..2a+1, 2b..2b+1), whose window origin is exactly (a, b).  A cell holds the four disjoint windows at
    origins {0, 3} x {0, 3}; the fine pixels around them form ordinary ratios with the same coarse values.  The last cell carries
    ``base_probes`` in its first fine pixels under a log-uniform coarse page: the 55 base slots meet them with area 1, the 9 window
    slots with another area.  Returns (dn, dn_1, plan), plan = [(page, sample, [fine indices], coarse index or None, bin)]: the
    quantised grid at [page, sample, fine, coarse] (every base slot where coarse is None) must hold level ``bin``."""
    by_dn = {}
    for p in threshold_window(table):
        by_dn.setdefault(float(p[2]), []).append(p)
    windows = [(dnv, ps[i:i + 9]) for dnv, ps in by_dn.items() for i in range(0, len(ps), 9)]
    cells = [("window", windows[i:i + 4]) for i in range(0, len(windows), 4)] + [("base", base_probes(table))]
    ratio = 1
    while ratio * ratio * B < len(cells):
        ratio += 1
    S = 16 * ratio
    dn = log_uniform(4000 + int(table), (B, 1, S, S), 0.5, 2.0).astype(np.float32)
    dn1 = log_uniform(5000 + int(table), (B, 1, S // 2, S // 2), 0.5, 2.0)
    plan = []
    for ci, (kind, items) in enumerate(cells):
        page, b = ci // B, ci % B
        pi, pj = page // ratio, page % ratio
        fine = dn[b, 0, 16 * pi:16 * pi + 16, 16 * pj:16 * pj + 16]
        coarse = dn1[b, 0, 8 * pi:8 * pi + 8, 8 * pj:8 * pj + 8]
        if kind == "window":
            for (oa, ob), (dnv, ps) in zip(_ORIGINS, items):
                fine[2 * oa:2 * oa + 2, 2 * ob:2 * ob + 2] = np.float32(dnv)
                pix = [(2 * oa + i) * 16 + 2 * ob + j for i in (0, 1) for j in (0, 1)]
                for s, pr in enumerate(ps):
                    jr, jc = oa + s // 3, ob + s % 3
                    coarse[jr, jc] = pr[3]
                    plan.append((page, b, pix, jr * 8 + jc, pr[4]))
        else:
            assert len(items) <= 256
            for s, (v, bin_) in enumerate(items):
                fine[s // 16, s % 16] = v
                plan.append((page, b, [s], None, bin_))
    return dn, dn1, plan


def dense_threshold_depths():
    """(1, 1, 9, 9) float32 depths for the DENSE grid (derived 008 table, thresholds rounded to float32 as torch compares a float32
    tensor with a python scalar): d[0] = 1, then float32(q[k]) and its float32 predecessor for every k.  R[i, 0] = d_i * (1 / 1) is then
    exactly the rounded threshold (bin k + 1) or the float32 number below it (bin k); the other columns are ordinary ratios.
    Returns (d, rows [(i, bin)])."""
    q, _ = tables()["008"]
    d, rows = [np.float32(1.0)], []
    for k in range(40):
        f = np.float32(q[k])
        d += [f, np.nextafter(f, np.float32(0))]
        rows += [(2 * k + 1, k + 1), (2 * k + 2, k)]
    return np.array(d, dtype=np.float32).reshape(1, 1, 9, 9), rows


# ------------------------------------------------------------------------------------------------------------------------------------
# whole maps and their per-page oracle
# ------------------------------------------------------------------------------------------------------------------------------------
def corner_marked(dn_1):
    """Put a distinct value into the four corner pixels and along the four edge rows / columns of every 8x8 page of ``dn_1``
    (in place): a 3x3 window whose origin is off by one at a page edge then reads a value nothing else holds."""
    B, _, S1, _ = dn_1.shape
    r = S1 // 8
    for pi in range(r):
        for pj in range(r):
            pg = dn_1[:, 0, 8 * pi:8 * pi + 8, 8 * pj:8 * pj + 8]
            t = 1.0 + 0.01 * (pi * r + pj)
            pg[:, 0, 1:7] *= 1.10 * t
            pg[:, 7, 1:7] *= 0.90 * t
            pg[:, 1:7, 0] *= 1.20 * t
            pg[:, 1:7, 7] *= 0.80 * t
            pg[:, 0, 0], pg[:, 0, 7], pg[:, 7, 0], pg[:, 7, 7] = 0.55 * t, 0.70 * t, 1.45 * t, 1.90 * t
    return dn_1


def paged_oracle(dn, dn_1, table, limit, pages=None):
    """Per page (row-major, as ocp.split_matrix orders them): the raw grid, the quantised grid, and the oracle's ALS on it.
    Returns {page: dict(raw, R, out (B, 256) float32, rec, kstar, margin)}."""
    q, inv = tables()[table]
    a, b = ocp.split_matrix(np.asarray(dn), np.asarray(dn_1))
    res = {}
    for p in (range(len(a)) if pages is None else pages):
        with np.errstate(divide="ignore", invalid="ignore"):
            raw = ocp.ratio_grid_raw(a[p], b[p])
        R = ocp.lloyd_quantization(raw, q, inv)[0]
        d = dict(raw=raw, R=R)
        if limit is not None:
            d["out"], d["rec"], d["kstar"], d["margin"] = oracle_als(R, limit)
        res[p] = d
    return res


MIXED_LATE = {0: (12, 14), 3: (36, 34)}          # page -> the Lloyd level of each of its two samples


def mixed_map(table="032", seed=7):
    """Side-32 map, B = 2, 4 pages: pages 0 and 3 are ``late_page`` under dn_1 == 1.0 (k* = limit for limit 8, 30 and 100), pages 1 and 2
    are log-uniform under a log-uniform coarse page (k* = 1).  dn_1 is explicit, not a resize of dn.  Returns (dn, dn_1)."""
    dn = log_uniform(seed, (2, 1, 32, 32), 0.5, 2.0).astype(np.float32)
    dn1 = log_uniform(seed + 1, (2, 1, 16, 16), 0.5, 2.0)
    for page, levels in MIXED_LATE.items():
        pi, pj = page // 2, page % 2
        dn[:, :, 16 * pi:16 * pi + 16, 16 * pj:16 * pj + 16] = late_page(table, levels)
        dn1[:, :, 8 * pi:8 * pi + 8, 8 * pj:8 * pj + 8] = 1.0
    return dn, dn1


def index_map(side, B, seed, marked=False):
    """Log-uniform ``dn`` (B, 1, side, side) float32 and its coarse map ocp.resize(dn, side / 2) (bit-exact with the library's resize);
    ``marked`` replaces the coarse map by a log-uniform one with ``corner_marked`` values at every page's corners and edges."""
    dn = log_uniform(seed, (B, 1, side, side), 0.5, 2.0).astype(np.float32)
    if marked:
        return dn, corner_marked(log_uniform(seed + 1, (B, 1, side // 2, side // 2), 0.8, 1.25))
    return dn, ocp.resize(dn, side // 2)


def nonfinite_map(seed=11):
    """Side-32 map, B = 2: page 1 holds a coarse pixel equal to 0.0 (an infinite ratio, bin 40) in sample 0 and a NaN ``dn`` pixel (bin
    0: NaN compares false) in sample 1; the other pages are clean.  Returns (dn, dn_1)."""
    dn = log_uniform(seed, (2, 1, 32, 32), 0.5, 2.0).astype(np.float32)
    dn1 = log_uniform(seed + 1, (2, 1, 16, 16), 0.5, 2.0)
    dn1[0, 0, 3, 8 + 4] = 0.0                       # page (0, 1): coarse rows 0..7, columns 8..15
    dn[1, 0, 9, 16 + 5] = np.nan                    # page (0, 1): fine rows 0..15, columns 16..31
    return dn, dn1


def gm_reference(x, e):
    """exp(e * fsum(log x)) per sample, float64, and x / gm."""
    gm = np.array([math.exp(e * math.fsum(math.log(v) for v in row)) for row in x])
    return gm, x / gm[:, None]


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases both test files use (the CPU test asserts k* and the margin of every one that runs ALS)
# ------------------------------------------------------------------------------------------------------------------------------------
REPLAY_CASES = [(256, "f32", 8), (256, "f32", 30), (256, "f64", 8), (256, "f64", 30), (64, "f64", 30), (64, "f32", 30)]    # (rows, grid dtype, limit), B = 3
MIXED_LIMITS = (8, 100)
KEEP_LIMITS = (0, 1, 7, 8)
INDEX_CASES = [(side, B) for side in (16, 48, 80) for B in (1, 3, 5)]
INDEX_TABLE = {16: "016", 48: "032", 80: "064"}        # sides 48 and 80 have no table of their own: any table serves the indexing
MARKED_CASE = (48, 3)
LIMIT = 100                                            # the decoders' iteration limit (RDM_Net.py Ordinal_Layer)


@functools.lru_cache(maxsize=None)
def replay_grid(rows):
    return late_grid(3, rows, 1)


@functools.lru_cache(maxsize=None)
def keep_grids():
    """(log-uniform 256x64 grid, late grid), B = 2"""
    return log_uniform(21, (2, 256, 64), 0.5, 2.0).astype(np.float32), late_grid(2, 256, 2)


@functools.lru_cache(maxsize=None)
def index_case(side, B, marked=False):
    dn, dn1 = index_map(side, B, 100 + side + B, marked)
    return dn, dn1, paged_oracle(dn, dn1, INDEX_TABLE[side], LIMIT)


@functools.lru_cache(maxsize=None)
def mixed_case(limit):
    dn, dn1 = mixed_map()
    return dn, dn1, paged_oracle(dn, dn1, "032", limit)


@functools.lru_cache(maxsize=None)
def threshold_case(table):
    dn, dn1, plan = threshold_map(table)
    return dn, dn1, plan, paged_oracle(dn, dn1, table, LIMIT)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    dn, dn1 = nonfinite_map()
    return dn, dn1, paged_oracle(dn, dn1, "032", LIMIT)
