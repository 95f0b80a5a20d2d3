"""include/rdm_cloud.h restated in numpy float64: the record bytes and counts rdm_depth_cloud must write.  Every float64 step is one numpy
operation on arrays (numpy contracts nothing), in the header's order; the float32 results are one ``astype`` each."""
import numpy as np


def record_bytes(normals, colour):
    return 12 + (12 if normals else 0) + (3 if colour else 0)


def valid_mask(depth, min_depth=0.0, max_depth=np.inf):
    """(…,h,w) bool: finite, > 0, inside [min_depth, max_depth] as float64"""
    d = np.asarray(depth, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0) & (d.astype(np.float64) >= min_depth) & (d.astype(np.float64) <= max_depth)


def points(depth, intr):
    """(h,w) float32 -> (h,w,3) float64 X, Y, Z (whatever the depth is; the caller masks)"""
    fx, fy, cx, cy = (float(v) for v in intr)
    h, w = depth.shape
    Z = depth.astype(np.float64)
    xs, ys = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        X = ((xs - cx) * Z) / fx
        Y = ((ys - cy) * Z) / fy
    return np.stack([X, Y, Z], axis=-1)


def _diff(P, valid, axis):
    """the header's difference along ``axis`` (0: b, vertical; 1: a, horizontal) -> ((h,w,3) float64, (h,w) bool: at least one neighbour is valid)"""
    h, w = valid.shape
    pad = [(0, 0), (0, 0), (0, 0)]
    pad[axis] = (1, 1)
    Pp = np.pad(P, pad)
    vp = np.pad(valid, pad[:2])
    lo = (slice(0, h), slice(None)) if axis == 0 else (slice(None), slice(0, w))
    hi = (slice(2, h + 2), slice(None)) if axis == 0 else (slice(None), slice(2, w + 2))
    Pl, Ph, vl, vh = Pp[lo], Pp[hi], vp[lo], vp[hi]
    with np.errstate(invalid="ignore", over="ignore"):
        both, fwd, bwd = Ph - Pl, Ph - P, P - Pl
    out = np.where((vl & vh)[..., None], both, np.where(vh[..., None], fwd, bwd))
    return out, vl | vh


def normals_of(P, valid):
    """(h,w,3) float64 unit normals facing the camera, (0,0,0) where the header says so; only meaningful at valid pixels"""
    a, ha = _diff(P, valid, 1)
    b, hb = _diff(P, valid, 0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        nx = b[..., 1] * a[..., 2] - b[..., 2] * a[..., 1]
        ny = b[..., 2] * a[..., 0] - b[..., 0] * a[..., 2]
        nz = b[..., 0] * a[..., 1] - b[..., 1] * a[..., 0]
        s = (nx * P[..., 0] + ny * P[..., 1]) + nz * P[..., 2]
        flip = s > 0
        nx, ny, nz = np.where(flip, -nx, nx), np.where(flip, -ny, ny), np.where(flip, -nz, nz)
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = ha & hb & np.isfinite(l) & (l > 0)
        n = np.stack([nx / l, ny / l, nz / l], axis=-1)
    return np.where(good[..., None], n, 0.0)


def sample_arrays(depth, intr, rgb=None, normals=False, min_depth=0.0, max_depth=np.inf, step=1):
    """one (h,w) sample -> dict: "valid" (sh,sw) bool of the sampled pixels, "xyz" (n,3) float32, "normals" (n,3) float32 | None, "rgb" (n,3) uint8 | None,
    "normals64" the float64 normals before rounding | None; n valid sampled pixels in row-major order"""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    valid = valid_mask(depth, min_depth, max_depth)
    P = points(depth, intr)
    keep = np.zeros_like(valid)
    keep[::step, ::step] = valid[::step, ::step]
    out = {"valid": valid[::step, ::step], "xyz": P[keep].astype(np.float32), "normals": None, "normals64": None, "rgb": None}
    if normals:
        out["normals64"] = normals_of(P, valid)[keep]
        out["normals"] = out["normals64"].astype(np.float32)
    if rgb is not None:
        out["rgb"] = np.ascontiguousarray(rgb, dtype=np.uint8)[keep]
    return out


def pack(arrays):
    """the record bytes of ``sample_arrays``' result"""
    parts = [arrays["xyz"].astype("<f4").view(np.uint8).reshape(-1, 12)]
    if arrays["normals"] is not None:
        parts.append(arrays["normals"].astype("<f4").view(np.uint8).reshape(-1, 12))
    if arrays["rgb"] is not None:
        parts.append(arrays["rgb"].reshape(-1, 3))
    return np.concatenate(parts, axis=1).tobytes()


def reference(depth, intr, rgb=None, normals=False, min_depth=0.0, max_depth=np.inf, step=1):
    """(B,h,w) float32 [, (B,h,w,3) uint8] -> ([record bytes of sample b], (B,) int32 counts)"""
    depth = np.asarray(depth, dtype=np.float32)
    recs, counts = [], []
    for b in range(depth.shape[0]):
        arr = sample_arrays(depth[b], intr, None if rgb is None else rgb[b], normals, min_depth, max_depth, step)
        recs.append(pack(arr))
        counts.append(len(arr["xyz"]))
    return recs, np.asarray(counts, dtype=np.int32)


def run_starts(valid_sampled, split):
    """record index at which each workgroup's run starts, and the total: run r of a sample owns the sampled pixels [r * ns // split, (r + 1) * ns // split)
    in row-major order, split taken as at most ns (include/rdm_cloud.h) -> (split + 1,) int64"""
    v = np.asarray(valid_sampled, dtype=bool).reshape(-1)
    ns = v.size
    split = min(int(split), ns)
    cum = np.concatenate([[0], np.cumsum(v)])
    return cum[[r * ns // split for r in range(split + 1)]]
