"""include/rdm_warp.h restated in numpy float64: the planes rdm_depth_warp must write.  Written from the header alone; shares no code with the
kernel.  Every arithmetic step is one numpy float64 operation in the header's order, so the comparison with the device is equality.
``sample`` is vectorised (a minimum over keys with ``np.minimum.at``, the fill by explicit loops over the holes); ``loops`` is the same
statement pixel by pixel for the CPU tests to compare the two."""
import math

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def valid(d, min_depth=0.0, max_depth=math.inf):
    """rdm_cloud.h's validity of float32 depths"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0) & (d.astype(np.float64) >= min_depth) & (d.astype(np.float64) <= max_depth)


def pose12(pose):
    p = np.asarray(pose, np.float64)
    return p[:3, :].reshape(12) if p.ndim == 2 else p.reshape(12)


def first_cell(u, s):
    return np.floor((u - (s - 1) * 0.5) + 0.5)


def keys_of(d, intr_src, intr_dst, pose, min_depth, max_depth, th, tw, splat):
    """(th, tw) uint64: the minimum key of every cell, EMPTY where none"""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    fx, fy, cx, cy = (np.float64(v) for v in intr_src)
    fxd, fyd, cxd, cyd = (np.float64(v) for v in intr_dst)
    T = pose12(pose)
    keys = np.full(th * tw, EMPTY, np.uint64)
    ok = valid(d, min_depth, max_depth)
    ys, xs = np.nonzero(ok)
    with np.errstate(all="ignore"):
        Z = d[ys, xs].astype(np.float64)
        X = ((xs.astype(np.float64) - cx) * Z) / fx
        Y = ((ys.astype(np.float64) - cy) * Z) / fy
        Qx = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3]
        Qy = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7]
        Qz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11]
        zf = Qz.astype(np.float32)
        u = (fxd * Qx) / Qz + cxd
        v = (fyd * Qy) / Qz + cyd
        keep = np.isfinite(Qz) & np.isfinite(zf) & (zf > 0) & np.isfinite(u) & np.isfinite(v)
        c0, r0 = first_cell(u, splat), first_cell(v, splat)
        keep &= (c0 >= 1 - splat) & (c0 <= tw - 1) & (r0 >= 1 - splat) & (r0 <= th - 1)          # in float64, before any conversion
    ys, xs, zf, c0, r0 = ys[keep], xs[keep], zf[keep], c0[keep].astype(np.int64), r0[keep].astype(np.int64)
    key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (ys * w + xs).astype(np.uint64)
    for dr in range(splat):
        for dc in range(splat):
            r, c = r0 + dr, c0 + dc
            inside = (r >= 0) & (r < th) & (c >= 0) & (c < tw)
            np.minimum.at(keys, (r * tw + c)[inside], key[inside])
    return keys.reshape(th, tw)


def resolve(keys, rgb, fill):
    """keys (th, tw) uint64 -> the four planes of one sample"""
    th, tw = keys.shape
    has = keys != EMPTY
    bits = (keys >> np.uint64(32)).astype(np.uint32)
    chosen = keys.copy()
    mask = has.astype(np.uint8)
    if fill > 0:
        for r, c in zip(*np.nonzero(~has)):
            left = next((keys[r, c - k] for k in range(1, fill + 1) if c - k >= 0 and has[r, c - k]), None)
            right = next((keys[r, c + k] for k in range(1, fill + 1) if c + k < tw and has[r, c + k]), None)
            if left is None and right is None:
                continue
            if left is not None and right is not None:
                zl, zr = np.uint32(left >> np.uint64(32)).view(np.float32), np.uint32(right >> np.uint64(32)).view(np.float32)
                pick = right if zr > zl else left
            else:
                pick = left if left is not None else right
            chosen[r, c], mask[r, c] = pick, 2
    got = mask > 0
    bits = (chosen >> np.uint64(32)).astype(np.uint32)
    index = (chosen & np.uint64(0xFFFFFFFF)).astype(np.int64)
    depth = np.where(got, bits.view(np.float32), np.float32(0.0)).astype(np.float32)
    out = {"depth": depth, "index": np.where(got, index, -1).astype(np.int32), "mask": mask}
    if rgb is not None:
        flat = np.asarray(rgb, np.uint8).reshape(-1, 3)
        out["rgb"] = np.where(got[..., None], flat[np.where(got, index, 0)], np.uint8(0)).astype(np.uint8)
    return out


def sample(d, intr_src, pose, rgb=None, out_hw=None, intr_dst=None, min_depth=0.0, max_depth=math.inf, splat=1, fill=0):
    d = np.asarray(d, np.float32)
    th, tw = d.shape if out_hw is None else out_hw
    keys = keys_of(d, intr_src, intr_src if intr_dst is None else intr_dst, pose, min_depth, max_depth, th, tw, splat)
    return resolve(keys, rgb, fill)


def reference(depth, intr_src, poses, rgb=None, **kw):
    """a batch: ``poses`` one pose or one per sample -> the planes stacked"""
    depth = np.asarray(depth, np.float32)
    P = np.asarray(poses, np.float64)
    P = np.broadcast_to(P[None] if P.ndim == 2 else P, (depth.shape[0],) + P.shape[-2:])
    outs = [sample(depth[b], intr_src, P[b], None if rgb is None else rgb[b], **kw) for b in range(depth.shape[0])]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def loops(d, intr_src, pose, rgb=None, out_hw=None, intr_dst=None, min_depth=0.0, max_depth=math.inf, splat=1, fill=0):
    """``sample`` pixel by pixel, with Python's float64 scalars"""
    d = np.asarray(d, np.float32)
    h, w = d.shape
    th, tw = d.shape if out_hw is None else out_hw
    fx, fy, cx, cy = (float(v) for v in intr_src)
    fxd, fyd, cxd, cyd = (float(v) for v in (intr_src if intr_dst is None else intr_dst))
    T = [float(v) for v in pose12(pose)]
    best = {}
    for y in range(h):
        for x in range(w):
            dv = d[y, x]
            if not (np.isfinite(dv) and dv > 0 and min_depth <= float(dv) <= max_depth):
                continue
            Z = float(dv)
            X = ((float(x) - cx) * Z) / fx
            Y = ((float(y) - cy) * Z) / fy
            Qx = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3]
            Qy = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7]
            Qz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11]
            with np.errstate(over="ignore"):
                zf = np.float32(Qz)
            if not (math.isfinite(Qz) and np.isfinite(zf) and zf > 0):
                continue
            u, v = (fxd * Qx) / Qz + cxd, (fyd * Qy) / Qz + cyd
            if not (math.isfinite(u) and math.isfinite(v)):
                continue
            c0, r0 = math.floor((u - (splat - 1) * 0.5) + 0.5), math.floor((v - (splat - 1) * 0.5) + 0.5)
            for r in range(max(r0, 0), min(r0 + splat, th)):
                for c in range(max(c0, 0), min(c0 + splat, tw)):
                    cand = (int(zf.view(np.uint32)), y * w + x)
                    if (r, c) not in best or cand < best[(r, c)]:
                        best[(r, c)] = cand
    keys = np.full((th, tw), EMPTY, np.uint64)
    for (r, c), (zb, i) in best.items():
        keys[r, c] = np.uint64((zb << 32) | i)
    return resolve(keys, rgb, fill)
