"""include/rdm_fuse.h restated in numpy float64: the planes rdm_tsdf_integrate must leave and the records rdm_tsdf_extract must write.  Written
from the header alone; shares no code with the kernels.  Every arithmetic step is one numpy float64 operation in the header's order over whole
volumes, so the comparison with the device is equality."""
import math

import numpy as np


def valid(d, min_depth=0.0, max_depth=math.inf):
    """rdm_cloud.h's validity of float32 depths"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > 0) & (d.astype(np.float64) >= min_depth) & (d.astype(np.float64) <= max_depth)


def centres(dims, geom):
    """Px (1,1,nx), Py (1,ny,1), Pz (nz,1,1) float64"""
    nx, ny, nz = dims
    ox, oy, oz, voxel = (np.float64(v) for v in geom[:4])
    return (ox + np.arange(nx, dtype=np.float64) * voxel).reshape(1, 1, nx), (oy + np.arange(ny, dtype=np.float64) * voxel).reshape(1, ny, 1), \
        (oz + np.arange(nz, dtype=np.float64) * voxel).reshape(nz, 1, 1)


def pose_rows(poses, batch):
    P = np.asarray(poses, np.float64)
    P = P.reshape(-1, 12) if P.shape[-1] == 12 else P[..., :3, :].reshape(-1, 12)
    assert P.shape[0] in (1, batch)
    return np.broadcast_to(P, (batch, 12))


def integrate(depth, rgb, intr, poses, dims, geom, tsdf, weight, color, min_depth=0.0, max_depth=math.inf, obs_weight=1.0, max_weight=64.0):
    """-> (tsdf, weight, color) after the frames of ``depth`` (B,h,w) in order; the inputs are not modified.  ``color`` None: no colour plane."""
    depth = np.asarray(depth, np.float32)
    B, h, w = depth.shape
    nx, ny, nz = dims
    fx, fy, cx, cy = (np.float64(v) for v in intr)
    trunc, ow, mw = np.float64(geom[4]), np.float64(obs_weight), np.float64(max_weight)
    Px, Py, Pz = centres(dims, geom)
    T, W = np.array(tsdf, np.float32).reshape(nz, ny, nx), np.array(weight, np.float32).reshape(nz, ny, nx)
    Cc = None if color is None else np.array(color, np.float32).reshape(nz, ny, nx, 3)
    R = pose_rows(poses, B)
    for b in range(B):
        r = R[b]
        with np.errstate(all="ignore"):
            Qx = ((r[0] * Px + r[1] * Py) + r[2] * Pz) + r[3]
            Qy = ((r[4] * Px + r[5] * Py) + r[6] * Pz) + r[7]
            Qz = ((r[8] * Px + r[9] * Py) + r[10] * Pz) + r[11]
            ok = np.isfinite(Qz) & (Qz > 0)
            u = (fx * Qx) / Qz + cx
            v = (fy * Qy) / Qz + cy
            ok &= np.isfinite(u) & np.isfinite(v)
            c, rr = np.floor(u + 0.5), np.floor(v + 0.5)
            ok &= (c >= 0) & (c <= w - 1) & (rr >= 0) & (rr <= h - 1)                  # in float64, before any conversion
            ci, ri = np.where(ok, c, 0.0).astype(np.int64), np.where(ok, rr, 0.0).astype(np.int64)
            d = depth[b][ri, ci]
            ok &= valid(d, min_depth, max_depth)
            sdf = d.astype(np.float64) - Qz
            ok &= ~(sdf < -trunc)
            s = sdf / trunc
            s = np.where(s > 1, np.float64(1.0), s)
            Wd = W.astype(np.float64)
            den = Wd + ow
            Tn = ((Wd * T.astype(np.float64) + ow * s) / den).astype(np.float32)
            if Cc is not None:
                px = np.asarray(rgb, np.uint8)[b][ri, ci].astype(np.float64)          # (nz,ny,nx,3)
                Cn = ((Wd[..., None] * Cc.astype(np.float64) + ow * px) / den[..., None]).astype(np.float32)
                Cc = np.where(ok[..., None], Cn, Cc)
            Wn = np.where(den > mw, mw, den).astype(np.float32)
        T, W = np.where(ok, Tn, T), np.where(ok, Wn, W)
    return T, W, Cc


def _shift(a, axis, by, fill):
    """a[idx + by] along ``axis``, ``fill`` where that is outside"""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    src, dst = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    if by > 0:
        src[axis], dst[axis] = slice(by, n), slice(0, n - by)
    else:
        src[axis], dst[axis] = slice(0, n + by), slice(-by, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def gradient(T, obs):
    """(nz,ny,nx,3) float64: g(V) per axis x, y, z"""
    T64 = T.astype(np.float64)
    out = np.zeros(T.shape + (3,), np.float64)
    for comp, axis in ((0, 2), (1, 1), (2, 0)):
        lo, hi = _shift(obs, axis, -1, False), _shift(obs, axis, 1, False)
        Tm, Tp = _shift(T64, axis, -1, 0.0), _shift(T64, axis, 1, 0.0)
        with np.errstate(all="ignore"):
            out[..., comp] = np.where(lo & hi, (Tp - Tm) * 0.5, np.where(hi, Tp - T64, np.where(lo, T64 - Tm, 0.0)))
    return out


def extract(tsdf, weight, color, dims, geom, min_weight=1.0, normals=True):
    """-> (records as bytes, count): every crossing, in the header's order"""
    nx, ny, nz = dims
    T, W = np.asarray(tsdf, np.float32).reshape(nz, ny, nx), np.asarray(weight, np.float32).reshape(nz, ny, nx)
    Cc = None if color is None else np.asarray(color, np.float32).reshape(nz, ny, nx, 3)
    ox, oy, oz, voxel = (np.float64(v) for v in geom[:4])
    origin = (ox, oy, oz)
    with np.errstate(invalid="ignore"):
        obs = np.isfinite(T) & (W.astype(np.float64) >= min_weight)
        inside = obs & (np.abs(T) < 1)
        neg = T < 0
    g = gradient(T, obs) if normals else None
    rec = 12 + (12 if normals else 0) + (3 if Cc is not None else 0)
    keys, rows = [], []
    for comp, axis in ((0, 2), (1, 1), (2, 0)):                                  # the x, y, z edges
        cross = inside & _shift(inside, axis, 1, False) & (neg != _shift(neg, axis, 1, False))
        k, j, i = np.nonzero(cross)
        idx0 = (k, j, i)
        idx1 = tuple(v + (1 if a == axis else 0) for a, v in enumerate(idx0))
        T0, T1 = T[idx0].astype(np.float64), T[idx1].astype(np.float64)
        with np.errstate(all="ignore"):
            a = T0 / (T0 - T1)
            pos = [origin[0] + i.astype(np.float64) * voxel, origin[1] + j.astype(np.float64) * voxel, origin[2] + k.astype(np.float64) * voxel]
            along = (i, j, k)[comp].astype(np.float64)
            pos[comp] = origin[comp] + (along + a) * voxel
            out = np.zeros((len(k), rec), np.uint8)
            out[:, :12] = np.stack(pos, axis=1).astype(np.float32).view(np.uint8).reshape(-1, 12)
            at = 12
            if normals:
                g0, g1 = g[idx0], g[idx1]
                n = g0 + a[:, None] * (g1 - g0)
                l = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
                good = np.isfinite(l) & (l > 0)
                n = np.where(good[:, None], n / np.where(good, l, 1.0)[:, None], 0.0)
                out[:, 12:24] = np.ascontiguousarray(n.astype(np.float32)).view(np.uint8).reshape(-1, 12)
                at = 24
            if Cc is not None:
                C0, C1 = Cc[idx0].astype(np.float64), Cc[idx1].astype(np.float64)
                ch = C0 + a[:, None] * (C1 - C0)
                q = np.floor(ch + 0.5)
                out[:, at:at + 3] = np.where(np.isnan(ch), 0.0, np.where(q <= 0, 0.0, np.where(q >= 255, 255.0, q))).astype(np.uint8)
        keys.append(((k.astype(np.int64) * ny + j) * nx + i) * 3 + comp)
        rows.append(out)
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    order = np.argsort(keys, kind="stable")
    return rows[order].tobytes(), len(keys)


def records_array(payload, count, normals, colour):
    """the payload as (count, 3) positions, (count, 3) normals or None, (count, 3) colours or None"""
    rec = 12 + (12 if normals else 0) + (3 if colour else 0)
    raw = np.frombuffer(payload, np.uint8)[:count * rec].reshape(count, rec)
    pos = np.ascontiguousarray(raw[:, :12]).view(np.float32)
    nrm = np.ascontiguousarray(raw[:, 12:24]).view(np.float32) if normals else None
    col = raw[:, rec - 3:] if colour else None
    return pos, nrm, col
