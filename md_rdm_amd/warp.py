"""A depth frame seen from another camera: every valid pixel of a metric depth frame (``depth.metric_frames``, or any sensor depth in metres)
unprojected, moved by a rigid pose, projected into a target pixel grid and kept where it is the nearest surface of its cell, with its colour and
its source index; optionally the holes of every row filled from the farther of their nearest neighbours (``rdm_depth_warp``,
include/rdm_warp.h: three launches, a 64-bit atomic minimum as the depth test, bit-for-bit reproducible).  The right eye of a stereo pair
(``stereo_pose``), a small camera move (``pose_from_rt``), or the depth of one frame in another frame's pixel grid.  A pinhole camera only, one
intrinsics pair per call, point splats rather than rasterised surfaces (a magnifying view cracks unless ``splat`` is raised), row-wise filling only
and no blending of several sources.  The defaults ``SPLAT`` and ``FILL`` are starting points: no trained checkpoint and no dataset were at hand,
so their effect on real predictions has not been measured.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, cloud

SPLAT, FILL = 1, 8                                  # the command line's --view_splat / --view_fill defaults: starting points, not measured
MAX_SPLAT, MAX_FILL = 4, 64                         # the library's ranges (include/rdm_warp.h)
PLANES = ("depth", "rgb", "index", "mask")


def stereo_pose(baseline):
    """(3,4) float64 pose of a camera ``baseline`` metres to the RIGHT of the source camera, looking the same way: R = I, t = (-baseline, 0, 0) - a
    point at X in the left camera is at X - baseline in the right one."""
    b = float(baseline)
    if not math.isfinite(b):
        raise _lib.RdmError("stereo_pose: baseline must be finite, got %r" % baseline)
    pose = np.zeros((3, 4), np.float64)
    pose[:, :3] = np.eye(3)
    pose[0, 3] = -b
    return pose


def pose_from_rt(rotvec, t):
    """(3,4) float64 pose [R | t] from a rotation vector (axis * angle in radians, Rodrigues' formula in float64 on the host:
    R = I + sin(a) K + (1 - cos(a)) K^2 with K the cross-product matrix of the unit axis; a = 0: R = I) and a translation in metres."""
    r, t = np.asarray(rotvec, np.float64).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    if r.shape != (3,) or t.shape != (3,) or not (np.isfinite(r).all() and np.isfinite(t).all()):
        raise _lib.RdmError("pose_from_rt: rotvec and t must be three finite values each, got %r and %r" % (rotvec, t))
    angle = float(np.sqrt((r * r).sum()))
    R = np.eye(3)
    if angle > 0:
        k = r / angle
        K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        R = R + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)
    return np.concatenate([R, t[:, None]], axis=1)


def pose_rows(pose, batch):
    """``pose`` ((3,4) | (4,4) | (B,3,4) | (B,4,4), numpy, a tensor or nested lists) -> float64 (1 | B, 12) on the host, the rows [R | t] of each"""
    p = pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else np.asarray(pose)
    try:
        p = p.astype(np.float64)
    except (TypeError, ValueError):
        raise _lib.RdmError("pose must be numeric, got %r" % (pose,))
    if p.ndim == 2:
        p = p[None]
    if p.ndim != 3 or p.shape[1:] not in ((3, 4), (4, 4)) or p.shape[0] not in (1, batch):
        raise _lib.RdmError("pose must be (3,4), (4,4), (%d,3,4) or (%d,4,4), got %s" % (batch, batch, np.asarray(p).shape))
    return np.ascontiguousarray(p[:, :3, :].reshape(p.shape[0], 12))


def check_params(splat, fill):
    """the library's ranges of splat and fill -> an error text, or None"""
    if not (isinstance(splat, (int, np.integer)) and 1 <= splat <= MAX_SPLAT):
        return "splat must be an integer in 1..%d, got %r" % (MAX_SPLAT, splat)
    if not (isinstance(fill, (int, np.integer)) and 0 <= fill <= MAX_FILL):
        return "fill must be an integer in 0..%d, got %r" % (MAX_FILL, fill)
    return None


def render(depth, intrinsics, pose, rgb=None, out_hw=None, intrinsics_out=None, min_depth=0.0, max_depth=math.inf, splat=1, fill=0,
           want=PLANES):
    """``rdm_depth_warp``: a dict of device tensors.  ``depth`` (B,h,w) float32 metres on the device; ``intrinsics`` (fx, fy, cx, cy) of that
    frame (or a name in ``cloud.INTRINSICS``); ``pose`` maps source-camera to target-camera coordinates, one for the batch or one per sample
    (``pose_rows``), moved to the device as float64 - a tensor already on the device is widened there and never visits the host; ``rgb``
    (B,h,w,3) uint8 on the device, or None.  The target camera has ``out_hw`` pixels (default (h, w)) and ``intrinsics_out`` (default
    ``intrinsics``): the same camera, moved.  A source pixel takes part iff its depth is finite, > 0
    and inside [min_depth, max_depth]; it covers ``splat`` x ``splat`` target cells around its projection, and a cell keeps the nearest point
    offered to it (the smaller source index at equal depth).  ``fill`` F > 0: an empty cell takes the farther of the nearest kept cells within F
    columns to its left and right in its row.  Planes, those named in ``want``: "depth" (B,th,tw) float32, 0 where empty; "rgb" (B,th,tw,3) uint8
    (only when ``rgb`` is given); "index" (B,th,tw) int32, the source pixel y * w + x, -1 where empty; "mask" (B,th,tw) uint8, 0 empty, 1 kept,
    2 filled.  The workspace is allocated per call."""
    bad = check_params(splat, fill)
    if bad:
        raise _lib.RdmError(bad)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in PLANES for k in want):
        raise _lib.RdmError("want must name planes of %s, got %r" % (", ".join(PLANES), want))
    if out_hw is not None and not (len(tuple(out_hw)) == 2 and all(isinstance(v, (int, np.integer)) and v > 0 for v in out_hw)):
        raise _lib.RdmError("out_hw must be two positive integers, got %r" % (out_hw,))
    src = cloud.intrinsics_params(intrinsics)
    dst = src if intrinsics_out is None else cloud.intrinsics_params(intrinsics_out)
    for name, vals in (("intrinsics", src), ("intrinsics_out", dst)):
        if not (all(math.isfinite(v) for v in vals) and vals[0] != 0 and vals[1] != 0):
            raise _lib.RdmError("%s must be finite with fx and fy not 0, got %r" % (name, vals))
    if not (float(min_depth) >= 0 and float(max_depth) >= float(min_depth)):
        raise _lib.RdmError("need 0 <= min_depth <= max_depth, got %r and %r" % (min_depth, max_depth))
    d, (B, h, w) = _lib.device_depth(depth, "warp.render")
    rgb = _lib.device_rgb(rgb, B, h, w)
    th, tw = (h, w) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    L = _lib.lib()
    if isinstance(pose, torch.Tensor) and pose.is_cuda:          # a pose on the device stays there: widened and cut to its rows on the caller's stream
        p = pose.detach().unsqueeze(0) if pose.dim() == 2 else pose.detach()
        if p.dim() != 3 or tuple(p.shape[1:]) not in ((3, 4), (4, 4)) or p.shape[0] not in (1, B) or p.device != d.device:
            raise _lib.RdmError("pose must be (3,4), (4,4), (%d,3,4) or (%d,4,4) on the depth's device, got %s" % (B, B, tuple(pose.shape)))
        poses = p.to(torch.float64)[:, :3, :].reshape(p.shape[0], 12).contiguous()
    else:
        poses = torch.from_numpy(pose_rows(pose, B)).to(d.device)
    out = {"depth": torch.empty(B, th, tw, dtype=torch.float32, device=d.device)}
    if rgb is not None and "rgb" in want:
        out["rgb"] = torch.empty(B, th, tw, 3, dtype=torch.uint8, device=d.device)
    if "index" in want:
        out["index"] = torch.empty(B, th, tw, dtype=torch.int32, device=d.device)
    if "mask" in want:
        out["mask"] = torch.empty(B, th, tw, dtype=torch.uint8, device=d.device)
    ws_bytes = L.rdm_depth_warp_workspace_bytes(B, th, tw)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=d.device)
    _lib.check(L.rdm_depth_warp(_lib.ptr(d), _lib.ptr(rgb), B, h, w, (C.c_double * 4)(*src), (C.c_double * 4)(*dst), _lib.ptr(poses),
                                12 if poses.shape[0] > 1 else 0, float(min_depth), float(max_depth), th, tw, int(splat), int(fill), _lib.ptr(out["depth"]),
                                _lib.ptr(out.get("rgb")), _lib.ptr(out.get("index")), _lib.ptr(out.get("mask")), _lib.ptr(ws), ws_bytes, _lib.stream()))
    return {k: v for k, v in out.items() if k in want}
