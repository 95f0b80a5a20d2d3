"""One model of a scene from many frames: metric depth frames (``depth.metric_frames``, ``anchor.metric_frames``, or any sensor depth in metres),
each with the pose of its camera, integrated into ONE truncated signed distance volume (``rdm_tsdf_integrate``, include/rdm_fuse.h: one launch
per call, the frame loop inside the thread, so a batch of frames costs one read and one write of the volume), and the volume's zero crossings
read out as oriented, coloured surface points (``rdm_tsdf_extract``: at most three launches) in ``cloud``'s record layout, which
``cloud.write_ply`` writes.  Bit-for-bit reproducible: no atomics, a fixed order of frames and of records.

Points, not a marching-cubes mesh; the volume is not raycast into a view; a dense volume only (``bounds`` sizes it from the frusta); one
intrinsics set per call; and a monocular frame's scale error blurs the surface unless the frames are anchored (``md_rdm_amd.anchor``).  The
defaults ``VOXEL``, ``TRUNC_VOXELS`` and ``MIN_WEIGHT`` are starting points: no trained checkpoint, no poses and no dataset were at hand, so
their effect on real data has not been measured.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, cloud, warp

VOXEL, TRUNC_VOXELS, MIN_WEIGHT, MAX_WEIGHT = 0.02, 4.0, 1.0, 64.0          # the command line's defaults: starting points, not measured
MAX_VOXELS = 2 ** 31 - 1                                                  # the library's index (include/rdm_fuse.h)


def _poses34(pose, who):
    p = pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else np.asarray(pose)
    try:
        p = p.astype(np.float64)
    except (TypeError, ValueError):
        raise _lib.RdmError("%s: pose must be numeric, got %r" % (who, pose))
    if p.ndim not in (2, 3) or p.shape[-2:] not in ((3, 4), (4, 4)):
        raise _lib.RdmError("%s: pose must be (3,4), (4,4), (B,3,4) or (B,4,4), got %s" % (who, p.shape))
    return p[..., :3, :]


def pose_inverse(pose):
    """The inverse of a rigid pose [R | t] in float64: [R^T | -R^T t], for (3,4) | (4,4) | (B,3,4) | (B,4,4) -> (3,4) | (B,3,4).  Camera-to-world
    poses (what SLAM systems write) become the world-to-camera poses ``Volume.integrate`` takes.  R is taken to be a rotation and is not checked."""
    p = _poses34(pose, "pose_inverse")
    Rt = np.swapaxes(p[..., :3], -1, -2)
    return np.concatenate([Rt, -(Rt @ p[..., 3:])], axis=-1)


def frustum_corners(frame_hw, intrinsics, poses_world_to_cam, max_depth):
    """(B,5,3) float64 world points: every camera's centre and the four corners of its frame (the pixels' outer edges, -0.5 and size - 0.5) at
    ``max_depth``"""
    h, w = int(frame_hw[0]), int(frame_hw[1])
    fx, fy, cx, cy = cloud.intrinsics_params(intrinsics)
    far = float(max_depth)
    if not (h > 0 and w > 0 and all(math.isfinite(v) for v in (fx, fy, cx, cy)) and fx != 0 and fy != 0 and math.isfinite(far) and far > 0):
        raise _lib.RdmError("bounds: need a positive frame, finite intrinsics with fx, fy not 0 and a finite max_depth > 0, got %r, %r, %r" % (frame_hw, intrinsics, max_depth))
    p = _poses34(poses_world_to_cam, "bounds")
    p = p[None] if p.ndim == 2 else p
    cam = np.array([[0.0, 0.0, 0.0]] + [[(x - cx) * far / fx, (y - cy) * far / fy, far] for y in (-0.5, h - 0.5) for x in (-0.5, w - 0.5)])
    inv = pose_inverse(p)                                                   # camera -> world
    return np.einsum("bij,kj->bki", inv[:, :, :3], cam) + inv[:, None, :, 3]


def bounds(frame_hw, intrinsics, poses_world_to_cam, max_depth, voxel):
    """(origin, dims) of the axis-aligned box of voxel centres that holds the frusta of all the cameras, cut at ``max_depth``: origin = the smallest
    corner (three floats, world metres), dims = (nx, ny, nz) with origin + (dims - 1) * voxel at or beyond the largest.  In numpy on the host."""
    voxel = float(voxel)
    if not (math.isfinite(voxel) and voxel > 0):
        raise _lib.RdmError("bounds: voxel must be finite and > 0, got %r" % (voxel,))
    pts = frustum_corners(frame_hw, intrinsics, poses_world_to_cam, max_depth).reshape(-1, 3)
    if not np.isfinite(pts).all():
        raise _lib.RdmError("bounds: the poses give frusta that are not finite")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    dims = tuple(int(v) for v in np.ceil((hi - lo) / voxel).astype(np.int64) + 1)
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise _lib.RdmError("bounds: %d x %d x %d voxels of %g m are beyond the library's 2^31 - 1; raise voxel or lower max_depth" % (dims + (voxel,)))
    return tuple(float(v) for v in lo), dims


class Volume:
    """A dense TSDF volume on the device.  ``dims`` (nx, ny, nz) voxels whose centres are origin + index * voxel in world metres; ``trunc`` the
    truncation distance in metres (default ``TRUNC_VOXELS`` * voxel); ``color``: also a colour plane; ``max_weight`` caps the running weight, so
    that a voxel keeps following the newer frames.  Planes: ``tsdf`` (nz,ny,nx) float32, 1 = free space; ``weight`` (nz,ny,nx) float32, 0 = never
    seen; ``color`` (nz,ny,nx,3) float32 or None."""

    def __init__(self, dims, origin, voxel, trunc=None, color=True, max_weight=MAX_WEIGHT, device=None):
        try:
            dims, origin = tuple(int(v) for v in dims), tuple(float(v) for v in origin)
            voxel, trunc, max_weight = float(voxel), TRUNC_VOXELS * float(voxel) if trunc is None else float(trunc), float(max_weight)
        except (TypeError, ValueError):
            raise _lib.RdmError("Volume: dims, origin, voxel, trunc and max_weight must be numbers, got %r, %r, %r, %r, %r" % (dims, origin, voxel, trunc, max_weight))
        if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise _lib.RdmError("Volume: dims must be three positive integers with a product of at most 2^31 - 1, got %r" % (dims,))
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin + (voxel, trunc)) or not (voxel > 0 and trunc > 0):
            raise _lib.RdmError("Volume: origin, voxel and trunc must be finite with voxel, trunc > 0, got %r, %r, %r" % (origin, voxel, trunc))
        if not max_weight > 0:
            raise _lib.RdmError("Volume: max_weight must be > 0, got %r" % (max_weight,))
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else torch.device("cpu" if device is None else device)
        if dev.type != "cuda":
            raise _lib.RdmError("fuse.Volume lives on the MI355X only; there is no CPU fallback")
        self.dims, self.origin, self.voxel, self.trunc, self.max_weight = dims, origin, voxel, trunc, max_weight
        nx, ny, nz = dims
        self.tsdf = torch.ones(nz, ny, nx, dtype=torch.float32, device=dev)
        self.weight = torch.zeros(nz, ny, nx, dtype=torch.float32, device=dev)
        self.color = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=dev) if color else None

    def geom(self):
        """the five doubles ox oy oz voxel trunc of include/rdm_fuse.h"""
        return (C.c_double * 5)(*(self.origin + (self.voxel, self.trunc)))

    def integrate(self, depth, intrinsics, poses, rgb=None, min_depth=0.0, max_depth=math.inf, weight=1.0):
        """``rdm_tsdf_integrate``: the planes updated in place from the frames of ``depth`` (B,h,w) float32 metres on the device, IN ORDER, in one
        launch.  ``intrinsics`` (fx, fy, cx, cy) of the frames (or a name in ``cloud.INTRINSICS``); ``poses`` map WORLD to camera coordinates,
        one for the batch or one per frame (``warp.pose_rows``; a tensor on the device is widened there and never visits the host); ``rgb``
        (B,h,w,3) uint8 on the device, required by a volume with colour; a pixel takes part iff its depth is finite, > 0 and inside
        [min_depth, max_depth]; ``weight`` is the weight of one observation.  Returns self."""
        src = cloud.intrinsics_params(intrinsics)
        if not (all(math.isfinite(v) for v in src) and src[0] != 0 and src[1] != 0):
            raise _lib.RdmError("intrinsics must be finite with fx and fy not 0, got %r" % (src,))
        if not (float(min_depth) >= 0 and float(max_depth) >= float(min_depth)):
            raise _lib.RdmError("need 0 <= min_depth <= max_depth, got %r and %r" % (min_depth, max_depth))
        if not (math.isfinite(float(weight)) and 0 < float(weight) <= self.max_weight):
            raise _lib.RdmError("weight must be finite, > 0 and at most max_weight %g, got %r" % (self.max_weight, weight))
        if self.color is not None and rgb is None:
            raise _lib.RdmError("this volume carries colour: integrate needs rgb, the frames' colours")
        d, (B, h, w) = _lib.device_depth(depth, "fuse.Volume.integrate")
        rgb = _lib.device_rgb(rgb, B, h, w) if self.color is not None else None
        if d.device != self.tsdf.device:
            raise _lib.RdmError("depth is on %s, the volume on %s" % (d.device, self.tsdf.device))
        if isinstance(poses, torch.Tensor) and poses.is_cuda:          # a pose on the device stays there (warp.render's rule)
            p = poses.detach().unsqueeze(0) if poses.dim() == 2 else poses.detach()
            if p.dim() != 3 or tuple(p.shape[1:]) not in ((3, 4), (4, 4)) or p.shape[0] not in (1, B) or p.device != d.device:
                raise _lib.RdmError("poses must be (3,4), (4,4), (%d,3,4) or (%d,4,4) on the depth's device, got %s" % (B, B, tuple(poses.shape)))
            rows = p.to(torch.float64)[:, :3, :].reshape(p.shape[0], 12).contiguous()
        else:
            rows = torch.from_numpy(warp.pose_rows(poses, B)).to(d.device)
        nx, ny, nz = self.dims
        _lib.check(_lib.lib().rdm_tsdf_integrate(_lib.ptr(d), _lib.ptr(rgb), B, h, w, (C.c_double * 4)(*src), _lib.ptr(rows), 12 if rows.shape[0] > 1 else 0,
                                                 float(min_depth), float(max_depth), float(weight), self.max_weight, nx, ny, nz, self.geom(), _lib.ptr(self.tsdf),
                                                 _lib.ptr(self.weight), _lib.ptr(self.color), _lib.stream()))
        return self

    def extract(self, normals=True, min_weight=MIN_WEIGHT):
        """``rdm_tsdf_extract``: (records, count).  The surface points of the volume in world coordinates, ``records`` a (count * record_bytes,)
        uint8 tensor on the device of ``cloud.record_bytes(normals, colour)``-byte records - x y z, the unit normal toward free space if
        ``normals``, r g b if the volume has colour - in row-major voxel order, from the voxels seen with a weight of at least ``min_weight``.
        Two calls: one that only counts, then - after ONE host synchronisation, the read of that count, which sizes the allocation - one that
        writes exactly ``count`` records.  Extraction is a once-per-sequence step."""
        if math.isnan(float(min_weight)):
            raise _lib.RdmError("min_weight must not be NaN")
        L = _lib.lib()
        nx, ny, nz = self.dims
        dev = self.tsdf.device
        ws_bytes = L.rdm_tsdf_extract_workspace_bytes(nx, ny, nz)
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)

        def call(records, capacity):
            _lib.check(L.rdm_tsdf_extract(_lib.ptr(self.tsdf), _lib.ptr(self.weight), _lib.ptr(self.color), nx, ny, nz, self.geom(), float(min_weight),
                                          1 if normals else 0, _lib.ptr(records), capacity, _lib.ptr(count), _lib.ptr(ws), ws_bytes, _lib.stream()))
        call(None, 0)
        n = int(count.item())                                               # the one host synchronisation
        records = torch.empty(n * cloud.record_bytes(normals, self.color is not None), dtype=torch.uint8, device=dev)
        if n:
            call(records, n)
        return records, n

    def write_ply(self, path, normals=True, min_weight=MIN_WEIGHT):
        """``extract`` into a binary little-endian PLY file (``cloud.write_ply``); returns the number of points"""
        records, n = self.extract(normals=normals, min_weight=min_weight)
        cloud.write_ply(path, records, n, normals, self.color is not None)
        return n
