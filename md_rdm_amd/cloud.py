"""Points a mesh or point-cloud tool can open: a metric depth frame (``depth.metric_frames``, or any sensor depth in metres) unprojected through
pinhole intrinsics to packed vertex records - position, optionally a unit normal facing the camera, optionally the pixel's colour - with the
invalid pixels dropped and the rest in row-major order, in ONE launch (``rdm_depth_cloud``, include/rdm_cloud.h), and the binary PLY file around
those records.  One intrinsics set per call, no lens distortion, and no depth-edge rejection for the normals: a normal across a depth step is
the normal of the step (the faces of ``md_rdm_amd.mesh``, which index these records, do reject depth edges).
"""
import ctypes as C
import math

import torch

from . import _lib

# fx, fy, cx, cy of the raw frame.  "nyu": the NYU Depth v2 toolbox's RGB camera parameters (camera_params.m) as remembered when this was
# written; they could not be checked against the toolbox then, so verify them before relying on them.  An explicit intrinsics tuple
# (--intrinsics on the command line) always takes their place.
INTRINSICS = {
    "nyu": (518.85790117450188, 519.46961112127485, 325.58244941119034, 253.73616633400465),
}


def intrinsics_params(intrinsics):
    """(fx, fy, cx, cy) floats of a name in ``INTRINSICS`` or of a 4-tuple"""
    if isinstance(intrinsics, str):
        if intrinsics not in INTRINSICS:
            raise _lib.RdmError("camera %r is not one of %s" % (intrinsics, ", ".join(INTRINSICS)))
        return INTRINSICS[intrinsics]
    vals = tuple(float(v) for v in intrinsics)
    if len(vals) != 4:
        raise _lib.RdmError("intrinsics must be (fx, fy, cx, cy), got %r" % (intrinsics,))
    return vals


def record_bytes(normals, colour):
    """size of one record: x y z float32, nx ny nz float32 if ``normals``, r g b uint8 if ``colour``"""
    return 12 + (12 if normals else 0) + (3 if colour else 0)


def intrinsics_in_view(intr, view, hw):
    """Intrinsics of the raw frame -> intrinsics of an (H, W) frame that shows the rectangle ``view`` = (vy0, vx0, vh, vw) of it (the convention of
    include/rdm_eval_view.h: pixel centres at +0.5, the view's edges the frame's edges): fx' = fx * W / vw, cx' = (cx + 0.5 - vx0) * W / vw - 0.5,
    likewise in y."""
    fx, fy, cx, cy = intrinsics_params(intr)
    vy0, vx0, vh, vw = (float(v) for v in view)
    H, W = float(hw[0]), float(hw[1])
    if not (vh > 0 and vw > 0 and H > 0 and W > 0):
        raise _lib.RdmError("intrinsics_in_view: view %r and frame %r must have positive extent" % (tuple(view), tuple(hw)))
    return (fx * W / vw, fy * H / vh, (cx + 0.5 - vx0) * W / vw - 0.5, (cy + 0.5 - vy0) * H / vh - 0.5)


def point_cloud(depth, intrinsics, rgb=None, normals=False, min_depth=0.0, max_depth=math.inf, step=1, split=0):
    """``rdm_depth_cloud``: (records, counts).  ``depth`` (B,h,w) float32 metres on the device; ``intrinsics`` (fx, fy, cx, cy) of that frame (or a
    name in ``INTRINSICS``); ``rgb`` (B,h,w,3) uint8 on the device, or None.  A pixel is kept iff its depth is finite, > 0 and inside
    [min_depth, max_depth], and y % step == 0 and x % step == 0.  ``records`` (B, stride) uint8: sample b's first counts[b] * record_bytes(normals,
    rgb is not None) bytes are its records in row-major pixel order, the rest of its row is not written; ``counts`` (B,) int32."""
    d, (B, h, w) = _lib.device_depth(depth, "point_cloud")
    rgb = _lib.device_rgb(rgb, B, h, w)
    step = int(step)
    if step < 1:
        raise _lib.RdmError("step must be positive, got %d" % step)
    intr = (C.c_double * 4)(*intrinsics_params(intrinsics))
    stride = -(-h // step) * -(-w // step) * record_bytes(normals, rgb is not None)
    records = torch.empty(B, stride, dtype=torch.uint8, device=d.device)
    counts = torch.empty(B, dtype=torch.int32, device=d.device)
    _lib.check(_lib.lib().rdm_depth_cloud(_lib.ptr(d), _lib.ptr(rgb), B, h, w, intr, float(min_depth), float(max_depth), step, 1 if normals else 0,
                                          _lib.ptr(records), stride, _lib.ptr(counts), int(split), _lib.stream()))
    return records, counts


def ply_header(count, normals, colour):
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % count, "property float x", "property float y", "property float z"]
    if normals:
        lines += ["property float nx", "property float ny", "property float nz"]
    if colour:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path, records, count, normals, colour):
    """A binary little-endian PLY file of ``count`` vertices: the header, then the first count * record_bytes(normals, colour) bytes of ``records``
    verbatim.  ``records``: one sample's row of ``point_cloud`` (a uint8 tensor on the device or the host; only the used prefix is copied), or bytes."""
    count = int(count)
    n = count * record_bytes(normals, colour)
    if isinstance(records, torch.Tensor):
        if records.dtype != torch.uint8 or records.dim() != 1:
            raise ValueError("write_ply: records must be one sample's (stride,) uint8 row, got %s %s" % (records.dtype, tuple(records.shape)))
        payload = records[:n].cpu().numpy().tobytes()
    else:
        payload = bytes(memoryview(records)[:n])
    if count < 0 or len(payload) != n:
        raise ValueError("write_ply: %d records of %d bytes need %d bytes, got %d" % (count, record_bytes(normals, colour), n, len(payload)))
    with open(path, "wb") as fh:
        fh.write(ply_header(count, normals, colour))
        fh.write(payload)
