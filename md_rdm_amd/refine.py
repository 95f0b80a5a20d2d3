"""Depth edges where the colour edges are: a metric depth frame (``depth.metric_frames``, or any sensor depth in metres) filtered by a joint
(cross) bilateral filter under the colour frame it belongs to, in ONE launch (``rdm_depth_refine``, include/rdm_refine.h).  The frames of
``metric_frames`` are a bicubic enlargement of a 128x128 map, so every depth edge in them is a ramp several pixels wide: blur in a depth PNG,
a sheet of points between foreground and background in a point cloud.  A tap whose colour differs from the pixel's gets little weight, so the
ramp's pixels take the depth of the side their colour belongs to; with ``fill`` the pixels without a measurement take the weighted mean of
their valid taps.  One pass, no depth-range term, no iteration.

The default parameters are a starting point only: no trained checkpoint and no dataset were at hand when this was written, so their effect on
depth accuracy has NOT been measured.
"""
import math

import torch

from . import _lib

MAX_RADIUS, MAX_STEP, MAX_HALO = 8, 16, 24          # the limits of include/rdm_refine.h
DEFAULTS = dict(radius=3, step=4, sigma_space=None, sigma_color=12.0, fill=False)


def check_params(radius, step, sigma_space, sigma_color):
    """the ranges of include/rdm_refine.h -> an error text, or None.  ``sigma_space`` None: radius * step / 2."""
    if not 1 <= radius <= MAX_RADIUS:
        return "radius must be in [1, %d] (got %d)" % (MAX_RADIUS, radius)
    if not 1 <= step <= MAX_STEP:
        return "step must be in [1, %d] (got %d)" % (MAX_STEP, step)
    if radius * step > MAX_HALO:
        return "radius * step must not exceed %d (got %d * %d)" % (MAX_HALO, radius, step)
    if sigma_space is not None and not sigma_space > 0:
        return "sigma_space must be positive (got %r)" % (sigma_space,)
    if not sigma_color > 0:
        return "sigma_color must be positive (got %r)" % (sigma_color,)
    return None


def joint_bilateral(depth, guide, radius=3, step=4, sigma_space=None, sigma_color=12.0, fill=False, unit=1e-3, want=("f32",)):
    """``rdm_depth_refine``: {"f32": (B,h,w) float32 metres, "u16": (B,h,w) uint16 steps of ``unit`` metres}, whichever of them ``want`` names, in one
    launch.  ``depth`` (B,h,w) or (B,1,h,w) float32 metres on the device; a depth is valid iff it is finite and > 0.  ``guide`` (B,h,w,3) uint8 on
    the device, the colour frame of the same geometry.  The taps of a pixel are the (2 radius + 1)^2 pixels at multiples of ``step`` around it
    (radius <= 8, step <= 16, radius * step <= 24); a tap's weight is exp(-distance^2 / (2 sigma_space^2)) times
    exp(-(dR^2 + dG^2 + dB^2) / (2 sigma_color^2)) of the guide's byte differences, and the result is the weighted mean of the valid taps.
    ``sigma_space`` None: radius * step / 2; math.inf for either sigma switches that term off.  ``fill``: a pixel whose own depth is not valid
    takes the mean of its valid taps (0 when it has none) instead of staying 0.
    The defaults are a starting point only; their effect on depth accuracy has not been measured."""
    if not isinstance(depth, torch.Tensor) or not depth.is_cuda:
        raise _lib.RdmError("joint_bilateral runs on the MI355X only; there is no CPU fallback")
    d = depth.squeeze(1) if depth.dim() == 4 and depth.shape[1] == 1 else depth
    if d.dim() != 3 or d.dtype != torch.float32 or d.numel() == 0:
        raise _lib.RdmError("depth must be (B,h,w) or (B,1,h,w) float32, got %s %s" % (depth.dtype, tuple(depth.shape)))
    B, h, w = d.shape
    if not isinstance(guide, torch.Tensor) or not guide.is_cuda:
        raise _lib.RdmError("guide must be on the device; there is no CPU fallback")
    if guide.dtype != torch.uint8 or tuple(guide.shape) != (B, h, w, 3):
        raise _lib.RdmError("guide must be (%d,%d,%d,3) uint8, got %s %s" % (B, h, w, guide.dtype, tuple(guide.shape)))
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in ("f32", "u16") for k in want):
        raise _lib.RdmError("want %r: name f32 and / or u16" % (want,))
    radius, step = int(radius), int(step)
    sigma_color = float(sigma_color)
    sigma_space = None if sigma_space is None else float(sigma_space)
    bad = check_params(radius, step, sigma_space, sigma_color)
    if bad:
        raise _lib.RdmError("joint_bilateral: " + bad)
    if sigma_space is None:
        sigma_space = radius * step / 2.0
    unit = float(unit)
    if not (unit > 0 and math.isfinite(unit)):
        raise _lib.RdmError("joint_bilateral: unit must be finite and positive (got %r)" % unit)
    d = d.detach().contiguous()
    g = guide.detach().contiguous()
    f32 = torch.empty(B, h, w, dtype=torch.float32, device=d.device) if "f32" in want else None
    u16 = torch.empty(B, h, w, dtype=torch.uint16, device=d.device) if "u16" in want else None
    _lib.check(_lib.lib().rdm_depth_refine(_lib.ptr(d), _lib.ptr(g), B, h, w, radius, step, sigma_space, sigma_color, 1 if fill else 0, unit, _lib.ptr(f32),
                                           _lib.ptr(u16), _lib.stream()))
    out = {}
    if f32 is not None:
        out["f32"] = f32
    if u16 is not None:
        out["u16"] = u16
    return out
