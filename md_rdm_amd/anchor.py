"""Metric depth tied to measurements: a prediction plus a sparse or partial frame of metric depth of the same view (SLAM / SfM landmarks, a LiDAR
sweep, a ToF frame with holes) -> a per-image log scale fitted to the measurements and a smooth correction field that takes out the
low-frequency error the scale leaves (include/rdm_anchor.h, three launches).  ``fit`` runs the cell sums of the log residuals
(``rdm_depth_anchor_cells``) and the fit with the smoothed field (``rdm_depth_anchor_field``); ``metric_frames`` writes the frames with the field
interpolated at every pixel (``rdm_depth_frames_corrected``).  Nothing here copies to the host or synchronises.
"""
import ctypes as C
import math

import torch

from . import _lib, depth

FITS = ("logmean", "median", "none")
DEFAULTS = {"fit": "logmean", "cell": 16, "sigma": 2.0, "lam": 1.0, "reject": None, "min_depth": 0.0, "max_depth": math.inf, "field": True}


def check_params(cell, sigma, lam, reject):
    """None, or what is wrong with the numeric parameters (the ranges are the library's, include/rdm_anchor.h)"""
    if int(cell) < 1:
        return "cell must be >= 1 (got %r)" % (cell,)
    if not (math.isfinite(sigma) and sigma >= 0):
        return "sigma must be finite and >= 0 (got %r)" % (sigma,)
    if math.ceil(3.0 * sigma) > _lib.ANCHOR_MAX_RADIUS:
        return "sigma %r gives a tap radius ceil(3 * sigma) above %d" % (sigma, _lib.ANCHOR_MAX_RADIUS)
    if not (math.isfinite(lam) and lam >= 0):
        return "lambda must be finite and >= 0 (got %r)" % (lam,)
    if reject is not None and not reject > 0:
        return "reject must be > 0 and not NaN (got %r)" % (reject,)
    return None


def _map(log_map, who):
    if not isinstance(log_map, torch.Tensor) or not log_map.is_cuda:
        raise _lib.RdmError("%s runs on the MI355X only; there is no CPU fallback" % who)
    m = log_map.squeeze(1) if log_map.dim() == 4 and log_map.shape[1] == 1 else log_map
    if m.dim() != 3 or tuple(m.shape[1:]) != (128, 128) or m.dtype != torch.float64:
        raise _lib.RdmError("log_map must be (B,1,128,128) or (B,128,128) float64, got %s %s" % (log_map.dtype, tuple(log_map.shape)))
    return m.detach().contiguous()


def _per_sample(t, B, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or t.numel() != B:
        raise _lib.RdmError("%s must be (B,) float64 on the device" % name)
    return t.detach().reshape(B).contiguous()


def view_rows(h, w, view):
    """(y0, x0, y1, x1): the pixels of an (h, w) frame whose centre lies inside ``view`` = (vy0, vx0, vh, vw), as a crop of
    rdm_eval_standard_view_f64; None when there is none.  The comparisons are rdm_anchor.h's, in float64."""
    vy0, vx0, vh, vw = (float(v) for v in view)

    def span(n, v0, v1):
        inside = [i for i in range(n) if v0 <= i + 0.5 < v1]
        return (inside[0], inside[-1] + 1) if inside else None
    ys, xs = span(h, vy0, vy0 + vh), span(w, vx0, vx0 + vw)
    return None if ys is None or xs is None else (ys[0], xs[0], ys[1], xs[1])


def median_log_scale(log_map, anchors, view=None, prior=None, min_depth=0.0, max_depth=math.inf):
    """(B,) float64 on the device: ln of the ratio of medians, median(a_valid) / median(exp(v)_valid) - column 11 of
    ``rdm_eval_standard_view_f64`` under ``align = MEDIAN`` with the anchors as the depth, the statistic ``evaluate --align median`` uses.
    Valid is that entry point's rule (finite, min_depth < a < max_depth: the limits themselves are excluded) among the pixels whose centre is
    inside the view (passed as its crop).  A sample without a valid anchor has a row of zeros there: its value is its ``prior`` (or 0), never
    ln 0.  One launch, and the logarithm is formed on the device."""
    m = _map(log_map, "anchor.median_log_scale")
    a, (B, h, w) = _lib.device_depth(anchors, "anchor.median_log_scale")
    if B != m.shape[0]:
        raise _lib.RdmError("anchors must have log_map's batch %d, got %d" % (m.shape[0], B))
    p = _per_sample(prior, B, "prior")
    base = p if p is not None else torch.zeros(B, dtype=torch.float64, device=m.device)
    if not 0 <= float(min_depth) < float(max_depth):
        raise _lib.RdmError("fit median needs 0 <= min_depth < max_depth, got %r, %r" % (min_depth, max_depth))
    crop = None
    if view is not None:
        crop = view_rows(h, w, view)
        if crop is None:                                  # no pixel inside the view: no anchor anywhere
            return base.clone()
    L = _lib.lib()
    need = L.rdm_eval_standard_workspace_bytes(B, h, w)
    ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=m.device)
    rows = torch.empty(B, 16, dtype=torch.float64, device=m.device)
    _lib.check(L.rdm_eval_standard_view_f64(_lib.ptr(m), _lib.ptr(a), 0, B, h, w, _lib.EVAL_ALIGN["median"], float(min_depth), float(max_depth),
                                            (C.c_int32 * 4)(*crop) if crop is not None else None,
                                            (C.c_double * 4)(*(float(t) for t in view)) if view is not None else None, _lib.ptr(rows), None, _lib.ptr(ws),
                                            ws.numel() * 8, _lib.stream()))
    has = rows[:, 0] > 0
    return torch.where(has, torch.log(torch.where(has, rows[:, 11], torch.ones_like(base))), base)


def fit(log_map, anchors, view=None, prior=None, fit="logmean", cell=16, sigma=2.0, lam=1.0, reject=None, min_depth=0.0, max_depth=math.inf, field=True):
    """{"log_scale": (B,) float64, "count": (B,) int32, "field": (B,gy,gx) float64 or None, "cell": int} on the device.
    ``log_map`` (B,1,128,128) float64 from ``predict``; ``anchors`` (B,h,w) float32 metres in the output frame's geometry, a pixel without a
    measurement 0 (or anything not finite, not positive or outside [min_depth, max_depth]); ``view`` = (vy0, vx0, vh, vw), the rectangle of the
    frame the map covers (anchors outside it are ignored); ``prior`` (B,) float64 log scale per sample, e.g. ``depth.sid_log_scale``.
    ``fit``: "logmean" - the mean log residual of the anchors against the prior-scaled prediction is added to the prior; "none" - the prior
    stands; "median" - the prior is REPLACED by ``median_log_scale`` (the ratio of medians; a sample without a valid anchor keeps its prior, or
    0) and stands.  ``reject`` (log units) drops anchors whose residual against the prior exceeds it; it needs a prior or fit "median".
    The field is the residuals left after the fit, summed over cells of ``cell`` pixels and smoothed over ``sigma`` cells by a normalised
    convolution; ``lam`` (in anchors) pulls it to 0 where there is little evidence.  ``field=False``: the scale alone."""
    if fit not in FITS:
        raise _lib.RdmError("fit %r is not one of %s" % (fit, ", ".join(FITS)))
    m = _map(log_map, "anchor.fit")
    a, (B, h, w) = _lib.device_depth(anchors, "anchor.fit")
    if B != m.shape[0]:
        raise _lib.RdmError("anchors must have log_map's batch %d, got %d" % (m.shape[0], B))
    bad = check_params(cell, float(sigma), float(lam), None if reject is None else float(reject))
    if bad:
        raise _lib.RdmError("anchor.fit: " + bad)
    cell = int(cell)
    gy, gx = -(-h // cell), -(-w // cell)
    if field and gy * gx > _lib.ANCHOR_MAX_CELLS:
        raise _lib.RdmError("anchor.fit: %d x %d cells is beyond the %d of rdm_depth_anchor_field; use a larger cell" % (gy, gx, _lib.ANCHOR_MAX_CELLS))
    p = _per_sample(prior, B, "prior")
    if fit == "median":
        p = median_log_scale(m, a, view=view, prior=p, min_depth=min_depth, max_depth=max_depth)
    if reject is not None and p is None:
        raise _lib.RdmError("anchor.fit: reject needs a prior (or fit='median') to gate against")
    L = _lib.lib()
    v = (C.c_double * 4)(*(float(t) for t in view)) if view is not None else None
    n = torch.empty(B, gy, gx, dtype=torch.int32, device=m.device)
    s = torch.empty(B, gy, gx, dtype=torch.float64, device=m.device)
    _lib.check(L.rdm_depth_anchor_cells(_lib.ptr(m), _lib.ptr(a), _lib.ptr(p), B, h, w, v, cell, float(min_depth), float(max_depth),
                                        math.inf if reject is None else float(reject), _lib.ptr(n), _lib.ptr(s), _lib.stream()))
    ls = torch.empty(B, dtype=torch.float64, device=m.device)
    count = torch.empty(B, dtype=torch.int32, device=m.device)
    F = torch.empty(B, gy, gx, dtype=torch.float64, device=m.device) if field else None
    _lib.check(L.rdm_depth_anchor_field(_lib.ptr(n), _lib.ptr(s), _lib.ptr(p), B, gy, gx, _lib.ANCHOR_FIT["logmean" if fit == "logmean" else "none"], float(sigma),
                                        float(lam), _lib.ptr(ls), _lib.ptr(count), _lib.ptr(F), _lib.stream()))
    return {"log_scale": ls, "count": count, "field": F, "cell": cell}


def metric_frames(log_map, frame_hw, fitted, view=None, unit=1e-3, outside="zero", want=("f32",)):
    """``rdm_depth_frames_corrected``: ``depth.metric_frames``' dict for D = exp((v + log_scale) + field interpolated at the pixel), with
    ``fitted`` the dict of ``fit`` for a frame of ``frame_hw``.  Without a field (``fit(field=False)``) it is ``depth.metric_frames`` with the
    fitted log scale."""
    ls, F = fitted["log_scale"], fitted["field"]
    if F is None:
        return depth.metric_frames(log_map, frame_hw, view=view, log_scale=ls, unit=unit, outside=outside, want=want)
    m = _map(log_map, "anchor.metric_frames")
    B, (h, w), cell = m.shape[0], (int(frame_hw[0]), int(frame_hw[1])), int(fitted["cell"])
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in ("f32", "u16", "log_scale") for k in want) or not ("f32" in want or "u16" in want):
        raise _lib.RdmError("want %r: name f32, u16 and / or log_scale, at least one of the two planes" % (want,))
    if outside not in _lib.DEPTH_OUTSIDE:
        raise _lib.RdmError("outside %r is not one of %s" % (outside, ", ".join(_lib.DEPTH_OUTSIDE)))
    if h < 1 or w < 1 or cell < 1:
        raise _lib.RdmError("frame_hw and cell must be positive, got %s, %d" % ((h, w), cell))
    ls = _per_sample(ls, B, "fitted['log_scale']")
    if not isinstance(F, torch.Tensor) or not F.is_cuda or F.dtype != torch.float64 or tuple(F.shape) != (B, -(-h // cell), -(-w // cell)):
        raise _lib.RdmError("fitted['field'] must be (%d,%d,%d) float64 on the device for a %dx%d frame at cell %d, got %s %s" % (
            B, -(-h // cell), -(-w // cell), h, w, cell, getattr(F, "dtype", type(F)), tuple(getattr(F, "shape", ()))))
    F = F.detach().contiguous()
    v = (C.c_double * 4)(*(float(t) for t in view)) if view is not None else None
    f32 = torch.empty(B, h, w, dtype=torch.float32, device=m.device) if "f32" in want else None
    u16 = torch.empty(B, h, w, dtype=torch.uint16, device=m.device) if "u16" in want else None
    so = torch.empty(B, dtype=torch.float64, device=m.device) if "log_scale" in want else None
    _lib.check(_lib.lib().rdm_depth_frames_corrected(_lib.ptr(m), None, 0, _lib.ptr(ls), None, B, h, w, v, _lib.DEPTH_OUTSIDE[outside], float(unit), _lib.ptr(f32),
                                                     _lib.ptr(u16), _lib.ptr(so), 0, _lib.ptr(F), F.shape[1], F.shape[2], cell, _lib.stream()))
    out = {}
    if f32 is not None:
        out["f32"] = f32
    if u16 is not None:
        out["u16"] = u16
    if so is not None:
        out["log_scale"] = so
    return out
