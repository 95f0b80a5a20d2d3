"""Depth a downstream tool can read: metres per pixel, in the geometry of the frame that went in, as float32 and as the 16-bit plane of a
depth PNG.  ``predict`` gives a (B,1,128,128) map of log RELATIVE depth (normalised by its geometric mean); the absolute estimate the network
carries is the d_1 DORN head, trained against ``depth2label_sid`` of the metric target (module.py:135-143).  ``metric_frames`` takes the map and
the head's label counts to metric frames in ONE launch (``rdm_depth_frames``, include/rdm_depth.h): the mean log depth of the labels under the
reference's ``get_depth_sid`` (utils.py:120-156) as the scale, the map resampled over the rectangle of the frame the network saw
(``dataloaders.nyu.test_view``), ``exp``, and the quantisation to ``unit`` metres per step.
"""
import ctypes as C
import math

import torch

from . import _lib

# alpha (metres of label 0), beta (metres of label K), K: the four parameter sets of the reference's get_depth_sid / get_labels_sid
SID = {
    "nyu": (0.02, 10.0, 90.0),
    "kitti": (0.001, 80.0, 71.0),
    "floorplan3d": (0.0552, 10.0, 68.0),
    "Structured3D": (0.02, 10.0, 68.0),
}


def sid_params(sid):
    """(alpha, beta, K) floats of a name in ``SID`` or of a triple"""
    if isinstance(sid, str):
        if sid not in SID:
            raise _lib.RdmError("sid %r is not one of %s" % (sid, ", ".join(SID)))
        return SID[sid]
    alpha, beta, K = (float(v) for v in sid)
    return alpha, beta, K


def sid_log_scale_value(total, count_n, sid="nyu", offset=0.0):
    """The float64 formula of include/rdm_depth.h on the host, for one sample whose ``count_n`` labels sum to ``total``:
    log(alpha) + log(beta / alpha) * (total / count_n + offset) / K, evaluated in that order."""
    alpha, beta, K = sid_params(sid)
    x = float(int(total)) / float(count_n)
    x = x + float(offset)
    x = math.log(beta / alpha) * x
    x = x / K
    return math.log(alpha) + x


def _counts(counts, B):
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda:
        raise _lib.RdmError("counts: the metric scale runs on the MI355X only; there is no CPU fallback")
    if counts.dtype != torch.int64 or counts.dim() < 1 or (B is not None and counts.shape[0] != B) or counts[0].numel() < 1:
        raise _lib.RdmError("counts must be (B,...) int64 label counts, got %s %s" % (counts.dtype, tuple(counts.shape)))
    return counts.detach().reshape(counts.shape[0], -1).contiguous()


def sid_log_scale(counts, sid="nyu", offset=0.0):
    """(B,) float64 on the device: per sample the mean over the head of log(get_depth_sid(label + offset)) - linear in the label, so the exact
    integer sum of the counts in ``sid_log_scale_value``'s formula, each step one IEEE float64 operation: bit for bit ``scale_out`` of
    rdm_depth_frames for the same counts."""
    alpha, beta, K = sid_params(sid)
    c = _counts(counts, None)
    def dev(v):                         # a divisor on the device: torch divides by a HOST scalar through its reciprocal, which is not the quotient
        return torch.full((1,), float(v), dtype=torch.float64, device=c.device)
    x = c.sum(dim=1).to(torch.float64) / dev(c.shape[1])
    x = x + float(offset)
    x = x * math.log(beta / alpha)
    x = x / dev(K)
    return x + math.log(alpha)


def metric_frames(log_map, frame_hw, view=None, counts=None, log_scale=None, sid="nyu", offset=0.0, unit=1e-3, outside="zero", want=("f32",), split=0):
    """``rdm_depth_frames``: {"f32": (B,h,w) float32 metres, "u16": (B,h,w) uint16 steps of ``unit`` metres, "log_scale": (B,) float64}, whichever
    of them ``want`` names (at least one of the two planes), in one launch.
    ``log_map`` (B,1,128,128) float64 from ``predict``; ``frame_hw`` the output frame; ``view`` = (vy0, vx0, vh, vw), the rectangle of that frame
    the map covers (None: all of it); ``counts`` the DORN counts of ``predict(return_counts=True)``: scale from ``sid`` (a name in ``SID`` or
    (alpha, beta, K)) at ``offset`` (0: lower bin edge, 0.5: bin centre); ``log_scale`` (B,) float64, added to it.  With neither, the frame
    is exp of the resampled map.  ``outside``: "zero" - pixels whose centre is outside the view are 0, no measurement - or "edge"."""
    if not isinstance(log_map, torch.Tensor) or not log_map.is_cuda:
        raise _lib.RdmError("metric_frames runs on the MI355X only; there is no CPU fallback")
    m = log_map.squeeze(1) if log_map.dim() == 4 and log_map.shape[1] == 1 else log_map
    if m.dim() != 3 or tuple(m.shape[1:]) != (128, 128) or m.dtype != torch.float64:
        raise _lib.RdmError("log_map must be (B,1,128,128) or (B,128,128) float64, got %s %s" % (log_map.dtype, tuple(log_map.shape)))
    m = m.detach().contiguous()
    B, (h, w) = m.shape[0], (int(frame_hw[0]), int(frame_hw[1]))
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in ("f32", "u16", "log_scale") for k in want) or not ("f32" in want or "u16" in want):
        raise _lib.RdmError("want %r: name f32, u16 and / or log_scale, at least one of the two planes" % (want,))
    if outside not in _lib.DEPTH_OUTSIDE:
        raise _lib.RdmError("outside %r is not one of %s" % (outside, ", ".join(_lib.DEPTH_OUTSIDE)))
    if h < 1 or w < 1:
        raise _lib.RdmError("frame_hw must be positive, got %s" % ((h, w),))
    c = _counts(counts, B) if counts is not None else None
    par = (C.c_double * 4)(*sid_params(sid), float(offset)) if c is not None else None
    ls = None
    if log_scale is not None:
        if not isinstance(log_scale, torch.Tensor) or not log_scale.is_cuda or log_scale.dtype != torch.float64 or log_scale.numel() != B:
            raise _lib.RdmError("log_scale must be (B,) float64 on the device")
        ls = log_scale.detach().reshape(B).contiguous()
    v = (C.c_double * 4)(*(float(t) for t in view)) if view is not None else None
    f32 = torch.empty(B, h, w, dtype=torch.float32, device=m.device) if "f32" in want else None
    u16 = torch.empty(B, h, w, dtype=torch.uint16, device=m.device) if "u16" in want else None
    so = torch.empty(B, dtype=torch.float64, device=m.device) if "log_scale" in want else None
    _lib.check(_lib.lib().rdm_depth_frames(_lib.ptr(m), _lib.ptr(c), c.shape[1] if c is not None else 0, _lib.ptr(ls), par, B, h, w, v, _lib.DEPTH_OUTSIDE[outside],
                                           float(unit), _lib.ptr(f32), _lib.ptr(u16), _lib.ptr(so), int(split), _lib.stream()))
    out = {}
    if f32 is not None:
        out["f32"] = f32
    if u16 is not None:
        out["u16"] = u16
    if so is not None:
        out["log_scale"] = so
    return out
