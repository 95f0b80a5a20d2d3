"""Depth maps a person can look at: the reference's ``colored_depthmap`` / ``merge_into_row`` / ``save_image`` (utils.py:71-117) on this stack.

``colorize`` and ``comparison_rows`` render on the device in ONE launch per batch (``rdm_viz_rows_u8``, include/rdm_viz.h): bicubic resize to the
output size, the colour range, matplotlib's jet table and the packing to uint8 RGB happen inside, and the result is byte for byte what the
reference's functions give after ``astype('uint8')``.  ``write_png`` is the one write path for pictures: 8-bit RGB with the standard library only
(Pillow is optional in this project and may be absent where the product runs); ``write_png16`` beside it writes a 16-bit greyscale plane, the
format of metric depth maps (md_rdm_amd.depth).
"""
import struct
import zlib

import torch

from . import _lib

_NAN = float("nan")


def _map(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.RdmError("%s: rendering runs on the MI355X only; there is no CPU fallback" % what)
    if t.dim() == 3:
        t = t.unsqueeze(1)
    if t.dim() != 4 or t.shape[1] != 1 or t.dtype not in (torch.float32, torch.float64):
        raise _lib.RdmError("%s must be (B,1,h,w) or (B,h,w) float32 / float64, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def render_rows(x, target, pred, h, w, d_min=None, d_max=None, split=0):
    """``rdm_viz_rows_u8``: (B,h,P*w,3) uint8 device tensor, panels [x | target | pred] with ``x`` and ``target`` optional.  ``d_min`` /
    ``d_max``: the colour range; None takes that end from the data, per image and shared by the image's depth panels."""
    b = _map(pred, "pred")
    a = _map(target, "target") if target is not None else None
    B = b.shape[0]
    if x is not None:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _lib.RdmError("x: rendering runs on the MI355X only; there is no CPU fallback")
        if tuple(x.shape) != (B, 3, h, w) or x.dtype != torch.float32:
            raise _lib.RdmError("x must be (%d,3,%d,%d) float32, got %s %s" % (B, h, w, x.dtype, tuple(x.shape)))
        x = x.detach().contiguous()
    if a is not None and a.shape[0] != B:
        raise _lib.RdmError("target and pred differ in batch size: %d, %d" % (a.shape[0], B))
    panels = (x is not None) + (a is not None) + 1
    out = torch.empty(B, h, panels * w, 3, dtype=torch.uint8, device=b.device)
    ha, wa = (a.shape[2], a.shape[3]) if a is not None else (0, 0)
    _lib.check(_lib.lib().rdm_viz_rows_u8(_lib.ptr(x), _lib.ptr(a), int(a is not None and a.dtype == torch.float64), ha, wa, _lib.ptr(b),
                                          int(b.dtype == torch.float64), b.shape[2], b.shape[3], B, h, w, _NAN if d_min is None else float(d_min),
                                          _NAN if d_max is None else float(d_max), _lib.ptr(out), int(split), _lib.stream()))
    return out


def colorize(maps, d_min=None, d_max=None, size=None):
    """utils.py:71-77 for a batch: (B,1,h,w) maps -> (B,H,W,3) uint8 jet images on the device.  ``size=(H, W)``: bicubic resize first (default:
    the maps' own size).  Without ``d_min`` / ``d_max`` every image is coloured over its own minimum / maximum."""
    m = _map(maps, "maps")
    h, w = (m.shape[2], m.shape[3]) if size is None else (int(size[0]), int(size[1]))
    return render_rows(None, None, m, h, w, d_min, d_max)


def comparison_rows(x, target, pred, d_min=None, d_max=None):
    """utils.py:80-91 for a batch: (B,H,3W,3) uint8 rows [input | target | prediction] at the input's size, both maps resized to it and coloured
    over ONE range per image (their joint minimum / maximum unless given).  ``target=None`` gives two panels, (B,H,2W,3)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.RdmError("comparison_rows: rendering runs on the MI355X only; there is no CPU fallback")
    if x.dim() != 4:
        raise _lib.RdmError("x must be (B,3,H,W) float32, got %s" % (tuple(x.shape),))
    return render_rows(x, target, pred, x.shape[2], x.shape[3], d_min, d_max)


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, array):
    """(H,W,3) uint8 (numpy array or tensor, host or device) -> 8-bit RGB PNG, every scan line with filter 0.  Standard library only."""
    import numpy as np
    a = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: need a uint8 (H,W,3) array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape[:2]
    raw = np.zeros((h, 1 + 3 * w), dtype=np.uint8)                    # filter byte 0 + the line
    raw[:, 1:] = a.reshape(h, 3 * w)
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(data)


def read_png16(path):
    """16-bit greyscale PNG (colour type 0, not interlaced: what ``write_png16`` and depth sensors' tools write) -> (H,W) uint16.  Standard
    library only; every scan-line filter of the format (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) is undone."""
    import numpy as np
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_png16: %s is not a PNG file" % path)
    at, head, idat = 8, None, []
    while at + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        at += 12 + n
    if head is None or head[2:] != (16, 0, 0, 0, 0):
        raise ValueError("read_png16: %s is not a 16-bit greyscale, non-interlaced PNG (IHDR %r)" % (path, head))
    w, h = head[0], head[1]
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + 2 * w):
        raise ValueError("read_png16: %s holds %d bytes of image data, %d expected" % (path, raw.size, h * (1 + 2 * w)))
    raw = raw.reshape(h, 1 + 2 * w)
    out = np.zeros((h, 2 * w), dtype=np.uint8)
    prev = np.zeros(2 * w, dtype=np.int64)
    for y in range(h):
        f, line = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        elif f == 1:                                                 # Sub: the byte two to the left, i.e. a running sum per byte lane
            cur = (np.cumsum(line.reshape(w, 2), axis=0) & 255).reshape(-1)
        elif f in (3, 4):
            cur = np.zeros(2 * w, dtype=np.int64)
            for i in range(2 * w):
                a, b, c = (int(cur[i - 2]), int(prev[i]), int(prev[i - 2])) if i >= 2 else (0, int(prev[i]), 0)
                if f == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
                cur[i] = (int(line[i]) + pred) & 255
        else:
            raise ValueError("read_png16: %s: scan line %d has the unknown filter %d" % (path, y, f))
        out[y] = cur
        prev = cur
    return out.view(">u2").astype(np.uint16).reshape(h, w)


def write_png16(path, array):
    """(H,W) uint16 (numpy array or tensor, host or device) -> 16-bit greyscale PNG (colour type 0, big-endian samples), every scan line with
    filter 0: the interchange format of depth maps (``depth.metric_frames``' "u16" plane: steps of ``unit`` metres, 0 = no measurement).
    Standard library only."""
    import numpy as np
    a = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.ndim != 2 or a.dtype != np.uint16 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png16: need a uint16 (H,W) array, got %s %s" % (a.dtype, a.shape))
    h, w = a.shape
    raw = np.zeros((h, 1 + 2 * w), dtype=np.uint8)                    # filter byte 0 + the line
    raw[:, 1:] = a.astype(">u2").view(np.uint8).reshape(h, 2 * w)
    data = b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)) + _chunk(b"IEND", b"")
    with open(path, "wb") as fh:
        fh.write(data)
