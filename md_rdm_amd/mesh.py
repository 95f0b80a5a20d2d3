"""A surface a mesh tool can open: the pixel grid of a metric depth frame (``depth.metric_frames``, or any sensor depth in metres) triangulated,
two triangles per cell along the diagonal of the smaller depth difference, and the triangles that span a depth discontinuity or touch a pixel
without a measurement left out (``rdm_depth_mesh``, include/rdm_mesh.h: two launches, plain stores, faces in row-major cell order).  The vertices
are ``cloud.point_cloud``'s records for the same validity arguments - a face's indices are record numbers - and ``write_ply`` puts both into one
binary PLY file.  One intrinsics set per call, no texture coordinates, vertices without a face stay in the file, no hole filling and no
simplification.  The default ``edge_ratio`` of 1.05 is a starting point only: no trained checkpoint and no dataset were at hand, so its effect has
not been measured.
"""
import math

import torch

from . import _lib, cloud

EDGE_RATIO = 1.05                                   # a starting point, not a measured optimum (module docstring)


def face_bytes(layout):
    """size of one face record: "i32": three little-endian int32; "ply": the byte 3 in front of them (PLY ``list uchar int``)"""
    if layout not in _lib.MESH_FACES:
        raise _lib.RdmError("layout %r is not one of %s" % (layout, ", ".join(_lib.MESH_FACES)))
    return 13 if layout == "ply" else 12


def faces(depth, min_depth=0.0, max_depth=math.inf, step=1, edge_ratio=EDGE_RATIO, layout="i32"):
    """``rdm_depth_mesh``: (faces, face_counts, vertex_counts).  ``depth`` (B,h,w) float32 metres on the device.  Validity and ``step`` are
    ``cloud.point_cloud``'s; cell (i, j) of the sampled grid has the corners A = (i, j), B = (i, j+1), C = (i+1, j), D = (i+1, j+1) and is cut along
    AD when A and D are valid and |dA - dD| <= |dB - dC| (or B, C are not both valid), along BC otherwise; a triangle is kept iff its three corners
    are valid and max depth <= min depth * ``edge_ratio`` (inf: every triangle of valid corners).  ``faces`` (B, stride) uint8: sample b's first
    face_counts[b] * face_bytes(layout) bytes are its faces in row-major cell order, the rest of its row is not written; the indices are record
    numbers of ``point_cloud(depth, ..., min_depth, max_depth, step)``; ``face_counts``, ``vertex_counts`` (B,) int32.  The workspace is
    allocated per call."""
    d, (B, h, w) = _lib.device_depth(depth, "mesh.faces")
    rec = face_bytes(layout)
    step = int(step)
    if step < 1:
        raise _lib.RdmError("step must be positive, got %d" % step)
    L = _lib.lib()
    stride = 2 * (-(-h // step) - 1) * (-(-w // step) - 1) * rec
    buf = torch.empty(max(B * stride, 1), dtype=torch.uint8, device=d.device)      # a frame without cells (one sampled row or column) still passes a pointer
    fcounts = torch.empty(B, dtype=torch.int32, device=d.device)
    vcounts = torch.empty(B, dtype=torch.int32, device=d.device)
    ws_bytes = L.rdm_depth_mesh_workspace_bytes(B, h, w, step)
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=d.device)
    _lib.check(L.rdm_depth_mesh(_lib.ptr(d), B, h, w, float(min_depth), float(max_depth), step, float(edge_ratio), _lib.MESH_FACES[layout],
                                _lib.ptr(buf), stride, _lib.ptr(fcounts), _lib.ptr(vcounts), _lib.ptr(ws), ws_bytes, _lib.stream()))
    return buf[:B * stride].view(B, stride), fcounts, vcounts


def depth_mesh(depth, intrinsics, rgb=None, normals=False, min_depth=0.0, max_depth=math.inf, step=1, edge_ratio=EDGE_RATIO):
    """``cloud.point_cloud`` and ``faces(layout="ply")`` of one frame with the same validity arguments: (records, vertex_counts, faces,
    face_counts) - the two payloads of ``write_ply``."""
    records, vcounts = cloud.point_cloud(depth, intrinsics, rgb=rgb, normals=normals, min_depth=min_depth, max_depth=max_depth, step=step)
    tri, fcounts, _ = faces(depth, min_depth=min_depth, max_depth=max_depth, step=step, edge_ratio=edge_ratio, layout="ply")
    return records, vcounts, tri, fcounts


def ply_header(vcount, fcount, normals, colour):
    """``cloud.ply_header``'s vertex element followed by a face element of ``fcount`` index lists"""
    head = cloud.ply_header(vcount, normals, colour).decode("ascii").split("\n")
    assert head[-2:] == ["end_header", ""]
    return ("\n".join(head[:-2] + ["element face %d" % fcount, "property list uchar int vertex_indices", "end_header"]) + "\n").encode("ascii")


def _prefix(what, data, n):
    if isinstance(data, torch.Tensor):
        if data.dtype != torch.uint8 or data.dim() != 1:
            raise ValueError("write_ply: %s must be one sample's (stride,) uint8 row, got %s %s" % (what, data.dtype, tuple(data.shape)))
        payload = data[:n].cpu().numpy().tobytes()
    else:
        payload = bytes(memoryview(data)[:n])
    if n < 0 or len(payload) != n:
        raise ValueError("write_ply: %s must hold %d bytes, got %d" % (what, n, len(payload)))
    return payload


def write_ply(path, records, vcount, normals, colour, faces, fcount):
    """A binary little-endian PLY file of ``vcount`` vertices and ``fcount`` triangles: the header, the first vcount * cloud.record_bytes(normals,
    colour) bytes of ``records`` and the first fcount * 13 bytes of ``faces`` ("ply" layout), both verbatim.  ``records`` / ``faces``: one sample's
    row of ``depth_mesh`` (uint8 tensors on the device or the host; only the used prefixes are copied), or bytes."""
    vcount, fcount = int(vcount), int(fcount)
    vertices = _prefix("records", records, vcount * cloud.record_bytes(normals, colour))
    triangles = _prefix("faces", faces, fcount * 13)
    with open(path, "wb") as fh:
        fh.write(ply_header(vcount, fcount, normals, colour))
        fh.write(vertices)
        fh.write(triangles)
