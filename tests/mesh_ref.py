"""include/rdm_mesh.h restated in numpy: the face bytes and the counts rdm_depth_mesh must write.  Validity is cloud_ref's; the only arithmetic
is float64 subtraction, fabs and ONE float64 multiplication (numpy contracts nothing); everything else is comparisons and integer counting."""
import numpy as np

import cloud_ref as cref

LAYOUTS = {"i32": 0, "ply": 1}


def face_bytes(layout):
    return {"i32": 12, "ply": 13}[layout]


def sample_faces(depth, min_depth=0.0, max_depth=np.inf, step=1, edge_ratio=1.05):
    """one (h,w) sample -> dict: "faces" (n,3) int32 in the header's order, "vertex_count", and what the tests ask about the cells:
    "valid" (sh,sw) bool, "index" (sh,sw) int64 vertex index (-1: invalid), "cell" (n,) flat cell number of every face, "cand" (n,) 0 | 1,
    "ad" (sh-1,sw-1) bool: the diagonal, "cut" (sh-1,sw-1,2) bool: candidates with three valid corners that the edge test removed"""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    d = depth[::step, ::step]
    valid = cref.valid_mask(depth, min_depth, max_depth)[::step, ::step]
    sh, sw = valid.shape
    index = np.where(valid, np.cumsum(valid.reshape(-1)).reshape(sh, sw) - 1, -1).astype(np.int64)
    out = {"valid": valid, "index": index, "vertex_count": int(valid.sum())}
    if sh < 2 or sw < 2:
        out.update(faces=np.zeros((0, 3), np.int32), cell=np.zeros(0, np.int64), cand=np.zeros(0, np.int64), ad=np.zeros((max(sh - 1, 0), max(sw - 1, 0)), bool),
                   cut=np.zeros((max(sh - 1, 0), max(sw - 1, 0), 2), bool))
        return out
    corner = lambda a: (a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:])
    dA, dB, dC, dD = corner(d)
    vA, vB, vC, vD = corner(valid)
    iA, iB, iC, iD = corner(index)
    f64 = lambda a: a.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ad = vA & vD & (~(vB & vC) | (np.abs(f64(dA) - f64(dD)) <= np.abs(f64(dB) - f64(dC))))

        def passes(a, b, c):                            # only read where the three are valid
            lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
            return f64(hi) <= f64(lo) * np.float64(edge_ratio)
        # candidate c of every cell: its corners' validity, its edge test and its indices, by diagonal
        three = np.stack([np.where(ad, vA & vC & vD, vA & vC & vB), np.where(ad, vA & vD & vB, vB & vC & vD)], axis=-1)
        edge = np.stack([np.where(ad, passes(dA, dC, dD), passes(dA, dC, dB)), np.where(ad, passes(dA, dD, dB), passes(dB, dC, dD))], axis=-1)
    tri = np.stack([np.stack([np.where(ad, iA, iA), np.where(ad, iC, iC), np.where(ad, iD, iB)], axis=-1),
                    np.stack([np.where(ad, iA, iB), np.where(ad, iD, iC), np.where(ad, iB, iD)], axis=-1)], axis=-2)        # (sh-1, sw-1, 2, 3)
    emit = three & edge
    cells = np.arange((sh - 1) * (sw - 1), dtype=np.int64).reshape(sh - 1, sw - 1, 1).repeat(2, 2)
    cands = np.zeros((sh - 1, sw - 1, 2), np.int64)
    cands[..., 1] = 1
    out.update(faces=tri[emit].astype(np.int32), cell=cells[emit], cand=cands[emit], ad=ad, cut=three & ~edge)      # boolean indexing is row-major: cell, then candidate
    return out


def pack(faces, layout):
    """(n,3) int32 -> the record bytes of a layout"""
    tri = np.ascontiguousarray(faces, dtype="<i4").view(np.uint8).reshape(-1, 12)
    if layout == "ply":
        tri = np.concatenate([np.full((len(tri), 1), 3, np.uint8), tri], axis=1)
    else:
        assert layout == "i32"
    return tri.tobytes()


def unpack(data, layout):
    """record bytes -> (n,3) int32; asserts the PLY count bytes"""
    a = np.frombuffer(data, dtype=np.uint8).reshape(-1, face_bytes(layout))
    if layout == "ply":
        assert (a[:, 0] == 3).all()
        a = a[:, 1:]
    return a.copy().view("<i4").reshape(-1, 3)


def reference(depth, min_depth=0.0, max_depth=np.inf, step=1, edge_ratio=1.05, layout="i32"):
    """(B,h,w) float32 -> ([face bytes of sample b], (B,) int32 face counts, (B,) int32 vertex counts)"""
    depth = np.asarray(depth, dtype=np.float32)
    recs, fc, vc = [], [], []
    for b in range(depth.shape[0]):
        s = sample_faces(depth[b], min_depth, max_depth, step, edge_ratio)
        recs.append(pack(s["faces"], layout))
        fc.append(len(s["faces"]))
        vc.append(s["vertex_count"])
    return recs, np.asarray(fc, dtype=np.int32), np.asarray(vc, dtype=np.int32)


def loops(depth, min_depth=0.0, max_depth=np.inf, step=1, edge_ratio=1.05):
    """the same contract as plain loops over one (h,w) sample -> (n,3) int32: an independent second statement the vectorised one is tested against"""
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    d = depth[::step, ::step]
    v = cref.valid_mask(depth, min_depth, max_depth)[::step, ::step]
    sh, sw = v.shape
    idx, n = {}, 0
    for i in range(sh):
        for j in range(sw):
            if v[i, j]:
                idx[(i, j)] = n
                n += 1
    faces = []
    for i in range(sh - 1):
        for j in range(sw - 1):
            A, B, C, D = (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
            ad = v[A] and v[D] and (not (v[B] and v[C]) or abs(float(d[A]) - float(d[D])) <= abs(float(d[B]) - float(d[C])))
            for tri in (((A, C, D), (A, D, B)) if ad else ((A, C, B), (B, C, D))):
                if all(v[p] for p in tri):
                    z = [d[p] for p in tri]
                    if float(max(z)) <= float(min(z)) * float(edge_ratio):      # Python floats are IEEE float64
                        faces.append([idx[p] for p in tri])
    return np.asarray(faces, dtype=np.int32).reshape(-1, 3)
