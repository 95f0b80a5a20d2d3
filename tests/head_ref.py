"""Plain float64 references of the head (DORN pair softmax, ordinal loss) and of the pyramid nodes (fine-detail prediction, candidate
mat-vec, recombination) with their gradients, for tests/test_head_ref_cpu.py and tests/test_gpu_head_grads.py.  numpy / torch on the CPU only;
what oracle/computations_cpu.py already restates is used from there, the rest follows the same formulas (computations.py:394-421, :512-528,
loss.py:8-59, RDM_Net.py:313-345).  Every gradient comes with S_abs, the sum of the absolute values of the terms behind each output: the
tolerances of the GPU tests are written in terms of it."""
import math

import numpy as np
import torch

from oracle import computations_cpu as ocp

F32_LO, F32_HI = np.float32(1e-8), np.float32(1e4)           # the DORN clamp bounds, as float32 (RDM_Net.py:334 clamps a float32 tensor)


def level_off(k):
    """first element of level k in a packed pyramid [d_0 (1x1) | F_1 (2x2) | ...]"""
    return ((1 << (2 * k)) - 1) // 3


def split_levels(packed, n_levels, first_level=0):
    """(B, level_off(n_levels)) -> [(B,1,s,s) for the levels first_level .. n_levels-1]"""
    p = np.asarray(packed)
    return [p[:, level_off(k):level_off(k + 1)].reshape(p.shape[0], 1, 1 << k, 1 << k) for k in range(first_level, n_levels)]


def pack_levels(levels, n_levels, first_level=0, fill=0.0, dtype=np.float64):
    B = levels[0].shape[0]
    out = np.full((B, level_off(n_levels)), fill, dtype=dtype)
    for k, l in zip(range(first_level, n_levels), levels):
        out[:, level_off(k):level_off(k + 1)] = np.asarray(l).reshape(B, -1)
    return out


# ----------------------------------------------------------------------------------
# DORN head
# ----------------------------------------------------------------------------------
def dorn_gate(x):
    """where the float32 clamp passes the gradient: lo <= x <= hi, equality included"""
    x = np.asarray(x, dtype=np.float32)
    return (x >= F32_LO) & (x <= F32_HI)


def dorn(x):
    """-> (decode int64 (B,1,H,W), P float64 (B,K,H,W))"""
    return ocp.dorn_ordinal_regression(x)


def dorn_backward64(x, gP):
    """gradient of sum(P * gP) w.r.t. the logits BEFORE the rounding to float32, and the gate"""
    x = np.asarray(x, dtype=np.float32)
    _, P = ocp.dorn_ordinal_regression(x)
    t = np.asarray(gP, dtype=np.float64) * P * (1.0 - P)
    dx = np.zeros(x.shape, dtype=np.float64)
    dx[:, 1::2] = t
    dx[:, 0::2] = -t
    gate = dorn_gate(x)
    return np.where(gate, dx, 0.0), gate


def dorn_backward(x, gP):
    """-> (dx float32, gate)"""
    return ocp.dorn_backward(x, gP), dorn_gate(x)


# ----------------------------------------------------------------------------------
# ordinal loss
# ----------------------------------------------------------------------------------
def _ordinal_q(P, target):
    P = np.asarray(P, dtype=np.float64)
    K = P.shape[1]
    lower = np.broadcast_to(np.arange(K, dtype=np.int64).reshape(1, K, 1, 1) <= np.asarray(target).astype(np.int64), P.shape)
    return lower, np.where(lower, P, 1.0 - P)


def ordinal_loss(P, target):
    """loss.py:8-59 with every sum in float64: -(sum log float32(clamp(q))) / (N*H*W), q = P where k <= target and 1 - P elsewhere.
    The logarithm is the float64 one of the float32 argument; the reference's float32 log and sums sit within their own rounding of it."""
    N, _, H, W = np.asarray(P).shape
    _, q = _ordinal_q(P, target)
    arg = np.clip(q, 1e-8, 1e8).astype(np.float32).astype(np.float64)
    return -math.fsum(np.log(arg).ravel()) / (N * H * W)


def ordinal_loss_gate(P, target):
    _, q = _ordinal_q(P, target)
    return (q >= 1e-8) & (q <= 1e8)


def ordinal_loss_grad(P, target, dloss=1.0):
    """-> (dP float64, gate): the float32 reciprocal of the reference's float32 log backward, scaled by dloss"""
    return dloss * ocp.ordinal_loss_grad(np.asarray(P, dtype=np.float64), np.asarray(target)), ordinal_loss_gate(P, target)


# ----------------------------------------------------------------------------------
# pyramid nodes
# ----------------------------------------------------------------------------------
def log32(levels):
    """float64(float32(log L)): what make_pred's ``.float()`` leaves of a level's logarithm"""
    return [np.log(np.asarray(l, dtype=np.float64)).astype(np.float32).astype(np.float64) for l in levels]


def fine_detail_pred(levels, w):
    """yhat_k = float32(log L_k) * w_k (float32 weights, product in float64: the float32 product is within half an ulp of it)"""
    return [l * float(np.float32(np.asarray(wk).reshape(-1)[0])) for l, wk in zip(log32(levels), w)]


def fine_detail_pred_grad(levels, dyhat):
    """dw_k = sum_{b,j} dyhat_k * float64(float32(log L_k)) -> (dw, S_abs), one entry per level"""
    dw, s_abs = [], []
    for l, d in zip(log32(levels), dyhat):
        t = (np.asarray(d, dtype=np.float64).reshape(l.shape) * l).ravel()
        dw.append(math.fsum(t))
        s_abs.append(math.fsum(np.abs(t)))
    return np.array(dw), np.array(s_abs)


def candidates_matvec(A, w):
    """out[b,m] = sum_k float32(A[b,k,m]) * w[k] -> (out (B,M), S_abs (B,M))"""
    A32 = np.asarray(A, dtype=np.float64).astype(np.float32).astype(np.float64)
    t = A32 * np.asarray(w, dtype=np.float32).astype(np.float64).reshape(1, -1, 1)
    return t.sum(axis=1), np.abs(t).sum(axis=1)


def candidates_matvec_grad(A, dout):
    """dw[k] = sum_{b,m} dout[b,m] * float32(A[b,k,m]) -> (dw (K,), S_abs (K,))"""
    A32 = np.asarray(A, dtype=np.float64).astype(np.float32).astype(np.float64)
    t = A32 * np.asarray(dout, dtype=np.float64)[:, None, :]
    K = A32.shape[1]
    return (np.array([math.fsum(t[:, k].ravel()) for k in range(K)]), np.array([math.fsum(np.abs(t[:, k]).ravel()) for k in range(K)]))


def _upsample(t, n):
    for _ in range(n):
        t = t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return t


def _recombine_torch(levels, n_out, first_level):
    """the reference's order: d_0 + ((c_1 + c_2) + ...) with level 0, (c_f + c_{f+1}) + ... without"""
    ups = [_upsample(l, n_out - k) for k, l in zip(range(first_level, first_level + len(levels)), levels)]
    rest = ups[1:] if first_level == 0 else ups
    r = None
    for u in rest:
        r = u if r is None else r + u
    if first_level == 0:
        r = ups[0] if r is None else ups[0] + r
    return r


def recombine(yhat_levels, n_out, first_level=0):
    """sum of the nearest-upsampled levels at side 2^n_out -> (out (B,1,S,S) float64, S_abs the same sum of absolute values)"""
    lv = [torch.from_numpy(np.ascontiguousarray(np.asarray(l, dtype=np.float64))) for l in yhat_levels]
    return _recombine_torch(lv, n_out, first_level).numpy(), _recombine_torch([l.abs() for l in lv], n_out, first_level).numpy()


def block_sums(dout, k):
    """adjoint of the nearest upsampling to level k: sums of dout (B,1,S,S) over the (S / 2^k)-square footprints -> (B,1,2^k,2^k)"""
    d = np.asarray(dout, dtype=np.float64)
    B, S, s = d.shape[0], d.shape[2], 1 << k
    f = S // s
    return d.reshape(B, s, f, s, f).sum(axis=(2, 4)).reshape(B, 1, s, s)


def recombine_grad(level_shapes, dout, n_out, first_level=0):
    """d sum(out * dout) / d yhat_k by torch float64 autograd through repeat_interleave -> ([dyhat_k], [S_abs_k])"""
    lv = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in level_shapes]
    d = torch.from_numpy(np.ascontiguousarray(np.asarray(dout, dtype=np.float64)))
    (_recombine_torch(lv, n_out, first_level) * d).sum().backward()
    s_abs = [block_sums(np.abs(np.asarray(dout, dtype=np.float64)), k) for k in range(first_level, first_level + len(lv))]
    return [l.grad.numpy() for l in lv], s_abs


# ----------------------------------------------------------------------------------
# edge inputs shared by the CPU and the GPU tests
# ----------------------------------------------------------------------------------
def dorn_planted_pairs():
    """(a, b) float32 logit pairs on and around the clamp bounds (the gate is >= / <=: torch's clamp backward passes at equality)"""
    f = np.float32
    lo, hi, inf = F32_LO, F32_HI, f(np.inf)
    return [(lo, f(0.75)), (f(0.3), lo), (hi, f(1.0)), (f(2.0), hi), (lo, hi),                          # exactly on a bound
            (np.nextafter(lo, -inf), f(0.5)), (f(0.5), np.nextafter(lo, inf)),                          # the float32 neighbours of 1e-8f
            (np.nextafter(hi, -inf), f(0.5)), (f(0.5), np.nextafter(hi, inf)),                          # ... and of 1e4f
            (f(1.25), f(1.25)),                                                                         # P = 0.5 exactly: not counted
            (f(1.0), np.nextafter(f(1.0), inf)), (np.nextafter(f(1.0), inf), f(1.0)),                   # neighbouring floats
            (f(-3.0), f(0.5)), (f(0.5), f(-1e-8)), (f(2e4), f(0.25)), (f(0.25), f(2e4))]


def dorn_inputs(filler, B, K, H, W):
    """list of (B,2K,H,W) float32 logits carrying every planted pair; one tensor where the pairs fit, several for the smallest shapes.
    The pairs are spread evenly from the first to the last (b, k, pixel), so the tail of the grid-stride loop holds some."""
    pairs, npairs = dorn_planted_pairs(), B * K * H * W
    out = []
    for g0 in range(0, len(pairs), npairs):
        group = pairs[g0:g0 + npairs]
        x = filler.uniform(f"hg.dorn.{B}x{K}x{H}x{W}", (B, 2 * K, H, W), -2.0, 3.0)
        pos = np.unique(np.linspace(0, npairs - 1, len(group)).astype(np.int64)) if len(group) > 1 else np.array([0])
        assert len(pos) == len(group)
        for j, (a, b) in zip(pos, group):
            bi, k, h, w = np.unravel_index(int(j), (B, K, H, W))
            x[bi, 2 * k, h, w], x[bi, 2 * k + 1, h, w] = a, b
        out.append(x)
    return out


ORDINAL_P = (0.0, 1.0, 1e-8, 5e-9, 1.0 - 1e-8, 0.5)


def ordinal_targets(K):
    """labels on and outside [0, K): -2**31 is what depth2label_sid gives a non-positive depth by default"""
    return (0, K - 1, K, 95, -1, -2 ** 31)


def ordinal_inputs(filler, B, K, H, W):
    """list of (P (B,K,H,W) float64, T (B,1,H,W) int32) carrying every planted probability under every planted label"""
    tv, npix, n = ordinal_targets(K), B * H * W, B * K * H * W
    key = f"hg.ol.{B}x{K}x{H}x{W}"
    if npix < 2 * len(tv):
        out = []
        for t in tv:
            for p in ORDINAL_P:
                P = filler.uniform(key + ".p", (B, K, H, W), 0.0, 1.0, dtype=np.float64)
                T = np.floor(filler.uniform(key + ".t", (B, 1, H, W), 0, K)).astype(np.int32)
                P.flat[0], T.flat[0] = p, t
                out.append((P, T))
        return out
    P = filler.uniform(key + ".p", (B, K, H, W), 0.0, 1.0, dtype=np.float64)
    T = np.floor(filler.uniform(key + ".t", (B, 1, H, W), 0, K)).astype(np.int32)
    pix = np.linspace(0, npix - 1, 2 * len(tv)).astype(np.int64)
    assert len(np.unique(pix)) == len(pix)
    for j, i in enumerate(pix):
        T.flat[i] = tv[j % len(tv)]
    idx = np.arange(0, n, 7)
    P.flat[idx] = np.array(ORDINAL_P)[np.arange(len(idx)) % len(ORDINAL_P)]
    for j, i in enumerate(pix):                                    # every planted label sees planted probabilities at both ends of its column
        b, r = divmod(int(i), H * W)
        P[b, 0].flat[r], P[b, K - 1].flat[r] = ORDINAL_P[j % 6], ORDINAL_P[(j + 3) % 6]
    P.flat[n - 1] = 1e-8
    return [(P, T)]
