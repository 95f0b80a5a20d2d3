"""Float64 restatements of the weight average (include/rdm_ema.h, harness.ema_decay_at) for tests/test_ema_cpu.py, tests/test_gpu_ema.py and the
data-parallel child.  numpy only.

The update is ema + (1 - d)(w - ema) with the FLOAT32-rounded 1 - d (the kernel's host side forms 1.f - d in float32), everything else in float64.
The bound the GPU tests apply to T successive float32 steps against this replay, fed the float32 weights the kernel stored: each step has three
float32 roundings - the difference w - ema (at most 2 M in magnitude, M the largest magnitude among the weights and averages seen), the product
with 1 - d <= 1, and the sum (at most M: a convex combination) - each below 2^-24 relative, so a step adds below (2 + 2 + 1) 2^-24 M = 5 x 2^-24 M,
and the error carried in from earlier steps only contracts, by d.  After T steps: 5 T 2^-24 M absolute."""
import numpy as np

F32 = np.float32


def one_minus(decay):
    """1.f - decay as float32 arithmetic gives it, as a float64"""
    return np.float64(F32(1.0) - F32(decay))


def ema_step(ema, w, decay):
    """one update in float64: ema, w arrays (any float dtype) -> float64"""
    e, w = np.asarray(ema, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return e + one_minus(decay) * (w - e)


def ema_replay(ema0, weights, decays):
    """ema0 advanced through the float32 post-step weights `weights[t]` with `decays[t]` -> (float64 average, M)"""
    e = np.asarray(ema0, dtype=np.float64)
    M = float(np.abs(e).max()) if e.size else 0.0
    for w, d in zip(weights, decays):
        e = ema_step(e, w, d)
        if e.size:
            M = max(M, float(np.abs(np.asarray(w, dtype=np.float64)).max()), float(np.abs(e).max()))
    return e, M


def bound(T, M):
    return 5.0 * T * 2.0 ** -24 * M


def decay_at(decay, updates, warmup=True):
    """harness.ema_decay_at restated: float64, rounded once to float32"""
    d = np.float64(decay)
    if warmup:
        d = min(d, (np.float64(1.0) + np.float64(updates)) / (np.float64(10.0) + np.float64(updates)))
    return float(F32(d))
