"""Late-producer harness for tests/test_gpu_streams.py: does an entry point order ALL its device work on the stream it is handed?

The null stream hides ordering mistakes, so every case runs like this (`late_run`):

 1. every input, output and workspace tensor exists beforehand (allocated on the null stream by the case's builder) and is filled with POISON -
    NaN for f32 / f64, 0xFFFF for bf16 (a NaN too), bytes of 0xEE for integers, bytes and argmax buffers (no label, count, tap index or image
    the library produces is 0xEE.. everywhere) - then `torch.cuda.synchronize()`;
 2. on a non-default stream S (`Delay.S`: created fresh for the module and PROVEN to run beside the null stream - see `_concurrent_stream`), with no host synchronisation in between: a DELAY kernel, the copies of the real inputs from pre-staged device
    copies into the poisoned input buffers, a second poison fill of every output / workspace / internally zeroed accumulator (so a memset the entry
    point owes is seen to be ordered on S), the call itself under `with torch.cuda.stream(S)` with `_lib.stream()` as its stream argument (so the
    wrapper that resolves the caller's stream is exercised by every case), copies of every output into `snap` tensors, `S.synchronize()`;
 3. `snap` is compared with what the same call computed on the null stream from the same inputs (`reference_run`).

Work that escapes to another stream runs during the delay: it reads poison, or its result is snapshotted before it exists, or it is overwritten by
the late poison fill.  Detection rests on the poison, not on a tolerance: outputs without float atomics are compared BIT FOR BIT (poisoned padding
columns included); the few that accumulate with float atomics are compared at the tolerance their own parity test states, and must be finite.

The delay is measured, not assumed (`Delay`): `torch.cuda._sleep` is calibrated once per module with events, and a case sleeps for
max(FLOOR_MS, MULTIPLE x the case's own null-stream time).  Values on the MI355X this was written on: 1 ms = ~2.4e6 sleep cycles (the spin kernel
counts shader clocks), FLOOR_MS = 5, MULTIPLE = 20; the operator cases take 0.01 .. 0.03 ms on the null stream, so they sleep the 5 ms floor; a training step (118 ms) sleeps 2.35 s.
That these values suffice is shown by a CONTROL per family (`late_run(..., wrong_stream=True)`): the same sequence with the call deliberately made
on the NULL stream must come out different from the reference and must contain poison.  The control only reads and writes valid buffers in the wrong
order; a control that does not detect fails the module (it never skips).
"""
import contextlib

import torch

FLOOR_MS = 5.0
MULTIPLE = 20.0

_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_INT_POISON = {torch.uint8: 0xEE, torch.int8: -0x12, torch.int16: -0x1112, torch.int32: -0x11111112, torch.int64: -0x1111111111111112}


def poison_(t):
    """fill `t` with its dtype's poison on the current stream"""
    if t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(-1)                          # 0xFFFF
    elif t.dtype.is_floating_point:
        t.fill_(float("nan"))
    else:
        t.fill_(_INT_POISON[t.dtype])
    return t


def has_poison(t):
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).any())
    return bool((t == _INT_POISON[t.dtype]).any())


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(_INT_VIEW[a.element_size()]), b.contiguous().view(_INT_VIEW[b.element_size()]))


class Case:
    """One call of one entry point.
    ins      {name: tensor} the values every buffer the call READS must hold when it starts (accumulators the CALLER zeroes included)
    scratch  {name: tensor} buffers the call only writes, or initialises itself: outputs, workspaces, accumulators the entry point zeroes
    const    {name: tensor} tables outside the data flow (quantiser levels, augmentation draws): never poisoned
    call     f(bufs, stream_handle) -> None | {name: tensor} (results a product wrapper allocated itself)
    outs     names in bufs that are compared (results returned by `call` are always compared)
    tol      {name: rtol of max|ref| - or ("each", rtol): of every element - } for outputs summed with float atomics, in the form the entry point's own
             parity test states it; everything else is compared bit for bit"""

    def __init__(self, ins, call, outs=(), scratch=None, const=None, tol=None):
        self.staged = {k: v.contiguous() for k, v in ins.items()}
        self.scratch = dict(scratch or {})
        self.bufs = {k: torch.empty_like(v) for k, v in self.staged.items()}
        self.bufs.update(self.scratch)
        self.const = dict(const or {})
        self.call, self.outs, self.tol = call, tuple(outs), dict(tol or {})
        self.null_ms = None

    def all_bufs(self):
        d = dict(self.const)
        d.update(self.bufs)
        return d


class Delay:
    """`torch.cuda._sleep` calibrated with events (a chain of matmuls on scratch tensors where this torch has no _sleep)."""

    def __init__(self, dev):
        self.dev = dev
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.a = torch.randn(1024, 1024, device=dev)
        self.b = torch.empty_like(self.a)
        unit = 1_000_000 if self.sleep is not None else 8
        self._spin(unit)                                                   # warm-up (module load)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._spin(unit)
        e1.record()
        torch.cuda.synchronize()
        self.units_per_ms = unit / max(e0.elapsed_time(e1), 1e-3)
        self.S = self._concurrent_stream()

    def second_stream(self):
        """another stream, proven to run beside the null stream AND beside `S` (for the two-streams-at-once test)"""
        return self._concurrent_stream(others=(self.S,))

    def _concurrent_stream(self, others=()):
        """A non-default stream that is PROVEN to run beside the null stream.  The runtime multiplexes its streams onto a few hardware queues
        (4 by default); a stream that shares the null stream's queue executes in submission order with it, and behind it a call that escaped to
        the null stream would look correct.  So: sleep on a fresh stream, run a fill on the null stream, and keep the stream only if the fill
        finished while the sleep was still running."""
        probe = torch.zeros(64, device=self.dev)
        for _ in range(32):
            S = torch.cuda.Stream()
            beside = True
            for other in (torch.cuda.default_stream(),) + tuple(others):
                torch.cuda.synchronize()
                with torch.cuda.stream(S):
                    self.enqueue(20.0)
                with torch.cuda.stream(other):
                    probe.add_(1.0)
                other.synchronize()
                beside = beside and not S.query()
                S.synchronize()
            if beside:
                return S
        raise AssertionError("no non-default stream ran beside the null stream: the late-producer tests would prove nothing")

    def _spin(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            for _ in range(int(units)):
                torch.mm(self.a, self.a, out=self.b)

    def ms_for(self, null_ms):
        return max(FLOOR_MS, MULTIPLE * null_ms)

    def enqueue(self, ms):
        """on the current stream; allocates nothing"""
        self._spin(max(1, int(ms * self.units_per_ms)))


def reference_run(case):
    """the call on the null stream from the real inputs (outputs / workspaces poisoned first); run twice, the second run timed for the case's delay"""
    from md_rdm_amd import _lib
    null = torch.cuda.default_stream()
    with torch.cuda.stream(null):
        for _ in range(2):                                                 # (the first call of a kernel pays its module load)
            for k, v in case.staged.items():
                case.bufs[k].copy_(v)
            for t in case.scratch.values():
                poison_(t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            extra = case.call(case.all_bufs(), _lib.stream()) or {}
            e1.record()
        ref = {k: case.bufs[k].clone() for k in case.outs}
        ref.update({k: v.detach().clone() for k, v in extra.items()})
    torch.cuda.synchronize()
    case.null_ms = e0.elapsed_time(e1)
    return ref


def late_run(case, delay, wrong_stream=False, stream=None):
    """steps 1-2 of the module docstring -> snap.  wrong_stream: the CONTROL - the call is made on the null stream instead of S."""
    from md_rdm_amd import _lib
    for t in case.bufs.values():
        poison_(t)
    torch.cuda.synchronize()
    S = stream if stream is not None else delay.S              # (one stream for the module: the one proven to run beside the null stream)
    ms = delay.ms_for(case.null_ms if case.null_ms is not None else 0.0)
    with torch.cuda.stream(S):
        delay.enqueue(ms)
        for k, v in case.staged.items():
            case.bufs[k].copy_(v, non_blocking=True)
        for t in case.scratch.values():
            poison_(t)
        ctx = torch.cuda.stream(torch.cuda.default_stream()) if wrong_stream else contextlib.nullcontext()
        with ctx:
            extra = case.call(case.all_bufs(), _lib.stream()) or {}
        snap = {k: case.bufs[k].clone() for k in case.outs}
        snap.update({k: v.detach().clone() for k, v in extra.items()})
    if stream is None:
        S.synchronize()
        torch.cuda.synchronize()              # (the control's null-stream work too, before any buffer is reused)
    return snap


def mismatches(case, snap, ref):
    """names of the outputs of `snap` that do not meet the comparison against `ref`"""
    bad = []
    assert set(snap) == set(ref) and snap, (sorted(snap), sorted(ref))
    for k in ref:
        if k in case.tol:
            # float atomics: the order of the adds differs from run to run; tolerance = the entry point's own parity test (named where the row is defined)
            s, r, tol = snap[k].double(), ref[k].double(), case.tol[k]
            if not bool(torch.isfinite(s).all()):
                bad.append(k)
            elif isinstance(tol, tuple):                                    # ("each", rtol): numpy.testing.assert_allclose(rtol=...) per element
                if bool(((s - r).abs() > tol[1] * r.abs()).any()):
                    bad.append(k)
            elif float((s - r).abs().max()) > tol * max(float(r.abs().max()), 1e-300):
                bad.append(k)
        elif not same_bits(snap[k], ref[k]):
            bad.append(k)
    return bad


def check(case, delay):
    """reference on the null stream, then the late producer on the module's non-default stream (`Delay.S`): every output must match"""
    ref = reference_run(case)
    snap = late_run(case, delay)
    bad = mismatches(case, snap, ref)
    assert not bad, "outputs %s differ from the null-stream run (delay %.1f ms, null-stream time %.3f ms)" % (bad, delay.ms_for(case.null_ms), case.null_ms)
    return ref


def control(case, delay):
    """the same sequence with the call on the NULL stream must be detected: different from the reference, and poisoned"""
    ref = reference_run(case)
    snap = late_run(case, delay, wrong_stream=True)
    bad = mismatches(case, snap, ref)
    poisoned = [k for k, v in snap.items() if has_poison(v) and not has_poison(ref[k])]
    ms = delay.ms_for(case.null_ms)
    print("control: delay %.1f ms (null-stream time %.3f ms): differing %s, poisoned %s" % (ms, case.null_ms, bad, poisoned))
    assert bad and poisoned, "a call on the wrong stream went undetected with a delay of %.1f ms (differing %s, poisoned %s)" % (ms, bad, poisoned)
    return ms
