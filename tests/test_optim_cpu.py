"""Gradient accumulation and global-norm clipping without a GPU: the C-ABI boundary of include/rdm_optim.h (declared == bound == exported; every
refusal is a status code with a message before any launch; the workspace size), train.py's two flags, and the window bookkeeping of
harness.train_epoch driven with a stub optimiser that records what it is asked to do."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rdm_optim.h")
NAMES = {"rdm_grad_accumulate_f32", "rdm_grad_sumsq_workspace_bytes", "rdm_grad_sumsq_f64", "rdm_adamw_fused_clip"}


def lib():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


# ---- the C ABI of include/rdm_optim.h --------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    text = open(HEADER).read()
    assert set(_lib.symbols("rdm_optim.h")) == NAMES        # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    for name in NAMES:
        assert name not in hip_h                                                                # rdm_hip.h keeps its declaration set
    assert '#include "rdm_hip.h"' in text
    # the clipped step takes rdm_adamw_fused's arguments, then sumsq, n_slots, max_norm, coef_out - and the stream stays last
    plain, clip = _lib.HEADERS["rdm_hip.h"]["rdm_adamw_fused"][1], _lib.HEADERS["rdm_optim.h"]["rdm_adamw_fused_clip"][1]
    assert clip[:len(plain) - 1] == plain[:-1] and clip[len(plain) - 1:] == [_lib.vp, _lib.i32, _lib.f32, _lib.vp, _lib.vp]
    for macro, value in (("RDM_GRAD_ACC_COPY", _lib.GRAD_ACC_COPY), ("RDM_GRAD_ACC_ADD", _lib.GRAD_ACC_ADD), ("RDM_CLIP_MAX_SLOTS", _lib.CLIP_MAX_SLOTS)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value


def test_sumsq_workspace_bytes():
    _, L = lib()
    W = L.rdm_grad_sumsq_workspace_bytes
    sizes = [0, 1, 3, 4, 255, 1024, 1025, 2 ** 20 + 5, 2 * 2097152 + 7, 90_500_000, 2 ** 33]
    got = [W(n) for n in sizes]
    assert all(g > 0 and g % 8 == 0 for g in got), got
    assert got == sorted(got), got                                                               # non-decreasing in n
    assert got[0] == 8 and got[-1] == got[-2]                                                    # one workgroup for n = 0; capped for large n
    assert W(-1) == 0 and W(-2 ** 40) == 0


def test_every_refusal_is_a_status_code_before_the_launch():
    """no GPU here: a call that got as far as a launch could not return RDM_ERR_BAD_ARGUMENT with these messages"""
    _, L = lib()
    p, odd4, odd8 = C.c_void_p(4096), C.c_void_p(4100), C.c_void_p(4104)
    err = L.rdm_last_error_string

    def refused(rc, word, tag):
        assert rc == -1 and tag in err() and word in err(), (rc, err())

    acc = L.rdm_grad_accumulate_f32
    refused(acc(None, p, 8, 0, None), b"NULL", b"grad_accumulate")
    refused(acc(p, None, 8, 1, None), b"NULL", b"grad_accumulate")
    refused(acc(odd4, p, 8, 0, None), b"aligned", b"grad_accumulate")
    refused(acc(p, odd8, 8, 0, None), b"aligned", b"grad_accumulate")
    refused(acc(p, p, -1, 0, None), b"negative", b"grad_accumulate")
    refused(acc(p, p, 8, 2, None), b"mode", b"grad_accumulate")
    refused(acc(p, p, 8, -1, None), b"mode", b"grad_accumulate")

    ss, need = L.rdm_grad_sumsq_f64, L.rdm_grad_sumsq_workspace_bytes(5000)
    assert need > 8
    refused(ss(None, 5000, p, p, need, None), b"NULL", b"grad_sumsq")
    refused(ss(p, 5000, None, p, need, None), b"NULL", b"grad_sumsq")
    refused(ss(p, 5000, p, None, need, None), b"NULL", b"grad_sumsq")
    refused(ss(odd8, 5000, p, p, need, None), b"aligned", b"grad_sumsq")
    refused(ss(p, 5000, odd4, p, need, None), b"aligned", b"grad_sumsq")
    refused(ss(p, 5000, p, odd4, need, None), b"aligned", b"grad_sumsq")
    refused(ss(p, -5, p, p, need, None), b"negative", b"grad_sumsq")
    refused(ss(p, 5000, p, p, need - 1, None), b"workspace", b"grad_sumsq")
    refused(ss(p, 0, p, p, 0, None), b"workspace", b"grad_sumsq")

    clip = L.rdm_adamw_fused_clip
    good = dict(p=p, g=p, m=p, v=p, n=64, step=1, sumsq=p, slots=3, max_norm=1.0, coef=None)
    for change, word in [(dict(p=None), b"bad argument"), (dict(g=None), b"bad argument"), (dict(m=None), b"bad argument"), (dict(v=None), b"bad argument"),
                         (dict(n=-1), b"bad argument"), (dict(step=0), b"bad argument"), (dict(p=odd4), b"16-byte"), (dict(v=odd8), b"16-byte"),
                         (dict(sumsq=None), b"sumsq"), (dict(sumsq=odd4), b"sumsq"), (dict(slots=0), b"n_slots"), (dict(slots=9), b"n_slots"), (dict(slots=-1), b"n_slots"),
                         (dict(max_norm=-1.0), b"max_norm"), (dict(max_norm=float("nan")), b"max_norm"), (dict(coef=C.c_void_p(4098)), b"coef_out")]:
        kw = dict(good, **change)
        rc = clip(kw["p"], kw["g"], kw["m"], kw["v"], kw["n"], 1e-4, 0.9, 0.999, 1e-8, 0.01, kw["step"], 1.0, kw["sumsq"], kw["slots"], kw["max_norm"], kw["coef"], None)
        refused(rc, word, b"adamw_fused_clip")


# ---- train.py's flags ------------------------------------------------------------------------------------------------------------------------
def test_new_flags_parse_and_refuse_bad_values():
    from md_rdm_amd import train
    P = train.build_parser()
    a = P.parse_args([])
    assert (a.accumulate_grad_batches, a.gradient_clip_val) == (1, 0.0)                          # the defaults: the loop of before
    a = P.parse_args(["--accumulate_grad_batches", "8", "--gradient_clip_val", "0.5"])
    assert (a.accumulate_grad_batches, a.gradient_clip_val) == (8, 0.5)
    for argv in (["--accumulate_grad_batches", "two"], ["--gradient_clip_val", "big"], ["--accumulate_grad_batches", "1.5"]):
        with pytest.raises(SystemExit):
            P.parse_args(argv)
    for argv, word in ((["--accumulate_grad_batches", "0"], "--accumulate_grad_batches"), (["--accumulate_grad_batches", "-3"], "--accumulate_grad_batches"),
                       (["--gradient_clip_val", "-0.1"], "--gradient_clip_val"), (["--gradient_clip_val", "nan"], "--gradient_clip_val")):
        with pytest.raises(SystemExit) as e:                                                     # refused with a message, before anything touches a GPU
            train.main(["--synthetic"] + argv)
        assert word in str(e.value), e.value


# ---- the window bookkeeping ------------------------------------------------------------------------------------------------------------------
class StubLoss:
    def __init__(self, log, tag):
        self.log, self.tag = log, tag

    def backward(self):
        self.log.append(("backward", self.tag, self.log.opt.silent))


class Log(list):
    opt = None


class StubOptimiser:
    """records the calls of harness.train_epoch; counts micro-batches as FusedAdamW does (accumulate_grad calls since zero_grad, + 1 at the step)"""

    def __init__(self, log):
        self.log, self.micro, self.silent = log, 0, False
        log.opt = self

    def zero_grad(self):
        self.log.append(("zero_grad",))
        self.micro = 0

    def accumulate_grad(self):
        self.log.append(("accumulate", 0 if self.micro == 0 else 1))                            # the mode FusedAdamW would use: copy first, add later
        self.micro += 1

    def no_sync(self):
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.silent = True
            try:
                yield
            finally:
                self.silent = False
        return scope()

    def step(self, sync=None):
        self.log.append(("step", self.micro + 1, 1.0 / (self.micro + 1), sync))
        self.micro = 0


def run_epoch(n_batches, k, sync="S"):
    from md_rdm_amd import harness
    log = Log()
    opt = StubOptimiser(log)
    seen = []
    steps = harness.train_epoch(None, opt, [(i, -i) for i in range(n_batches)], accumulate=k, sync=sync, on_step=lambda it, n, loss, parts: seen.append((it, n, loss.tag)),
                                step_fn=lambda model, x, y: (StubLoss(log, x), {"x": x, "y": y}))
    return steps, log, seen


def test_windows_cut_the_batches_and_flush_the_last():
    from md_rdm_amd import harness
    W = lambda n, k: [(b, i, last) for b, i, last in harness.accumulation_windows(range(n), k)]
    assert W(0, 3) == []
    assert W(1, 3) == [(0, 0, True)]
    assert W(3, 1) == [(0, 0, True), (1, 0, True), (2, 0, True)]
    assert W(6, 3) == [(0, 0, False), (1, 1, False), (2, 2, True), (3, 0, False), (4, 1, False), (5, 2, True)]
    assert W(5, 3) == [(0, 0, False), (1, 1, False), (2, 2, True), (3, 0, False), (4, 1, True)]          # the partial window closes on the last batch
    assert W(4, 3)[-1] == (3, 0, True)
    assert W(7, 8) == [(b, b, b == 6) for b in range(7)]
    assert [b for b, _, _ in harness.accumulation_windows(iter(range(5)), 2)] == list(range(5))          # a one-shot generator is consumed once, in order
    with pytest.raises(ValueError):
        list(harness.accumulation_windows(range(3), 0))


def test_default_window_is_the_plain_loop():
    steps, log, seen = run_epoch(3, 1)
    assert steps == 3 and seen == [(0, 1, 0), (1, 1, 1), (2, 1, 2)]
    assert list(log) == [("zero_grad",), ("backward", 0, False), ("step", 1, 1.0, "S")] + [("zero_grad",), ("backward", 1, False), ("step", 1, 1.0, "S")] + \
        [("zero_grad",), ("backward", 2, False), ("step", 1, 1.0, "S")]


@pytest.mark.parametrize("n,k,windows", [(6, 3, [3, 3]), (7, 3, [3, 3, 1]), (5, 2, [2, 2, 1]), (4, 8, [4]), (8, 4, [4, 4]), (1, 4, [1])])
def test_window_bookkeeping(n, k, windows):
    steps, log, seen = run_epoch(n, k)
    assert steps == len(windows)
    assert seen == [(i, w, sum(windows[:i + 1]) - 1) for i, w in enumerate(windows)]             # reported once per step, with the window's LAST batch
    expect, b = [], 0
    for w in windows:
        expect.append(("zero_grad",))                                                            # cleared at the window boundary only
        for j in range(w - 1):
            expect += [("backward", b, True), ("accumulate", 0 if j == 0 else 1)]                # non-final: inside no_sync (the hook stays silent); copy, then add
            b += 1
        expect += [("backward", b, False), ("step", w, 1.0 / w, "S")]                            # final: the hook runs; the scale is 1 / (batches actually seen)
        b += 1
    assert list(log) == expect and b == n
    assert sum(1 for e in log if e[0] == "backward" and not e[2]) == len(windows)                # one exchange-issuing backward per optimiser step


def test_fused_adamw_counts_like_the_stub():
    """the stub's bookkeeping is FusedAdamW's: same method names, and the source applies 1 / k with k = accumulate_grad calls + 1"""
    import inspect

    from md_rdm_amd import harness
    for name in ("zero_grad", "accumulate_grad", "no_sync", "step", "attach_sync"):
        assert callable(getattr(harness.FusedAdamW, name))
    src = inspect.getsource(harness.FusedAdamW.step)
    assert "k = self.micro + 1" in src and "float(grad_scale) / (k * sync.world)" in src and "float(grad_scale) / k" in src
    sig = inspect.signature(harness.FusedAdamW.__init__)
    assert sig.parameters["clip"].default is None and inspect.signature(harness.FusedAdamW.step).parameters["clip"].default is None
