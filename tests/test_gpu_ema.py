"""-m gpu: the weight average.  The kernels of include/rdm_ema.h on raw guarded buffers, harness.FusedAdamW(ema_decay=...) on the smallest real
model, and the checkpoint round trip.

Sizes: n in {0, 1, 3, 4, 5, 4 x 255 + 3, 4 x 256, 4 x 256 + 1, 4 x 2048 x 256 + 4 x 300 + 2}: nothing; tail only; exactly one quad; a quad and a tail; one
workgroup not full, with a tail; the 256 quads at which adamw_grid still launches one workgroup, and one element more; and past the 2048 x 256 quads one
trip of the grid covers, so the grid-stride loop takes a second trip and the tail runs too.

Bounds.  param, exp_avg and exp_avg_sq against rdm_adamw_fused / rdm_adamw_fused_clip on cloned inputs: bit for bit.  The average against the float64
replay of tests/ema_ref.py, fed the float32 weights the kernel stored: 5 T 2^-24 M absolute after T steps (derived in ema_ref's docstring).  The swap
and everything about swapping back: bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import ema_ref as er
import normpool_ref as nr
import stream_probe as sp
from md_rdm_amd import filler

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 3, 4, 5, 4 * 255 + 3, 4 * 256, 4 * 256 + 1, 4 * 2048 * 256 + 4 * 300 + 2]
GUARD = 64                                                    # floats on either side of every buffer
F32 = np.float32
HP = dict(lr=float(F32(1e-2)), b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-8)), wd=float(F32(0.1)))
T, DECAY = 4, float(F32(0.9))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def lb():
    from md_rdm_amd import _lib
    return _lib


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Guarded:
    """n floats with GUARD floats of a recognisable pattern before and behind them; .t is the whole tensor, .ptr the first of the n"""

    def __init__(self, values, dev):
        n = int(values.size)
        host = np.empty(n + 2 * GUARD, F32)
        host[:GUARD] = -7777.25 - np.arange(GUARD)
        host[GUARD + n:] = 8888.5 + np.arange(GUARD)
        host[GUARD:GUARD + n] = values
        self.n, self.t = n, torch.from_numpy(host).to(dev)
        assert (self.t.data_ptr() + 4 * GUARD) % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * GUARD)

    @property
    def body(self):
        return self.t[GUARD:GUARD + self.n]

    def clone(self):
        g = object.__new__(Guarded)
        g.n, g.t = self.n, self.t.clone()
        return g

    def guards_like(self, other):
        return same(self.t[:GUARD], other.t[:GUARD]) and same(self.t[GUARD + self.n:], other.t[GUARD + self.n:])


_INPUTS = {}


def inputs(n):
    """hash-filled p, g, m, v (tests/normpool_ref.adamw_inputs) and an average of the weights' magnitude that differs from them; host arrays, made once"""
    if n not in _INPUTS:
        if n == 0:
            _INPUTS[n] = {k: np.zeros(0, F32) for k in "pgmve"}
        else:
            inp = nr.adamw_inputs(n, key="ema.adamw")
            _INPUTS[n] = dict(p=inp["p"], g=inp["g"], m=inp["m0"], v=inp["v0"], e=filler.uniform(f"ema.adamw.{n}.e", (n,), -2e-3, 2e-3))
    return _INPUTS[n]


def state(n, dev):
    return {k: Guarded(np.asarray(v, dtype=F32), dev) for k, v in inputs(n).items()}


def clone(st):
    return {k: v.clone() for k, v in st.items()}


def call_ema(st, step, gs, decay, slots=None, n_slots=0, max_norm=0.0, coef=None, stream=None, n=None):
    L, _lib = lb().lib(), lb()
    return L.rdm_adamw_fused_ema(st["p"].ptr, st["g"].ptr, st["m"].ptr, st["v"].ptr, st["e"].ptr, st["p"].n if n is None else n, HP["lr"], HP["b1"], HP["b2"], HP["eps"],
                                 HP["wd"], step, float(gs), None if slots is None else _lib.ptr(slots), n_slots, float(max_norm), None if coef is None else _lib.ptr(coef),
                                 float(decay), _lib.stream() if stream is None else stream)


def call_plain(st, step, gs):
    L, _lib = lb().lib(), lb()
    _lib.check(L.rdm_adamw_fused(st["p"].ptr, st["g"].ptr, st["m"].ptr, st["v"].ptr, st["p"].n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step, float(gs), _lib.stream()))


def call_clip(st, step, gs, slots, n_slots, max_norm, coef):
    L, _lib = lb().lib(), lb()
    _lib.check(L.rdm_adamw_fused_clip(st["p"].ptr, st["g"].ptr, st["m"].ptr, st["v"].ptr, st["p"].n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step, float(gs),
                                      _lib.ptr(slots), n_slots, float(max_norm), _lib.ptr(coef), _lib.stream()))


def sumsq_slots(g, dev):
    """slot 0 written by rdm_grad_sumsq_f64 from the gradient's n elements"""
    L, _lib = lb().lib(), lb()
    slots = torch.zeros(8, dtype=torch.float64, device=dev)
    need = int(L.rdm_grad_sumsq_workspace_bytes(g.n))
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    _lib.check(L.rdm_grad_sumsq_f64(g.ptr, g.n, _lib.ptr(slots), _lib.ptr(ws), need, _lib.stream()))
    return slots


# ---- rdm_adamw_fused_ema on raw buffers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("n", SIZES)
def test_fused_step_bytes_and_average(dev, n, clipped):
    st0 = state(n, dev)
    a, b = clone(st0), clone(st0)                                                           # a: the fused call; b: the step without the average
    gs = 0.3
    slots = coef_a = coef_b = None
    max_norm = 0.0
    if clipped:
        slots = sumsq_slots(st0["g"], dev)
        max_norm = 0.37 * float(slots[0]) ** 0.5 * gs                                       # well below the scaled gradient's norm: the step clips
        coef_a, coef_b = torch.full((1,), 7.0, device=dev), torch.full((1,), 7.0, device=dev)
    posts = []
    for t in range(T):
        if clipped:
            lb().check(call_ema(a, t + 1, gs, DECAY, slots, 1, max_norm, coef_a))
            call_clip(b, t + 1, gs, slots, 1, max_norm, coef_b)
        else:
            lb().check(call_ema(a, t + 1, gs, DECAY))
            call_plain(b, t + 1, gs)
        for k in ("p", "m", "v", "g"):                                                      # (i) the step's bytes, and (iii) the guards with them
            assert same(a[k].t, b[k].t), f"{k} differs from the step without the average: step {t + 1}, n={n}"
        posts.append(a["p"].body.cpu().numpy().copy())
    for k in "pgmve":                                                                       # (iii) nothing before the buffer, nothing at or beyond n
        assert a[k].guards_like(st0[k]), f"guards of {k} touched, n={n}"
    assert same(a["g"].t, st0["g"].t)
    if clipped and n:
        assert same(coef_a, coef_b) and 0.0 < float(coef_a[0]) < 1.0                        # the same coefficient, and it did clip
    if n == 0:
        assert all(same(a[k].t, st0[k].t) for k in "pgmve")                                 # nothing launched
        assert not clipped or float(coef_a[0]) == 7.0
        return
    assert not same(a["p"].body, st0["p"].body) and not same(a["e"].body, st0["e"].body)
    want, M = er.ema_replay(inputs(n)["e"], posts, [DECAY] * T)                             # (ii)
    err = float(np.abs(a["e"].body.cpu().numpy().astype(np.float64) - want).max())
    print(f"BOUND ema n={n} {'clipped' if clipped else 'unclipped'}: max error {err:.3g} of {er.bound(T, M):.3g} (M = {M:.3g})")
    assert err <= er.bound(T, M), (n, err, er.bound(T, M))


@pytest.mark.parametrize("n", [5, 4 * 256 + 1, 4 * 2048 * 256 + 4 * 300 + 2])
def test_decay_one_leaves_the_average_bit_unchanged(dev, n):
    st0 = state(n, dev)
    spots = [i for i in (0, 1, n // 2, n - 2, n - 1) if 0 <= i < n]                         # in the quads and in the tail
    st0["e"].body[spots[0]] = -0.0
    st0["e"].body[spots[-1]] = float("nan")
    a, b = clone(st0), clone(st0)
    lb().check(call_ema(a, 3, 1.0, 1.0))
    call_plain(b, 3, 1.0)
    assert same(a["e"].t, st0["e"].t)                                                       # (iv)
    assert all(same(a[k].t, b[k].t) for k in ("p", "m", "v")) and not same(a["p"].body, st0["p"].body)


def test_refusals_leave_the_buffers_alone(dev):
    L, n = lb().lib(), 4 * 256 + 1
    st0 = state(n, dev)
    st = clone(st0)
    slots, coef = torch.full((8,), 2.0, dtype=torch.float64, device=dev), torch.full((1,), 7.0, device=dev)
    nan = float("nan")
    null = type("Null", (), dict(ptr=None, n=n))()
    off4 = lambda g: type("Off", (), dict(ptr=C.c_void_p(g.ptr.value + 4), n=n))()
    odd_slots = slots.view(torch.float32)[1:3].view(torch.float32)                          # 4 bytes off an 8-byte boundary
    unclipped, clip = dict(), dict(slots=slots, n_slots=1, max_norm=1.0, coef=coef)
    rows = [("param NULL", dict(st, p=null), dict(), b"bad argument"), ("grad NULL", dict(st, g=null), dict(), b"bad argument"),
            ("exp_avg NULL", dict(st, m=null), dict(), b"bad argument"), ("exp_avg_sq NULL", dict(st, v=null), dict(), b"bad argument"),
            ("n negative", st, dict(n=-1), b"bad argument"), ("step 0", st, dict(step=0), b"bad argument"),
            ("param misaligned", dict(st, p=off4(st["p"])), dict(), b"16-byte"), ("exp_avg_sq misaligned", dict(st, v=off4(st["v"])), dict(), b"16-byte"),
            ("ema NULL", dict(st, e=null), dict(), b"ema must"), ("ema misaligned", dict(st, e=off4(st["e"])), dict(), b"ema must"),
            ("ema is param", dict(st, e=st["p"]), dict(), b"overlaps"),
            ("ema inside param", dict(st, e=type("In", (), dict(ptr=C.c_void_p(st["p"].ptr.value + 16 * 8), n=n))()), dict(), b"overlaps"),
            ("decay below 0", st, dict(decay=-0.01), b"ema_decay"), ("decay above 1", st, dict(decay=1.5), b"ema_decay"), ("decay NaN", st, dict(decay=nan), b"ema_decay"),
            ("slots without sumsq", st, dict(n_slots=1), b"n_slots"), ("sumsq without slots", st, dict(slots=slots, n_slots=0), b"n_slots"),
            ("sumsq misaligned", st, dict(clip, slots=odd_slots), b"sumsq"), ("nine slots", st, dict(clip, n_slots=9), b"n_slots"),
            ("max_norm negative", st, dict(clip, max_norm=-1.0), b"max_norm"), ("max_norm NaN", st, dict(clip, max_norm=nan), b"max_norm"),
            ("coef_out misaligned", st, dict(clip, coef=type("T", (), dict(is_contiguous=lambda s: True, data_ptr=lambda s: coef.data_ptr() + 2))()), b"coef_out")]
    for tag, bufs, kw, word in rows:
        kw = dict(dict(step=1, gs=1.0, decay=DECAY), **kw)
        rc = call_ema(bufs, kw.pop("step"), kw.pop("gs"), kw.pop("decay"), **kw)
        msg = L.rdm_last_error_string()
        assert rc == -1 and b"adamw_fused_ema" in msg and word in msg, (tag, rc, msg)       # (vi) RDM_ERR_BAD_ARGUMENT, with a message
    torch.cuda.synchronize()
    assert all(same(st[k].t, st0[k].t) for k in "pgmve") and float(coef[0]) == 7.0 and bool((slots == 2.0).all())


# ---- the caller's stream -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(dev):
    """stream_probe's calibrated delay and proven stream.  torch.cuda.Stream() hands out the 32 streams of torch's pool round-robin, so every call
    moves the ring for the rest of the process; this module takes a whole turn of it, which leaves the modules behind it the streams they met before
    it existed (as tests/test_gpu_optim.py does)."""
    lb().lib()
    real, taken = torch.cuda.Stream, []

    def counted(*a, **kw):
        taken.append(1)
        return real(*a, **kw)
    torch.cuda.Stream = counted
    try:
        d = sp.Delay(dev)
    finally:
        torch.cuda.Stream = real
    for _ in range(-len(taken) % 32):
        real()
    return d


def draws(n, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dev)


def case_ema(dev, clipped):
    L, n, P = lb().lib(), 2 ** 20 + 5, lb().ptr
    ins = dict(p=draws(n, 44, dev, 1e-3), g=draws(n, 45, dev), m=draws(n, 46, dev, 0.1), v=draws(n, 47, dev).square(), e=draws(n, 48, dev, 1e-3),
               slots=torch.tensor([2.0e5, 3.0e5], dtype=torch.float64, device=dev))
    if clipped:
        call = lambda b, st: lb().check(L.rdm_adamw_fused_ema(P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["e"]), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, P(b["slots"]), 2, 1.0,
                                                              P(b["coef"]), DECAY, st))
        return sp.Case(ins, call, outs=("p", "m", "v", "e", "coef"), scratch=dict(coef=torch.empty(1, device=dev)))
    call = lambda b, st: lb().check(L.rdm_adamw_fused_ema(P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), P(b["e"]), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, None, 0, 0.0, None, DECAY, st))
    return sp.Case(ins, call, outs=("p", "m", "v", "e"))


def case_swap(dev):
    L, n, P = lb().lib(), 2 ** 20 + 5, lb().ptr
    return sp.Case(dict(a=draws(n, 51, dev), b=draws(n, 52, dev)), lambda b, st: lb().check(L.rdm_ema_swap_f32(P(b["a"]), P(b["b"]), n, st)), outs=("a", "b"))


@pytest.mark.parametrize("name", ["adamw_fused_ema", "adamw_fused_ema clipped", "ema_swap"])
def test_entry_point_on_a_late_non_default_stream(dev, delay, name):
    """(v) tests/test_gpu_streams.py's late producer: the real inputs reach the poisoned buffers on a non-default stream behind a long delay kernel with the
    null stream blocked, the call follows on that stream, and its outputs must equal the null-stream run's bit for bit.  include/rdm_ema.h is outside that
    file's table, so the check lives here."""
    case = {"adamw_fused_ema": lambda: case_ema(dev, False), "adamw_fused_ema clipped": lambda: case_ema(dev, True), "ema_swap": lambda: case_swap(dev)}[name]()
    torch.cuda.synchronize()
    sp.check(case, delay)


def test_control_a_call_on_the_null_stream_is_detected(dev, delay):
    """the probe's own control, on the clipped case: it has an output that is no input (coef_out), which the late copy of the inputs cannot cover up"""
    case = case_ema(dev, True)
    torch.cuda.synchronize()
    sp.control(case, delay)


# ---- rdm_ema_swap_f32 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_swap_is_an_exact_exchange_and_twice_the_identity(dev, n):
    L, _lib = lb().lib(), lb()
    a0, b0 = Guarded(np.asarray(inputs(n)["p"], F32), dev), Guarded(np.asarray(inputs(n)["v"], F32), dev)
    for i, val in ((0, -0.0), (n - 1, float("nan")), (n // 2, float("inf"))):               # bytes, not values: -0, NaN and infinity travel too
        if 0 <= i < n and n >= 3:
            a0.body[i] = val
    a, b = a0.clone(), b0.clone()
    _lib.check(L.rdm_ema_swap_f32(a.ptr, b.ptr, n, _lib.stream()))
    assert same(a.body, b0.body) and same(b.body, a0.body)
    assert a.guards_like(a0) and b.guards_like(b0)
    _lib.check(L.rdm_ema_swap_f32(a.ptr, b.ptr, n, _lib.stream()))
    assert same(a.t, a0.t) and same(b.t, b0.t)


def test_swap_refusals(dev):
    L, _lib, n = lb().lib(), lb(), 4 * 256 + 1
    a0, b0 = Guarded(np.asarray(inputs(n)["p"], F32), dev), Guarded(np.asarray(inputs(n)["v"], F32), dev)
    a, b = a0.clone(), b0.clone()
    st, off = _lib.stream(), lambda g, nbytes: C.c_void_p(g.ptr.value + nbytes)
    for tag, args, word in (("a NULL", (None, b.ptr, n), b"NULL"), ("b NULL", (a.ptr, None, n), b"NULL"),
                            ("a misaligned", (off(a, 4), b.ptr, n - 1), b"aligned"), ("b misaligned", (a.ptr, off(b, 8), n - 2), b"aligned"),
                            ("n negative", (a.ptr, b.ptr, -1), b"negative"), ("the same range", (a.ptr, a.ptr, n), b"overlap"),
                            ("b inside a", (a.ptr, off(a, 64), n - 16), b"overlap"), ("a inside b", (off(b, 64), b.ptr, 17), b"overlap")):
        rc = L.rdm_ema_swap_f32(*args, st)
        msg = L.rdm_last_error_string()
        assert rc == -1 and b"ema_swap" in msg and word in msg, (tag, rc, msg)
    torch.cuda.synchronize()
    assert same(a.t, a0.t) and same(b.t, b0.t)


# ---- FusedAdamW on the smallest real model -------------------------------------------------------------------------------------------------------
_PRISTINE = []


def host_model():
    """a hash-filled default DepthEstimationNet on the host; built and filled once, copied from then on"""
    import copy

    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    if not _PRISTINE:
        m = DepthEstimationNet()
        filler.fill_state_dict(m.state_dict())
        _PRISTINE.append(m)
    return copy.deepcopy(_PRISTINE[0])


def make_model(dev):
    m = host_model().to(dev).train()
    m.flatten_parameters()
    m.direct_grads = True
    return m


def smalls(m):
    return [p for p in m.weight_layer.parameters() if p.requires_grad]


def trainable_mask(m, dev):
    """True on the flat elements that hold a tensor the optimiser updates (not d_1.conv1.*, not alignment padding)"""
    flat, _, entries = m._flat
    mask = torch.zeros(flat.numel(), dtype=torch.bool, device=dev)
    for k, p, o, n, _ in entries:
        if p.requires_grad and not k.startswith("d_1.conv1."):
            mask[o:o + n] = True
    return mask


def replay_on_device(ema0, weights, decays):
    """ema_ref.ema_replay in torch float64 on the device (the flat buffer holds 90 M elements): the same operations in the same order"""
    e = ema0.double()
    M = float(e.abs().max())
    for w, d in zip(weights, decays):
        e = e + float(er.one_minus(d)) * (w.double() - e)
        M = max(M, float(w.abs().max()), float(e.abs().max()))
    return e, M


def check_average(opt, init, posts, small_init, small_posts, decays, mask, tag):
    """opt.ema on the trained elements and the scalar averages against the float64 replay; everything else equals the initial copy"""
    steps = len(posts)
    want, M = replay_on_device(init[mask], [p[mask] for p in posts], decays)
    head, _ = er.ema_replay(init[mask][:4099].cpu().numpy(), [p[mask][:4099].cpu().numpy() for p in posts], decays)
    assert np.array_equal(want[:4099].cpu().numpy(), head)                                 # the device replay IS the host restatement
    err = float((opt.ema[mask].double() - want).abs().max())
    print(f"BOUND {tag}: flat average max error {err:.3g} of {er.bound(steps, M):.3g} (M = {M:.3g})")
    assert err <= er.bound(steps, M), (tag, err, er.bound(steps, M))
    assert same(opt.ema[~mask], init[~mask]), tag                                          # (c) d_1.conv1.* and padding: the initial copy
    for i, e in enumerate(opt.ema_small):
        want, M = er.ema_replay(small_init[i].cpu().numpy(), [sp_[i].cpu().numpy() for sp_ in small_posts], decays)
        err = float(np.abs(e.cpu().numpy().astype(np.float64) - want).max())
        assert e.dtype == torch.float32 and err <= er.bound(steps, M), (tag, i, err, er.bound(steps, M))


@pytest.fixture(scope="module", params=[True, False], ids=["warm-up", "no warm-up"])
def trained(dev, request):
    """three real training steps (B = 2 at 226 x 226) with the average on; a second optimiser without it is fed the recorded gradients"""
    from md_rdm_amd import harness
    warmup = request.param
    m, m2 = make_model(dev), make_model(dev)
    flat, gflat, _ = m._flat
    flat2, gflat2, _ = m2._flat
    opt = harness.FusedAdamW(m, lr=1e-3, ema_decay=0.9, ema_warmup=warmup)
    opt2 = harness.FusedAdamW(m2, lr=1e-3)
    assert opt.ema is None and opt2.ema is None                                            # allocated at the first step only, and only when on
    init, small_init = flat.detach().clone(), [p.detach().clone() for p in smalls(m)]
    posts, small_posts, decays = [], [], []
    for s in range(3):
        x, y = filler.synthetic_batch(2, 226, 226, seed=31 + s)
        opt.zero_grad()
        loss, _ = harness.training_step(m, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
        loss.backward()
        opt2.zero_grad()
        gflat2.copy_(gflat)
        for p, q in zip(smalls(m), smalls(m2)):
            q.grad = p.grad.detach().clone()
        decays.append(harness.ema_decay_at(0.9, opt.ema_updates, warmup))
        opt.step()
        opt2.step()
        posts.append(flat.detach().clone())
        small_posts.append([p.detach().clone() for p in smalls(m)])
    torch.cuda.synchronize()
    return dict(m=m, m2=m2, opt=opt, opt2=opt2, init=init, small_init=small_init, posts=posts, small_posts=small_posts, decays=decays, warmup=warmup)


def test_weights_are_those_of_the_optimiser_without_the_average(trained):
    m, m2, opt, opt2 = trained["m"], trained["m2"], trained["opt"], trained["opt2"]
    assert same(m._flat[0], m2._flat[0]) and same(opt.m, opt2.m) and same(opt.v, opt2.v)   # (a)
    assert all(same(p.detach(), q.detach()) for p, q in zip(smalls(m), smalls(m2)))
    assert opt2.ema is None and set(opt2.state_dict()) == {"step", "lr", "exp_avg", "exp_avg_sq", "small"}
    assert opt.ema_updates == 3 == opt.step_count and not same(trained["posts"][-1], trained["init"])
    assert trained["decays"] == ([float(F32(0.1)), float(F32(2 / 11)), float(F32(0.25))] if trained["warmup"] else [float(F32(0.9))] * 3)


def test_average_matches_the_float64_replay(trained, dev):
    t = trained
    assert t["opt"].ema.dtype == torch.float32 and t["opt"].ema.shape == t["m"]._flat[0].shape and len(t["opt"].ema_small) == len(smalls(t["m"])) == 4
    check_average(t["opt"], t["init"], t["posts"], t["small_init"], t["small_posts"], t["decays"], trainable_mask(t["m"], dev), "three steps")   # (b), (c)
    assert not same(t["opt"].ema, t["init"]) and not same(t["opt"].ema, t["posts"][-1])


def test_inside_the_context_the_model_holds_the_average(trained, dev):
    m, opt = trained["m"], trained["opt"]
    flat, _, entries = m._flat
    live, avg = flat.detach().clone(), opt.ema.detach().clone()
    live_small, avg_small = [p.detach().clone() for p in smalls(m)], [e.clone() for e in opt.ema_small]
    live_sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.from_numpy(filler.synthetic_batch(2, 226, 226, seed=77)[0]).to(dev)
    m.eval()
    try:
        first = {prec: m.set_precision(prec).predict(x).clone() for prec in ("f32", "bf16")}
        with opt.ema_weights() as inside:                                                  # (d)
            assert inside is opt
            mask = trainable_mask(m, dev)
            expect = torch.where(mask, avg, live)                                          # (padding inside a range is swept along: zero on both sides)
            assert same(flat, expect) and same(opt.ema, torch.where(mask, live, avg))
            sd = m.state_dict()
            names = set()
            for k, p, o, n, _ in entries:                                                  # the averaged tensors, through the (OIHW) views of the flat buffer
                names.add(k)
                if n:
                    assert p.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
                    want = torch.as_strided(expect, p.shape, p.stride(), p.storage_offset() - flat.storage_offset())
                    assert same(sd[k], want), k
                    if p.requires_grad and not k.startswith("d_1.conv1."):
                        assert not same(sd[k], live_sd[k]) or not bool(live_sd[k].any()), k
            for p, e in zip(smalls(m), avg_small):
                assert same(p.detach(), e)
            for k in live_sd:                                                              # BatchNorm statistics (and whatever else is no weight) stay the live ones
                if k not in names and not k.startswith("weight_layer."):
                    assert same(sd[k], live_sd[k]), k
            averaged = {prec: m.set_precision(prec).predict(x).clone() for prec in ("f32", "bf16")}
            assert not same(averaged["f32"], first["f32"])
            assert not same(averaged["bf16"], first["bf16"])                               # the bf16 copies were rebuilt from the averaged weights
            with pytest.raises(lb().RdmError, match="ema_weights"):                        # (e)
                opt.step()
            with pytest.raises(lb().RdmError, match="ema_weights"):
                opt.state_dict()
        assert same(flat, live) and same(opt.ema, avg)                                     # bit-identical to before
        assert all(same(p.detach(), q) for p, q in zip(smalls(m), live_small)) and all(same(e, q) for e, q in zip(opt.ema_small, avg_small))
        for prec in ("f32", "bf16"):
            assert same(m.set_precision(prec).predict(x), first[prec]), prec               # and the second live predict is the first, bit for bit
        with pytest.raises(ZeroDivisionError):                                             # the exit swap runs when the body raises
            with opt.ema_weights():
                1 / 0
        assert same(flat, live) and same(opt.ema, avg) and opt.step_count == 3 and opt.ema_updates == 3
    finally:
        m.set_precision("f32")
        m.train()


class Recorder:
    """stands in front of the library's optimiser entry points and notes which are called"""
    NAMES = ("rdm_adamw_fused", "rdm_adamw_fused_clip", "rdm_adamw_fused_ema", "rdm_ema_swap_f32")

    def __init__(self):
        self.L, self.calls, self.real = lb().lib(), [], {}

    def __enter__(self):
        for name in self.NAMES:
            self.real[name] = getattr(self.L, name)
            setattr(self.L, name, (lambda nm: lambda *a: (self.calls.append(nm), self.real[nm](*a))[1])(name))
        return self

    def __exit__(self, *exc):
        for name, fn in self.real.items():
            setattr(self.L, name, fn)


def planted_step(opts, gen, dev, micro, clip):
    """the same `micro` planted micro-batch gradients through every optimiser of `opts`, as one accumulation window"""
    N = opts[0].model._flat[0].numel()
    mask = trainable_mask(opts[0].model, dev)                                              # as backward leaves it: no gradient in alignment padding or d_1.conv1.*
    gs = [torch.randn(N, generator=gen, device=dev) * 1e-3 * mask for _ in range(micro)]
    ss = [[torch.randn(p.shape, generator=gen, device=dev) for p in smalls(opts[0].model)] for _ in range(micro)]
    for opt in opts:
        opt.zero_grad()
        for i in range(micro):
            opt.model._flat[1].copy_(gs[i])
            for p, s in zip(smalls(opt.model), ss[i]):
                p.grad = s.clone() if p.grad is None else p.grad + s
            if i < micro - 1:
                opt.accumulate_grad()
        opt.step(clip=clip)


def test_clipping_and_accumulation_update_the_average_once_per_step(dev):
    from md_rdm_amd import harness
    m, m2 = make_model(dev), make_model(dev)
    opt, opt2 = harness.FusedAdamW(m, lr=1e-3, clip=1e-3, ema_decay=0.9), harness.FusedAdamW(m2, lr=1e-3, clip=1e-3)
    flat = m._flat[0]
    init, small_init = flat.detach().clone(), [p.detach().clone() for p in smalls(m)]
    gen = torch.Generator(device=dev).manual_seed(9)
    posts, small_posts, decays = [], [], []
    ranges = opt.trainable_ranges()
    for s in range(2):                                                                     # (f) two windows of K = 2, clipped
        decays.append(harness.ema_decay_at(0.9, s, True))
        with Recorder() as rec:
            planted_step([opt, opt2], gen, dev, 2, None)
        assert rec.calls == ["rdm_adamw_fused_ema"] * len(ranges) + ["rdm_adamw_fused_clip"] * len(ranges)       # one launch per range: no extra pass
        assert float(opt._coef[0]) < 1.0 and same(opt._coef, opt2._coef)
        posts.append(flat.detach().clone())
        small_posts.append([p.detach().clone() for p in smalls(m)])
    assert opt.ema_updates == 2 == opt.step_count
    assert same(flat, m2._flat[0]) and same(opt.m, opt2.m) and same(opt.v, opt2.v)
    assert all(same(p.detach(), q.detach()) for p, q in zip(smalls(m), smalls(m2)))
    check_average(opt, init, posts, small_init, small_posts, decays, trainable_mask(m, dev), "clipped windows of 2")
    with Recorder() as rec:
        with opt.ema_weights():
            pass
    assert rec.calls == ["rdm_ema_swap_f32"] * (2 * len(ranges))                           # one exchange launch per range, each way


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(dev, tmp_path):
    from md_rdm_amd import checkpoint, harness
    m = make_model(dev)
    opt = harness.FusedAdamW(m, lr=1e-3, ema_decay=0.9)
    gen = torch.Generator(device=dev).manual_seed(13)
    for _ in range(2):
        planted_step([opt], gen, dev, 1, None)
    with opt.ema_weights():
        averaged = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    path = str(tmp_path / "ema.ckpt")
    torch.save(checkpoint.to_lightning(m, {"epoch": 0}, optimizer=opt), path)
    fresh = host_model()
    _, ckpt = checkpoint.from_lightning(fresh, path, ema=True)
    got = fresh.state_dict()
    assert set(got) == set(averaged) and all(same(got[k].cpu(), averaged[k]) for k in averaged)
    live = host_model()
    checkpoint.from_lightning(live, path)
    assert any(not same(live.state_dict()[k], averaged[k]) for k in averaged)              # the default entry holds the live weights
    live = live.to(dev).train()
    live.flatten_parameters()
    live.direct_grads = True
    assert same(live._flat[0], m._flat[0])
    resumed = harness.FusedAdamW(live, lr=1e-3, ema_decay=0.9)
    assert checkpoint.restore_training_state(ckpt, resumed)
    assert same(resumed.ema, opt.ema) and resumed.ema_updates == opt.ema_updates == 2 and all(same(a, b) for a, b in zip(resumed.ema_small, opt.ema_small))
    planted_step([opt, resumed], gen, dev, 1, None)                                        # the next step of both gives equal averages
    assert resumed.ema_updates == 3 and same(resumed.ema, opt.ema) and same(live._flat[0], m._flat[0]) and all(same(a, b) for a, b in zip(resumed.ema_small, opt.ema_small))
    plain = harness.FusedAdamW(m, lr=1e-3)                                                 # a checkpoint of a run without the average has no such entry
    unaveraged = checkpoint.to_lightning(m, optimizer=plain)
    assert "state_dict_ema" not in unaveraged and "ema" not in unaveraged["optimizer_states"][0]
    with pytest.raises(checkpoint.NoAveragedWeights):
        checkpoint.from_lightning(fresh, unaveraged, ema=True)
