"""-m gpu: the optimiser-side gradient kernels of include/rdm_optim.h through the C ABI, harness.FusedAdamW's accumulation window and clipped step on
the real model's flat buffers (no forward pass), and train.py with both flags end to end.

Sizes: n in {1, 3, 255, 1025, 2^20 + 5, 2 x 2 097 152 + 7}: tail only; fewer quads than a workgroup's threads; two workgroups with a tail of one; 4096 full
workgroups and a tail; and 1 048 577 quads, past the 2048 x 256 that one trip of the accumulate / AdamW grid covers (1024 x 256 for the sum of squares),
so the grid-stride loop takes a second trip and the tail runs too.

Bounds.  accumulate and the clipped step against the plain one: bit for bit.  Sum of squares on integer-valued data: the exact integer.  On random data
against math.fsum of the float64 squares: 1e-12 relative - each square is exact in float64 and each addition rounds by at most 2^-53 of the running sum
of non-negative terms; a result passes through at most 4 x 4 (a thread's elements per trip, four or five trips) + 6 (shuffle) + 4 (wavefronts) + 4 + 6 + 4
(the partials) = 44 dependent additions, so about 44 x 1.1e-16 = 5e-15: two decades of margin.  The clipped step against torch's clip_grad_norm_ (on a
float64 copy of the gradient, so the reference's own coefficient is exact to 1e-16) and the float64 restatement tests/normpool_ref.adamw: the per-element
bound tests/test_gpu_norm_pool_edges.adamw_check applies to rdm_adamw_fused.  That bound counts the roundings of the update from float32 INPUTS, and
clipping adds one float32 product to g; so the restatement is fed that product, g * float32(torch's coefficient), formed in float32, and no number is
added.  (Fed torch's float64-clipped gradient instead, the product's rounding is charged to the kernel, twice in v = .. + (1 - b2) g^2: measured on one
MI355X at n = 2^20 + 5, step 1, 69 of 1 048 581 elements of v at up to 1.02 of the 4 x 2^-24 bound, m inside its own.)"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import normpool_ref as nr
import stream_probe as sp
from md_rdm_amd import filler
from test_gpu_norm_pool_edges import adamw_check

pytestmark = pytest.mark.gpu
SIZES = [1, 3, 255, 1025, 2 ** 20 + 5, 2 * 2097152 + 7]
PAD = 9                                                       # NaN elements behind every buffer: nothing beyond n is touched
F32 = np.float32
HP = dict(lr=float(F32(1e-2)), b1=float(F32(0.9)), b2=float(F32(0.999)), eps=float(F32(1e-8)), wd=float(F32(0.1)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    torch.set_num_threads(16)
    return torch.device("cuda:0")


def lb():
    from md_rdm_amd import _lib
    return _lib


def P(t):
    return lb().ptr(t)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def padded(values, dev):
    """device buffer of n + PAD elements: the values, then NaN"""
    t = torch.full((values.numel() + PAD,), float("nan"), dtype=values.dtype, device=dev)
    t[:values.numel()] = values.to(dev)
    return t


def draws(n, seed, dev, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(dev)


def sumsq(g, n, out=None, slot=0):
    L, _lib = lb().lib(), lb()
    out = torch.full((8,), float("nan"), dtype=torch.float64, device=g.device) if out is None else out
    need = int(L.rdm_grad_sumsq_workspace_bytes(n))
    ws = torch.full((need // 8 + 1,), float("nan"), dtype=torch.float64, device=g.device)
    _lib.check(L.rdm_grad_sumsq_f64(P(g), n, C.c_void_p(out.data_ptr() + 8 * slot), P(ws), need, _lib.stream()))
    assert bool(torch.isnan(ws[need // 8:]).all())                                        # the workspace's stated size is all it uses
    return out


# ---- rdm_grad_accumulate_f32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_accumulate_both_modes_bit_for_bit(dev, n):
    L, _lib = lb().lib(), lb()
    src, dst0 = draws(n, 11, dev), draws(n, 12, dev, 3.0)
    s = padded(src, dev)
    for mode, want in ((0, src.clone()), (1, dst0 + src)):
        d = padded(dst0, dev)
        _lib.check(L.rdm_grad_accumulate_f32(P(d), P(s), n, mode, _lib.stream()))
        assert same(d[:n], want), f"mode {mode} n={n}"
        assert bool(torch.isnan(d[n:]).all()) and same(s[:n], src) and bool(torch.isnan(s[n:]).all())
    d = padded(dst0, dev)
    _lib.check(L.rdm_grad_accumulate_f32(P(d), P(s), 0, 0, _lib.stream()))                # n = 0: nothing moves
    assert same(d[:n], dst0)


# ---- rdm_grad_sumsq_f64 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_exact_on_integers(dev, n):
    g = torch.Generator().manual_seed(21)
    v = torch.randint(-2000, 2001, (n,), generator=g)                                      # squares <= 4e6, their sum <= 1.7e13 < 2^53
    exact = int((v * v).sum())
    assert exact < 2 ** 53
    out = sumsq(padded(v.float(), dev), n)
    assert float(out[0]) == float(exact) and bool(torch.isnan(out[1:]).all()), (float(out[0]), exact)


def magnitude_mix(n, seed):
    """signs x 10^U(-20, 15), a block of exact zeros: squares from 1e-40 to 1e30"""
    r = np.random.default_rng(seed)
    v = (r.choice([-1.0, 1.0], n) * 10.0 ** r.uniform(-20.0, 15.0, n)).astype(F32)
    v[n // 3:n // 3 + n // 7] = 0
    return v


@pytest.mark.parametrize("n", SIZES)
def test_sumsq_random_against_fsum_and_repeatable(dev, n):
    for tag, v in (("mix", magnitude_mix(n, 31)), ("normal", np.random.default_rng(32).standard_normal(n).astype(F32))):
        want = math.fsum((v.astype(np.float64) ** 2).tolist())
        g = padded(torch.from_numpy(v), dev)
        a, b = sumsq(g, n), sumsq(g, n)
        rel = abs(float(a[0]) - want) / want
        print(f"BOUND sumsq {tag} n={n}: relative error {rel:.3g} of 1e-12")
        assert rel <= 1e-12, (tag, n, float(a[0]), want)
        assert same(a[:1], b[:1])                                                          # a repeated call gives the same bytes
    for bad, check in ((float("nan"), math.isnan), (float("inf"), math.isinf), (float("-inf"), math.isinf)):
        w = v.copy()
        w[n // 2] = bad
        assert check(float(sumsq(padded(torch.from_numpy(w), dev), n)[0])), bad


def test_sumsq_of_nothing_is_zero(dev):
    out = sumsq(torch.full((16,), float("nan"), device=dev), 0)
    assert float(out[0]) == 0.0 and not math.copysign(1.0, float(out[0])) < 0


# ---- rdm_adamw_fused_clip ------------------------------------------------------------------------------------------------------------------
def host_coef(slots, max_norm, grad_scale):
    """the coefficient exactly as include/rdm_optim.h states it, in IEEE float64 -> (float32 c, float32 grad_scale * c)"""
    total = np.float64(slots[0])
    for s in slots[1:]:
        total = total + np.float64(s)
    with np.errstate(all="ignore"):
        q = np.float64(F32(max_norm)) / (np.sqrt(total) * np.abs(np.float64(F32(grad_scale))) + np.float64(1e-6))
    c = np.float64(1.0) if q > 1.0 else q
    return F32(c), F32(grad_scale) * F32(c)


def adamw_state(n, dev):
    inp = nr.adamw_inputs(n, key="optim.adamw")
    return inp, {k: padded(torch.from_numpy(np.asarray(inp[src], dtype=F32)), dev) for k, src in (("p", "p"), ("g", "g"), ("m", "m0"), ("v", "v0"))}


def call_plain(st, n, step, gs):
    L, _lib = lb().lib(), lb()
    _lib.check(L.rdm_adamw_fused(P(st["p"]), P(st["g"]), P(st["m"]), P(st["v"]), n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step, float(gs), _lib.stream()))


def call_clip(st, n, step, gs, slots, n_slots, max_norm, coef):
    L, _lib = lb().lib(), lb()
    _lib.check(L.rdm_adamw_fused_clip(P(st["p"]), P(st["g"]), P(st["m"]), P(st["v"]), n, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], step, float(gs),
                                      P(slots), n_slots, float(max_norm), None if coef is None else P(coef), _lib.stream()))


@pytest.mark.parametrize("n", SIZES)
def test_clipped_step_is_the_plain_step_with_the_scaled_coefficient(dev, n):
    inp, st0 = adamw_state(n, dev)
    gs, step = 0.3, 7
    slots = sumsq(st0["g"], n)                                                             # slot 0 from the kernel, two more planted: summed left to right
    slots[1], slots[2] = 0.1 * float(slots[0]) + 1e-3, 3.0e-7
    h = slots[:3].cpu().numpy()
    norm = math.sqrt(float(h.sum())) * gs
    for tag, max_norm in (("clipping", 0.37 * norm), ("not clipping", 10.0 * norm + 1.0), ("infinite", float("inf"))):
        c, gs_c = host_coef(h, max_norm, gs)
        assert (c < 1) == (tag == "clipping") and (tag == "clipping" or c == 1)
        a = {k: v.clone() for k, v in st0.items()}
        b = {k: v.clone() for k, v in st0.items()}
        coef = torch.full((3,), float("nan"), device=dev)
        call_clip(a, n, step, gs, slots, 3, max_norm, coef)
        call_plain(b, n, step, float(gs_c))
        for k in ("p", "m", "v"):
            assert same(a[k][:n], b[k][:n]), f"{k} differs, {tag}, n={n}, c={c!r}"
            assert bool(torch.isnan(a[k][n:]).all())
        assert same(a["g"], st0["g"])
        assert same(coef[:1], torch.tensor([c], device=dev)) and bool(torch.isnan(coef[1:]).all())
        if tag != "clipping":                                                              # c == 1: the plain call with the caller's own scale
            b = {k: v.clone() for k, v in st0.items()}
            call_plain(b, n, step, gs)
            assert all(same(a[k], b[k]) for k in ("p", "m", "v"))
    a = {k: v.clone() for k, v in st0.items()}                                             # coef_out is optional
    b = {k: v.clone() for k, v in st0.items()}
    call_clip(a, n, step, gs, slots, 3, 0.37 * norm, None)
    call_clip(b, n, step, gs, slots, 3, 0.37 * norm, torch.empty(1, device=dev))
    assert all(same(a[k], b[k]) for k in ("p", "m", "v"))
    slots[1] = float("nan")                                                                # a NaN norm propagates, as torch's does
    coef = torch.zeros(1, device=dev)
    call_clip(a, n, step, gs, slots, 3, 1.0, coef)
    assert math.isnan(float(coef[0])) and bool(torch.isnan(a["p"][:n]).all())


@pytest.mark.parametrize("n", [3, 1027, 2 ** 20 + 5])
def test_clipped_step_against_torch_clip_and_float64_adamw(dev, n):
    inp, st = adamw_state(n, dev)
    for step, m0, v0, gs in ((1, np.zeros(n, F32), np.zeros(n, F32), 1.0), (1000, inp["m0"], inp["v0"], 0.5)):
        p64 = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p64.grad = torch.from_numpy(inp["g"].astype(np.float64)) * gs                      # the scaled gradient, as the optimiser sees it
        norm = float(p64.grad.norm())
        max_norm = float(F32(0.4 * norm))
        unclipped = p64.grad.clone()
        total = torch.nn.utils.clip_grad_norm_([p64], max_norm)
        assert abs(float(total) - norm) <= 1e-12 * norm and float(p64.grad.norm()) < 0.41 * norm
        c = max_norm / (float(total) + 1e-6)                                               # torch's coefficient, from the norm torch returned ...
        assert c < 1 and bool(((p64.grad - unclipped * c).abs() <= 4e-16 * unclipped.abs()).all())      # ... shown to be the one torch applied
        # the reference is fed float32 state, as everywhere in adamw_check: the clipped gradient is the ONE float32 product g * float32(c)
        ref = nr.adamw(inp["p"], np.asarray(inp["g"], dtype=F32) * F32(c), m0, v0, step, HP["lr"], HP["b1"], HP["b2"], HP["eps"], HP["wd"], gs)
        st["p"][:n], st["m"][:n], st["v"][:n] = (torch.from_numpy(np.asarray(a, dtype=F32)).to(dev) for a in (inp["p"], m0, v0))
        slots, coef = sumsq(st["g"], n), torch.zeros(1, device=dev)
        call_clip(st, n, step, gs, slots, 1, max_norm, coef)
        got = {k: st[k][:n].cpu().numpy() for k in ("p", "m", "v")}
        assert abs(float(coef[0]) - max_norm / (norm + 1e-6)) <= 2.0 ** -23 * float(coef[0])
        adamw_check(got, ref, inp["p"], f"clipped, step {step} n={n} grad_scale={gs}")


# ---- the caller's stream -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delay(dev):
    """stream_probe's calibrated delay and proven stream.  torch.cuda.Stream() hands out the 32 streams of torch's pool round-robin, so every call
    moves the ring for the rest of the process; this module takes a whole turn of it, which leaves the modules behind it the streams they met before
    it existed."""
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


def case_accumulate(dev, mode):
    L, n = lb().lib(), 2 ** 20 + 5
    return sp.Case(dict(dst=draws(n, 41, dev), src=draws(n, 42, dev)),
                   lambda b, st: lb().check(L.rdm_grad_accumulate_f32(P(b["dst"]), P(b["src"]), n, mode, st)), outs=("dst",))


def case_sumsq(dev):
    L, n = lb().lib(), 2 ** 20 + 5
    need = int(L.rdm_grad_sumsq_workspace_bytes(n))
    return sp.Case(dict(g=draws(n, 43, dev)), lambda b, st: lb().check(L.rdm_grad_sumsq_f64(P(b["g"]), n, P(b["out"]), P(b["ws"]), need, st)), outs=("out",),
                   scratch=dict(out=torch.empty(1, dtype=torch.float64, device=dev), ws=torch.empty(need // 8, dtype=torch.float64, device=dev)))


def case_clip(dev):
    L, n = lb().lib(), 2 ** 20 + 5
    ins = dict(p=draws(n, 44, dev, 1e-3), g=draws(n, 45, dev), m=draws(n, 46, dev, 0.1), v=draws(n, 47, dev).square(), slots=torch.tensor([2.0e5, 3.0e5], dtype=torch.float64, device=dev))
    return sp.Case(ins, lambda b, st: lb().check(L.rdm_adamw_fused_clip(P(b["p"]), P(b["g"]), P(b["m"]), P(b["v"]), n, 1e-4, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, P(b["slots"]), 2,
                                                                         1.0, P(b["coef"]), st)),
                   outs=("p", "m", "v", "coef"), scratch=dict(coef=torch.empty(1, device=dev)))


@pytest.mark.parametrize("name", ["accumulate copy", "accumulate add", "sumsq", "adamw_fused_clip"])
def test_entry_point_on_a_late_non_default_stream(dev, delay, name):
    """tests/test_gpu_streams.py's late producer: the real inputs reach the poisoned buffers on a non-default stream behind a long delay kernel, the call
    follows on that stream, and its outputs must equal the null-stream run's bit for bit"""
    case = {"accumulate copy": lambda: case_accumulate(dev, 0), "accumulate add": lambda: case_accumulate(dev, 1), "sumsq": lambda: case_sumsq(dev),
            "adamw_fused_clip": lambda: case_clip(dev)}[name]()
    torch.cuda.synchronize()
    sp.check(case, delay)


def test_control_a_call_on_the_null_stream_is_detected(dev, delay):
    case = case_sumsq(dev)
    torch.cuda.synchronize()
    sp.control(case, delay)


# ---- FusedAdamW on the real model's flat buffers ---------------------------------------------------------------------------------------------
def make_model(dev, freeze):
    from md_rdm_amd.network.RDM_Net import DepthEstimationNet
    m = DepthEstimationNet()
    filler.fill_state_dict(m.state_dict())
    m = m.to(dev).train()
    if freeze:
        m.freeze_encoder()
    m.flatten_parameters()
    m.direct_grads = True
    return m


class Recorder:
    """stands in front of the library's optimiser entry points and notes which are called"""
    NAMES = ("rdm_adamw_fused", "rdm_adamw_fused_clip", "rdm_grad_accumulate_f32", "rdm_grad_sumsq_f64")

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


@pytest.mark.parametrize("freeze", [False, True], ids=["all trainable", "frozen encoder"])
def test_fused_adamw_window_and_clip_on_the_flat_buffers(dev, freeze):
    from md_rdm_amd import harness
    L, _lib = lb().lib(), lb()
    m = make_model(dev, freeze)
    flat, gflat, entries = m._flat
    N = flat.numel()
    init = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = harness.FusedAdamW(m, lr=1e-3)
    ranges = opt.trainable_ranges()
    assert freeze or len(ranges) == 2                                                      # [conv_e1 .. last dense layer], [d_1.conv2.*]; d_1.conv1.* lies between
    smalls = [p for p in m.weight_layer.parameters() if p.requires_grad]
    ref_small = [torch.nn.Parameter(p.detach().clone()) for p in smalls]
    ref_opt = torch.optim.AdamW(ref_small, lr=1e-3)
    pref, mref, vref = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    gen = torch.Generator(device=dev).manual_seed(5)

    def window(k, clip):
        """k micro-batches of planted gradients through the optimiser -> (the window's flat sum in the kernel's order, the small gradients' sums)"""
        gs = [torch.randn(N, generator=gen, device=dev) * 1e-3 for _ in range(k)]
        ss = [[torch.randn(p.shape, generator=gen, device=dev) for p in smalls] for _ in range(k)]
        opt.zero_grad()
        assert all(p.grad is None for p in smalls)
        for i in range(k):
            gflat.copy_(gs[i])
            for p, s in zip(smalls, ss[i]):
                p.grad = s.clone() if p.grad is None else p.grad + s                      # as autograd accumulates
            if i < k - 1:
                opt.accumulate_grad()
        opt.step(clip=clip)
        total = gs[0]
        for g in gs[1:-1]:
            total = total + g                                                              # acc = g1; acc += g2; ...
        total = gs[-1] + total if k > 1 else total                                         # g_k += acc
        small = ss[0]
        for s in ss[1:]:
            small = [a + b for a, b in zip(small, s)]
        return total, small

    def reference(total, small, k, step, scale_c=None):
        scale = float(F32(1.0 / k)) if scale_c is None else float(scale_c)
        for a, b in ranges:
            o = lambda t: C.c_void_p(t.data_ptr() + 4 * a)
            _lib.check(L.rdm_adamw_fused(o(pref), o(total), o(mref), o(vref), b - a, opt.lr, opt.betas[0], opt.betas[1], opt.eps, opt.wd, step, scale, _lib.stream()))
        for p, s in zip(ref_small, small):
            p.grad = s * (1.0 / k) if k > 1 else s

    def check(tag):
        assert same(flat, pref) and same(opt.m, mref) and same(opt.v, vref), tag
        for k, p in m.named_parameters():
            if k.startswith("d_1.conv1.") or (freeze and k.startswith("encoder.")):
                assert torch.equal(p.detach(), init[k]), (tag, k)                          # no decay, no moments: bit-unchanged

    # a window of three, no clipping: (g3 + (g1 + g2)) / 3
    total, small = window(3, None)
    reference(total, small, 3, 1)
    ref_opt.step()
    check("window of 3")
    for p, r in zip(smalls, ref_small):
        assert torch.equal(p.detach(), r.detach())
    moved =sum(int(not torch.equal(p.detach(), init[k])) for k, p in m.named_parameters() if p.numel())
    assert moved > 90

    # a window of two with clipping: the coefficient from the slots the step left on the device, formed on the host as the header states
    scale = 0.5
    total2_norm_guess = 1e-3 * math.sqrt(2.0 * sum(b - a for a, b in ranges)) * scale
    max_norm = 0.25 * total2_norm_guess                                                    # well below the norm: the step clips
    total, small = window(2, max_norm)
    n_slots = len(ranges) + 1
    h = opt._slots[:n_slots].cpu().numpy()
    c, scale_c = host_coef(h, max_norm, scale)
    assert c < 1 and same(opt._coef, torch.tensor([c], device=dev))
    reference(total, small, 2, 2, scale_c)
    params = [torch.nn.Parameter(total[a:b] * scale) for a, b in ranges]                   # torch's clip over everything that trains, on the scaled gradient
    for q in params:
        q.grad = q.detach().clone()
    tnorm = torch.nn.utils.clip_grad_norm_(params + ref_small, max_norm)
    ref_opt.step()
    check("clipped window of 2")
    assert abs(float(opt.last_grad_norm) - float(tnorm)) <= 1e-5 * float(tnorm)
    for i, (a, b) in enumerate(ranges):                                                    # one slot per range, then the small gradients'
        want = float(total[a:b].double().square().sum())
        assert abs(float(h[i]) - want) <= 1e-9 * want
    for p, r in zip(smalls, ref_small):                                                    # torch forms its coefficient in float32: 1e-6 of the gradient, less of the step
        np.testing.assert_allclose(p.detach().cpu().numpy(), r.detach().cpu().numpy(), rtol=1e-5, atol=1e-8)

    # defaults: exactly the launches of the plain step
    opt.zero_grad()
    gflat.normal_(generator=gen)
    before = int(L.rdm_launch_count())
    with Recorder() as rec:
        opt.step()
    assert rec.calls == ["rdm_adamw_fused"] * len(ranges) and int(L.rdm_launch_count()) - before == len(ranges)
    with Recorder() as rec:                                                                # and the new paths use the new entry points
        opt.zero_grad()
        opt.accumulate_grad()
        opt.step(clip=1.0)
    assert rec.calls == ["rdm_grad_accumulate_f32"] * (2 * len(ranges)) + ["rdm_grad_sumsq_f64"] * len(ranges) + ["rdm_adamw_fused_clip"] * len(ranges)


def test_clip_with_reduce_scatter_raises(dev):
    from md_rdm_amd import _lib, harness

    class Sync:
        world, exchange = 2, "reduce_scatter"
    m = make_model(dev, False)
    opt = harness.FusedAdamW(m, lr=1e-4, clip=1.0)
    with pytest.raises(_lib.RdmError, match="reduce_scatter"):
        opt.step(sync=Sync())
    with pytest.raises(ValueError):
        harness.FusedAdamW(m, clip=-1.0)


# ---- train.py end to end ---------------------------------------------------------------------------------------------------------------------
def test_train_with_accumulation_and_clipping(dev, capsys, monkeypatch):
    from md_rdm_amd import harness, train
    from md_rdm_amd import utils as u
    monkeypatch.setattr(u, "NAN_LABEL", u.NAN_LABEL)                                       # train.main switches it for the process: put back afterwards
    made = []

    class Capturing(harness.FusedAdamW):
        def __init__(self, model, *a, **kw):
            super().__init__(model, *a, **kw)
            self.start = model._flat[0].detach().clone()
            made.append(self)
    monkeypatch.setattr(harness, "FusedAdamW", Capturing)
    moved = []
    for clip in ("1.0", "1e-9"):
        train.main(["--synthetic", "--batch_size", "2", "--size", "228", "228", "--max_steps", "4", "--accumulate_grad_batches", "2", "--gradient_clip_val", clip, "--seed", "3"])
        out = capsys.readouterr().out
        lines = [ln for ln in out.splitlines() if re.match(r"epoch 0 step \d+ ", ln)]
        assert len(lines) == 2 and [ln.split()[3] for ln in lines] == ["0", "1"], out      # one line per OPTIMISER step
        for ln in lines:
            vals = dict(re.findall(r"(loss|MSE|Ord_Loss|Fine_Detail|grad_norm) (\S+)", ln))
            assert set(vals) == {"loss", "MSE", "Ord_Loss", "Fine_Detail", "grad_norm"} and all(math.isfinite(float(v)) for v in vals.values()), ln
            assert float(vals["grad_norm"]) > 0
        opt = made[-1]
        assert opt.step_count == 2 and opt.clip == float(clip)
        flat = opt.model._flat[0]
        assert bool(torch.isfinite(flat).all())
        moved.append(float((flat - opt.start).double().norm()))
    assert same(made[0].start, made[1].start)                                              # the same start (the seed), so the two distances compare
    print(f"moved {moved[0]:.6g} with clip 1.0, {moved[1]:.6g} with clip 1e-9")
    assert moved[0] > 0 and moved[1] < moved[0]
