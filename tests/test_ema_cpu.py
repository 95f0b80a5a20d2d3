"""The weight average without a GPU: the float64 restatements of tests/ema_ref.py, the decay schedule, the C-ABI boundary of include/rdm_ema.h
(declared == bound == exported; every refusal is a status code with a message before any launch), FusedAdamW's state keys on a stub model (there is
no CPU path for the update itself), the new flags of the three commands, and from_lightning(ema=True) on a checkpoint without averaged weights."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ema_ref as er
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "rdm_ema.h")
NAMES = {"rdm_adamw_fused_ema", "rdm_ema_swap_f32"}
F32 = np.float32


def lib():
    from md_rdm_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------
def test_update_restatement():
    e, w = np.array([1.0, -2.0, 0.0], F32), np.array([3.0, -2.0, 1.0], F32)
    assert er.one_minus(0.9) == np.float64(F32(1.0) - F32(0.9)) != 1.0 - 0.9                # the float32-rounded 1 - d, not the float64 one
    got = er.ema_step(e, w, 0.9)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, e.astype(np.float64) + er.one_minus(0.9) * (w.astype(np.float64) - e.astype(np.float64)))
    np.testing.assert_array_equal(er.ema_step(e, w, 1.0), e)                                 # decay 1: the average stays
    np.testing.assert_array_equal(er.ema_step(e, w, 0.0), w)                                 # decay 0: the average is the weight
    avg, M = er.ema_replay(e, [w, w, w], [0.5, 0.5, 0.5])
    np.testing.assert_allclose(avg, w - (w.astype(np.float64) - e) / 8.0, rtol=0, atol=1e-15)
    assert M == 3.0 and er.bound(4, 2.0) == 5.0 * 4 * 2.0 ** -24 * 2.0


def test_decay_schedule():
    from md_rdm_amd import harness
    f = harness.ema_decay_at
    assert f(0.999, 0) == float(F32(0.1)) and f(0.999, 1) == float(F32(2.0 / 11.0))
    assert f(0.999, 10 ** 7) == float(F32(0.999)) and f(0.999, 8900) < float(F32(0.999)) == f(0.999, 9100)       # (1 + u) / (10 + u) = 0.999 at u = 8990
    for u in (0, 1, 5, 10 ** 6):
        assert f(0.999, u, warmup=False) == float(F32(0.999)) == f(0.999, u, False)
    assert f(0.05, 0) == float(F32(0.05))                                                    # a decay below the ramp holds from the start
    for d in (0.0, 0.5, 0.9, 0.999, 0.9999, 1.0):
        for u in (0, 1, 2, 9, 10, 100, 8990, 8991, 10 ** 5):
            for wu in (True, False):
                got = f(d, u, wu)
                assert got == er.decay_at(d, u, wu) and got == float(F32(got)) and 0.0 <= got <= 1.0, (d, u, wu)
    seq = [f(0.999, u) for u in range(20000)]
    assert seq == sorted(seq)                                                                # the ramp never steps back


# ---- the C ABI of include/rdm_ema.h ----------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_bound():
    from md_rdm_amd import _lib
    assert set(_lib.symbols("rdm_ema.h")) == NAMES          # declared == bound == exported, with the header's types: test_abi_cpu.py
    hip_h = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    for name in NAMES:
        assert name not in hip_h                                                              # rdm_hip.h keeps its declaration set
    assert '#include "rdm_optim.h"' in open(HEADER).read()
    # the clipped step's arguments with ema after exp_avg_sq and ema_decay before the stream
    clip, ema = _lib.HEADERS["rdm_optim.h"]["rdm_adamw_fused_clip"][1], _lib.HEADERS["rdm_ema.h"]["rdm_adamw_fused_ema"][1]
    assert ema == clip[:4] + [_lib.vp] + clip[4:-1] + [_lib.f32, _lib.vp]


def test_every_refusal_is_a_status_code_before_the_launch():
    """no GPU here: a call that got as far as a launch could not return RDM_ERR_BAD_ARGUMENT with these messages"""
    _, L = lib()
    p, q, odd4, odd8 = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(4100), C.c_void_p(4104)
    err = L.rdm_last_error_string

    def refused(rc, word, tag):
        assert rc == -1 and tag in err() and word in err(), (rc, err())

    good = dict(p=p, g=p, m=p, v=p, e=q, n=64, step=1, sumsq=None, slots=0, max_norm=0.0, coef=None, decay=0.9)
    clipped = dict(good, sumsq=p, slots=3, max_norm=1.0)
    nan = float("nan")
    rows = [(good, dict(p=None), b"bad argument"), (good, dict(g=None), b"bad argument"), (good, dict(m=None), b"bad argument"), (good, dict(v=None), b"bad argument"),
            (good, dict(n=-1), b"bad argument"), (good, dict(step=0), b"bad argument"), (good, dict(p=odd4), b"16-byte"), (good, dict(v=odd8), b"16-byte"),
            (good, dict(e=None), b"ema must"), (good, dict(e=odd4), b"ema must"), (good, dict(e=C.c_void_p((1 << 20) + 8)), b"ema must"),
            (good, dict(e=p), b"overlaps"), (good, dict(e=C.c_void_p(4096 + 4 * 48)), b"overlaps"), (good, dict(e=C.c_void_p(4096 - 4 * 60)), b"overlaps"),
            (good, dict(decay=-0.01), b"ema_decay"), (good, dict(decay=1.0001), b"ema_decay"), (good, dict(decay=nan), b"ema_decay"),
            (good, dict(slots=1), b"n_slots"), (good, dict(sumsq=p), b"n_slots"),                 # NULL with slots, slots without NULL
            (clipped, dict(p=None), b"bad argument"), (clipped, dict(e=None), b"ema must"), (clipped, dict(decay=nan), b"ema_decay"),
            (clipped, dict(sumsq=odd4), b"sumsq"), (clipped, dict(slots=9), b"n_slots"), (clipped, dict(slots=-1), b"n_slots"),
            (clipped, dict(max_norm=-1.0), b"max_norm"), (clipped, dict(max_norm=nan), b"max_norm"), (clipped, dict(coef=C.c_void_p(4098)), b"coef_out")]
    for base, change, word in rows:
        kw = dict(base, **change)
        rc = L.rdm_adamw_fused_ema(kw["p"], kw["g"], kw["m"], kw["v"], kw["e"], kw["n"], 1e-4, 0.9, 0.999, 1e-8, 0.01, kw["step"], 1.0, kw["sumsq"], kw["slots"],
                                   kw["max_norm"], kw["coef"], kw["decay"], None)
        refused(rc, word, b"adamw_fused_ema")
    # ranges that touch without sharing a byte are accepted as far as the argument checks go: n = 0 returns before any launch
    assert L.rdm_adamw_fused_ema(p, p, p, p, p, 0, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 1.0, None, 0, 0.0, None, 0.9, None) == 0

    swap = L.rdm_ema_swap_f32
    refused(swap(None, q, 8, None), b"NULL", b"ema_swap")
    refused(swap(p, None, 8, None), b"NULL", b"ema_swap")
    refused(swap(odd4, q, 8, None), b"aligned", b"ema_swap")
    refused(swap(p, odd8, 8, None), b"aligned", b"ema_swap")
    refused(swap(p, q, -1, None), b"negative", b"ema_swap")
    refused(swap(p, p, 8, None), b"overlap", b"ema_swap")
    refused(swap(p, C.c_void_p(4096 + 16), 8, None), b"overlap", b"ema_swap")
    refused(swap(C.c_void_p(4096 + 16), p, 5, None), b"overlap", b"ema_swap")
    assert swap(p, q, 0, None) == 0 and swap(p, p, 0, None) == 0                               # n = 0: nothing to overlap, nothing launched


# ---- FusedAdamW's state on a stub model ------------------------------------------------------------------------------------------------------
class StubModel:
    """what FusedAdamW's constructor, state_dict and load_state_dict touch: four scalars and a flat buffer"""

    def __init__(self):
        self.weight_layer = torch.nn.ParameterList([torch.nn.Parameter(torch.tensor(float(i + 1))) for i in range(4)])
        self._flat = (torch.arange(128, dtype=torch.float32), torch.zeros(128), [])


OLD_KEYS = {"step", "lr", "exp_avg", "exp_avg_sq", "small"}


def test_state_keys_unchanged_when_off_and_extended_when_on():
    import inspect

    from md_rdm_amd import harness
    sig = inspect.signature(harness.FusedAdamW.__init__)
    assert sig.parameters["ema_decay"].default is None and sig.parameters["ema_warmup"].default is True
    off = harness.FusedAdamW(StubModel())
    assert set(off.state_dict()) == OLD_KEYS and off.ema is None and off.ema_small is None    # no new key, no new buffer
    on = harness.FusedAdamW(StubModel(), ema_decay=0.9)
    assert set(on.state_dict()) == OLD_KEYS | {"ema", "ema_small", "ema_updates", "ema_decay"}
    assert on.state_dict()["ema"] is None and on.state_dict()["ema_decay"] == 0.9             # before the first step: nothing allocated yet
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            harness.FusedAdamW(StubModel(), ema_decay=bad)


def test_state_round_trip_and_a_state_without_the_average():
    from md_rdm_amd import harness
    a = harness.FusedAdamW(StubModel(), ema_decay=0.9)
    a.m, a.v = torch.full((128,), 0.5), torch.full((128,), 0.25)
    a.ema, a.ema_small, a.ema_updates, a.step_count = torch.arange(128, dtype=torch.float32) * 0.5, [torch.tensor(float(-i)) for i in range(4)], 7, 7
    sd = a.state_dict()
    b = harness.FusedAdamW(StubModel(), ema_decay=0.9)
    b.load_state_dict(sd)
    assert torch.equal(b.ema, a.ema) and b.ema_updates == 7 and all(torch.equal(x, y) for x, y in zip(b.ema_small, a.ema_small))
    assert b.ema.data_ptr() != sd["ema"].data_ptr()
    old = {k: v for k, v in sd.items() if k in OLD_KEYS}                                      # a state from a run without the average
    b.load_state_dict(old)
    assert b.ema is None and b.ema_small is None and b.ema_updates == 0 and b.step_count == 7 # re-seeded at the next step
    c = harness.FusedAdamW(StubModel())                                                       # the average off: the entries are ignored
    c.load_state_dict(sd)
    assert c.ema is None and set(c.state_dict()) == OLD_KEYS
    sd["ema"] = torch.zeros(64)
    with pytest.raises(ValueError):
        b.load_state_dict(sd)


def test_swap_without_the_average_raises():
    from md_rdm_amd import _lib, harness
    off = harness.FusedAdamW(StubModel())
    with pytest.raises(_lib.RdmError, match="ema_decay"):
        off.swap_ema()
    with pytest.raises(_lib.RdmError, match="ema_decay"):
        with off.ema_weights():
            pass


# ---- the commands' flags ---------------------------------------------------------------------------------------------------------------------
def test_train_flags():
    from md_rdm_amd import train
    P = train.build_parser()
    a = P.parse_args([])
    assert a.ema_decay is None and a.no_ema_warmup is False                                   # the defaults: the loop of before
    a = P.parse_args(["--ema_decay", "0.999", "--no_ema_warmup"])
    assert a.ema_decay == 0.999 and a.no_ema_warmup is True
    with pytest.raises(SystemExit):
        P.parse_args(["--ema_decay", "most"])
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit) as e:                                                  # refused with a message, before anything touches a GPU
            train.main(["--synthetic", "--ema_decay", bad])
        assert "--ema_decay" in str(e.value), e.value


def test_evaluate_and_predict_flags():
    from md_rdm_amd import evaluate, predict
    for mod, argv in ((evaluate, ["--synthetic", "2"]), (predict, ["--synthetic", "2", "--out", "unused"])):
        P = mod.build_parser()
        assert P.parse_args(argv).ema is False
        assert P.parse_args(argv + ["--ema", "--checkpoint", "x.ckpt"]).ema is True
        with pytest.raises(SystemExit) as e:                                                  # the averaged weights live in a checkpoint
            mod.main(argv + ["--ema"])
        assert "--ema needs --checkpoint" in str(e.value), e.value


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------------------
def test_from_lightning_ema_needs_the_entry(tmp_path):
    from md_rdm_amd import checkpoint

    class Model:
        loaded = None

        def load_state_dict(self, sd, strict=True):
            self.loaded = sd
            return "ok"
    live, avg = {"model.w": torch.ones(2)}, {"model.w": torch.zeros(2)}
    m = Model()
    with pytest.raises(KeyError, match="state_dict_ema") as e:
        checkpoint.from_lightning(m, {"state_dict": live}, ema=True)
    assert isinstance(e.value, checkpoint.NoAveragedWeights) and m.loaded is None
    path = str(tmp_path / "plain.ckpt")
    torch.save({"state_dict": live}, path)
    with pytest.raises(checkpoint.NoAveragedWeights, match="plain.ckpt"):                     # the error names the file
        checkpoint.from_lightning(m, path, ema=True)
    res, _ = checkpoint.from_lightning(m, {"state_dict": live, "state_dict_ema": avg}, ema=True)
    assert res == "ok" and set(m.loaded) == {"w"} and torch.equal(m.loaded["w"], avg["model.w"])
    checkpoint.from_lightning(m, {"state_dict": live, "state_dict_ema": avg})                 # the default stays the live weights
    assert torch.equal(m.loaded["w"], live["model.w"])
