"""The plan's routing table (csrc/net.hip resolve_routes, read through rdm_net_route): structural invariants between the kernel family of each
GEMM and the operand encodings its producers write, over a sweep of geometries and options, and the values that ship at the headline
geometry.  CPU only: a plan needs no device."""
import ctypes as C
import itertools

import pytest

from md_rdm_amd import _lib

LAYERS = (6, 12, 36, 24)
BATCHES = (1, 2, 3, 4, 8, 16)
SIZES = ((33, 33), (97, 129), (228, 228), (228, 304), (352, 1216))
SHIPPED = {_lib.NET_OPT_SPLIT_BWD: 1, _lib.NET_OPT_SPLIT_FWD: 1}           # what DepthEstimationNet sets on top of the library's defaults
OPTION_SETS = {
    "shipped": {},
    "f32": {_lib.NET_OPT_SPLIT_BWD: 0, _lib.NET_OPT_SPLIT_FWD: 0},
    "deterministic": {_lib.NET_OPT_DETERMINISTIC: 1},
    "gemm_bf16_1": {_lib.NET_OPT_GEMM_BF16: 1},
    "gemm_bf16_2": {_lib.NET_OPT_GEMM_BF16: 2},
    "gemm_bf16_3": {_lib.NET_OPT_GEMM_BF16: 3},
    "no_split_rows": {_lib.NET_OPT_SPLIT_ROWS: 0},
    "no_defer_norm1": {_lib.NET_OPT_DEFER_NORM1: 0},
}
BITS = ("PIPELINED", "RAW", "WINO_FWD", "WINO_X6", "XF", "DEFER", "WG3_XS", "WG3_WINO", "DG3_XS", "DG1_XS", "WG1_XS", "NP1", "G_FRAME", "DZ_BF16",
        "DY_SPLIT", "XH_SPLIT")                                            # rdm_net_route_flags, bit 0 upwards
XS_BITS = ("WG3_XS", "DG3_XS", "DG1_XS", "WG1_XS")


@pytest.fixture(scope="module")
def L():
    from md_rdm_amd import build
    build.build(verbose=False)
    return _lib.lib()


def block_pixels(B, H, W):
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1          # 7x7 / stride 2 / pad 3 stem
    h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1          # 3x3 / stride 2 / pad 1 max-pool
    out = []
    for _ in range(4):
        out.append(B * h * w)
        h, w = (h + 1) // 2, (w + 1) // 2              # transition: pad bottom / right, 2x2 average pool
    return out


class Plan:
    def __init__(self, L, B, H, W, options):
        self.L, self.h = L, C.c_void_p()
        _lib.check(L.rdm_net_create(B, H, W, C.byref(self.h)))
        for k, v in {**SHIPPED, **options}.items():
            self.set(k, v)

    def set(self, option, value):
        _lib.check(self.L.rdm_net_set_option(self.h, option, value))

    def route(self, b, i, has_grad):
        f = C.c_int32()
        _lib.check(self.L.rdm_net_route(self.h, b, i, has_grad, C.byref(f)))
        return {name for k, name in enumerate(BITS) if f.value >> k & 1}

    def table(self):
        return [[(self.route(b, i, 0), self.route(b, i, 1)) for i in range(LAYERS[b])] for b in range(4)]

    def close(self):
        self.L.rdm_net_destroy(self.h)


def test_flag_names_match_the_header():
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    body = re.search(r"typedef enum rdm_net_route_flags \{(.*?)\} rdm_net_route_flags;", hdr, re.S).group(1)
    found = re.findall(r"RDM_ROUTE_([A-Z0-9_]+) = 1 << (\d+)", body)
    assert [(n, int(k)) for n, k in found] == [(n, k) for k, n in enumerate(BITS)]


@pytest.mark.parametrize("opts", list(OPTION_SETS))
def test_encodings_follow_the_kernel_routes(L, opts):
    """For every layer of every block: an operand encoding is only written where every kernel that reads it can read it."""
    for B, (H, W) in itertools.product(BATCHES, SIZES):
        if B * H * W >= 1 << 28:
            continue
        p = Plan(L, B, H, W, OPTION_SETS[opts])
        pixels = block_pixels(B, H, W)
        try:
            for b, layers in enumerate(p.table()):
                where = (opts, B, H, W, b)
                for r0, r1 in layers:
                    for has_grad, r in ((0, r0), (1, r1)):
                        np3 = "NP1" not in r
                        if "DY_SPLIT" in r:
                            assert "DG1_XS" in r and np3 and (not has_grad or "WG1_XS" in r), where
                        if "XH_SPLIT" in r:
                            assert "WG1_XS" in r and np3 and has_grad, where
                        if "G_FRAME" in r:
                            assert "WG3_XS" in r and np3, where
                        if "DZ_BF16" in r:
                            assert not np3 and {"DG3_XS", "DG1_XS", "WG1_XS"} <= r, where
                        assert not {"WG3_XS", "WG3_WINO"} <= r, where
                        if "WINO_X6" in r:
                            assert "WINO_FWD" in r, where
                        if "RAW" in r:
                            assert "PIPELINED" in r, where
                        if r & set(XS_BITS):
                            assert pixels[b] >= 1024, where              # the sizes plan() lays the pack buffers out for
                        if "XF" in r:
                            assert pixels[b] >= 8192, where
                        if opts == "deterministic":
                            assert not r & (set(XS_BITS) | {"XF", "PIPELINED", "RAW"}), where
                    # only the encodings depend on the gradient slot
                    enc = {"G_FRAME", "DZ_BF16", "DY_SPLIT", "XH_SPLIT"}
                    assert r0 - enc == r1 - enc, where
                defer = {"DEFER" in r for pair in layers for r in pair}
                assert len(defer) == 1, where                            # uniform over the block
                if defer == {True}:
                    assert all("DG1_XS" in r for pair in layers for r in pair), where
                block_bits = {"PIPELINED", "RAW", "WINO_FWD", "WINO_X6", "XF", "DEFER"}
                assert len({frozenset(r & block_bits) for pair in layers for r in pair}) == 1, where
        finally:
            p.close()


def test_table_is_a_pure_function_of_geometry_and_options(L):
    a, b = Plan(L, 4, 228, 304, {}), Plan(L, 4, 228, 304, {})
    try:
        t = a.table()
        assert t == b.table()
        assert any("DG1_XS" in r for blk in t for pair in blk for r in pair)
        a.set(_lib.NET_OPT_SPLIT_BWD, 0)                                   # after a query: the table follows the option
        assert not any(r & (set(XS_BITS) | {"DEFER", "G_FRAME", "DY_SPLIT", "XH_SPLIT"}) for blk in a.table() for pair in blk for r in pair)
        a.set(_lib.NET_OPT_JOIN_PER_SEGMENT, 1)                            # routes nothing
        a.set(_lib.NET_OPT_SPLIT_BWD, 1)
        assert a.table() == t
        a.set(_lib.NET_OPT_GEMM_BF16, 3)
        assert all("NP1" in r for blk in a.table() for pair in blk for r in pair)
        a.set(_lib.NET_OPT_GEMM_BF16, 0)
        a.set(_lib.NET_OPT_SPLIT_FWD, 0)
        assert not any("XF" in r for blk in a.table() for pair in blk for r in pair)
    finally:
        a.close()
        b.close()


def test_bad_arguments_are_status_codes(L):
    p = Plan(L, 1, 33, 33, {})
    f = C.c_int32()
    try:
        assert L.rdm_net_route(p.h, 4, 0, 1, C.byref(f)) == -1
        assert L.rdm_net_route(p.h, 0, 6, 1, C.byref(f)) == -1 and b"no layer 6" in L.rdm_last_error_string()
        assert L.rdm_net_route(p.h, -1, 0, 1, C.byref(f)) == -1
        assert L.rdm_net_route(p.h, 0, 0, 1, None) == -1
        assert L.rdm_net_route(None, 0, 0, 1, C.byref(f)) == -1
    finally:
        p.close()


def test_headline_geometry_routes_what_ships(L):
    """B=16 228x304 with the shipped options: dense blocks of 69 312 / 17 632 / 4 560 / 1 280 pixels."""
    assert block_pixels(16, 228, 304) == [69312, 17632, 4560, 1280]
    p = Plan(L, 16, 228, 304, {})
    try:
        t = p.table()
    finally:
        p.close()
    for b in range(4):
        for r0, r1 in t[b]:
            # every gradient GEMM but the 3x3 weight gradient of the two few-pixel blocks (4 560, 1 280 < 8 192) on the split kernels
            assert {"DG3_XS", "DG1_XS", "WG1_XS", "DEFER"} <= r1 and "NP1" not in r1, (b, r1)
            assert ("WG3_XS" in r1) == (b < 2) and "WG3_WINO" not in r1, (b, r1)
            assert ("XF" in r1) == (b < 2) and ("WINO_FWD" in r1) == (b < 2) and "WINO_X6" not in r1, (b, r1)
            assert ("PIPELINED" in r1) == (b >= 2) and ("RAW" in r1) == (b >= 2), (b, r1)
            assert ("G_FRAME" in r1) == (b < 2), (b, r1)
            assert {"DY_SPLIT", "XH_SPLIT"} <= r1 and "DZ_BF16" not in r1, (b, r1)
            assert "DY_SPLIT" in r0 and "XH_SPLIT" not in r0, (b, r0)
