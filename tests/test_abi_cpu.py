"""The C-ABI boundary of every public header, derived from the headers themselves (needs no GPU): each header of _lib.HEADERS declares exactly the
names of its ctypes table, no name belongs to two headers, each is exported from its own library and from no other, every parameter and return type
agrees with its ctypes entry, and the build depends on every header.  A wrong ctypes entry loads and launches with garbage arguments; this is its check."""
import ctypes as C
import os
import subprocess

import pytest

import abi_header
from conftest import ROOT

from md_rdm_amd import _lib, build

INCLUDE = os.path.join(ROOT, "include")
# C type -> the ctypes entries that carry it.  A C type that is not here fails the comparison by name: extend the maps on purpose, never around them.
PARAM = {"int32_t": (C.c_int32, C.c_int), "int": (C.c_int32, C.c_int), "int64_t": (C.c_int64,), "size_t": (C.c_size_t,), "double": (C.c_double,),
         "float": (C.c_float,), "rdm_stream_t": (C.c_void_p,)}
RETURN = {"int": C.c_int, "int32_t": C.c_int32, "size_t": C.c_size_t, "int64_t": C.c_int64, "double": C.c_double, "const char*": C.c_char_p, "void": None}


def _carries(ctype, c_type):
    if c_type == "*":
        return ctype in (C.c_void_p, C.c_char_p) or isinstance(ctype, type) and issubclass(ctype, C._Pointer)
    return ctype in PARAM[c_type]


def mismatches(header_text, table):
    """Every disagreement between the declarations of a header and a table {name: (restype, [argtypes])}, one string each; [] when they agree."""
    declared = {name: (ret, params) for ret, name, params in abi_header.declarations(header_text)}
    out = ["%s: declared, not in the table" % n for n in sorted(set(declared) - set(table))]
    out += ["%s: in the table, not declared" % n for n in sorted(set(table) - set(declared))]
    for name in sorted(set(declared) & set(table)):
        (ret, params), (restype, argtypes) = declared[name], table[name]
        if ret not in RETURN:
            out.append("%s: return type %r is not in the map" % (name, ret))
        elif RETURN[ret] is not restype:
            out.append("%s: returns %s, restype is %s" % (name, ret, getattr(restype, "__name__", restype)))
        if len(params) != len(argtypes):
            out.append("%s: %d parameters, %d argtypes" % (name, len(params), len(argtypes)))
            continue
        for i, (param, ctype) in enumerate(zip(params, argtypes)):
            c_type = abi_header.param_type(param)
            if c_type != "*" and c_type not in PARAM:
                out.append("%s: parameter %d %r: type %r is not in the map" % (name, i, param, c_type))
            elif not _carries(ctype, c_type):
                out.append("%s: parameter %d %r is bound as %s" % (name, i, param, ctype.__name__))
    return out


@pytest.fixture(scope="module")
def libs():
    """{is it the bench library: (the loaded library, its defined dynamic symbols)}"""
    build.build(verbose=False)

    def defined(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
        return {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    return {False: (_lib.lib(), defined(_lib.LIB_PATH)), True: (_lib.bench_lib(), defined(_lib.BENCH_LIB_PATH))}


@pytest.mark.parametrize("header", list(_lib.HEADERS))
def test_header_agrees_with_its_table(header, libs):
    table, is_bench = _lib.HEADERS[header], header == _lib.BENCH_HEADER
    text = open(os.path.join(INCLUDE, header)).read()
    names = [name for _, name, _ in abi_header.declarations(text)]
    # same names, and only once: in this header, and in every other header and table
    assert names and len(names) == len(set(names)) and set(names) == set(table) and _lib.symbols(header) == list(table)
    for other in _lib.HEADERS:
        if other != header:
            elsewhere = {name for _, name, _ in abi_header.declarations(open(os.path.join(INCLUDE, other)).read())} | set(_lib.HEADERS[other])
            assert not set(names) & elsewhere, (other, sorted(set(names) & elsewhere))
    # parameter and return types, per declaration
    assert mismatches(text, table) == []
    # exported from its own library and not from the other one, and bound there as the table says
    (L, mine), (_, theirs) = libs[is_bench], libs[not is_bench]
    assert set(names) <= mine and not set(names) & theirs, (sorted(set(names) - mine), sorted(set(names) & theirs))
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    # the build depends on it: the registry is the headers on disk, and the objects are stale when one of them changes
    assert sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h")) == sorted(_lib.HEADERS) and _lib.BENCH_HEADER in _lib.HEADERS
    deps = {bench: {os.path.realpath(p) for p in build.header_deps(bench=bench)} for bench in (False, True)}
    assert os.path.realpath(os.path.join(INCLUDE, header)) in deps[True] and deps[False] <= deps[True]
    assert (os.path.realpath(os.path.join(INCLUDE, header)) in deps[False]) == (not is_bench)
    assert all(os.path.isfile(p) for p in deps[True])


SAMPLE = """
#include "rdm_hip.h"
/* int rdm_hidden(int32_t n); is a comment */
int rdm_one(const float* x, int32_t n, int64_t stride,   // int rdm_also_hidden(void);
            double eps, rdm_stream_t stream);
size_t rdm_two(int32_t batch, size_t bytes);
const char *rdm_three(void);
"""
i32, i64, f32, f64, vp, sz = _lib.i32, _lib.i64, _lib.f32, _lib.f64, _lib.vp, _lib.sz
GOOD = {"rdm_one": (C.c_int, [vp, i32, i64, f64, vp]), "rdm_two": (sz, [i32, sz]), "rdm_three": (C.c_char_p, [])}


def test_the_comparator_reports_each_kind_of_drift():
    """the guard against a parser that matches nothing: one doctored table per kind of error, each reported, and nothing on the matching table"""
    assert [(ret, name, len(params)) for ret, name, params in abi_header.declarations(SAMPLE)] == [("int", "rdm_one", 5), ("size_t", "rdm_two", 2), ("const char*", "rdm_three", 0)]
    assert mismatches(SAMPLE, GOOD) == []
    assert mismatches(SAMPLE, {**GOOD, "rdm_one": (C.c_int, [C.POINTER(f32), C.c_int, i64, f64, vp])}) == []        # the other spellings of the same classes

    def only(table, name, *words):
        got = mismatches(SAMPLE, table)
        assert len(got) == 1 and got[0].startswith(name + ":") and all(w in got[0] for w in words), got
    only({k: v for k, v in GOOD.items() if k != "rdm_two"}, "rdm_two", "not in the table")                       # a missing name
    only({**GOOD, "rdm_four": (C.c_int, [])}, "rdm_four", "not declared")                                         # an extra name
    only({**GOOD, "rdm_one": (C.c_int, [vp, i32, i64, f64])}, "rdm_one", "5 parameters, 4 argtypes")              # one argument too few
    only({**GOOD, "rdm_one": (C.c_int, [vp, i32, i32, f64, vp])}, "rdm_one", "parameter 2", "int64_t stride")     # c_int32 against int64_t
    only({**GOOD, "rdm_one": (C.c_int, [vp, i32, i64, f32, vp])}, "rdm_one", "parameter 3", "c_float")            # c_float against double
    only({**GOOD, "rdm_one": (C.c_int, [i64, i32, i64, f64, vp])}, "rdm_one", "parameter 0")                      # an integer against a pointer
    only({**GOOD, "rdm_one": (C.c_int, [vp, i32, i64, f64, i64])}, "rdm_one", "parameter 4", "rdm_stream_t")      # an integer against the stream
    only({**GOOD, "rdm_two": (C.c_int, [i32, sz])}, "rdm_two", "returns size_t")                                  # a wrong restype
    only({**GOOD, "rdm_three": (None, [])}, "rdm_three", "returns const char*")
    assert any("'unsigned'" in m and "not in the map" in m for m in mismatches("int rdm_u(unsigned n);", {"rdm_u": (C.c_int, [i32])}))
    assert any("'uint8_t'" in m and "not in the map" in m for m in mismatches("uint8_t rdm_u(void);", {"rdm_u": (C.c_int, [])}))
