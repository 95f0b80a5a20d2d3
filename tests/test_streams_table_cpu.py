"""The table of tests/test_gpu_streams.py against include/rdm_hip.h (needs no GPU): every declaration with an rdm_stream_t parameter is a row of
the table or an explicitly exempted function that enqueues no device work, and neither names anything the header does not declare."""
import importlib
import inspect
import os
import re

import conftest
import test_gpu_streams as T
from abi_header import stream_taking_declarations

HEADER = os.path.join(conftest.ROOT, "include", "rdm_hip.h")


def test_the_parser_sees_the_header():
    names = stream_taking_declarations(open(HEADER).read())
    assert len(names) == len(set(names)) and len(names) >= 70
    for known in ("rdm_conv2d_fwd", "rdm_net_backward_stage", "rdm_adamw_fused", "rdm_als_rank1_paged", "rdm_eval_target_metrics_f64"):
        assert known in names
    for streamless in ("rdm_net_create", "rdm_als_workspace_bytes", "rdm_profile_read", "rdm_net_route"):
        assert streamless not in names
    sample = "int rdm_a(const float* x, rdm_stream_t stream);\nsize_t rdm_b(int32_t n);\n/* int rdm_c(rdm_stream_t s); */\nint rdm_d(int32_t n,\n   rdm_stream_t s);"
    assert stream_taking_declarations(sample) == ["rdm_a", "rdm_d"]


def test_every_stream_taking_entry_point_is_a_row_or_exempt():
    declared = set(stream_taking_declarations(open(HEADER).read()))
    rows, exempt = set(T.ROWS), set(T.EXEMPT)
    assert not rows & exempt, sorted(rows & exempt)
    assert not declared - rows - exempt, "declared in the header, neither a row nor exempt: %s" % sorted(declared - rows - exempt)
    assert not rows - declared, "rows the header does not declare: %s" % sorted(rows - declared)
    assert not exempt - declared, "exemptions the header does not declare: %s" % sorted(exempt - declared)
    for name, reason in T.EXEMPT.items():
        assert isinstance(reason, str) and reason.strip() and "\n" not in reason, name


def test_rows_are_runnable_and_every_family_has_a_control():
    families = set()
    for name, (family, how) in T.ROWS.items():
        families.add(family)
        if callable(how):
            assert how.__name__.startswith("row_"), name
        else:
            assert callable(getattr(T, how, None)) and how.startswith("test_plan_"), (name, how)     # a whole-plan test of the module drives it
    assert families - {"plan"} == set(T.CONTROLS), (sorted(families), sorted(T.CONTROLS))
    for family, name in T.CONTROLS.items():
        assert T.ROWS[name][0] == family and callable(T.ROWS[name][1])
    assert callable(T.test_control_plan_forward_on_the_null_stream_is_detected)                      # the plan family's control


def _calls(source, name):
    """`<library>.name` appears: called, or picked as the function to call"""
    return re.search(r"\.%s\b" % re.escape(name), source) is not None


def _source_with_helpers(fn):
    """source of a builder / test plus the module-level helpers of the table's module that it names (one level)"""
    src = inspect.getsource(fn)
    for helper, obj in vars(T).items():
        if inspect.isfunction(obj) and obj is not fn and obj.__module__ == T.__name__ and re.search(r"\b%s\b" % re.escape(helper), src):
            src += inspect.getsource(obj)
    return src


def test_every_row_reaches_the_entry_point_it_is_keyed_by():
    """the builder (or the whole-plan test) calls the entry point by name, or names a product wrapper (VIA) whose source calls it"""
    assert not set(T.VIA) - set(T.ROWS), sorted(set(T.VIA) - set(T.ROWS))
    for name, (family, how) in T.ROWS.items():
        fn = how if callable(how) else getattr(T, how)
        src = _source_with_helpers(fn)
        if name in T.VIA:
            mod, path = T.VIA[name].split(":")
            obj = importlib.import_module(mod)
            for part in path.split("."):
                obj = getattr(obj, part)
            assert _calls(inspect.getsource(obj), name), (name, T.VIA[name])
        else:
            assert _calls(src, name), "%s: %s never calls it" % (name, fn.__name__)
