"""CPU-only: sjmi_filter_plan_compile through ctypes on libsjmi.so (no device is needed, as in test_select_plan.py): which terms
a filter plan accepts, every SJMI_ERR_ARG case of include/sjmi.h, and each limit at its edge; binding.FilterPlan on top."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import filter_common as FC
from tests.conftest import ROOT

SJMI_OK, SJMI_ERR_ARG = 0, -2


def _header():
    return open(os.path.join(ROOT, "include", "sjmi.h")).read()


LIMITS = {k: int(v) for k, v in re.findall(r"#define SJMI_FILTER_(MAX_\w+) (\d+)u", _header())}
OPS = {k.lower(): int(v, 16) for k, v in re.findall(r"#define SJMI_F_(\w+) (0x[0-9A-Fa-f]+)u", _header())}


@pytest.fixture(scope="module")
def lib():
    import simdjson_java_amd as S
    S.build()
    L = C.CDLL(S.lib_path())
    L.sjmi_filter_plan_compile.restype = C.c_int
    L.sjmi_filter_plan_compile.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.sjmi_filter_plan_destroy.restype = None
    L.sjmi_filter_plan_destroy.argtypes = [C.c_void_p]
    return L


def raw_rc(lib, terms, blob=b"", n_terms=None, n_bytes=None, null_terms=False, null_bytes=False):
    """terms: (column, op number, operand word) as they go into sjmi_filter_term"""
    enc = np.zeros(max(len(terms), 1), dtype=FC.TERM)
    for k, t in enumerate(terms):
        enc[k] = t
    consts = np.frombuffer(blob + b"\0", dtype=np.uint8)
    h = C.c_void_p(0xDEAD)
    rc = lib.sjmi_filter_plan_compile(None if null_terms else enc.ctypes.data, len(terms) if n_terms is None else n_terms,
                                      None if null_bytes else consts.ctypes.data, len(blob) if n_bytes is None else n_bytes, C.byref(h))
    if rc == SJMI_OK:
        assert h.value
        lib.sjmi_filter_plan_destroy(h)
    else:
        assert not h.value  # (no plan is handed out with an error)
    return rc


def compile_rc(lib, terms):
    enc, blob = FC.encode(terms)
    return raw_rc(lib, [tuple(int(x) for x in t) for t in enc.tolist()], blob)


def test_the_header_states_the_limits_and_the_ops():
    assert LIMITS == {"MAX_TERMS": 16, "MAX_CONST_BYTES": 1024, "MAX_STRING": 256}
    assert sorted(OPS) == sorted(FC.ALL_OPS) and len(set(OPS.values())) == len(OPS)
    # the reference module's own table of the numbers, which the host simulation's tests encode with
    assert all(OPS[op] == (FC.KINDS[op.split("_")[0]] << 4 | FC.CMPS[op.split("_")[1]]) for op in FC.ALL_OPS)


def test_an_empty_plan(lib):
    assert raw_rc(lib, []) == SJMI_OK
    assert raw_rc(lib, [], null_terms=True, null_bytes=True) == SJMI_OK
    assert lib.sjmi_filter_plan_compile(None, 0, None, 0, None) == SJMI_ERR_ARG  # nowhere to put the plan
    lib.sjmi_filter_plan_destroy(None)


def test_every_op_compiles(lib):
    consts = {"type": ord("t"), "long": -5, "double": 2.5, "string": b"ja"}
    for op in FC.ALL_OPS:
        assert compile_rc(lib, [(3, op, consts[op.split("_")[0]])]) == SJMI_OK, op
    assert compile_rc(lib, [(0, "long_ge", FC.INT64_MIN), (0, "long_le", FC.INT64_MAX), (0xFFFFFFFF, "double_lt", math.inf),
                            (1, "double_gt", -math.inf), (2, "double_eq", -0.0), (0, "type_eq", 0), (0, "type_ne", 255), (1, "string_eq", b"")]) == SJMI_OK


def test_unknown_ops(lib):
    known = set(OPS.values())
    for op in list(range(0, 0x50)) + [0x100, 0x136, 0xFFFFFFFF, 0x80000010]:
        want = SJMI_OK if op in known else SJMI_ERR_ARG
        assert raw_rc(lib, [(0, op, 0)]) == want, hex(op)
    assert raw_rc(lib, [(0, OPS["long_eq"], 1), (0, 0x16, 1)]) == SJMI_ERR_ARG  # the second term's


def test_type_operands(lib):
    for op in ("type_eq", "type_ne"):
        assert raw_rc(lib, [(0, OPS[op], 255)]) == SJMI_OK
        assert raw_rc(lib, [(0, OPS[op], 256)]) == SJMI_ERR_ARG
        assert raw_rc(lib, [(0, OPS[op], 1 << 40)]) == SJMI_ERR_ARG


def test_a_nan_does_not_compile(lib):
    for bits in (FC.bits_of(math.nan), 0x7FF0000000000001, 0xFFF8000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000123):
        for cmp in FC.NUM_CMPS:
            assert raw_rc(lib, [(0, OPS["double_" + cmp], bits)]) == SJMI_ERR_ARG
        assert raw_rc(lib, [(0, OPS["long_eq"], bits)]) == SJMI_OK  # (the same word is an int64 like any other)
    assert raw_rc(lib, [(0, OPS["double_eq"], 0x7FF0000000000000)]) == SJMI_OK and raw_rc(lib, [(0, OPS["double_eq"], 0xFFF0000000000000)]) == SJMI_OK


def test_the_term_limit_at_its_edge(lib):
    term = (0, OPS["type_ne"], 0)
    assert raw_rc(lib, [term] * 16) == SJMI_OK
    assert raw_rc(lib, [term] * 17) == SJMI_ERR_ARG
    assert raw_rc(lib, [term], n_terms=1 << 40) == SJMI_ERR_ARG
    assert raw_rc(lib, [term], null_terms=True) == SJMI_ERR_ARG


def test_the_string_limit_at_its_edge(lib):
    for op in ("string_eq", "string_ne", "string_prefix"):
        assert compile_rc(lib, [(0, op, b"x" * 256)]) == SJMI_OK
        assert compile_rc(lib, [(0, op, b"x" * 257)]) == SJMI_ERR_ARG


def test_the_constants_limit_at_its_edge(lib):
    four = [(k, "string_eq", bytes([65 + k]) * 256) for k in range(4)]
    assert compile_rc(lib, four) == SJMI_OK                                  # 1024 bytes in total
    assert compile_rc(lib, four + [(0, "string_prefix", b"y")]) == SJMI_ERR_ARG  # 1025
    assert raw_rc(lib, [(0, OPS["string_eq"], (1 << 32) | 1023)], b"z" * 1024) == SJMI_OK
    assert raw_rc(lib, [(0, OPS["string_eq"], (1 << 32) | 0)], b"z" * 1025) == SJMI_ERR_ARG
    assert raw_rc(lib, [], b"z" * 1025) == SJMI_ERR_ARG


def test_a_string_constant_outside_the_bytes(lib):
    eq = OPS["string_eq"]
    assert raw_rc(lib, [(0, eq, (3 << 32) | 2)], b"hello") == SJMI_OK           # ends where the bytes end
    assert raw_rc(lib, [(0, eq, (3 << 32) | 3)], b"hello") == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, (0 << 32) | 5)], b"hello") == SJMI_OK           # empty, at the end
    assert raw_rc(lib, [(0, eq, (0 << 32) | 6)], b"hello") == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, (1 << 32) | 0xFFFFFFFF)], b"hello") == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, (0xFFFFFFFF << 32) | 1)], b"hello") == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, (2 << 32) | 0)], b"hello", null_bytes=True) == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, (2 << 32) | 0)], b"hello", n_bytes=1) == SJMI_ERR_ARG
    assert raw_rc(lib, [(0, eq, 0)], b"", null_bytes=True) == SJMI_OK           # an empty constant needs no bytes
    assert raw_rc(lib, [(0, eq, (2 << 32) | 1), (1, OPS["string_prefix"], (3 << 32) | 0)], b"hello") == SJMI_OK  # constants may share bytes


def test_filter_plan_of_the_binding():
    import simdjson_java_amd as S
    S.build()
    plan = S.FilterPlan([(0, "long_gt", 1000), (1, "string_eq", b"ja"), (1, "string_prefix", "j"), (2, "type_ne", 0), (2, "type_eq", "t"),
                         (3, "double_le", 2.5), (0, "long_ge", FC.INT64_MIN)])
    assert plan.n_terms == 7 and plan._h
    plan.close()
    plan.close()
    empty = S.FilterPlan([])
    assert empty.n_terms == 0
    empty.close()
    for bad in ([(0, "long_between", 1)], [(0, "between", 1)], [(0, "string_lt", b"a")], [(0, "type_lt", 0)], [(0, "double_eq", math.nan)],
                [(0, "type_eq", 256)], [(0, "long_eq", 1 << 63)], [(0, "string_eq", b"x" * 257)], [(0, "type_ne", 0)] * 17,
                [(k, "string_ne", b"x" * 205) for k in range(5)]):
        with pytest.raises(ValueError):
            S.FilterPlan(bad)
