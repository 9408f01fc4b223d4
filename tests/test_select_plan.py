"""CPU-only: sjmi_select_plan_compile through ctypes on libsjmi.so (no device is needed, as in test_abi_exports.py): which
JSON Pointers a plan accepts, which it refuses with SJMI_ERR_ARG, and each limit of include/sjmi.h at its edge."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT

SJMI_OK, SJMI_ERR_ARG = 0, -2


def _limits():
    text = open(os.path.join(ROOT, "include", "sjmi.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define SJMI_SELECT_(MAX_\w+) (\d+)u", text)}


LIMITS = _limits()


@pytest.fixture(scope="module")
def lib():
    import simdjson_java_amd as S
    S.build()
    L = C.CDLL(S.lib_path())
    L.sjmi_select_plan_compile.restype = C.c_int
    L.sjmi_select_plan_compile.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.sjmi_select_plan_destroy.restype = None
    L.sjmi_select_plan_destroy.argtypes = [C.c_void_p]
    return L


def compile_rc(lib, pointers):
    ptrs = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    blob = np.frombuffer(b"".join(ptrs) + b"\0", dtype=np.uint8)
    offs = np.zeros(len(ptrs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in ptrs], dtype=np.uint64)
    h = C.c_void_p(0xDEAD)
    rc = lib.sjmi_select_plan_compile(blob.ctypes.data, offs.ctypes.data, len(ptrs), C.byref(h))
    if rc == SJMI_OK:
        assert h.value
        lib.sjmi_select_plan_destroy(h)
    else:
        assert not h.value  # (no plan is handed out with an error)
    return rc


def test_the_header_states_the_limits():
    assert LIMITS == {"MAX_PATHS": 64, "MAX_STEPS": 16, "MAX_NAME_BYTES": 4096}
    src = open(os.path.join(ROOT, "simdjson-java_amd", "csrc", "sj_select.h")).read()
    for name, value in LIMITS.items():
        assert int(re.search(r"SEL_%s\s*=\s*(\d+)" % name, src).group(1)) == value


@pytest.mark.parametrize("pointers", [
    [""], ["/"], ["//"], ["/a"], ["/a/b"], ["/a~0b"], ["/a~1b"], ["/~0"], ["/~1"], ["/~01"], ["/~10"], ["/~0~1~0"], ["/0"], ["/01"], ["/-"],
    ["/a/"], ["/ "], ["/é"], [b"/\xff\xfe"], ['/k"l', "/i\\j"], ["", "", "/a", "/a"], ["/a", "/a/b", "/a/b/c", "/ab"], [],
    ["/99999999999999999999999999999999"],
])
def test_accepted(lib, pointers):
    assert compile_rc(lib, pointers) == SJMI_OK


@pytest.mark.parametrize("pointers", [
    ["a"], ["a/b"], [" /a"], ["~0"], ["0"], ["/a~"], ["/a~2"], ["/~"], ["/~a"], ["/a/~"], ["/a~~0"], ["/~/"], ["/a", "b"], ["/ok", "/bad~"],
    ["#/a"],
])
def test_rejected(lib, pointers):
    assert compile_rc(lib, pointers) == SJMI_ERR_ARG


def test_null_arguments(lib):
    offs = np.zeros(2, dtype=np.uint64)
    assert lib.sjmi_select_plan_compile(None, offs.ctypes.data, 1, None) == SJMI_ERR_ARG
    h = C.c_void_p()
    assert lib.sjmi_select_plan_compile(None, None, 1, C.byref(h)) == SJMI_ERR_ARG
    assert lib.sjmi_select_plan_compile(None, offs.ctypes.data, 1, C.byref(h)) == SJMI_OK  # (one empty pointer: no byte is read)
    lib.sjmi_select_plan_destroy(h)
    lib.sjmi_select_plan_destroy(None)


def test_path_limit_at_its_edge(lib):
    n = LIMITS["MAX_PATHS"]
    assert compile_rc(lib, ["/p%d" % i for i in range(n)]) == SJMI_OK
    assert compile_rc(lib, ["/p%d" % i for i in range(n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, ["/same"] * n) == SJMI_OK
    assert compile_rc(lib, ["/same"] * (n + 1)) == SJMI_ERR_ARG  # (the limit counts paths, not trie nodes)
    assert compile_rc(lib, [""] * n) == SJMI_OK


def test_step_limit_at_its_edge(lib):
    n = LIMITS["MAX_STEPS"]
    assert compile_rc(lib, ["/a" * n]) == SJMI_OK
    assert compile_rc(lib, ["/a" * (n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, ["/" * n]) == SJMI_OK  # (sixteen empty keys)
    assert compile_rc(lib, ["/" * (n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, ["/x", "/a" * (n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, ["/%d" % i for i in range(LIMITS["MAX_PATHS"] - 1)] + ["/z" * n]) == SJMI_OK


def test_name_limit_at_its_edge(lib):
    n = LIMITS["MAX_NAME_BYTES"]
    assert compile_rc(lib, ["/" + "k" * n]) == SJMI_OK
    assert compile_rc(lib, ["/" + "k" * (n + 1)]) == SJMI_ERR_ARG
    # every distinct (prefix, token) pair takes its bytes rounded up to 8: 512 pairs of 8 bytes fill the table ...
    full = ["/" + "/".join("%07d%x" % (p, s) for s in range(16)) for p in range(32)]
    assert compile_rc(lib, full) == SJMI_OK
    assert compile_rc(lib, full + ["/x"]) == SJMI_ERR_ARG  # ... and one more byte needs a ninth word
    assert compile_rc(lib, full + [full[3]]) == SJMI_OK  # (a pair the plan already holds costs nothing)
    assert compile_rc(lib, full + ["", "/"]) == SJMI_OK  # (neither do the root and an empty token)
    # a shared prefix is stored once: 64 paths x 16 steps of 8 bytes would be 8 KiB if it were not
    shared = ["/" + "/".join(["commonab"] * 15 + ["leaf%04d" % p]) for p in range(64)]
    assert compile_rc(lib, shared) == SJMI_OK
    # '~0' and '~1' count as the one byte they stand for
    assert compile_rc(lib, ["/" + "~0" * n]) == SJMI_OK
    assert compile_rc(lib, ["/" + "~1" * (n + 1)]) == SJMI_ERR_ARG
