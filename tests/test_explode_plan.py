"""CPU-only: sjmi_explode_plan_compile through ctypes on libsjmi.so (no device is needed): which base and element pointers an
explode plan accepts, which it refuses with SJMI_ERR_ARG, and each limit of include/sjmi.h at its edge -- the rules of
sjmi_select_plan_compile (tests/test_select_plan.py), for the base and for the element pointers."""
import ctypes as C

import numpy as np
import pytest

from tests.test_select_plan import LIMITS, SJMI_ERR_ARG, SJMI_OK


@pytest.fixture(scope="module")
def lib():
    import simdjson_java_amd as S
    S.build()
    L = C.CDLL(S.lib_path())
    L.sjmi_explode_plan_compile.restype = C.c_int
    L.sjmi_explode_plan_compile.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
    L.sjmi_explode_plan_destroy.restype = None
    L.sjmi_explode_plan_destroy.argtypes = [C.c_void_p]
    return L


def compile_rc(lib, base, pointers):
    base = base.encode("utf-8") if isinstance(base, str) else base
    ptrs = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    bblob = np.frombuffer(base + b"\0", dtype=np.uint8)
    blob = np.frombuffer(b"".join(ptrs) + b"\0", dtype=np.uint8)
    offs = np.zeros(len(ptrs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(p) for p in ptrs], dtype=np.uint64)
    h = C.c_void_p(0xDEAD)
    rc = lib.sjmi_explode_plan_compile(bblob.ctypes.data, len(base), blob.ctypes.data, offs.ctypes.data, len(ptrs), C.byref(h))
    if rc == SJMI_OK:
        assert h.value
        lib.sjmi_explode_plan_destroy(h)
    else:
        assert not h.value  # (no plan is handed out with an error)
    return rc


GOOD = ["", "/", "//", "/a", "/a/b", "/a~0b", "/a~1b", "/~0", "/~1", "/~01", "/0", "/01", "/-", "/a/", "/é", b"/\xff\xfe", '/k"l',
        "/99999999999999999999999999999999"]
BAD = ["a", "a/b", " /a", "~0", "0", "/a~", "/a~2", "/~", "/~a", "/a/~", "/a~~0", "/~/", "#/a"]


@pytest.mark.parametrize("base", GOOD)
def test_accepted_base_pointers(lib, base):
    assert compile_rc(lib, base, ["", "/x"]) == SJMI_OK


@pytest.mark.parametrize("base", BAD)
def test_malformed_base_pointers(lib, base):
    assert compile_rc(lib, base, ["", "/x"]) == SJMI_ERR_ARG
    assert compile_rc(lib, base, []) == SJMI_ERR_ARG


@pytest.mark.parametrize("pointer", GOOD)
def test_accepted_element_pointers(lib, pointer):
    assert compile_rc(lib, "/arr", [pointer]) == SJMI_OK
    assert compile_rc(lib, "", ["/ok", pointer]) == SJMI_OK


@pytest.mark.parametrize("pointer", BAD)
def test_malformed_element_pointers(lib, pointer):
    assert compile_rc(lib, "/arr", [pointer]) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/ok", pointer]) == SJMI_ERR_ARG


def test_an_empty_path_list_and_duplicate_element_pointers(lib):
    assert compile_rc(lib, "/arr", []) == SJMI_OK  # (the offsets alone are worth a call)
    assert compile_rc(lib, "", []) == SJMI_OK
    assert compile_rc(lib, "/arr", ["/a", "/a", "", "", "/a"]) == SJMI_OK
    assert compile_rc(lib, "/arr", ["/same"] * LIMITS["MAX_PATHS"]) == SJMI_OK


def test_null_arguments(lib):
    offs = np.zeros(2, dtype=np.uint64)
    h = C.c_void_p()
    assert lib.sjmi_explode_plan_compile(None, 0, None, offs.ctypes.data, 1, None) == SJMI_ERR_ARG
    assert lib.sjmi_explode_plan_compile(None, 1, None, offs.ctypes.data, 1, C.byref(h)) == SJMI_ERR_ARG  # (a base of one byte at NULL)
    assert lib.sjmi_explode_plan_compile(None, 0, None, None, 1, C.byref(h)) == SJMI_ERR_ARG
    assert lib.sjmi_explode_plan_compile(None, 0, None, offs.ctypes.data, 1, C.byref(h)) == SJMI_OK  # (empty base, one empty pointer: no byte is read)
    lib.sjmi_explode_plan_destroy(h)
    assert lib.sjmi_explode_plan_compile(None, 0, None, None, 0, C.byref(h)) == SJMI_OK
    lib.sjmi_explode_plan_destroy(h)
    lib.sjmi_explode_plan_destroy(None)


def test_path_limit_at_its_edge(lib):
    n = LIMITS["MAX_PATHS"]
    assert compile_rc(lib, "/arr", ["/p%d" % i for i in range(n)]) == SJMI_OK
    assert compile_rc(lib, "/arr", ["/p%d" % i for i in range(n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/arr", ["/same"] * (n + 1)) == SJMI_ERR_ARG  # (the limit counts paths, not trie nodes)
    assert compile_rc(lib, "/arr", [""] * n) == SJMI_OK  # (the base is not one of the 64)


def test_step_limits_at_their_edges(lib):
    n = LIMITS["MAX_STEPS"]
    assert compile_rc(lib, "/a" * n, ["/b" * n]) == SJMI_OK  # (sixteen steps each: the two are not added up)
    assert compile_rc(lib, "/a" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/a" * (n + 1), []) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/b" * (n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/" * n, ["/" * n]) == SJMI_OK  # (sixteen empty keys)
    assert compile_rc(lib, "/" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/a", ["/x", "/b" * (n + 1)]) == SJMI_ERR_ARG


def test_name_limits_at_their_edges(lib):
    n = LIMITS["MAX_NAME_BYTES"]
    assert compile_rc(lib, "/" + "k" * n, ["/" + "e" * n]) == SJMI_OK  # (a table for the base and one for the element pointers)
    assert compile_rc(lib, "/" + "k" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/" + "e" * (n + 1)]) == SJMI_ERR_ARG
    full = ["/" + "/".join("%07d%x" % (p, s) for s in range(16)) for p in range(32)]
    assert compile_rc(lib, "/base", full) == SJMI_OK
    assert compile_rc(lib, "/base", full + ["/x"]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/base", full + [full[3], ""]) == SJMI_OK


def test_no_device_is_needed(lib):
    """the binding's ExplodePlan compiles and closes without a context"""
    import simdjson_java_amd as S
    plan = S.ExplodePlan("/statuses", ["/id", "/user/name", ""])
    assert plan.n_paths == 3 and plan.base == b"/statuses"
    plan.close()
    with pytest.raises(ValueError):
        S.ExplodePlan("statuses", ["/id"])
    with pytest.raises(ValueError):
        S.ExplodePlan("/statuses", ["id"])
    assert {"sjmi_explode_plan_compile", "sjmi_explode_plan_destroy", "sjmi_explode_batch_device"} <= set(S.binding.EXPORTS)
