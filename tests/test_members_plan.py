"""CPU-only: sjmi_explode_members_plan_compile through ctypes on libsjmi.so (no device is needed): the rules, limits and
SJMI_ERR_ARG cases of sjmi_explode_plan_compile (tests/test_explode_plan.py, whose pointer lists are used here), with one
difference -- at most SJMI_EXPLODE_MEMBERS_MAX_PATHS element pointers, read from include/sjmi.h: the key takes the 64th cell."""
import ctypes as C

import numpy as np
import pytest

from tests import members_common as MC
from tests.test_explode_plan import BAD, GOOD
from tests.test_select_plan import LIMITS, SJMI_ERR_ARG, SJMI_OK

MAX_PATHS = MC.header_constant("SJMI_EXPLODE_MEMBERS_MAX_PATHS")


@pytest.fixture(scope="module")
def lib():
    import simdjson_java_amd as S
    S.build()
    L = C.CDLL(S.lib_path())
    L.sjmi_explode_members_plan_compile.restype = C.c_int
    L.sjmi_explode_members_plan_compile.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
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
    rc = lib.sjmi_explode_members_plan_compile(bblob.ctypes.data, len(base), blob.ctypes.data, offs.ctypes.data, len(ptrs), C.byref(h))
    if rc == SJMI_OK:
        assert h.value
        lib.sjmi_explode_plan_destroy(h)  # (the same plan type, the same destroy)
    else:
        assert not h.value  # (no plan is handed out with an error)
    return rc


def test_the_limit_is_the_headers():
    assert MAX_PATHS == LIMITS["MAX_PATHS"] - 1 == 63


def test_path_limit_at_its_edge(lib):
    assert compile_rc(lib, "/obj", ["/p%d" % i for i in range(MAX_PATHS)]) == SJMI_OK
    assert compile_rc(lib, "/obj", ["/p%d" % i for i in range(MAX_PATHS + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/obj", ["/same"] * (MAX_PATHS + 1)) == SJMI_ERR_ARG  # (the limit counts paths, not trie nodes)
    assert compile_rc(lib, "/obj", [""] * MAX_PATHS) == SJMI_OK
    assert compile_rc(lib, "", [""] * (MAX_PATHS + 1)) == SJMI_ERR_ARG


@pytest.mark.parametrize("base", GOOD)
def test_accepted_base_pointers(lib, base):
    assert compile_rc(lib, base, ["", "/x"]) == SJMI_OK


@pytest.mark.parametrize("base", BAD)
def test_malformed_base_pointers(lib, base):
    assert compile_rc(lib, base, ["", "/x"]) == SJMI_ERR_ARG
    assert compile_rc(lib, base, []) == SJMI_ERR_ARG


@pytest.mark.parametrize("pointer", GOOD)
def test_accepted_element_pointers(lib, pointer):
    assert compile_rc(lib, "/obj", [pointer]) == SJMI_OK
    assert compile_rc(lib, "", ["/ok", pointer]) == SJMI_OK


@pytest.mark.parametrize("pointer", BAD)
def test_malformed_element_pointers(lib, pointer):
    assert compile_rc(lib, "/obj", [pointer]) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/ok", pointer]) == SJMI_ERR_ARG


def test_an_empty_path_list_and_duplicate_element_pointers(lib):
    assert compile_rc(lib, "/obj", []) == SJMI_OK  # (the key column alone)
    assert compile_rc(lib, "", []) == SJMI_OK
    assert compile_rc(lib, "/obj", ["/a", "/a", "", "", "/a"]) == SJMI_OK


def test_null_arguments(lib):
    offs = np.zeros(2, dtype=np.uint64)
    h = C.c_void_p()
    f = lib.sjmi_explode_members_plan_compile
    assert f(None, 0, None, offs.ctypes.data, 1, None) == SJMI_ERR_ARG
    assert f(None, 1, None, offs.ctypes.data, 1, C.byref(h)) == SJMI_ERR_ARG  # (a base of one byte at NULL)
    assert f(None, 0, None, None, 1, C.byref(h)) == SJMI_ERR_ARG
    assert f(None, 0, None, offs.ctypes.data, 1, C.byref(h)) == SJMI_OK  # (empty base, one empty pointer: no byte is read)
    lib.sjmi_explode_plan_destroy(h)
    assert f(None, 0, None, None, 0, C.byref(h)) == SJMI_OK
    lib.sjmi_explode_plan_destroy(h)


def test_step_limits_at_their_edges(lib):
    n = LIMITS["MAX_STEPS"]
    assert compile_rc(lib, "/a" * n, ["/b" * n]) == SJMI_OK
    assert compile_rc(lib, "/a" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/a" * (n + 1), []) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/b" * (n + 1)]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "/a", ["/x", "/b" * (n + 1)]) == SJMI_ERR_ARG


def test_name_limits_at_their_edges(lib):
    n = LIMITS["MAX_NAME_BYTES"]
    assert compile_rc(lib, "/" + "k" * n, ["/" + "e" * n]) == SJMI_OK
    assert compile_rc(lib, "/" + "k" * (n + 1), [""]) == SJMI_ERR_ARG
    assert compile_rc(lib, "", ["/" + "e" * (n + 1)]) == SJMI_ERR_ARG
    full = ["/" + "/".join("%07d%x" % (p, s) for s in range(16)) for p in range(32)]
    assert compile_rc(lib, "/base", full) == SJMI_OK
    assert compile_rc(lib, "/base", full + ["/x"]) == SJMI_ERR_ARG


def test_the_binding_plan(lib):
    """ExplodePlan(..., members=True) compiles and closes without a context; n_columns counts the key"""
    import simdjson_java_amd as S
    plan = S.ExplodePlan("/payload", ["", "/id"], members=True)
    assert plan.members and plan.n_paths == 2 and plan.n_columns == 3 and plan.base == b"/payload"
    plan.close()
    plain = S.ExplodePlan("/payload", ["", "/id"])
    assert not plain.members and plain.n_columns == plain.n_paths == 2
    plain.close()
    S.ExplodePlan("", ["/p%d" % i for i in range(MAX_PATHS + 1)]).close()  # (64 paths: an array plan still takes them)
    with pytest.raises(ValueError):
        S.ExplodePlan("", ["/p%d" % i for i in range(MAX_PATHS + 1)], members=True)
    with pytest.raises(ValueError):
        S.ExplodePlan("payload", [""], members=True)
    assert {"sjmi_explode_members_plan_compile", "sjmi_key_census_device"} <= set(S.binding.EXPORTS)
