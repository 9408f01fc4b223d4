"""CPU check of the NDJSON splitter's passes (simdjson-java_amd/csrc/sj_ndjson.h, which csrc/ndjson.hip compiles verbatim)
against the reference of tests/ndjson_common.py: tests/host_sim/ndjson_sim.cpp runs the tile summaries, their scan and the emit
sequentially, at tiles of 64 and 128 bytes and at the kernels' own, with the buffer at every alignment and '\\n' / 'a' bytes
around it."""
import ctypes as C

import numpy as np
import pytest

from tests import host_sim_lib
from tests import ndjson_common as NC

SHIFTS = (0, 1, 7, 15)


def load_sim():
    """tests/host_sim/ndjson_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("ndjson", ("sj_block32.h", "sj_ndjson.h"))
    lib.sim_ndjson.restype = C.c_int
    lib.sim_ndjson.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.sim_ndjson_tile_blocks.restype = C.c_uint32
    lib.sim_nd_combine.restype = C.c_uint64
    lib.sim_nd_combine.argtypes = [C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


def run_sim(lib, buf, shift, tile, capacity):
    offs = np.full(capacity + 4, NC.CANARY, dtype=np.uint64)
    res = np.zeros(3, dtype=np.uint64)
    rc = lib.sim_ndjson(buf, len(buf), shift, tile, NC.PAD_FILL, len(NC.PAD_FILL), offs.ctypes.data, capacity, res.ctypes.data)
    assert rc == 0, rc
    return offs, res


def check_all(lib, what, buf, tile, shifts=SHIFTS):
    ref = NC.ndjson_reference(buf)
    n_docs = len(ref[0]) - 1
    for shift in shifts:
        for capacity in sorted({n_docs + 3, n_docs + 1, n_docs, 1, 0}):
            offs, res = run_sim(lib, buf, shift, tile, capacity)
            NC.check("%s, tile %d, shift %d, capacity %d" % (what, tile, shift, capacity), buf, capacity, offs, res, ref=ref)
    return n_docs


def real_tile(lib):
    return 64 * lib.sim_ndjson_tile_blocks()


def test_the_reference_on_examples_read_by_hand():
    R = NC.ndjson_reference
    assert R(b"") == ([0], 0, True)
    assert R(b"a") == ([0], 0, False)
    assert R(b"\n") == ([0], 1, True)
    assert R(b"a\n") == ([0, 2], 2, True)
    assert R(b"\n\na\n\r\n \nb\n\n c") == ([0, 8, 11], 11, False)
    assert R(b" \r\n\t\n") == ([0], 5, True)
    assert R(b"\f\n") == ([0, 2], 2, True)


def test_the_state_operator_is_associative_with_identity_zero(lib):
    HAS, SEEN = 1 << 63, 1 << 62
    states = [0, SEEN] + [HAS | s | p for s in (0, SEEN) for p in (0, 5, 77)]
    op = lib.sim_nd_combine
    for a in states:
        assert op(a, 0) == a and op(0, a) == a
        for b in states:
            for c in states:
                assert op(op(a, b), c) == op(a, op(b, c)), (a, b, c)


@pytest.mark.parametrize("tile", (64, 128, 0), ids=("tile64", "tile128", "tile_of_the_kernels"))
def test_edge_cases(lib, tile):
    T = tile or real_tile(lib)
    docs = 0
    for name, buf in NC.edge_cases(T):
        docs += check_all(lib, name, buf, T)
    assert docs > 2 * T  # (the densest case alone has T + 1 documents)


@pytest.mark.parametrize("tile", (64, 128, 0), ids=("tile64", "tile128", "tile_of_the_kernels"))
def test_fuzz(lib, tile):
    T = tile or real_tile(lib)
    docs = blank_tails = 0
    for k, buf in enumerate(NC.fuzz_inputs(200 if tile else 60, T, seed=20260 + T)):
        docs += check_all(lib, "fuzz input %d (%d bytes)" % (k, len(buf)), buf, T, shifts=(SHIFTS[k % 4],) if tile else (0, 7))
        blank_tails += NC.ndjson_reference(buf)[2]
    assert docs > 100 and 0 < blank_tails < 200


def test_many_tiles(lib):
    T = 64
    for n_tiles in (1023, 1024, 1025):
        buf = NC.sparse_input(n_tiles, T)
        assert check_all(lib, "%d tiles" % n_tiles, buf, T, shifts=(0, 15)) > n_tiles // 4
