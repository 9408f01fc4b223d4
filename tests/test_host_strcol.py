"""CPU check of the string-column gather's passes (simdjson-java_amd/csrc/sj_strcol.h, which csrc/strcol.hip compiles verbatim)
against the numpy reference of tests/strcol_common.py: tests/host_sim/strcol_sim.cpp runs the chunk sums, their scan, the
offsets and the copy sequentially, at chunks of 64 and 128 rows and at the kernels' own.  The string buffer ends at a page that
cannot be read and NULL rows carry wild value words, so one dereference of such a word ends the test process."""
import ctypes as C

import numpy as np
import pytest

from tests import host_sim_lib
from tests import strcol_common as SC

SB_SIZE = 5000
CHUNKS = pytest.mark.parametrize("chunk", (64, 128, 0), ids=("chunk64", "chunk128", "chunk_of_the_kernels"))


def load_sim():
    """tests/host_sim/strcol_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("strcol", ("sj_strcol.h",))
    lib.sim_strcol.restype = C.c_int
    lib.sim_strcol.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p]
    lib.sim_strcol_chunk_rows.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


@pytest.fixture(scope="module")
def sb():
    return SC.string_buffer(np.random.default_rng(11), SB_SIZE)


def run_sim(lib, types, values, sb, chunk, capacity, validity=True, type_shift=0):
    n = len(types)
    # the type column at an odd address: a slice of a larger array
    store = np.zeros(n + 16, dtype=np.uint8)
    t = store[type_shift:type_shift + n]
    t[:] = types
    values = np.ascontiguousarray(values, dtype=np.uint64)
    offsets, words, data, res = SC.out_buffers(n, capacity, validity)
    rc = lib.sim_strcol(t.ctypes.data, values.ctypes.data, n, sb.ctypes.data, sb.size, chunk, offsets.ctypes.data,
                        words.ctypes.data if validity else None, data.ctypes.data if capacity else None, capacity, res.ctypes.data)
    assert rc == 0, rc
    return offsets, words, data, res


def check_all(lib, what, types, values, sb, chunk, caps=None):
    ref = SC.reference(types, values, sb)
    total = len(ref[2])
    for k, capacity in enumerate(SC.capacities(total) if caps is None else caps):
        got = run_sim(lib, types, values, sb, chunk, capacity, validity=k != 1, type_shift=(3 * k + 1) % 16)
        SC.check("%s, chunk %d, capacity %d of %d" % (what, chunk, capacity, total), *got, ref, capacity)
    return total


def test_the_reference_on_an_example_read_by_hand():
    sb = np.frombuffer(b"....abc.....de", dtype=np.uint8)
    types = [ord('"'), 0, ord('"'), ord("n"), ord("l"), ord('"')]
    values = [(3 << 32) | 4, SC.WILD[0], 0 << 32 | 9, SC.WILD[2], 7, (2 << 32) | 12]
    offsets, words, data, n_valid, n_other = SC.reference(types, values, sb)
    assert offsets.tolist() == [0, 3, 3, 3, 3, 3, 5] and words.tolist() == [0b100101] and data == b"abcde" and (n_valid, n_other) == (3, 1)
    assert SC.reference([], [], sb)[0].tolist() == [0] and SC.reference([], [], sb)[1].size == 0


@CHUNKS
def test_row_counts(lib, sb, chunk):
    R = chunk or lib.sim_strcol_chunk_rows()
    rng = np.random.default_rng(100 + R)
    for n in sorted({0, 1, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1, 5 * R + 63}):
        t, v = SC.random_column(rng, n, 9, SB_SIZE)
        check_all(lib, "%d rows" % n, t, v, sb, R)


@CHUNKS
def test_lengths_in_every_position(lib, chunk):
    R = chunk or lib.sim_strcol_chunk_rows()
    rng = np.random.default_rng(200 + R)
    big = SC.string_buffer(rng, SC.LONG + 100)
    total = 0
    for name, t, v in SC.length_cases(rng, big.size):
        long_one = int(v[t == SC.STRING].max() >> 32) == SC.LONG
        total += check_all(lib, name, t, v, big, R, caps=None if not long_one or "300" in name else (SC.LONG + 5, SC.LONG // 2, 0))
    assert total > 5 * SC.LONG


@CHUNKS
def test_column_shapes(lib, sb, chunk):
    R = chunk or lib.sim_strcol_chunk_rows()
    rng = np.random.default_rng(300 + R)
    for name, t, v in SC.shape_cases(rng, SB_SIZE):
        check_all(lib, name, t, v, sb, R)


@CHUNKS
def test_fuzz(lib, sb, chunk):
    R = chunk or lib.sim_strcol_chunk_rows()
    rng = np.random.default_rng(400 + R)
    valid = other = 0
    for k in range(60 if chunk else 12):
        n = int(rng.integers(1, 4 * R))
        t, v = SC.random_column(rng, n, int(rng.choice([0, 3, 20, 200])), SB_SIZE, p_string=float(rng.choice([0.05, 0.5, 0.95])),
                                src_align=int(rng.integers(0, 16)))
        ref = SC.reference(t, v, sb)
        total = len(ref[2])
        # every capacity for one column in four, for the others the exact one and one inside the column
        check_all(lib, "fuzz column %d (%d rows)" % (k, n), t, v, sb, R, caps=None if k % 4 == 0 else (total, int(rng.integers(0, total + 1))))
        valid += ref[3]
        other += ref[4]
    assert valid > 1000 and other > 100


def test_a_string_that_ends_the_buffer_and_a_wild_word_beside_it(lib):
    """the guard page is live: the last byte in front of it is read, and the wild words next to it are not"""
    sb = SC.string_buffer(np.random.default_rng(5), 256)
    types = np.array([0, SC.STRING, ord("n"), ord("{")] * 40, dtype=np.uint8)
    values = np.array([SC.WILD[0], (200 << 32) | 56, SC.WILD[3], SC.WILD[5]] * 40, dtype=np.uint64)
    assert check_all(lib, "at the guard page", types, values, sb, 64) == 40 * 200


def test_argument_errors(lib, sb):
    res = np.zeros(4, dtype=np.uint64)
    offs = np.zeros(4, dtype=np.uint64)
    assert lib.sim_strcol(None, None, 0, sb.ctypes.data, sb.size, 100, offs.ctypes.data, None, None, 0, res.ctypes.data) == -2
    assert lib.sim_strcol(None, None, 0, sb.ctypes.data, sb.size, 64, offs.ctypes.data, None, None, 5, res.ctypes.data) == -2
