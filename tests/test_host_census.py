"""CPU check of the key census's passes (simdjson-java_amd/csrc/sj_census.h, which csrc/census.hip compiles verbatim) against the
Counter reference of tests/members_common.py: tests/host_sim/census_sim.cpp runs the clear, the LDS path and the global path
with a sequential workgroup, the groups / chunks in three orders; a stand-alone program runs them under ASan and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import host_sim_lib
from tests import members_common as MC

CANARY = 0xC0FFEE0DDF00D5
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 64 * 1024 + 1]


def load_sim():
    """tests/host_sim/census_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("census", ("sj_census.h", "sj_fieldcol.h"))
    lib.sim_census.restype = C.c_int
    lib.sim_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                               C.c_void_p]
    for name in ("sim_census_lds_keys", "sim_census_chunk_rows", "sim_census_class", "sim_census_grid"):
        getattr(lib, name).restype = C.c_uint32
    lib.sim_census_class.argtypes = [C.c_uint32]
    lib.sim_census_grid.argtypes = [C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


@pytest.fixture(scope="module")
def lds_keys(lib):
    n = lib.sim_census_lds_keys()
    assert n == MC.header_constant("SJMI_CENSUS_LDS_KEYS") and MC.header_constant("SJMI_CENSUS_CLASSES") == MC.CLASSES == 8
    return n


def column(n_rows, n_keys, seed, kind="uniform"):
    """-> (indices int32, validity words uint64, types uint8): uniform = every index in range, all type bytes; wild = indices out
    of range among them; skewed = wild, with half the rows in three bins; one_bin = every row (n_keys // 2, 'l')"""
    rng = np.random.default_rng(seed)
    if kind == "one_bin":
        indices = np.full(n_rows, n_keys // 2, dtype=np.int32)
        types = np.full(n_rows, ord("l"), dtype=np.uint8)
    else:
        indices = rng.integers(0, max(n_keys, 1), n_rows).astype(np.int32)
        types = rng.choice(np.frombuffer(b'ld"tfn[{\0x', dtype=np.uint8), n_rows)
        if kind == "skewed":
            hot = rng.random(n_rows) < 0.5
            indices[hot] = rng.choice(np.array([0, n_keys // 3, n_keys - 1], dtype=np.int32), int(hot.sum()))
            types[hot] = ord("l")
        if kind in ("wild", "skewed"):
            wild = np.array([-1, n_keys, INT32_MIN, INT32_MAX, n_keys + 7, -n_keys - 1], dtype=np.int64).astype(np.int32)
            hit = rng.random(n_rows) < 0.25
            indices[hit] = rng.choice(wild, int(hit.sum()))
    bits = rng.random(n_rows) < 0.8
    return indices, MC.pack_bits(bits), types, bits


def run(lib, indices, words, types, n_keys, row_count=None, chunk=0, order=0, cap=0, n_rows=None):
    """-> (counts [n_keys, 8], result [4]); canaries in front of and behind the counts are checked here"""
    n_rows = indices.size if n_rows is None else n_rows
    block = np.full(n_keys * 8 + 16, CANARY, dtype=np.uint64)
    result = np.full(4, CANARY, dtype=np.uint64)
    rc = None if row_count is None else np.array([row_count], dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    got = lib.sim_census(ptr(indices), ptr(words), ptr(types), n_rows, None if rc is None else rc.ctypes.data, n_keys, chunk, order, cap,
                         block[8:].ctypes.data if n_keys else None, result.ctypes.data)
    assert got == 0
    assert (block[:8] == CANARY).all() and (block[8 + n_keys * 8:] == CANARY).all(), "a word outside the counts was written"
    return block[8:8 + n_keys * 8].reshape(n_keys, 8), result


def check(lib, indices, words, bits, types, n_keys, row_count=None, what="", **kw):
    live = indices.size if row_count is None else min(indices.size, row_count)
    want, counted, outside = MC.expected_census(indices, bits, types, n_keys, live)
    counts, result = run(lib, indices, words, types, n_keys, row_count, **kw)
    assert [int(x) for x in result] == [live, counted, outside, 0], what
    assert counts.tolist() == want, what
    return counted, outside


def test_classes_of_every_type_byte(lib):
    got = [lib.sim_census_class(t) for t in range(256)]
    assert got == [MC.census_class(t) for t in range(256)]
    assert [got[c] for c in b'ld"tfn[{'] == [0, 1, 2, 3, 3, 4, 5, 6] and got[0] == 7 and got.count(7) == 256 - 8


def test_the_two_forms_of_the_reference_agree():
    for n_keys in (0, 1, 9):
        indices, words, types, bits = column(777, n_keys, 3, "wild")
        for b in (None, bits):
            for live in (0, 500, 777):
                assert MC.expected_census(indices, b, types, n_keys, live) == MC.expected_census_large(indices, b, types, n_keys, live)


def test_the_grid_keeps_a_bin_below_2_to_the_32(lib, lds_keys):
    """the bound the header states: a workgroup of the LDS path takes fewer than 2^32 rows"""
    R = lib.sim_census_chunk_rows()
    for n_rows in (1, R, 8 << 20, (1 << 40) - 1):
        for n_keys in (0, 1, 8, lds_keys):
            grid = lib.sim_census_grid(n_rows, n_keys)
            chunks = (n_rows + R - 1) // R
            assert 1 <= grid <= 512 and ((chunks + grid - 1) // grid) * R < 1 << 32


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_key_counts_on_both_paths(lib, lds_keys, n_rows):
    for n_keys in (0, 1, lds_keys, lds_keys + 1):
        for kind in ("uniform", "wild"):
            indices, words, types, bits = column(n_rows, n_keys, 1000 * n_rows + n_keys, kind)
            counted, outside = check(lib, indices, words, bits, types, n_keys, what=(n_rows, n_keys, kind))
            if n_keys == 0:
                assert counted == 0 and outside == int(bits.sum())
            if kind == "wild" and n_rows >= 63 and n_keys:
                assert outside > 0 and counted > 0


@pytest.mark.parametrize("n_keys_of", [lambda L: 8, lambda L: L, lambda L: L + 1], ids=["8", "lds", "lds_plus_1"])
def test_all_rows_in_one_bin_and_a_null_validity(lib, lds_keys, n_keys_of):
    n_keys = n_keys_of(lds_keys)
    indices, words, types, bits = column(64 * 1024 + 1, n_keys, 7, "one_bin")
    counts, result = run(lib, indices, None, types, n_keys)
    assert [int(x) for x in result] == [indices.size, indices.size, 0, 0]
    assert int(counts[n_keys // 2][0]) == indices.size and int(counts.sum()) == indices.size
    check(lib, indices, words, bits, types, n_keys, what="one bin, with validity")


def test_every_class_byte(lib, lds_keys):
    types = np.arange(256, dtype=np.uint8).repeat(3)
    indices = (np.arange(types.size) % 5).astype(np.int32)
    for n_keys in (5, lds_keys + 1):
        counts, result = run(lib, indices, None, types, n_keys)
        want, counted, outside = MC.expected_census(indices, None, types, n_keys, types.size)
        assert counts.tolist() == want and [int(x) for x in result] == [types.size, counted, 0, 0]
        assert int(counts[:, 7].sum()) == 3 * (256 - 8)


def test_indices_outside_the_keys_touch_nothing(lib, lds_keys):
    for n_keys in (0, 1, 4, lds_keys, lds_keys + 1):
        indices = np.array([-1, n_keys, INT32_MIN, INT32_MAX, 0, n_keys - 1, -n_keys, n_keys + 1] * 33, dtype=np.int64).astype(np.int32)
        types = np.full(indices.size, ord("{"), dtype=np.uint8)
        counts, result = run(lib, indices, None, types, n_keys)
        want, counted, outside = MC.expected_census(indices, None, types, n_keys, indices.size)
        assert counts.tolist() == want and [int(x) for x in result] == [indices.size, counted, outside, 0]
        assert outside >= 4 * 33


def test_live_rows(lib, lds_keys):
    """a device row count of 0, inside the rows, at them and above them: rows at or above it are not read"""
    for n_keys in (3, lds_keys + 1):
        indices, words, types, bits = column(1025, n_keys, 5, "wild")
        for row_count in (0, 1, 64, 1000, 1024, 1025, 5000, 1 << 50):
            live = min(1025, row_count)
            # (what lies at or above the live rows is poison: an index that would hit a bin, a type of class 0)
            ix, ty = indices.copy(), types.copy()
            ix[live:], ty[live:] = 0, ord("l")
            want, counted, outside = MC.expected_census(indices, bits, types, n_keys, live)
            counts, result = run(lib, ix, words, ty, n_keys, row_count)
            assert counts.tolist() == want and [int(x) for x in result] == [live, counted, outside, 0], (n_keys, row_count)


def test_schedules_do_not_matter(lib, lds_keys):
    """groups / chunks ascending, descending and odd-first, small chunks, a grid cap that gives a group many chunks"""
    for n_keys in (2, lds_keys, lds_keys + 1):
        indices, words, types, bits = column(5 * 1024 + 77, n_keys, 11, "wild")
        want, counted, outside = MC.expected_census(indices, bits, types, n_keys, indices.size)
        for chunk in (64, 256, 0):
            for order in (0, 1, 2):
                for cap in (0, 1, 3):
                    counts, result = run(lib, indices, words, types, n_keys, chunk=chunk, order=order, cap=cap)
                    assert counts.tolist() == want and [int(x) for x in result] == [indices.size, counted, outside, 0], (n_keys, chunk, order, cap)


def test_argument_errors(lib):
    ok = np.zeros(8, dtype=np.uint64)
    ix, ty = np.zeros(4, dtype=np.int32), np.zeros(8, dtype=np.uint8)
    p = lambda a, off=0: a.ctypes.data + off
    f = lib.sim_census
    assert f(p(ix), None, p(ty), 4, None, 1, 0, 0, 0, p(ok), p(ok)) == 0
    assert f(p(ix), None, p(ty), 4, None, 1, 0, 0, 0, p(ok), None) == -2
    assert f(None, None, p(ty), 4, None, 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), None, None, 4, None, 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), None, p(ty), 4, None, 1, 0, 0, 0, None, p(ok)) == -2
    assert f(None, None, None, 0, None, 0, 0, 0, 0, None, p(ok)) == 0  # (nothing at all: a zero record)
    assert f(p(ix), None, p(ty), 4, None, (1 << 20) + 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), None, p(ty), 1 << 40, None, 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix, 2), None, p(ty), 1, None, 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), p(ok, 4), p(ty), 4, None, 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), None, p(ty), 4, p(ok, 4), 1, 0, 0, 0, p(ok), p(ok)) == -2
    assert f(p(ix), None, p(ty), 4, None, 1, 0, 0, 0, p(ok, 4), p(ok)) == -2
    assert f(p(ix), None, p(ty), 4, None, 1, 0, 0, 0, p(ok), p(ok, 4)) == -2
    assert f(p(ix), None, p(ty, 3), 4, None, 1, 0, 0, 0, p(ok), p(ok)) == 0  # (types: any alignment)


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/census_asan_main.cpp: random adversarial columns in heap blocks of exactly their size, every schedule, all
    runs compared with a plain loop.  Run as a child process."""
    exe = str(tmp_path / "census_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "census_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "120"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
