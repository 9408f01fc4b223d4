"""CPU check of the group statistics' passes (simdjson-java_amd/csrc/sj_groupstats.h, which csrc/groupstats.hip compiles verbatim)
against the reference of tests/groupstats_common.py: tests/host_sim/groupstats_sim.cpp runs the clear, the LDS path, the global
path and the finish with a sequential workgroup, the groups / chunks in three orders; a stand-alone program runs them under ASan
and UBSan."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import groupstats_common as GC
from tests import host_sim_lib
from tests.members_common import header_constant

CANARY = 0xC0FFEE0DDF00D5
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 64 * 1024 + 1]
W = GC.WORDS


def load_sim():
    """tests/host_sim/groupstats_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("groupstats", ("sj_groupstats.h", "sj_fieldcol.h"))
    lib.sim_group_stats.restype = C.c_int
    lib.sim_group_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_void_p]
    for name in ("sim_group_lds_keys", "sim_group_chunk_rows", "sim_group_grid"):
        getattr(lib, name).restype = C.c_uint32
    lib.sim_group_grid.argtypes = [C.c_uint64, C.c_uint64]
    for name in ("sim_group_okey", "sim_group_okey_bits"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_uint64, [C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


@pytest.fixture(scope="module")
def lds_keys(lib):
    n = lib.sim_group_lds_keys()
    assert n == header_constant("SJMI_GROUP_LDS_KEYS") and header_constant("SJMI_GROUP_STATS_WORDS") == W
    return n


def run(lib, indices, words, types, values, n_keys, row_count=None, chunk=0, order=0, cap=0, n_rows=None):
    """-> (stats uint64 [n_keys, 10], result [5]); canaries in front of and behind the stats are checked here"""
    n_rows = indices.size if n_rows is None else n_rows
    block = np.full(n_keys * W + 16, CANARY, dtype=np.uint64)
    result = np.full(5, CANARY, dtype=np.uint64)
    rc = None if row_count is None else np.array([row_count], dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    got = lib.sim_group_stats(ptr(indices), ptr(words), ptr(types), ptr(values), n_rows, None if rc is None else rc.ctypes.data, n_keys, chunk, order,
                              cap, block[8:].ctypes.data if n_keys else None, result.ctypes.data)
    assert got == 0
    assert (block[:8] == CANARY).all() and (block[8 + n_keys * W:] == CANARY).all(), "a word outside the stats was written"
    return block[8:8 + n_keys * W].reshape(n_keys, W).copy(), result


def check(lib, indices, words, bits, types, values, n_keys, row_count=None, what="", exact_sum=False, **kw):
    live = indices.size if row_count is None else min(indices.size, row_count)
    want, (grouped, outside, nan) = GC.expected(indices, bits, types, values, n_keys, live)
    stats, result = run(lib, indices, words, types, values, n_keys, row_count, **kw)
    assert [int(x) for x in result] == [live, grouped, outside, nan, 0], what
    GC.check_stats(stats, want, exact_sum=exact_sum, what=str(what))
    return stats, (grouped, outside, nan)


def test_the_ordered_key_is_total_order_on_the_non_nan_doubles(lib):
    xs = [-math.inf, -1e300, -2.5, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.5, 1e300, math.inf]
    keys = [lib.sim_group_okey(GC.bits_of(x)) for x in xs]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and 0 < keys[0] and keys[-1] < (1 << 64) - 1
    assert [lib.sim_group_okey_bits(k) for k in keys] == [GC.bits_of(x) for x in xs]


def test_the_two_forms_of_the_reference_agree():
    for n_keys in (0, 1, 9):
        indices, words, bits = GC.keys_column(777, n_keys, 3, "wild")
        types, values = GC.value_column(777, 3, "mixed")
        for b in (None, bits):
            for live in (0, 500, 777):
                assert GC.expected(indices, b, types, values, n_keys, live) == GC.expected_large(indices, b, types, values, n_keys, live)
    indices, words, bits, types, values = GC.nan_case(500, 4, 8)
    assert GC.expected(indices, bits, types, values, 4, 500) == GC.expected_large(indices, bits, types, values, 4, 500)


def test_the_grid_is_capped_and_no_larger_than_the_flush_allows(lib, lds_keys):
    """gs_lds_grid: at most 512 groups, and no more than one per (n_keys * 10 / 256) chunks: on average a group has at least four
    rows per word of the stats it may have to flush; a 32-bit count of a group cannot overflow below 2^32 rows"""
    R = lib.sim_group_chunk_rows()
    for n_rows in (1, R, 8 << 20, (1 << 32) - 1):
        for n_keys in (0, 1, 8, lds_keys):
            grid = lib.sim_group_grid(n_rows, n_keys)
            chunks = (n_rows + R - 1) // R
            per = max(1, n_keys * W // 256)
            assert 1 <= grid <= 512 and grid == min(512, (chunks + per - 1) // per) and ((chunks + grid - 1) // grid) * R < 1 << 32


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_key_counts_on_both_paths(lib, lds_keys, n_rows):
    for n_keys in (0, 1, lds_keys, lds_keys + 1):
        for kind, vkind in (("uniform", "mixed"), ("wild", "mixed"), ("wild", "exact")):
            indices, words, bits = GC.keys_column(n_rows, n_keys, 1000 * n_rows + n_keys, kind)
            types, values = GC.value_column(n_rows, n_rows + n_keys, vkind)
            _, (grouped, outside, nan) = check(lib, indices, words, bits, types, values, n_keys, what=(n_rows, n_keys, kind, vkind),
                                               exact_sum=vkind == "exact")
            if n_keys == 0:
                assert grouped == 0 and outside == int(bits.sum())
            if kind == "wild" and n_rows >= 63 and n_keys:
                assert outside > 0 and grouped > 0


@pytest.mark.parametrize("n_keys_of", [lambda L: 8, lambda L: L, lambda L: L + 1], ids=["8", "lds", "lds_plus_1"])
def test_all_rows_in_one_key_and_a_null_validity(lib, lds_keys, n_keys_of):
    n_keys = n_keys_of(lds_keys)
    indices, words, bits = GC.keys_column(64 * 1024 + 1, n_keys, 7, "one_bin")
    types, values = GC.value_column(indices.size, 7, "mixed")
    stats, (grouped, _, _) = check(lib, indices, None, None, types, values, n_keys, what="one key, no validity")
    assert grouped == indices.size and int(stats[:, :3].sum()) == indices.size == int(stats[n_keys // 2, :3].sum())
    check(lib, indices, words, bits, types, values, n_keys, what="one key, with validity")


@pytest.mark.parametrize("scale", GC.SCALES, ids=GC.SCALE_IDS)
def test_scaled_columns_are_summed_exactly(lib, lds_keys, scale):
    """doubles m * scale, |m| < 2^20: subnormal cells and sums at 2^-1074, sums that cross into the normal range at 2^-1040, sums
    next to the overflow at 2^970 -- every partial sum is exact, so sum_double EQUALS math.fsum.  The sequential form of what
    tests/test_gpu_groupstats.py runs through the device's f64 atomics: a failure there and not here is the device's"""
    for n_rows, kind in ((64 * 1024 + 1, "one_bin"), (5 * 1024, "uniform")):
        types, values = GC.value_column(n_rows, 3, "scaled", scale=scale)
        for n_keys in (1, lds_keys, lds_keys + 1):
            indices, words, bits = GC.keys_column(n_rows, n_keys, 3, kind)
            stats, _ = check(lib, indices, words, bits, types, values, n_keys, what=(scale, n_rows, kind, n_keys), exact_sum=True)
            sums = stats[:, 5].view(np.float64)
            assert scale != GC.SCALES[0] or ((np.abs(sums) < 2.0 ** -1022).all() and (sums != 0).any())  # (subnormal sums, and kept)


def test_the_128_bit_sum(lib, lds_keys):
    """1025 x INT64_MAX, 1025 x INT64_MIN and a mix that cancels, on both paths"""
    n = 1025
    big, small = np.full(n, GC.INT64_MAX, dtype=np.int64), np.full(n, GC.INT64_MIN, dtype=np.int64)
    mix = np.where(np.arange(n) % 2 == 1, GC.INT64_MAX, -GC.INT64_MAX).astype(np.int64)
    mix[0] = 0
    types = np.full(n, ord("l"), dtype=np.uint8)
    for n_keys in (2, lds_keys + 1):
        indices = np.full(n, n_keys - 1, dtype=np.int32)
        for column, total in ((big, n * GC.INT64_MAX), (small, n * GC.INT64_MIN), (mix, 0)):
            stats, _ = check(lib, indices, None, None, types, column.view(np.uint64), n_keys, what=(n_keys, total))
            hi, lo = int(stats[n_keys - 1, 4]), int(stats[n_keys - 1, 3])
            assert ((hi - (1 << 64) if hi >> 63 else hi) << 64) + lo == total and int(stats[n_keys - 1, 0]) == n
            assert abs(total) > 1 << 64 or total == 0


def test_a_value_word_behind_a_type_that_is_no_number_is_not_read(lib, lds_keys):
    """two columns that differ in every value word behind a type byte other than 'l' / 'd' give the same words, bit for bit"""
    for n_keys in (5, lds_keys + 1):
        indices, words, bits = GC.keys_column(3000, n_keys, 21, "wild")
        types, values = GC.value_column(3000, 21, "exact")
        other = (types != ord("l")) & (types != ord("d"))
        assert other.sum() > 500
        a = run(lib, indices, words, types, values, n_keys)
        for poison in (0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 0x7FF0000000000000, 1):
            changed = values.copy()
            changed[other] = poison
            b = run(lib, indices, words, types, changed, n_keys)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_nan_cells_count_in_n_nan_only(lib, lds_keys):
    for n_keys in (4, lds_keys + 1):
        indices, words, bits, types, values = GC.nan_case(3000, n_keys, 31)
        stats, (grouped, outside, nan) = check(lib, indices, words, bits, types, values, n_keys, what=("nan", n_keys))
        assert nan > 100 and int(stats[:, :3].sum()) == grouped


def test_infinite_cells_follow_ieee_addition(lib, lds_keys):
    indices, types, values, n_keys = GC.infinity_case()
    for extra in (0, lds_keys + 1):
        stats, _ = check(lib, indices, None, None, types, values, n_keys + extra, what="infinities")
        f = stats.view(np.float64)
        assert f[0, 5] == math.inf and math.isnan(f[1, 5]) and f[2, 5] == -math.inf and math.isfinite(f[3, 5])
        assert (f[1, 8], f[1, 9]) == (-math.inf, math.inf) and (f[0, 8], f[0, 9]) == (-2.0, math.inf)
        assert int(stats[3, 8]) == GC.bits_of(-0.0) and (f[4, 8], f[4, 9]) == (math.inf, -math.inf)


def test_indices_outside_the_keys_touch_nothing(lib, lds_keys):
    for n_keys in (0, 1, 4, lds_keys, lds_keys + 1):
        indices = np.array([-1, n_keys, GC.INT32_MIN, GC.INT32_MAX, 0, n_keys - 1, -n_keys, n_keys + 1] * 33, dtype=np.int64).astype(np.int32)
        types, values = GC.value_column(indices.size, 5, "mixed")
        _, (grouped, outside, nan) = check(lib, indices, None, None, types, values, n_keys)
        assert outside >= 4 * 33


def test_live_rows(lib, lds_keys):
    """a device row count of 0, inside the rows, at them and above them: rows at or above it are not read"""
    for n_keys in (3, lds_keys + 1):
        indices, words, bits = GC.keys_column(1025, n_keys, 5, "wild")
        types, values = GC.value_column(1025, 5, "mixed")
        for row_count in (0, 1, 64, 1000, 1024, 1025, 5000, 1 << 50):
            live = min(1025, row_count)
            # (what lies at or above the live rows is poison: an index that would hit a key, a long that would move its words)
            ix, ty, va = indices.copy(), types.copy(), values.copy()
            ix[live:], ty[live:], va[live:] = 0, ord("l"), 1 << 62
            want, counts = GC.expected(indices, bits, types, values, n_keys, live)
            stats, result = run(lib, ix, words, ty, va, n_keys, row_count)
            assert [int(x) for x in result] == [live, *counts, 0], (n_keys, row_count)
            GC.check_stats(stats, want, what=str((n_keys, row_count)))


def test_schedules_do_not_matter(lib, lds_keys):
    """groups / chunks ascending, descending and odd-first, small chunks, a grid cap that gives a group many chunks: the same
    words, sum_double included on the exact column"""
    for n_keys in (2, lds_keys, lds_keys + 1):
        indices, words, bits = GC.keys_column(5 * 1024 + 77, n_keys, 11, "wild")
        for vkind in ("exact", "mixed"):
            types, values = GC.value_column(indices.size, 11, vkind)
            want, counts = GC.expected(indices, bits, types, values, n_keys, indices.size)
            first = None
            for chunk in (64, 256, 0):
                for order in (0, 1, 2):
                    for cap in (0, 1, 3):
                        stats, result = run(lib, indices, words, types, values, n_keys, chunk=chunk, order=order, cap=cap)
                        assert [int(x) for x in result] == [indices.size, *counts, 0], (n_keys, chunk, order, cap)
                        GC.check_stats(stats, want, exact_sum=vkind == "exact", what=str((n_keys, vkind, chunk, order, cap)))
                        first = stats if first is None else first
                        assert GC.same_but_sum_double(first, stats) and (vkind != "exact" or (first == stats).all())


def test_argument_errors(lib):
    ok = np.zeros(16, dtype=np.uint64)
    ix, ty, va = np.zeros(4, dtype=np.int32), np.zeros(8, dtype=np.uint8), np.zeros(5, dtype=np.uint64)
    p = lambda a, off=0: a.ctypes.data + off
    f = lib.sim_group_stats
    S, R = p(ok), p(ok, 88)
    assert f(p(ix), None, p(ty), p(va), 4, None, 1, 0, 0, 0, S, R) == 0
    assert f(p(ix), None, p(ty), p(va), 4, None, 1, 0, 0, 0, S, None) == -2
    assert f(None, None, p(ty), p(va), 4, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, None, p(va), 4, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), None, 4, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), p(va), 4, None, 1, 0, 0, 0, None, R) == -2
    assert f(None, None, None, None, 0, None, 0, 0, 0, 0, None, R) == 0  # (nothing at all: a zero record)
    assert f(p(ix), None, p(ty), p(va), 4, None, (1 << 20) + 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), p(va), 1 << 32, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix, 2), None, p(ty), p(va), 1, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), p(ok, 4), p(ty), p(va), 4, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), p(va, 4), 4, None, 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), p(va), 4, p(ok, 4), 1, 0, 0, 0, S, R) == -2
    assert f(p(ix), None, p(ty), p(va), 4, None, 1, 0, 0, 0, p(ok, 4), R) == -2
    assert f(p(ix), None, p(ty), p(va), 4, None, 1, 0, 0, 0, S, p(ok, 92)) == -2
    assert f(p(ix), None, p(ty, 3), p(va), 4, None, 1, 0, 0, 0, S, R) == 0  # (types: any alignment)


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/groupstats_asan_main.cpp: random adversarial columns in heap blocks of exactly their size, every schedule,
    all runs compared with a plain loop that sums in 128 bits.  Run as a child process."""
    exe = str(tmp_path / "groupstats_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "groupstats_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "120"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
