"""CPU check of the sort's passes (simdjson-java_amd/csrc/sj_sortrows.h, which csrc/sortrows.hip compiles verbatim) against the
reference of tests/sortrows_common.py: tests/host_sim/sortrows_sim.cpp runs the clear, the range pass, the plan, the count / scan /
emit, the eight digit passes and the gather with a sequential workgroup, the groups, chunks and tiles in three orders; a
stand-alone program runs them under ASan and UBSan.  All results are integers: every comparison is an equality."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import host_sim_lib
from tests import sortrows_common as SO
from tests import toprows_common as TC
from tests.members_common import header_constant

CANARY = 0xC0FFEE0DDF00D5
TILE = 4096
POSITIONS = [0, 1, 63, 64, 65, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 64 * 1024 + 1]
SPREAD_BITS = [0, 7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 55, 56, 63]  # msb(min ^ max): every n_digits, both parities
L, D = TC.LONG, TC.DOUBLE


def load_sim():
    """tests/host_sim/sortrows_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("sortrows", ("sj_sortrows.h", "sj_toprows.h", "sj_filter.h", "sj_okey.h", "sj_arrowcol.h", "sj_fieldcol.h"))
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.sim_sort_rows.restype = C.c_int
    lib.sim_sort_rows.argtypes = [P, P, P, U64, P, U64, P, U32, U32, P, P, U64, U64, P, P, P, U64, P, U32, U32, U32, U32]
    lib.sim_sort_chunk_rows.restype = lib.sim_sort_tile_rows.restype = U32
    lib.sim_sort_workspace_words.restype, lib.sim_sort_workspace_words.argtypes = U64, [U64]
    return lib


@pytest.fixture(scope="module")
def lib():
    lib = load_sim()
    assert lib.sim_sort_tile_rows() == TILE and lib.sim_sort_chunk_rows() == 1024
    assert (header_constant("SJMI_SORT_LONG"), header_constant("SJMI_SORT_DOUBLE"), header_constant("SJMI_SORT_DESCENDING")) == (L, D, SO.DESCENDING)
    assert header_constant("SJMI_SORT_BAD_ROW") == SO.BAD_ROW and header_constant("SJMI_SORT_RESULT_WORDS") == SO.RESULT_WORDS
    return lib


def run(lib, types, words, values, kind, descending, rows_in=None, n_rows=None, carry=None, row_count=None, chunk=0, tile=0, order=0, cap=0,
        shift=0, pad=3):
    """-> (rows uint64 [n_rows], out_types [n_cols, stride], out_values [n_cols, stride], result [9]); the output stride is n_rows +
    pad.  Canaries in front of and behind every output are checked here, and the entries at or behind `live` must still hold
    them.  shift: the types columns (the key's and the carried ones) begin at this odd offset"""
    n_source = values.size
    n_rows = (n_source if rows_in is None else rows_in.size) if n_rows is None else n_rows
    n_cols = 0 if carry is None else carry[0].shape[0]
    col_stride = 0 if carry is None else carry[0].shape[1]
    stride = n_rows + pad if n_cols else 0
    rows = np.full(n_rows + 16, CANARY, dtype=np.uint64)
    out_values = np.full(n_cols * stride + 16, CANARY, dtype=np.uint64)
    out_types = np.full(n_cols * stride + 16 + shift, 0xC5, dtype=np.uint8)
    result = np.full(SO.RESULT_WORDS + 2, CANARY, dtype=np.uint64)
    rc = None if row_count is None else np.array([row_count], dtype=np.uint64)
    moved = lambda a: None if a is None else np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])
    kt, ct = moved(types), moved(None if carry is None else carry[0])
    ptr = lambda a, off=0: a.ctypes.data + off if a is not None and a.size > off else None
    got = lib.sim_sort_rows(ptr(kt, shift), ptr(words), ptr(values), n_source, ptr(rows_in), n_rows, ptr(rc), kind,
                            SO.DESCENDING if descending else 0, ptr(ct, shift), None if carry is None else ptr(carry[1]), n_cols, col_stride,
                            rows[8:].ctypes.data if n_rows else None, out_types[8 + shift:].ctypes.data if n_cols * stride else None,
                            out_values[8:].ctypes.data if n_cols * stride else None, stride, result[1:].ctypes.data, chunk, tile, order, cap)
    assert got == 0
    live = int(result[1])
    assert live <= n_rows and result[0] == CANARY and result[-1] == CANARY
    assert (rows[:8] == CANARY).all() and (rows[8 + live:] == CANARY).all(), "a word outside rows[0, live) was written"
    ov, ot = out_values[8:8 + n_cols * stride].reshape(n_cols, stride), out_types[8 + shift:8 + shift + n_cols * stride].reshape(n_cols, stride)
    assert (out_values[:8] == CANARY).all() and (out_values[8 + n_cols * stride:] == CANARY).all() and (ov[:, live:] == CANARY).all()
    assert (out_types[:8 + shift] == 0xC5).all() and (out_types[8 + shift + n_cols * stride:] == 0xC5).all() and (ot[:, live:] == 0xC5).all()
    return rows[8:8 + n_rows], ot, ov, result[1:-1]


def carried_cells(carry, want_rows):
    """the cells of the carried columns at the expected rows: type byte 0 and value 0 for a BAD entry"""
    good = want_rows < np.uint64(carry[0].shape[1])
    at = np.where(good, want_rows, 0).astype(np.int64)
    return np.where(good, carry[0][:, at], 0).astype(np.uint8), np.where(good, carry[1][:, at], 0).astype(np.uint64)


def check(sort, types, words, bits, values, kind, descending, rows_in=None, n_rows=None, carry=None, row_count=None, what="", want=None, **kw):
    """sort = a function with run()'s arguments behind the library: the host simulation here, the GPU in tests/test_gpu_sortrows.py"""
    n = (values.size if rows_in is None else rows_in.size) if n_rows is None else n_rows
    live = n if row_count is None else min(n, row_count)
    want_rows, want, _ = want or SO.expected(types, bits, values, rows_in, n, live, kind, descending)
    rows, ot, ov, result = sort(types, words, values, kind, descending, rows_in, n_rows, carry, row_count, **kw)
    assert [int(x) for x in result] == want, (what, [int(x) for x in result], want)
    assert want[1] + want[2] + want[3] + want[4] + want[6] == want[0] == live
    assert (rows[:live] == want_rows).all(), what
    if carry is not None:
        ct, cv = carried_cells(carry, want_rows)
        assert (ot[:, :live] == ct).all() and (ov[:, :live] == cv).all(), what
    return rows[:live], want


@pytest.fixture(scope="module")
def sim(lib):
    return lambda *a, **kw: run(lib, *a, **kw)


def longs_column(vals):
    v = np.array(vals, dtype=np.int64).view(np.uint64)
    return np.full(v.size, ord("l"), dtype=np.uint8), v


def spread_column(n, bit, seed):
    """longs whose keys differ at most in bits [0, bit], and in bit `bit` for sure: a base above, random bits below"""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, 1 << bit, n, dtype=np.uint64) if bit else np.zeros(n, dtype=np.uint64)
    top = (np.arange(n, dtype=np.uint64) % np.uint64(3) == 0).astype(np.uint64) << np.uint64(bit)
    base = np.uint64(0x2AAAAAAAAAAAAAAA) & ~np.uint64((1 << (bit + 1)) - 1)
    return np.full(n, ord("l"), dtype=np.uint8), base | top | low


def test_the_two_forms_of_the_reference_agree():
    rng = np.random.default_rng(3)
    for what, kind in (("longs", L), ("counters", L), ("equal", L), ("doubles", D), ("doubles", L), ("longs", D)):
        types, values = TC.typed_column(1500, 5, what)
        words, bits = TC.validity(1500, 5)
        perm = rng.permutation(1500).astype(np.uint64)
        perm[::40], perm[3], perm[9] = 1500, SO.BAD_ENTRIES[0], SO.BAD_ENTRIES[1]
        for rows_in, n_rows in ((None, 1500), (perm, 1500), (perm, 1100)):
            for t, b in ((types, bits), (types, None), (None, bits), (None, None)):
                if t is None and kind == D and what != "doubles":
                    continue
                for descending in (False, True):
                    for live in (1500, 700, 0):
                        a = SO.expected(t, b, values, rows_in, n_rows, live, kind, descending)
                        c = SO.expected_by_python_sort(t, b, values, rows_in, n_rows, live, kind, descending)
                        assert a[0].tolist() == c[0].tolist() and a[1] == c[1] and a[2].tolist() == c[2].tolist(), (what, kind, descending, live)
    types, values = TC.typed_column(4000, 9, "doubles")
    _, want, _ = SO.expected(types, None, values, None, 4000, 4000, D, False)
    assert want[4] > 50 and want[5] > 50 and want[2] > 100 and want[3] > 100  # (NaNs, inexact longs, nulls and others are all there)


def test_the_scratch(lib):
    for n in (0, 1, 1024, 1025, TILE, TILE + 1, 8 << 20, (1 << 32) - 1):
        chunks, tiles = (n + 1023) // 1024, (n + TILE - 1) // TILE
        # the state, two words per chunk, 256 words per tile, 256 totals, two buffers of n keys and n 32-bit positions
        assert lib.sim_sort_workspace_words(n) == 6 + 2 * chunks + 256 * tiles + 256 + 2 * (n + (n + 1) // 2)


@pytest.mark.parametrize("n_rows", POSITIONS)
def test_positions_in_both_kinds_and_directions(sim, n_rows):
    for what, kind in (("longs", L), ("counters", L), ("equal", L), ("doubles", D)):
        types, values = TC.typed_column(n_rows, 100 + n_rows, what)
        words, bits = TC.validity(n_rows, n_rows)
        carry = TC.carried(2, n_rows, n_rows + 5, n_rows)
        for descending in (False, True):
            check(sim, types, words, bits, values, kind, descending, carry=carry, what=(n_rows, what, descending), shift=1 + 2 * descending)


@pytest.mark.parametrize("bit", SPREAD_BITS)
def test_every_number_of_digit_passes(sim, bit):
    """msb(min ^ max) at both edges of every digit: n_passes, and the buffer the gather reads, follow"""
    for n in (TILE + 77, 300):
        types, values = spread_column(n, bit, bit)
        for descending in (False, True):
            _, want = check(sim, types, None, None, values, L, descending, what=(bit, n, descending))
            assert want[7] == bit // 8 + 1


def test_one_value_only_moves_nothing(sim):
    for n in (1, 64, 1025, 2 * TILE + 1):
        types, values = longs_column([42] * n)
        for descending in (False, True):
            rows, want = check(sim, types, None, None, values, L, descending)
            assert want[7] == 0 and rows.tolist() == list(range(n))
    # one candidate among nulls
    types, values = TC.typed_column(3000, 1, "longs")
    types[types == ord("l")] = ord("n")
    types[1234], values[1234] = ord("l"), 5
    rows, want = check(sim, types, None, None, values, L, False)
    assert want[1] == 1 and want[7] == 0 and rows[0] == 1234


def test_bins_of_a_tile(sim):
    """every pair of a tile in one bin; all 256 bins used in one tile; one bin straddling a tile edge"""
    n = 3 * TILE
    one = np.full(n, 7, dtype=np.int64)
    one[TILE:2 * TILE] = 9          # (a whole tile in one bin, another bin in front of and behind it)
    every = np.arange(n, dtype=np.int64) % 256
    straddle = np.repeat(np.arange(6, dtype=np.int64)[::-1], n // 6)  # (runs of n / 6 = 2048 + ...: the bins' edges move across the tiles)
    straddle[TILE - 3:TILE + 3] = 200
    for vals in (one, every, every[::-1].copy(), straddle, (every << 8) | 3):
        types, values = longs_column(vals)
        for descending in (False, True):
            for tile in (0, 64, 1024):
                check(sim, types, None, None, values, L, descending, tile=tile, what=(descending, tile))


def test_the_ends_of_the_range_and_the_doubles(sim):
    types, values = longs_column([TC.INT64_MAX, TC.INT64_MIN, 0, -1, TC.INT64_MIN, TC.INT64_MAX, 1] * 30)
    rows, want = check(sim, types, None, None, values, L, False)
    assert want[7] == 8 and rows[:60].tolist() == sorted(list(range(1, 210, 7)) + list(range(4, 210, 7)))
    check(sim, types, None, None, values, L, True)
    xs = [0.0, -0.0, math.inf, -math.inf, 1.5, -1.5, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4] * 40
    values = np.array(xs, dtype=np.float64).view(np.uint64).copy()
    for k, nan in enumerate(TC.NAN_BITS):
        values[7 + 13 * k] = nan
    types = np.full(values.size, ord("d"), dtype=np.uint8)
    for descending in (False, True):
        rows, want = check(sim, types, None, None, values, D, descending)
        assert want[4] == len(TC.NAN_BITS) and rows[want[1]:].tolist() == [7 + 13 * k for k in range(len(TC.NAN_BITS))]
    # -0.0 in front of +0.0, each run in position order
    types, values = np.full(200, ord("d"), dtype=np.uint8), np.array([0.0, -0.0] * 100).view(np.uint64)
    rows, _ = check(sim, types, None, None, values, D, False)
    assert rows.tolist() == list(range(1, 200, 2)) + list(range(0, 200, 2))
    rows, _ = check(sim, types, None, None, values, D, True)
    assert rows.tolist() == list(range(0, 200, 2)) + list(range(1, 200, 2))


def test_longs_that_round_are_counted_and_tie_as_doubles(sim):
    types, values = longs_column([(1 << 53) + 1, 1 << 53, (1 << 53) + 2, 5, (1 << 53) + 3, -(1 << 53) - 1])
    rows, want = check(sim, types, None, None, values, D, True)
    assert want[5] == 3 and rows.tolist() == [4, 2, 0, 1, 3, 5]
    rows, want = check(sim, types, None, None, values, D, False)
    assert rows.tolist() == [5, 3, 0, 1, 2, 4]  # (2^53 + 1 rounds to 2^53: a tie with row 1, by position)
    types, values = TC.typed_column(5000, 77, "doubles")
    _, want = check(sim, types, None, None, values, D, False)
    assert want[5] > 50


@pytest.mark.parametrize("what", ["counters", "equal"])
def test_equal_values_keep_their_positions(sim, what):
    """stability: heavy ties, both directions, the identity, a permutation and a filter-like ascending subset as rows_in"""
    n = 2 * TILE + 500
    types, values = TC.typed_column(n, 31, what)
    rng = np.random.default_rng(31)
    perm = rng.permutation(n).astype(np.uint64)
    subset = np.nonzero(rng.random(n) < 0.4)[0].astype(np.uint64)
    for rows_in in (None, perm, subset, np.concatenate([subset, subset])):  # (duplicates are legal)
        for descending in (False, True):
            for tile in (0, 256):
                rows, want = check(sim, types, None, None, values, L, descending, rows_in=rows_in, tile=tile, what=(what, descending, tile))
                if what == "equal":
                    src = np.arange(n, dtype=np.uint64) if rows_in is None else rows_in
                    assert rows[:want[1]].tolist() == src[types[src.astype(np.int64)] == ord("l")].tolist()


def test_bad_entries_are_counted_never_read_and_ordered_with_the_nulls(sim):
    n = 1500
    types, values = TC.typed_column(n, 8, "longs")
    words, bits = TC.validity(n, 8)
    rows_in = np.random.default_rng(8).permutation(n).astype(np.uint64)
    bad_at = [0, 63, 64, 700, 1024, 1499]
    for k, i in enumerate(bad_at):
        rows_in[i] = ((n,) + SO.BAD_ENTRIES)[k % 3]
    carry = TC.carried(2, n, n, 8)  # (the source columns end exactly at n_source_rows)
    for descending in (False, True):
        rows, want = check(sim, types, words, bits, values, L, descending, rows_in=rows_in, carry=carry, shift=1)
        assert want[6] == len(bad_at) and want[8] == SO.BAD_ROW
        tail = rows[want[1] + want[4] + want[3]:]
        assert sorted(int(x) for x in tail if x >= n) == sorted(int(rows_in[i]) for i in bad_at)
    # every position bad, and no source row at all
    all_bad = np.array([5, 6, SO.BAD_ENTRIES[1]], dtype=np.uint64)
    rows, want = check(sim, types[:5], None, None, values[:5], L, False, rows_in=all_bad, carry=TC.carried(1, 5, 5, 1))
    assert want == [3, 0, 0, 0, 0, 0, 3, 0, 1] and rows.tolist() == all_bad.tolist()
    rows, want = check(sim, types[:0], None, None, values[:0], L, False, rows_in=all_bad)
    assert want == [3, 0, 0, 0, 0, 0, 3, 0, 1]


@pytest.mark.parametrize("n_keys", [2, 3])
def test_chained_keys_against_lexsort(sim, n_keys):
    n = TILE + 333
    rng = np.random.default_rng(n_keys)
    cols = [rng.integers(0, m, n, dtype=np.int64) for m in (5, 7, 1000)][:n_keys]
    descending = [False, True, False][:n_keys]
    rows = None
    for vals, desc in list(zip(cols, descending))[::-1]:  # (last key first)
        types, values = longs_column(vals)
        rows, _ = check(sim, types, None, None, values, L, desc, rows_in=rows)
        rows = rows.copy()
    want = np.lexsort(tuple(-v if d else v for v, d in list(zip(cols, descending))[::-1]))
    assert rows.tolist() == want.tolist()
    keys = [(longs_column(v)[0], None, longs_column(v)[1], L, d) for v, d in zip(cols, descending)]
    assert SO.chain(keys, n)[0].tolist() == want.tolist()


def test_live_positions(sim):
    """a device row count of 0, inside the positions, at them and above them: positions at or above it are not read"""
    n = 1025
    types, values = TC.typed_column(n, 5, "longs")
    words, bits = TC.validity(n, 5)
    rows_in = np.random.default_rng(5).permutation(n).astype(np.uint64)
    for row_count in (0, 1, 64, 1000, 1024, 1025, 5000, 1 << 50):
        live = min(n, row_count)
        poisoned = rows_in.copy()
        poisoned[live:] = SO.BAD_ENTRIES[1]  # (would be counted if it were read)
        want = SO.expected(types, bits, values, rows_in, n, live, L, False)
        check(sim, types, words, bits, values, L, False, rows_in=poisoned, row_count=row_count, want=want, what=row_count)
        check(sim, types, words, bits, values, L, True, row_count=row_count, what=row_count)
    check(sim, types, words, bits, values, L, False, n_rows=700)
    check(sim, types, words, bits, values, L, False, rows_in=rows_in, n_rows=700)
    _, want = check(sim, types[:0], None, None, values[:0], L, False)
    assert want == [0] * 9


def test_the_empty_cases(sim):
    types, values = TC.typed_column(300, 2, "longs")
    types[:] = ord("t")
    _, want = check(sim, types, None, None, values, L, False, carry=TC.carried(1, 300, 300, 2))  # (no candidate)
    assert want[:4] == [300, 0, 0, 300]
    check(sim, types, None, None, values, L, False, row_count=0, carry=TC.carried(1, 300, 300, 2))
    check(sim, types, None, None, values, L, False, n_rows=0)
    check(sim, types, None, None, values, L, False, rows_in=np.zeros(0, dtype=np.uint64))


def test_a_value_word_behind_a_type_that_makes_no_candidate_is_not_read(sim):
    for kind, what in ((L, "longs"), (D, "doubles")):
        types, values = TC.typed_column(3000, 21, what)
        dead = (types != ord("l")) & ((types != ord("d")) | (kind == L))
        assert dead.sum() > 500
        a = sim(types, None, values, kind, False)
        for poison in (0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 1):
            changed = values.copy()
            changed[dead] = poison
            b = sim(types, None, changed, kind, False)
            assert all((x == y).all() for x, y in zip(a, b))


def test_schedules_do_not_matter(sim):
    """groups, chunks and tiles ascending, descending and odd-first, small chunks and tiles, a grid cap: the same outputs"""
    for what, kind in (("longs", L), ("counters", L), ("doubles", D)):
        types, values = TC.typed_column(2 * 1024 + 77, 11, what)
        words, bits = TC.validity(values.size, 11)
        carry = TC.carried(1, values.size, values.size, 11)
        first = None
        for chunk, tile in ((64, 64), (256, 1024), (0, 0)):
            for order in (0, 1, 2):
                for cap in (0, 1, 3):
                    check(sim, types, words, bits, values, kind, True, carry=carry, chunk=chunk, tile=tile, order=order, cap=cap,
                          what=(what, chunk, tile, order, cap))
                    got = sim(types, words, values, kind, True, None, None, carry, chunk=chunk, tile=tile, order=order, cap=cap)
                    first = got if first is None else first
                    assert all((x == y).all() for x, y in zip(first, got))


def test_argument_errors(lib):
    ok = np.zeros(64, dtype=np.uint64)
    ty, va = np.zeros(16, dtype=np.uint8), np.zeros(9, dtype=np.uint64)
    p = lambda a, off=0: a.ctypes.data + off
    R, O, V, S, RI = p(ok), p(ok, 64), p(ok, 128), p(ok, 256), p(ok, 384)  # rows, out_types, out_values, result, rows_in

    def f(kt=p(ty), kv=None, kval=p(va), ns=4, ri=None, n=4, rc=None, kind=L, flags=0, t=p(ty), v=p(va), n_cols=1, stride=4, rows=R, ot=O, ov=V,
          ostride=4, res=S):
        return lib.sim_sort_rows(kt, kv, kval, ns, ri, n, rc, kind, flags, t, v, n_cols, stride, rows, ot, ov, ostride, res, 0, 0, 0, 0)

    assert f() == 0
    assert f(kt=None) == 0 and f(kt=None, kv=p(ok, 8)) == 0  # (both NULL is legal: every live row is a candidate)
    assert f(kt=p(ty, 3), t=p(ty, 5), ot=O + 1) == 0  # (types: any alignment)
    assert f(kind=0) == -2 and f(kind=3) == -2 and f(flags=2) == -2 and f(flags=3) == -2 and f(flags=1) == 0
    assert f(n=1 << 32, ri=RI, ostride=1 << 32) == -2 and f(ns=1 << 32, stride=1 << 32) == -2
    assert f(n=5, ostride=5) == -2 and f(n=5, ostride=5, ri=RI) == 0  # (without rows_in the positions are rows)
    assert f(kval=None) == -2 and f(kval=None, n=0) == 0 and f(kval=None, ns=0, n=2, ri=RI, stride=0) == 0
    assert f(rows=None) == -2 and f(rows=None, n=0, t=None, v=None, ot=None, ov=None) == 0
    assert f(t=None) == -2 and f(v=None) == -2 and f(ot=None) == -2 and f(ov=None) == -2
    assert f(t=None, v=None, ot=None, ov=None, n_cols=0, stride=0, ostride=0) == 0
    assert f(stride=3) == -2 and f(ostride=3) == -2 and f(stride=3, ostride=3, n_cols=0) == 0
    assert f(kv=p(ok, 4)) == -2 and f(kval=p(va, 4)) == -2 and f(rc=p(ok, 4)) == -2 and f(v=p(va, 4)) == -2 and f(ri=RI + 4) == -2
    assert f(rows=R + 4) == -2 and f(ov=V + 4) == -2 and f(res=S + 4) == -2 and f(res=None) == -2


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/sortrows_asan_main.cpp: random adversarial columns in heap blocks of exactly their size, every schedule, all
    runs compared with std::stable_sort.  Run as a child process."""
    exe = str(tmp_path / "sortrows_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "sortrows_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "60"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
