"""CPU check of the top rows' passes (simdjson-java_amd/csrc/sj_toprows.h, which csrc/toprows.hip compiles verbatim) against the
reference of tests/toprows_common.py: tests/host_sim/toprows_sim.cpp runs the clear, the range pass, the plan, the six digit
passes, the mark / scan / emit and the sort with a sequential workgroup, the groups and chunks in three orders; a stand-alone
program runs them under ASan and UBSan.  All results are integers: every comparison is an equality."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import host_sim_lib
from tests import toprows_common as TC
from tests.members_common import header_constant

CANARY = 0xC0FFEE0DDF00D5
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 64 * 1024 + 1]
KS = [0, 1, 2, 63, 64, 65, 2047, 2048]
L, D = TC.LONG, TC.DOUBLE


def load_sim():
    """tests/host_sim/toprows_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("toprows", ("sj_toprows.h", "sj_okey.h", "sj_arrowcol.h", "sj_fieldcol.h"))
    lib.sim_top_rows.restype = C.c_int
    lib.sim_top_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                 C.c_uint32, C.c_void_p]
    for name in ("sim_top_max_k", "sim_top_chunk_rows", "sim_top_grid"):
        getattr(lib, name).restype = C.c_uint32
    lib.sim_top_grid.argtypes = [C.c_uint64]
    lib.sim_top_workspace_words.restype, lib.sim_top_workspace_words.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    lib = load_sim()
    assert lib.sim_top_max_k() == header_constant("SJMI_TOP_MAX_K") == TC.MAX_K and header_constant("SJMI_TOP_RESULT_WORDS") == TC.RESULT_WORDS
    assert (header_constant("SJMI_TOP_LONG"), header_constant("SJMI_TOP_DOUBLE"), header_constant("SJMI_TOP_SMALLEST")) == (L, D, TC.SMALLEST)
    return lib


def run(lib, types, words, values, kind, largest, k, carry=None, row_count=None, n_rows=None, chunk=0, order=0, cap=0, shift=0):
    """-> (rows uint64 [k], out_types [n_cols, k], out_values [n_cols, k], result [9], the plan's digits); canaries in front of
    and behind every output are checked here, and entries that the call did not have to write must still hold them.  shift:
    the types columns (the key's and the carried ones) begin at this odd offset"""
    n_rows = values.size if n_rows is None else n_rows
    n_cols = 0 if carry is None else carry[0].shape[0]
    stride = 0 if carry is None else carry[0].shape[1]
    rows = np.full(k + 16, CANARY, dtype=np.uint64)
    out_values = np.full(n_cols * k + 16, CANARY, dtype=np.uint64)
    out_types = np.full(n_cols * k + 16 + shift, 0xC5, dtype=np.uint8)
    result = np.full(TC.RESULT_WORDS + 2, CANARY, dtype=np.uint64)
    rc = None if row_count is None else np.array([row_count], dtype=np.uint64)
    digits = C.c_uint32(99)
    moved = lambda a: None if a is None else np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])
    kt, ct = moved(types), moved(None if carry is None else carry[0])
    ptr = lambda a, off=0: a.ctypes.data + off if a is not None and a.size > off else None
    got = lib.sim_top_rows(ptr(kt, shift), ptr(words), ptr(values), n_rows, ptr(rc), kind, 0 if largest else TC.SMALLEST, k, ptr(ct, shift),
                           None if carry is None else ptr(carry[1]), n_cols, stride, rows[8:].ctypes.data if k else None,
                           out_types[8 + shift:].ctypes.data if n_cols * k else None, out_values[8:].ctypes.data if n_cols * k else None,
                           result[1:].ctypes.data, chunk, order, cap, C.addressof(digits))
    assert got == 0
    n_out = int(result[7])
    assert n_out <= k and result[0] == CANARY and result[-1] == CANARY
    assert (rows[:8] == CANARY).all() and (rows[8 + n_out:] == CANARY).all(), "a word outside rows[0, n_out) was written"
    ov, ot = out_values[8:8 + n_cols * k].reshape(n_cols, k), out_types[8 + shift:8 + shift + n_cols * k].reshape(n_cols, k)
    assert (out_values[:8] == CANARY).all() and (out_values[8 + n_cols * k:] == CANARY).all() and (ov[:, n_out:] == CANARY).all()
    assert (out_types[:8 + shift] == 0xC5).all() and (out_types[8 + shift + n_cols * k:] == 0xC5).all() and (ot[:, n_out:] == 0xC5).all()
    return rows[8:8 + k], ot, ov, result[1:-1], digits.value


def check(lib, types, words, bits, values, kind, largest, k, carry=None, row_count=None, what="", **kw):
    n_rows = kw.get("n_rows", values.size)
    live = n_rows if row_count is None else min(n_rows, row_count)
    want_rows, want = TC.expected(types, bits, values, live, kind, largest, k)
    rows, ot, ov, result, digits = run(lib, types, words, values, kind, largest, k, carry, row_count, **kw)
    assert [int(x) for x in result] == want, (what, [int(x) for x in result], want)
    n_out = want[6]
    assert rows[:n_out].astype(np.int64).tolist() == want_rows.tolist(), what
    assert want[1] + want[2] + want[3] + want[4] == want[0]
    if carry is not None:
        assert (ot[:, :n_out] == carry[0][:, want_rows]).all() and (ov[:, :n_out] == carry[1][:, want_rows]).all(), what
    return want_rows, want, digits


def test_the_two_forms_of_the_reference_agree():
    for what, kind in (("longs", L), ("counters", L), ("equal", L), ("doubles", D), ("doubles", L), ("longs", D)):
        types, values = TC.typed_column(1500, 5, what)
        words, bits = TC.validity(1500, 5)
        for t, b in ((types, bits), (types, None), (None, bits), (None, None)):
            if t is None and kind == D and what != "doubles":
                continue
            for largest in (True, False):
                for k, live in ((0, 1500), (1, 1500), (100, 1500), (2048, 1500), (100, 700), (5, 0)):
                    a = TC.expected(t, b, values, live, kind, largest, k)
                    c = TC.expected_by_python_sort(t, b, values, live, kind, largest, k)
                    assert a[0].tolist() == c[0].tolist() and a[1] == c[1], (what, kind, largest, k, live)
    types, values = TC.typed_column(4000, 9, "doubles")
    _, want = TC.expected(types, None, values, 4000, D, True, 10)
    assert want[4] > 50 and want[5] > 50 and want[2] > 100 and want[3] > 100  # (NaNs, inexact longs, nulls and others are all there)


def test_the_grid_and_the_scratch(lib):
    R = lib.sim_top_chunk_rows()
    for n_rows in (1, R, R + 1, 8 << 20, (1 << 32) - 1):
        chunks = (n_rows + R - 1) // R
        assert lib.sim_top_grid(n_rows) == min(512, chunks)
        for k in (0, 1, 2047, 2048):
            # the state, six histograms of 2048 32-bit bins, a word per chunk, k keys and k 32-bit rows
            assert lib.sim_top_workspace_words(n_rows, k) == 6 + 6 * 1024 + chunks + k + (k + 1) // 2
    assert lib.sim_top_workspace_words(0, 0) == 6 + 6 * 1024


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_k_in_both_kinds_and_directions(lib, n_rows):
    ks = KS if n_rows <= 1025 else [1, 65, 2048]
    for what, kind in (("longs", L), ("counters", L), ("doubles", D)):
        types, values = TC.typed_column(n_rows, 100 + n_rows, what)
        carry = TC.carried(2, n_rows, n_rows + 5, n_rows)
        for largest in (True, False):
            for k in ks:
                check(lib, types, None, None, values, kind, largest, k, carry, what=(n_rows, what, largest, k))
    # k above the candidates
    types, values = TC.typed_column(n_rows, 7, "longs")
    _, want, _ = check(lib, types, None, None, values, L, True, 2048)
    assert want[6] == min(2048, want[1])


@pytest.mark.parametrize("kind,what", [(L, "longs"), (L, "counters"), (D, "doubles")])
def test_the_four_forms_of_the_key_column(lib, kind, what):
    """types and validity, types alone, validity alone (a finished Arrow array), neither"""
    n = 3000
    types, values = TC.typed_column(n, 3, what)
    words, bits = TC.validity(n, 3)
    plain = TC.longs_full(n, 4) if kind == L else TC.doubles_wide(n, 4)  # (without types every valid word is a number)
    for largest in (True, False):
        for t, w, b, v in ((types, words, bits, values), (types, None, None, values), (None, words, bits, plain), (None, None, None, plain)):
            for shift in (0, 1, 3):
                _, want, _ = check(lib, t, w, b, v, kind, largest, 100, TC.carried(1, n, n, 8), shift=shift)
                assert want[6] == 100 and (t is not None or want[3] == 0) and (b is not None or t is not None or want[2] == 0)
    # a NaN without types is a NaN; under LONG the same word is a long
    v = plain.copy()
    v[::7] = TC.NAN_BITS[0]
    _, want, _ = check(lib, None, words, bits, v, kind, True, 50)
    assert want[4] == (int(bits[::7].sum()) if kind == D else 0)


def test_live_rows(lib):
    """a device row count of 0, inside the rows, at them and above them: rows at or above it are not read"""
    n = 1025
    types, values = TC.typed_column(n, 5, "longs")
    words, bits = TC.validity(n, 5)
    for row_count in (0, 1, 64, 1000, 1024, 1025, 5000, 1 << 50):
        live = min(n, row_count)
        ty, va = types.copy(), values.copy()
        ty[live:], va[live:] = ord("l"), TC.INT64_MAX  # (poison: a long that would win)
        for k in (1, 70):
            want_rows, want = TC.expected(types, bits, values, live, L, True, k)
            rows, _, _, result, _ = run(lib, ty, words, va, L, True, k, row_count=row_count)
            assert [int(x) for x in result] == want and rows[:want[6]].astype(np.int64).tolist() == want_rows.tolist(), (row_count, k)
    # n_rows below the column, and no row at all
    check(lib, types, words, bits, values, L, False, 9, n_rows=700)
    _, want, _ = check(lib, types[:0], None, None, values[:0], L, True, 9)
    assert want == [0] * 9


@pytest.mark.parametrize("n_cols", [0, 1, 3])
def test_carried_columns(lib, n_cols):
    n = 2000
    types, values = TC.typed_column(n, 6, "counters")
    carry = None if n_cols == 0 else TC.carried(n_cols, n, n + 9, 6)
    for k in (0, 1, 300, 2048):
        for shift in (0, 1):
            check(lib, types, None, None, values, L, True, k, carry, shift=shift)


def test_a_value_word_behind_a_type_that_makes_no_candidate_is_not_read(lib):
    for kind, what in ((L, "longs"), (D, "doubles")):
        types, values = TC.typed_column(3000, 21, what)
        dead = (types != ord("l")) & ((types != ord("d")) | (kind == L))
        assert dead.sum() > 500
        a = run(lib, types, None, values, kind, True, 500)
        for poison in (0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000, 0x7FF0000000000000, 1):
            changed = values.copy()
            changed[dead] = poison
            b = run(lib, types, None, changed, kind, True, 500)
            assert all((x == y).all() for x, y in zip(a[:4], b[:4]))


# ---- shapes where the select can go wrong --------------------------------------------------------------------------------------
def longs_column(vals):
    v = np.array(vals, dtype=np.int64).view(np.uint64)
    return np.full(v.size, ord("l"), dtype=np.uint8), v


def test_all_values_equal_take_no_digit_and_ties_decide(lib):
    for n in (1, 64, 1025, 5000):
        types, values = longs_column([42] * n)
        for largest in (True, False):
            for k in (1, 63, 2048):
                rows, want, digits = check(lib, types, None, None, values, L, largest, k)
                assert digits == 0 and rows.tolist() == list(range(min(k, n))) and want[7] == 42


def test_values_that_differ_in_one_bit(lib):
    """only in bit 0: one digit; only in bit 63 (INT64_MIN with INT64_MAX): all six"""
    for lo, hi, want_digits in ((6, 7, 1), (TC.INT64_MIN, TC.INT64_MAX, 6), (-1, 0, 6), (0, 1 << 62, 6)):
        rng = np.random.default_rng(1)
        types, values = longs_column(np.where(rng.random(3000) < 0.5, lo, hi))
        for largest in (True, False):
            for k in (1, 1400, 1600, 2048):
                _, _, digits = check(lib, types, None, None, values, L, largest, k, what=(lo, hi, largest, k))
                assert digits == want_digits


@pytest.mark.parametrize("bit", TC.DIGIT_EDGES)
def test_pairs_that_differ_exactly_at_a_digit_boundary(lib, bit):
    """two values that differ in one bit next to a digit's edge, with a base that fills the bits around it"""
    base = 0x2AAAAAAAAAAAAAAA & ~(1 << bit)
    rng = np.random.default_rng(bit)
    types, values = longs_column(np.where(rng.random(2500) < 0.4, base, base | (1 << bit)))
    for largest in (True, False):
        for k in (1, 900, 1100, 1500, 2048):
            _, _, digits = check(lib, types, None, None, values, L, largest, k, what=(bit, largest, k))
            assert digits == bit // 11 + 1


def test_a_tie_group_at_the_threshold_across_wave_chunk_and_grid_stride_boundaries(lib):
    """a run of equal values that begins in one wave and ends behind the next chunk (and, with small chunks and a grid cap, in
    another trip of the grid stride); need_equal of 1 and of all but one"""
    n = 3 * 1024
    for first, last in ((60, 70), (1000, 1100), (1020, 2100), (0, n)):
        vals = np.arange(n, dtype=np.int64) % 50  # (below the ties)
        vals[first:last] = 1000
        vals[5], vals[n - 5] = 5000, 5001  # (two above)
        ties = int((vals == 1000).sum())
        types, values = longs_column(vals)
        for k in (2 + 1, 2 + ties - 1, 2 + ties):
            if k > 2048:
                continue
            for chunk, cap in ((0, 0), (64, 3), (256, 1)):
                for order in (0, 1, 2):
                    rows, want, _ = check(lib, types, None, None, values, L, True, k, chunk=chunk, cap=cap, order=order, what=(first, last, k))
                    tied = [r for r in range(n) if vals[r] == 1000]
                    assert rows.tolist() == [n - 5, 5] + tied[:k - 2] and want[7] == 1000


def test_the_threshold_bin_holds_every_candidate(lib):
    """all candidates agree in the first digit that is looked at and differ only in the last"""
    vals = (1 << 40) + (np.arange(4000, dtype=np.int64) * 7) % 2000
    types, values = longs_column(vals)
    _, _, digits = check(lib, types, None, None, values, L, True, 100)
    assert digits == 1
    vals[0] = (1 << 40) + (1 << 30)  # (one row makes it three digits: the first two bins hold all but one)
    types, values = longs_column(vals)
    for k in (1, 2, 100):
        _, _, digits = check(lib, types, None, None, values, L, True, k)
        assert digits == 3


def test_zeros_infinities_and_nans_of_doubles(lib):
    xs = [0.0, -0.0, math.inf, -math.inf, 1.5, -1.5, 5e-324, -5e-324] * 40
    values = np.array(xs, dtype=np.float64).view(np.uint64).copy()
    values[3::16] = TC.NAN_BITS[1]
    types = np.full(values.size, ord("d"), dtype=np.uint8)
    for largest in (True, False):
        for k in (1, 20, 21, 60, 100, 2048):
            rows, want, _ = check(lib, types, None, None, values, D, largest, k)
            got = [TC.double_of(values[r]) for r in rows]
            assert not any(math.isnan(x) for x in got) and want[4] == 20
    # -0.0 against +0.0 alone: the key differs in its top bit
    types, values = np.full(200, ord("d"), dtype=np.uint8), np.array([0.0, -0.0] * 100).view(np.uint64)
    rows, want, _ = check(lib, types, None, None, values, D, True, 101)
    assert rows.tolist() == list(range(0, 200, 2)) + [1] and want[7] == TC.bits_of(-0.0)
    rows, want, _ = check(lib, types, None, None, values, D, False, 3)
    assert rows.tolist() == [1, 3, 5] and want[7] == TC.bits_of(-0.0)


def test_longs_that_round_are_counted_and_tie_as_doubles(lib):
    types, values = longs_column([(1 << 53) + 1, 1 << 53, (1 << 53) + 2, 5, (1 << 53) + 3, -(1 << 53) - 1])
    rows, want, _ = check(lib, types, None, None, values, D, True, 6)
    assert want[5] == 3 and rows.tolist() == [4, 2, 0, 1, 3, 5] and want[7] == TC.bits_of(-float(1 << 53))
    types, values = TC.typed_column(5000, 77, "doubles")
    _, want, _ = check(lib, types, None, None, values, D, False, 2048)
    assert want[5] > 50


def test_schedules_do_not_matter(lib):
    """groups and chunks ascending, descending and odd-first, small chunks, a grid cap that gives a group many chunks: the same
    outputs, word for word"""
    for what, kind in (("longs", L), ("counters", L), ("doubles", D)):
        types, values = TC.typed_column(5 * 1024 + 77, 11, what)
        words, bits = TC.validity(values.size, 11)
        carry = TC.carried(1, values.size, values.size, 11)
        for k in (1, 100, 2048):
            first = None
            for chunk in (64, 256, 0):
                for order in (0, 1, 2):
                    for cap in (0, 1, 3):
                        check(lib, types, words, bits, values, kind, True, k, carry, chunk=chunk, order=order, cap=cap, what=(what, k, chunk, order, cap))
                        got = run(lib, types, words, values, kind, True, k, carry, chunk=chunk, order=order, cap=cap)[:4]
                        first = got if first is None else first
                        assert all((x == y).all() for x, y in zip(first, got))


def test_argument_errors(lib):
    ok = np.zeros(64, dtype=np.uint64)
    ty, va = np.zeros(16, dtype=np.uint8), np.zeros(9, dtype=np.uint64)
    p = lambda a, off=0: a.ctypes.data + off
    R, O, V, S = p(ok), p(ok, 64), p(ok, 128), p(ok, 256)  # rows, out_types, out_values, result

    def f(kt=p(ty), kv=None, kval=p(va), n=4, rc=None, kind=L, flags=0, k=2, t=p(ty), v=p(va), n_cols=1, stride=4, rows=R, ot=O, ov=V, res=S):
        return lib.sim_top_rows(kt, kv, kval, n, rc, kind, flags, k, t, v, n_cols, stride, rows, ot, ov, res, 0, 0, 0, None)

    assert f() == 0
    assert f(kt=None) == 0 and f(kt=None, kv=p(ok, 8)) == 0  # (both NULL is legal: every live row is a candidate)
    assert f(kt=p(ty, 3), t=p(ty, 5), ot=O + 1) == 0  # (types: any alignment)
    assert f(kind=0) == -2 and f(kind=3) == -2 and f(flags=2) == -2 and f(flags=3) == -2 and f(flags=1) == 0
    assert f(k=2049) == -2 and f(k=2048, rows=None) == -2
    assert f(n=1 << 32, stride=1 << 32) == -2
    assert f(kval=None) == -2 and f(kval=None, n=0, stride=0) == 0
    assert f(rows=None) == -2 and f(rows=None, k=0) == 0
    assert f(t=None) == -2 and f(v=None) == -2 and f(ot=None) == -2 and f(ov=None) == -2
    assert f(t=None, v=None, ot=None, ov=None, k=0, rows=None) == 0 and f(t=None, v=None, ot=None, ov=None, n_cols=0, stride=0) == 0
    assert f(stride=3) == -2 and f(stride=3, n_cols=0) == 0
    assert f(kv=p(ok, 4)) == -2 and f(kval=p(va, 4)) == -2 and f(rc=p(ok, 4)) == -2 and f(v=p(va, 4)) == -2
    assert f(rows=R + 4) == -2 and f(ov=V + 4) == -2 and f(res=S + 4) == -2 and f(res=None) == -2


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/toprows_asan_main.cpp: random adversarial columns in heap blocks of exactly their size, every schedule, all
    runs compared with std::stable_sort.  Run as a child process."""
    exe = str(tmp_path / "toprows_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "toprows_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "120"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
