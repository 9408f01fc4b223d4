"""CPU check of the dictionary encoder's passes (simdjson-java_amd/csrc/sj_dictcol.h and sj_strcol.h, which csrc/dictcol.hip
compiles verbatim) against the Python-dict reference of tests/dictcol_common.py: tests/host_sim/dictcol_sim.cpp runs every pass
sequentially, at chunks of 64 and 128 rows and at the kernels' own, with the chunks in three orders and with table loads that
answer stale values.  The string buffer ends at a page that cannot be read and NULL rows carry wild value words, so one
dereference of such a word ends the test process.  A stand-alone program runs the same passes under ASan and UBSan as a child
process (nothing sanitized is loaded into Python)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dictcol_common as DC
from tests import host_sim_lib

CHUNKS = pytest.mark.parametrize("chunk", (64, 128, 0), ids=("chunk64", "chunk128", "chunk_of_the_kernels"))
SCHEDULES = ((0, 0), (1, 0), (2, 1), (0, 1))  # (order of the chunks, stale loads)


def load_sim():
    """tests/host_sim/dictcol_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("dictcol", ("sj_dictcol.h", "sj_strcol.h", "sj_fieldcol.h"))
    lib.sim_dictcol.restype = C.c_int
    lib.sim_dictcol.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.sim_dictcol_chunk_rows.restype = C.c_uint32
    lib.sim_dc_hash.restype = C.c_uint64
    lib.sim_dc_hash.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


def run_sim(lib, types, values, sb, chunk, dict_capacity, byte_capacity, order=0, stale=0, row_count=None, validity=True, dict_rows=True,
            type_shift=0):
    n = len(types)
    store = np.zeros(n + 16, dtype=np.uint8)  # the type column at an odd address: a slice of a larger array
    t = store[type_shift:type_shift + n]
    t[:] = types
    values = np.ascontiguousarray(values, dtype=np.uint64)
    out = DC.Out(n, dict_capacity, byte_capacity)
    rc_word = None if row_count is None else np.array([row_count], dtype=np.uint64)
    ptr = lambda a: a.ctypes.data
    rc = lib.sim_dictcol(ptr(t), ptr(values), n, None if rc_word is None else ptr(rc_word), ptr(sb), sb.size, chunk, order, stale,
                         ptr(out.view("indices")), ptr(out.view("validity")) if validity else None, dict_capacity,
                         ptr(out.view("dict_rows")) if dict_rows else None, ptr(out.view("dict_offsets")),
                         ptr(out.view("dict_bytes")) if byte_capacity else None, byte_capacity, ptr(out.view("result")))
    assert rc == 0, rc
    return out


def check_all(lib, what, types, values, sb, chunk, dict_capacity, caps=None, row_count=None, schedules=SCHEDULES):
    """every schedule at every byte capacity (None: the exact one) -> the reference"""
    R = chunk or lib.sim_dictcol_chunk_rows()
    ref = DC.reference(types, values, sb, row_count)
    total = len(ref.dict_bytes)
    for k, cap in enumerate((None, 0) if caps is None else caps):
        cap = total if cap is None else cap
        for j, (order, stale) in enumerate(schedules):
            out = run_sim(lib, types, values, sb, R, dict_capacity, cap, order, stale, row_count, validity=(k + j) % 3 != 2, dict_rows=(k + j) % 4 != 3,
                          type_shift=(3 * k + j) % 16)
            DC.check("%s, chunk %d, order %d, stale %d, capacity %d of %d" % (what, R, order, stale, cap, total), out, ref, dict_capacity, cap,
                     validity=(k + j) % 3 != 2, dict_rows=(k + j) % 4 != 3)
    return ref


def test_the_reference_on_an_example_read_by_hand():
    sb = np.frombuffer(b"..bb.a.bb..a", dtype=np.uint8)
    types = [ord("l"), ord('"'), ord('"'), 0, ord('"'), ord('"'), ord('"'), ord("n")]
    values = [7, (2 << 32) | 2, (1 << 32) | 5, DC.SC.WILD[0], (2 << 32) | 7, (0 << 32) | 3, (1 << 32) | 11, DC.SC.WILD[1]]
    ref = DC.reference(types, values, sb)
    assert ref.indices.tolist() == [0, 0, 1, 0, 0, 2, 1, 0] and ref.validity.tolist() == [0b01110110]
    assert ref.dict_rows.tolist() == [1, 2, 5] and ref.dict_offsets.tolist() == [0, 2, 3, 3] and ref.dict_bytes == b"bba"
    assert (ref.n_valid, ref.n_other, ref.n_distinct) == (5, 1, 3)
    assert DC.reference(types, values, sb, live=2).dict_rows.tolist() == [1]
    empty = DC.reference([], [], sb)
    assert empty.dict_offsets.tolist() == [0] and empty.n_distinct == 0 and empty.validity.size == 0


def test_the_python_hash_is_the_headers(lib):
    rng = np.random.default_rng(1)
    seen = set()
    for length in list(range(0, 301)) + [8, 16, 24] * 5:
        s = bytes(rng.integers(0, 256, size=length, dtype=np.uint8))
        want = DC.dc_hash(s)
        for tail in (0, 1, 3, int(rng.integers(0, 8))):  # (the string at different addresses modulo 8, and ending the buffer)
            assert lib.sim_dc_hash(s, length, tail) == want, (length, tail)
        seen.add(want)
    assert len(seen) > 300
    # a string and the same with a zero byte behind it are different values
    assert DC.dc_hash(b"ab") != DC.dc_hash(b"ab\0") and DC.dc_hash(b"") != DC.dc_hash(b"\0")
    words = rng.integers(0, 1 << 40, size=50, dtype=np.uint64)
    assert DC.dc_hash_words(words, 5).tolist() == [DC.dc_hash(int(w).to_bytes(8, "little")[:5]) for w in words]


def test_the_colliding_strings_collide():
    for slot in (17, 63, 5):
        assert {DC.start_slot(s, 64) for s in DC.strings_starting_at(slot, 64, 8)} == {slot}
    for last in (False, True):
        a, b = DC.tag_twins(64, 6, last)
        assert a != b and len(a) == len(b) == 6 and DC.tag(a) == DC.tag(b) and DC.start_slot(a, 64) == DC.start_slot(b, 64)
        assert not last or (a[:5] == b[:5] and a[5] != b[5])


@CHUNKS
def test_row_counts(lib, chunk):
    R = chunk or lib.sim_dictcol_chunk_rows()
    rng = np.random.default_rng(100 + R)
    for n in sorted(set(DC.ROW_COUNTS) | {R - 1, R, R + 1, 2 * R + 1}):
        t, v, sb = DC.column_of(rng, DC.mixed_cells(rng, n, DC.NINE))
        ref = check_all(lib, "%d rows" % n, t, v, sb, chunk, 16)
        assert n < 200 or ref.n_distinct == 9


@CHUNKS
def test_late_first_occurrences(lib, chunk):
    t, v, sb = DC.column_of(np.random.default_rng(2), DC.late_first_cells())
    ref = check_all(lib, "late first rows", t, v, sb, chunk, 8)
    assert ref.dict_rows.tolist() == [1024, 1087, 2048]


@CHUNKS
def test_uniform_columns(lib, chunk):
    rng = np.random.default_rng(3)
    for name, cells, capacity in DC.uniform_cases():
        t, v, sb = DC.column_of(rng, cells)
        check_all(lib, name, t, v, sb, chunk, capacity)


@CHUNKS
def test_forced_collisions(lib, chunk):
    rng = np.random.default_rng(4)
    for name, cells, place in DC.collision_cases():
        t, v, sb = DC.column_of(rng, cells, place=place)
        ref = check_all(lib, name, t, v, sb, chunk, 32)
        assert ref.n_distinct == len({c for c in cells if c is not None}) <= 32


def test_overflow(lib):
    rng = np.random.default_rng(5)
    cells = DC.mixed_cells(rng, 300, [b"v%d" % k for k in range(33)], p_null=0.2)
    t, v, sb = DC.column_of(rng, cells)
    assert check_all(lib, "capacity + 1 values", t, v, sb, 64, 32, caps=(None, 0, 50)).n_distinct == 33
    check_all(lib, "exactly the capacity", t, v, sb, 64, 33)
    cells = DC.mixed_cells(rng, 500, [b"value %d" % k for k in range(40)], p_null=0.1)
    t, v, sb = DC.column_of(rng, cells)
    check_all(lib, "40 values, capacity 2: the table fills", t, v, sb, 128, 2, caps=(None, 9))
    check_all(lib, "capacity 0 with a VALID row", t, v, sb, 64, 0, caps=(0, 9))
    t, v, sb = DC.column_of(rng, [None] * 130)
    assert check_all(lib, "capacity 0 without one", t, v, sb, 64, 0, caps=(0, 9)).n_distinct == 0
    t, v, sb = DC.column_of(rng, [None, b"one"])
    check_all(lib, "capacity 0, one row", t, v, sb, 64, 0)
    check_all(lib, "capacity 1, one value", t, v, sb, 64, 1)


def test_byte_capacities_and_the_empty_string(lib):
    rng = np.random.default_rng(6)
    t, v, sb = DC.column_of(rng, DC.mixed_cells(rng, 400, DC.NINE))
    total = len(DC.reference(t, v, sb).dict_bytes)
    check_all(lib, "byte capacities", t, v, sb, 128, 9, caps=(0, total - 1, total, total + 7, 1))
    t, v, sb = DC.column_of(rng, [None, b"", None, b"", b""])
    ref = check_all(lib, "the empty string alone", t, v, sb, 64, 4, caps=(0, 5))
    assert ref.n_distinct == 1 and ref.dict_offsets.tolist() == [0, 0]


def test_live_rows_below_the_rows_given(lib):
    rng = np.random.default_rng(7)
    cells = DC.mixed_cells(rng, 700, DC.NINE[:5]) + [b"behind the live rows %d" % k for k in range(300)]
    t, v, sb = DC.column_of(rng, cells)
    for live in (700, 0, 1, 64, 129, 999, 1000, 5000):
        ref = check_all(lib, "%d live rows" % live, t, v, sb, 128, 512, row_count=live, schedules=SCHEDULES[:3:2])
        assert ref.live == min(live, 1000) and (live > 700 or ref.n_distinct <= 5)


def test_contention_and_the_second_slice_of_the_scan(lib):
    """64 * 1024 + 1 rows at chunks of 64: chunk 1024 is the first of the scan's second slice, and its one row is a new value;
    every other row is one of three values.  (The GPU test has 1024 * 1024 + 1 rows at its chunks of 1024.)"""
    t, v, sb, ref = DC.contention_column(np.random.default_rng(8), 64 * 1024 + 1)
    outs = [run_sim(lib, t, v, sb, 64, 8, len(ref.dict_bytes), order, stale) for order, stale in ((0, 0), (1, 1), (2, 1))]
    for out in outs:
        DC.check("the scan's second slice", out, ref, 8, len(ref.dict_bytes))
    assert all(np.array_equal(getattr(outs[0], s + "_store"), getattr(o, s + "_store")) for o in outs[1:] for s in DC.Out.STORES)


def test_behind_the_filter_simulation_with_its_n_kept_as_the_row_count():
    """tests/host_sim/filter_sim.cpp keeps the string rows of the first 1100 rows and compacts them into columns of 1400 entries;
    the dictionary simulation reads the filter's own record as its row count.  What lies at or above n_kept in the compacted
    column are strings that would add entries."""
    from tests import filter_common as FC
    from tests import test_host_filter as HF
    flt, lib = HF.load_sim(), load_sim()
    rng = np.random.default_rng(7)
    cells = DC.mixed_cells(rng, 1100, DC.NINE[:5]) + [b"behind the live rows %d" % k for k in range(300)]
    t, v, sb = DC.column_of(rng, cells)
    n = len(cells)
    kept = [r for r in range(1100) if cells[r] is not None]
    enc, _ = FC.encode([(0, "type_eq", DC.STRING)])
    out_types, out_values = t.copy(), v.copy()
    rows, result = np.zeros(n, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert flt.sim_filter(enc.ctypes.data, 1, None, 0, t.ctypes.data, v.ctypes.data, 1, n, 1100, sb.ctypes.data, sb.size, 128, None, rows.ctypes.data, n,
                          out_types.ctypes.data, out_values.ctypes.data, result.ctypes.data) == 0
    assert int(result[0]) == len(kept) < 1100 and (out_types[len(kept):] == DC.STRING).sum() >= 300
    ref = DC.reference(out_types, out_values, sb, len(kept))
    assert ref.values == DC.reference_from_cells([(DC.STRING, cells[r]) for r in kept]).values
    out = DC.Out(n, 512, 8192)
    assert lib.sim_dictcol(out_types.ctypes.data, out_values.ctypes.data, n, result.ctypes.data, sb.ctypes.data, sb.size, 128, 2, 1,
                           out.view("indices").ctypes.data, out.view("validity").ctypes.data, 512, out.view("dict_rows").ctypes.data,
                           out.view("dict_offsets").ctypes.data, out.view("dict_bytes").ctypes.data, 8192, out.view("result").ctypes.data) == 0
    DC.check("behind the filter simulation", out, ref, 512, 8192)


def test_fuzz(lib):
    rng = np.random.default_rng(8)
    distinct = 0
    for k in range(40):
        vocabulary = [bytes(rng.integers(97, 100, size=int(rng.integers(0, 12)), dtype=np.uint8)) for _ in range(int(rng.choice([1, 3, 40, 400])))]
        n = int(rng.integers(1, 700))
        t, v, sb = DC.column_of(rng, DC.mixed_cells(rng, n, vocabulary, p_null=float(rng.choice([0.0, 0.3, 0.9]))), sb_gap=int(rng.integers(0, 9)))
        capacity = int(rng.choice([0, 1, 2, 8, 64, 1000]))
        distinct += check_all(lib, "fuzz column %d" % k, t, v, sb, int(rng.choice([64, 128, 0])), capacity,
                              row_count=None if k % 3 else int(rng.integers(0, n + 5)), schedules=SCHEDULES[k % 2::2]).n_distinct
    assert distinct > 300


def test_a_string_that_ends_the_buffer(lib):
    """the guard page is live: the last word in front of it is read, and the wild words of the NULL rows are not followed"""
    rng = np.random.default_rng(9)
    cells = [None, b"x", None, b"ends the buffer!"] * 20
    t, v, sb = DC.column_of(rng, cells)
    assert int(v[-1] & np.uint64(0xFFFFFFFF)) + 16 == sb.size
    assert check_all(lib, "at the guard page", t, v, sb, 64, 4).n_distinct == 2


def test_pyarrow_takes_the_outputs(lib):
    pa = pytest.importorskip("pyarrow")
    rng = np.random.default_rng(10)
    cells = DC.mixed_cells(rng, 333, [b"PushEvent", b"", b"en", b"\xe6\x97\xa5\xe6\x9c\xac", b"WatchEvent"])
    t, v, sb = DC.column_of(rng, cells)
    ref = DC.reference(t, v, sb)
    out = run_sim(lib, t, v, sb, 64, 8, len(ref.dict_bytes))
    DC.check("pyarrow", out, ref, 8, len(ref.dict_bytes))
    nd, n = ref.n_distinct, len(cells)
    dictionary = pa.LargeStringArray.from_buffers(nd, pa.py_buffer(out.view("dict_offsets")[:nd + 1].tobytes()),
                                                  pa.py_buffer(out.view("dict_bytes")[:len(ref.dict_bytes)].tobytes()))
    indices = pa.Array.from_buffers(pa.int32(), n, [pa.py_buffer(out.view("validity")[:(n + 63) // 64].tobytes()),
                                                    pa.py_buffer(out.view("indices")[:n].tobytes())])
    got = pa.DictionaryArray.from_arrays(indices, dictionary)
    got.validate(full=True)
    want = pa.array([None if c is None else c.decode() for c in cells], type=pa.large_string()).dictionary_encode()
    assert got.dictionary.to_pylist() == want.dictionary.to_pylist()
    assert got.indices.to_pylist() == want.indices.to_pylist() and got.to_pylist() == want.to_pylist()


def test_argument_errors(lib):
    sb = np.zeros(8, dtype=np.uint8)
    w = np.zeros(8, dtype=np.uint64)
    p = w.ctypes.data
    assert lib.sim_dictcol(None, None, 0, None, sb.ctypes.data, 8, 100, 0, 0, p, None, 1, None, p, None, 0, p) == -2
    assert lib.sim_dictcol(None, None, 0, None, sb.ctypes.data, 8, 64, 0, 0, p, None, 1, None, p, None, 5, p) == -2
    assert lib.sim_dictcol(None, None, 0, None, sb.ctypes.data, 8, 64, 0, 0, p, None, DC.MAX_ENTRIES + 1, None, p, None, 0, p) == -2


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/dictcol_asan_main.cpp: random adversarial columns in heap blocks of exactly their size, every schedule, all
    runs of a case compared with a std::map reference.  Run as a child process."""
    exe = str(tmp_path / "dictcol_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "dictcol_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "120"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
