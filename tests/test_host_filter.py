"""CPU check of the row filter's passes (simdjson-java_amd/csrc/sj_filter.h, which csrc/filter.hip compiles verbatim) against the
Python reference of tests/filter_common.py: tests/host_sim/filter_sim.cpp runs the terms, the scan of the chunk counts and the
emit sequentially, at chunks of 64 and 128 rows and at the kernels' own.  The string buffer ends at a page that cannot be read
and cells that are no strings carry wild value words, so one use of such a word as an offset ends the test process."""
import ctypes as C

import numpy as np
import pytest

from tests import host_sim_lib
from tests import filter_common as FC

CHUNKS = pytest.mark.parametrize("chunk", (64, 128, 0), ids=("chunk64", "chunk128", "chunk_of_the_kernels"))


def load_sim():
    """tests/host_sim/filter_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("filter", ("sj_filter.h",))
    lib.sim_filter.restype = C.c_int
    lib.sim_filter.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                               C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sim_filter_chunk_rows.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


_REFERENCES = {}


def reference(case):
    """the reference of a case, computed once for all chunk sizes (the generators are seeded: a name is a case)"""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = FC.reference(case)
    return _REFERENCES[case.name]


def run_sim(lib, case, chunk, capacity, keep=True, outs=True, type_shift=0, expect=0):
    n_cols, stride = case.types.shape
    store = np.zeros(n_cols * stride + 16, dtype=np.uint8)  # the type columns at an odd address: a slice of a larger array
    t = store[type_shift:type_shift + n_cols * stride]
    t[:] = case.types.reshape(-1)
    values = np.ascontiguousarray(case.values, dtype=np.uint64)
    enc, blob = FC.encode(case.terms)
    consts = np.frombuffer(blob + b"\0", dtype=np.uint8)
    words, rows, otypes, ovalues, res = FC.out_buffers(case.n_rows, n_cols, capacity, keep, outs)
    ostore = np.full((otypes.size if outs else 0) + 16, FC.CANARY, dtype=np.uint8)  # ... and so the compacted types
    ot = ostore[(type_shift + 5) % 16:][:otypes.size] if outs else None
    rc = lib.sim_filter(enc.ctypes.data if len(enc) else None, len(enc), consts.ctypes.data if blob else None, len(blob), t.ctypes.data,
                        values.ctypes.data, n_cols, stride, case.n_rows, case.sb.ctypes.data, case.sb.size, chunk,
                        words.ctypes.data if keep else None, rows.ctypes.data if outs else None, capacity, ot.ctypes.data if outs else None,
                        ovalues.ctypes.data if outs else None, res.ctypes.data)
    assert rc == expect, (case.name, rc)
    return words, rows, ot, ovalues, res


def check_all(lib, case, chunk, caps=None):
    """the case at every capacity (caps=None) or at those given, each optional output left out in turn"""
    keep = reference(case)
    n_kept = int(keep.sum())
    for k, capacity in enumerate(FC.capacities(n_kept) if caps is None else caps):
        got = run_sim(lib, case, chunk, capacity, keep=k % 3 != 1, outs=capacity > 0 or k % 2 == 0, type_shift=(3 * k + 1) % 16)
        FC.check("%s, chunk %d, capacity %d of %d" % (case.name, chunk, capacity, n_kept), *got, case, keep, capacity)
    return n_kept


def test_the_reference_on_an_example_read_by_hand():
    sb = np.frombuffer(b"..ja.jax", dtype=np.uint8)
    S, L, D = FC.STRING, FC.LONG, FC.DOUBLE
    types = np.array([[S, S, 0, S, L], [L, D, L, ord("n"), L]], dtype=np.uint8)
    values = np.array([[(2 << 32) | 2, (3 << 32) | 5, FC.WILD[0], (2 << 32) | 5, 7], [1000, FC.bits_of(1000.5), 5000, FC.WILD[1], (1 << 64) - 1]], dtype=np.uint64)
    case = lambda terms: FC.Case("by hand", terms, types, values, 5, sb)
    assert FC.reference(case([(0, "string_eq", b"ja")])).tolist() == [True, False, False, True, False]
    assert FC.reference(case([(0, "string_prefix", b"ja")])).tolist() == [True, True, False, True, False]
    assert FC.reference(case([(0, "string_ne", b"ja")])).tolist() == [False, True, False, False, False]
    assert FC.reference(case([(1, "long_gt", 1000)])).tolist() == [False, True, True, False, False]
    assert FC.reference(case([(1, "long_ne", 1000)])).tolist() == [False, True, True, False, True]  # (not the null cell)
    assert FC.reference(case([(0, "string_prefix", b"ja"), (1, "double_le", 1000.5)])).tolist() == [True, True, False, False, False]
    assert FC.reference(case([(0, "type_ne", 0), (1, "type_eq", L)])).tolist() == [True, False, False, False, True]
    assert FC.reference(case([])).tolist() == [True] * 5
    assert FC.words_of(np.array([True, False, True])).tolist() == [5]
    # the mixed comparisons are those of the real numbers: numpy's float64 would call the first pair equal
    big = FC.Case("2^53 + 1", [(0, "double_gt", 2.0 ** 53)], np.array([[L, L]], dtype=np.uint8), np.array([[(1 << 53) + 1, 1 << 53]], dtype=np.uint64), 2, sb)
    assert FC.reference(big).tolist() == [True, False]
    assert FC.reference(big._replace(terms=[(0, "double_eq", 2.0 ** 53)])).tolist() == [False, True]


@CHUNKS
def test_row_counts_and_capacities(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    kept = 0
    for n in sorted(set(FC.ROW_COUNTS) | {R - 1, R, R + 1, 2 * R + 1}):
        kept += check_all(lib, FC.row_count_case(n), R)
    assert kept > 500


@CHUNKS
def test_keep_patterns(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    for case in FC.keep_pattern_cases():
        check_all(lib, case, R)


@CHUNKS
def test_every_op_on_a_cell_of_every_type(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    kept = {}
    for case in FC.op_table_cases():
        n = check_all(lib, case, R, caps=(int(reference(case).sum()),))
        op = case.terms[0][1]
        kept[op] = kept.get(op, 0) + n
    assert sorted(kept) == sorted(FC.ALL_OPS) and all(kept.values()), kept  # every op is true somewhere


@CHUNKS
def test_numeric_edges(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    kept = sum(check_all(lib, case, R, caps=(int(reference(case).sum()), 1)) for case in FC.numeric_edge_cases())
    assert kept > 1000


@CHUNKS
def test_string_edges(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    kept = sum(check_all(lib, case, R, caps=(int(reference(case).sum()),)) for case in FC.string_edge_cases())
    # per length and alignment EQ keeps 2 cells, NE 4 and PREFIX 3; with the empty constant 2, 1 and 3
    assert kept == 16 * (6 * 9 + 6)


@CHUNKS
def test_layouts(lib, chunk):
    R = chunk or lib.sim_filter_chunk_rows()
    for case in FC.layout_cases():
        n_kept = check_all(lib, case, R)
        assert case.terms == [] or 0 < n_kept < case.n_rows, case.name


def test_fuzz(lib):
    """200 seeded cases at every chunk size; at least a quarter of them keep some rows but not all, by the REFERENCE's counts"""
    R = lib.sim_filter_chunk_rows()
    partial = 0
    for seed in range(200):
        case = FC.fuzz_case(5000 + seed)
        keep = FC.reference(case)
        n_kept = int(keep.sum())
        partial += 0 < n_kept < case.n_rows
        for chunk in (64, 128, R):
            for k, capacity in enumerate(FC.capacities(n_kept) if seed % 8 == 0 else (n_kept, n_kept // 2)):
                got = run_sim(lib, case, chunk, capacity, keep=(seed + k) % 3 != 0, outs=capacity > 0, type_shift=seed % 16)
                FC.check("%s, chunk %d, capacity %d of %d" % (case.name, chunk, capacity, n_kept), *got, case, keep, capacity)
    assert partial >= 50, partial


def test_a_string_that_ends_the_buffer_and_wild_words_beside_it(lib):
    """the guard page is live: the last byte in front of it is read (the cell is EQ only if it is), the wild words are not used"""
    sb = np.frombuffer(b"x" * 56 + b"y" * 199 + b"z", dtype=np.uint8)
    S = FC.STRING
    types = np.array([[0, S, ord("n"), ord("{"), S] * 40], dtype=np.uint8)
    values = np.array([[FC.WILD[0], (200 << 32) | 56, FC.WILD[3], FC.WILD[5], (200 << 32) | 55] * 40], dtype=np.uint64)
    case = FC.Case("at the guard page", [(0, "string_eq", b"y" * 199 + b"z")], types, values, 200, sb)
    assert check_all(lib, case, 64) == 40


def test_argument_errors(lib):
    case = FC.row_count_case(65)
    run_sim(lib, case, 100, 0, outs=False, expect=-2)                                                  # a chunk that is no multiple of 64
    run_sim(lib, case._replace(terms=[(3, "type_eq", 0)]), 64, 0, outs=False, expect=-2)               # column >= n_cols
    run_sim(lib, case._replace(terms=[(0, "double_eq", float("nan"))]), 64, 0, outs=False, expect=-2)  # a plan that does not compile
    run_sim(lib, case._replace(terms=[(0, "type_eq", 0)] * 17), 64, 0, outs=False, expect=-2)
