"""CPU check of the Arrow column export's passes (simdjson-java_amd/csrc/sj_arrowcol.h, which csrc/arrowcol.hip compiles verbatim)
against the Python reference of tests/arrowcol_common.py: tests/host_sim/arrowcol_sim.cpp runs the conversion and the sum of the
chunk counts sequentially, at chunks of 64 and 128 rows and at the kernels' own.  The type block, the value block and both output
blocks end at pages that cannot be touched, the type and value blocks right behind the last column's last LIVE row: one read of
a row at or above the live rows there, or one write past the last field's slice, ends the test process."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import arrowcol_common as AC
from tests import fieldcol_common as F
from tests import host_sim_lib

CHUNKS = pytest.mark.parametrize("chunk", (64, 128, 0), ids=("chunk64", "chunk128", "chunk_of_the_kernels"))


def load_sim():
    """tests/host_sim/arrowcol_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("arrowcol", ("sj_arrowcol.h", "sj_fieldcol.h"))
    lib.sim_arrowcol.restype = C.c_int
    lib.sim_arrowcol.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint32,
                                 C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.sim_arrowcol_chunk_rows.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


_REFERENCES = {}


def reference(case):
    """the reference of a case, computed once for all chunk sizes (the generators are seeded: a name is a case)"""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = AC.reference(case)
    return _REFERENCES[case.name]


def run_sim(lib, case, chunk, *how, **over):
    return F.run_sim(lib.sim_arrowcol, AC, case, chunk, *how, **over)


def check_all(lib, case, chunk, forms=((True, True), (True, False), (False, True), (False, False)), shift=1):
    """the case with both blocks, without the validity, as the counting call, and as the counting call without validity"""
    ref = reference(case)
    for k, (data, validity) in enumerate(forms):
        got = run_sim(lib, case, chunk, data, validity, type_shift=(5 * k + shift) % 16)
        AC.check("%s, chunk %d, data %s, validity %s" % (case.name, chunk, data, validity), *got, case, ref)
    return ref


def test_the_reference_on_an_example_read_by_hand():
    L, D, T, F, N, S = AC.LONG, AC.DOUBLE, AC.TRUE, AC.FALSE, AC.NULL, AC.STRING
    types = np.array([[L, D, N, 0, S, D, L], [T, F, N, T, L, 0, T]], dtype=np.uint8)
    values = np.array([[7, AC.bits_of(2.0), AC.WILD[0], AC.WILD[1], AC.WILD[2], AC.bits_of(2.5), (1 << 53) + 1],
                       [AC.WILD[0], AC.WILD[1], 0, 0, 1, 0, 0]], dtype=np.uint64)
    case = AC.make_case("by hand", [(0, "int64"), (0, "int64", "integral_doubles"), (0, "float64"), (1, "bool")], types, values, 7)
    ref = AC.reference(case)
    assert ref.live == 7
    assert ref.data[0] == [7, 0, 0, 0, 0, 0, (1 << 53) + 1] and ref.validity[0] == [0b1000001] and ref.records[0] == (7, 2, 3, 0)
    assert ref.data[1] == [7, 2, 0, 0, 0, 0, (1 << 53) + 1] and ref.validity[1] == [0b1000011] and ref.records[1] == (7, 3, 2, 0)
    assert ref.data[2] == [AC.bits_of(7.0), AC.bits_of(2.0), 0, 0, 0, AC.bits_of(2.5), AC.bits_of(2.0 ** 53)]
    assert ref.validity[2] == [0b1100011] and ref.records[2] == (7, 4, 1, 1)
    assert ref.data[3] == [0b1001001] and ref.validity[3] == [0b1001011] and ref.records[3] == (7, 4, 1, 0)
    # a row count cuts every field; above n_rows it is clamped
    cut = AC.reference(case._replace(row_count=2))
    assert cut.live == 2 and cut.data[0] == [7, 0] and cut.validity[3] == [0b11] and cut.records[2] == (2, 2, 0, 0)
    assert AC.reference(case._replace(row_count=99)).records == ref.records
    none = AC.reference(case._replace(row_count=0))
    assert none.data == [[], [], [], []] and none.validity == [[], [], [], []] and none.records == [(0, 0, 0, 0)] * 4
    # the edges of the issue, one by one
    one = lambda kind, ty, word, *flags: AC.cell(kind, flags, ty, word)
    assert one("float64", L, (1 << 53) + 1) == (AC.bits_of(2.0 ** 53), True, False, True)
    assert one("float64", L, 1 << 53) == (AC.bits_of(2.0 ** 53), True, False, False)
    assert one("float64", L, (1 << 53) + 3) == (AC.bits_of(2.0 ** 53 + 4), True, False, True)        # (a tie: to the even neighbour)
    assert one("float64", L, AC.INT64_MIN & AC.MASK) == (AC.bits_of(-2.0 ** 63), True, False, False)
    assert one("float64", L, AC.INT64_MAX) == (AC.bits_of(2.0 ** 63), True, False, True)
    assert one("float64", L, (1 << 62) + (1 << 9))[3] and not one("float64", L, (1 << 62) + (1 << 10))[3]
    assert one("int64", D, AC.bits_of(-0.0), "integral_doubles") == (0, True, False, False)
    assert one("int64", D, AC.bits_of(-2.0 ** 63), "integral_doubles") == (1 << 63, True, False, False)
    assert one("int64", D, AC.bits_of(2.0 ** 63), "integral_doubles") == (0, False, True, False)
    assert one("int64", D, AC.bits_of(math.nextafter(2.0 ** 63, 0.0)), "integral_doubles") == ((1 << 63) - 1024, True, False, False)
    assert one("int64", D, AC.bits_of(5.0)) == (0, False, True, False)
    for x in (math.inf, -math.inf, math.nan, 0.5, 5e-324):
        assert one("int64", D, AC.bits_of(x), "integral_doubles") == (0, False, True, False)
        assert one("float64", D, AC.bits_of(x)) == (AC.bits_of(x), True, False, False)
    assert one("int64", D, AC.bits_of(1e300), "integral_doubles") == (0, False, True, False)
    assert one("bool", T, AC.WILD[0]) == (1, True, False, False) and one("bool", F, AC.WILD[0]) == (0, True, False, False)
    assert one("bool", L, 1) == (0, False, True, False) and one("bool", 0, 1) == (0, False, False, False)
    assert AC.pack_bits([1] + [0] * 63 + [1, 1]) == [1, 3]


@CHUNKS
def test_row_counts_and_live_counts(lib, chunk):
    R = chunk or lib.sim_arrowcol_chunk_rows()
    valid = 0
    for n in sorted(set(AC.ROW_COUNTS) | {R - 1, R, R + 1, 2 * R + 1}):
        for case in AC.row_count_cases(n):
            valid += sum(r[1] for r in check_all(lib, case, R, shift=n % 16).records)
    assert valid > 5000


@CHUNKS
def test_the_types_at_every_shift(lib, chunk):
    R = chunk or lib.sim_arrowcol_chunk_rows()
    case = AC.type_shift_case()
    for shift in range(16):
        AC.check("shift %d" % shift, *run_sim(lib, case, R, type_shift=shift), case, reference(case))


@CHUNKS
def test_every_kind_on_a_cell_of_every_type(lib, chunk):
    R = chunk or lib.sim_arrowcol_chunk_rows()
    case = AC.kind_table_case()
    ref = check_all(lib, case, R)
    n = case.n_rows
    # INT64: the 4 longs; with the flag 0.0, 5.0 and -7.0 too; FLOAT64: all 9 numbers; BOOL: the 6 booleans.  MISSING and 'n'
    # are the only cells that are not "other"
    assert ref.records == [(n, 4, n - 4 - 2, 0), (n, 7, n - 7 - 2, 0), (n, 9, n - 9 - 2, 1), (n, 6, n - 6 - 2, 0)]


@CHUNKS
def test_numeric_edges(lib, chunk):
    R = chunk or lib.sim_arrowcol_chunk_rows()
    case = AC.numeric_edge_case()
    ref = check_all(lib, case, R)
    n, nl, nd = case.n_rows, len(AC.EDGE_LONGS), len(AC.EDGE_DOUBLES)
    # inexact: INT64_MAX, +-(2^53 + 1), 2^53 + 3, 2^62 + 2^9; integral doubles in range: -0.0, -2^63, the double below 2^63, 0.0, 1.0, -7.0, 2^53
    assert ref.records == [(n, nl, 0, 0), (n, nl, 0, 0), (n, nl, 0, 5), (n, 0, nd, 0), (n, 7, nd - 7, 0), (n, nd, 0, 0)]


@CHUNKS
def test_schemas(lib, chunk):
    R = chunk or lib.sim_arrowcol_chunk_rows()
    for case in AC.schema_cases():
        ref = check_all(lib, case, R)
        assert any(0 < r[1] < r[0] for r in ref.records), case.name


def test_fuzz(lib):
    """200 seeded cases at every chunk size.  The generator's conditions are asserted from the REFERENCE's counts: a quarter of
    all fields have both a VALID and a NULL row, 30 fields have an other-typed row, 30 an inexact conversion"""
    R = lib.sim_arrowcol_chunk_rows()
    fields = mixed = other = inexact = 0
    for seed in AC.FUZZ_SEEDS:
        case = AC.fuzz_case(seed)
        ref = AC.reference(case)
        fields += len(ref.records)
        mixed += sum(0 < r[1] < r[0] for r in ref.records)
        other += sum(r[2] > 0 for r in ref.records)
        inexact += sum(r[3] > 0 for r in ref.records)
        for chunk in (64, 128, R):
            forms = ((True, True), (False, False)) if seed % 8 == 0 else ((True, True),) if seed % 3 else ((True, False), (False, True))
            for k, (data, validity) in enumerate(forms):
                got = run_sim(lib, case, chunk, data, validity, type_shift=(seed + k) % 16)
                AC.check("%s, chunk %d, data %s, validity %s" % (case.name, chunk, data, validity), *got, case, ref)
    assert 4 * mixed >= fields and other >= 30 and inexact >= 30, (fields, mixed, other, inexact)


def test_argument_errors(lib):
    case = AC.row_count_cases(65)[0]
    n_fields = len(case.fields)
    bad_field = lambda **kw: np.array([tuple(dict(dict(column=0, kind=1, flags=0, reserved=0), **kw).values())], dtype=AC.FIELD)
    run_sim(lib, case, 100, expect=-2)                                                     # a chunk that is no multiple of 64
    run_sim(lib, case, 64, fields=np.zeros(0, dtype=AC.FIELD), expect=-2)                  # no field
    run_sim(lib, case._replace(fields=[(0, "bool")] * 65), 64, expect=-2)                  # more than 64
    assert n_fields == 4
    for f in (dict(kind=0), dict(kind=4), dict(kind=2, flags=1), dict(kind=3, flags=1), dict(flags=2), dict(reserved=1), dict(column=3)):
        one = case._replace(fields=[(0, "int64")])
        run_sim(lib, one, 64, fields=bad_field(**f), expect=-2)
    run_sim(lib, case._replace(fields=[(0, "int64")]), 64, fields=bad_field(flags=1))     # (legal: the flag of an INT64 field)
    run_sim(lib, case, 64, col_stride=64, readable=0, expect=-2)                           # col_stride < n_rows
    run_sim(lib, case, 64, data_stride=64, expect=-2)                                      # data_stride < n_rows
    run_sim(lib, case, 64, data=False, data_stride=65, expect=-2)                          # a stride without d_data
    run_sim(lib, case, 64, validity_stride=1, expect=-2)                                   # validity_stride < ceil(n_rows / 64)
    run_sim(lib, case, 64, results=None, expect=-2)


def test_the_layout_is_arrows():
    """pyarrow.Array.from_buffers over the reference's buffers = pyarrow.array of the Python values, one case per kind"""
    pa = pytest.importorskip("pyarrow")
    L, D, T, F, N = AC.LONG, AC.DOUBLE, AC.TRUE, AC.FALSE, AC.NULL
    rows = 70  # (a second word of both bitmaps)
    cells = [[(L, 5), (N, 0), (L, (-3) & AC.MASK), (0, 0), (D, AC.bits_of(4.0))], [(D, AC.bits_of(1.5)), (L, 2), (N, 0), (D, AC.bits_of(-0.25)), (0, 0)],
             [(T, 0), (F, 0), (N, 0), (T, 0), (L, 1)]]
    values = [[5, None, -3, None, 4], [1.5, 2.0, None, -0.25, None], [True, False, None, True, None]]
    t = np.array([[c[k % 5][0] for k in range(rows)] for c in cells], dtype=np.uint8)
    v = np.array([[c[k % 5][1] for k in range(rows)] for c in cells], dtype=np.uint64)
    case = AC.make_case("pyarrow", [(0, "int64", "integral_doubles"), (1, "float64"), (2, "bool")], t, v, rows)
    ref = AC.reference(case)
    for f, ty in enumerate((pa.int64(), pa.float64(), pa.bool_())):
        buffers = [pa.py_buffer(np.array(ref.validity[f], dtype="<u8").tobytes()), pa.py_buffer(np.array(ref.data[f], dtype="<u8").tobytes())]
        got = pa.Array.from_buffers(ty, rows, buffers, null_count=rows - ref.records[f][1])
        got.validate(full=True)
        assert got.equals(pa.array([values[f][k % 5] for k in range(rows)], type=ty)), (f, got)
