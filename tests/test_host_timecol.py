"""CPU check of the timestamp column export's passes (simdjson-java_amd/csrc/sj_timecol.h, which csrc/timecol.hip compiles verbatim)
against the Python reference of tests/timecol_common.py: tests/host_sim/timecol_sim.cpp runs the parse and the sum of the chunk
counts sequentially, at chunks of 64, 128 and 1024 rows and at the kernels' own (256), with BOTH forms of the byte fetch.  The type block,
the value block, the string buffer and both output blocks end at pages that cannot be touched -- the type and value blocks right
behind the last column's last LIVE row, the string buffer right behind its last string -- and a second run has the string buffer
BEGIN behind such a page: one read of a row that is not live, of a byte outside the buffer, or one write past the last field's
slice, ends the test process.  The reference itself is checked against values worked out by hand and against datetime."""
import ctypes as C
import datetime

import numpy as np
import pytest

from tests import fieldcol_common as F
from tests import host_sim_lib
from tests import timecol_common as TC

CHUNKS = pytest.mark.parametrize("chunk", (64, 128, 1024, 0), ids=("chunk64", "chunk128", "chunk1024", "chunk_of_the_kernels"))
FORMS = ((True, True), (True, False), (False, True), (False, False))  # both blocks, no validity, the counting call, records only


def load_sim():
    """tests/host_sim/timecol_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("timecol", ("sj_timecol.h", "sj_fieldcol.h"))
    lib.sim_timecol.restype = C.c_int
    lib.sim_timecol.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.sim_timecol_chunk_rows.restype = C.c_uint32
    return lib


@pytest.fixture(scope="module")
def lib():
    return load_sim()


_REFERENCES = {}


def reference(case):
    """the reference of a case, computed once for all chunk sizes and forms (the generators are seeded: a name is a case)"""
    if case.name not in _REFERENCES:
        _REFERENCES[case.name] = TC.reference(case)
    return _REFERENCES[case.name]


def run_sim(lib, case, chunk, *how, **over):
    return F.run_sim(lib.sim_timecol, TC, case, chunk, *how, **over)


def check_all(lib, case, chunk, forms=FORMS, shift=1):
    """the case with both blocks, without the validity, as the counting call, and as the counting call without validity -- the
    fetch forms in turn, and both on the first"""
    ref = reference(case)
    for k, (data, validity) in enumerate(forms):
        for words in ((0, 1) if k == 0 else (k % 2,)):
            got = run_sim(lib, case, chunk, data, validity, type_shift=(5 * k + shift) % 16, words=words)
            TC.check("%s, chunk %d, data %s, validity %s, words %d" % (case.name, chunk, data, validity, words), *got, case, ref)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------------------
def test_the_reference_on_values_worked_out_by_hand(lib):
    """... and the passes on the same strings: their words are compared with the numbers written here, not with the reference"""
    hand = list(TC.NANO_EDGES) + [b"0000-01-01T00:00:00Z", b"9999-12-31T23:59:59.999999999-23:59", b"1969-12-31T23:59:59.5Z"]
    case = TC.make_case("by hand", [(0, "ns"), (0, "us"), (0, "s")], [hand], pad=0)
    data, _, results = run_sim(lib, case, 64)
    ns, us, sec = data[TC.FRONT:TC.FRONT + 21].reshape(3, 7).tolist()
    assert ns == [TC.INT64_MAX, 0, TC.INT64_MIN & TC.MASK, 0, 0, 0, (-500000000) & TC.MASK]
    assert us[4:] == [(-62167219200000000) & TC.MASK, (253402300799 + 86340) * 1000000 + 999999, (-500000) & TC.MASK] and sec[6] == TC.MASK
    assert results.reshape(3, 6).tolist() == [[7, 3, 0, 0, 4, 0], [7, 7, 0, 0, 0, 5], [7, 7, 0, 0, 0, 6]]
    v = lambda text, unit, naive=False: TC.string_value(text, unit, naive)
    assert TC.days_from_civil(1970, 1, 1) == 0 and TC.days_from_civil(1969, 12, 31) == -1 and TC.days_from_civil(2000, 3, 1) == 11017
    assert TC.days_from_civil(0, 1, 1) == -719528 and TC.days_from_civil(9999, 12, 31) == 2932896
    assert v(b"2015-01-01T15:00:00Z", "s") == (1420124400, True, False) and v(b"2015-01-01T15:00:00Z", "us") == (1420124400000000, True, False)
    assert v(b"1970-01-01T00:00:00Z", "ns") == (0, True, False)
    assert v(b"1969-12-31T23:59:59.5Z", "s") == (-1, True, True) and v(b"1969-12-31T23:59:59.5Z", "ms") == (-500, True, False)
    assert v(b"1969-12-31T23:59:59.999999999Z", "us") == (-1, True, True) and v(b"1969-12-31T23:59:59.999999999Z", "ns") == (-1, True, False)
    assert v(b"2015-01-01T15:00:00.125000Z", "ms") == (1420124400125, True, False) and v(b"2015-01-01T15:00:00.1259Z", "ms") == (1420124400125, True, True)
    assert v(b"2015-01-01T15:00:00+00:01", "s")[0] == 1420124400 - 60 and v(b"2015-01-01T15:00:00-23:59", "s")[0] == 1420124400 + 86340
    assert v(b"2015-01-01T15:00:00-00:00", "s")[0] == 1420124400 and v(b"2015-01-01t15:00:00z", "s")[0] == 1420124400 == v(b"2015-01-01 15:00:00Z", "s")[0]
    # the four edges of NANO, and the widest MICRO values
    assert v(TC.NANO_EDGES[0], "ns") == (TC.INT64_MAX, True, False) and v(TC.NANO_EDGES[1], "ns") == (TC.INT64_MAX + 1, False, False)
    assert v(TC.NANO_EDGES[2], "ns") == (TC.INT64_MIN, True, False) and v(TC.NANO_EDGES[3], "ns") == (TC.INT64_MIN - 1, False, False)
    assert v(TC.NANO_EDGES[1], "us")[1] and v(TC.NANO_EDGES[3], "us") == ((TC.INT64_MIN - 1) // 1000, True, True)
    assert v(b"0000-01-01T00:00:00Z", "us") == (-62167219200000000, True, False)
    assert v(b"9999-12-31T23:59:59.999999999-23:59", "us") == ((253402300799 + 86340) * 1000000 + 999999, True, True)
    # the calendar and the shapes
    valid = lambda text, naive=False: v(text, "s", naive) is not None
    assert [valid(b"%04d-02-29T00:00:00Z" % y) for y in (1900, 2000, 2023, 2024, 0, 2100)] == [False, True, False, True, True, False]
    assert not valid(b"2015-01-00T00:00:00Z") and not valid(b"2015-01-32T00:00:00Z") and not valid(b"2015-04-31T00:00:00Z") and valid(b"2015-04-30T00:00:00Z")
    assert not valid(b"2015-00-10T00:00:00Z") and not valid(b"2015-13-10T00:00:00Z") and not valid(b"2015-01-01T24:00:00Z")
    assert not valid(b"2015-01-01T23:60:00Z") and not valid(b"2015-01-01T23:59:60Z") and valid(b"2015-01-01T23:59:59Z")
    assert not valid(b"2015-01-01T00:00:00+24:00") and not valid(b"2015-01-01T00:00:00+00:60") and valid(b"2015-01-01T00:00:00+23:59")
    assert not valid(b"2015-01-01T15:00:0Z") and not valid(b"2015-01-01T15:00:00") and valid(b"2015-01-01T15:00:00", True) and valid(TC.CANONICAL)
    assert len(TC.CANONICAL) == 35 and not valid(TC.CANONICAL + b"0") and not valid(b"2015-01-01T15:00:00.1234567890Z") and not valid(b"2015-01-01T15:00:00.Z")
    assert not valid(b"2015-01-01T15:00:00Z ") and not valid(b"+2015-01-01T15:00:00Z") and not valid(b"2015-01-01") and not valid(b"2015-01-01", True)
    assert not valid(b"2015-01-01T15:00:00.5") and valid(b"2015-01-01T15:00:00.5", True) and not valid(b"2015-01-01T15:00:00.", True)
    # a cell: the value word only behind '"', the counts
    sb = np.frombuffer(b"xx2015-01-01T15:00:00Zyy", dtype=np.uint8)
    assert TC.cell("s", (), TC.STRING, (20 << 32) | 2, sb) == (1420124400, True, False, False, False, False)
    assert TC.cell("s", (), TC.STRING, (21 << 32) | 2, sb) == (0, False, False, True, False, False)
    assert TC.cell("s", (), TC.LONG, 1420124400, sb) == (0, False, True, False, False, False) and TC.cell("s", (), TC.NULL, 7, sb) == (0,) + (False,) * 5
    assert TC.cell("ns", (), TC.STRING, 30 << 32, np.frombuffer(TC.NANO_EDGES[1], dtype=np.uint8)) == (0, False, False, False, True, False)


def test_the_reference_agrees_with_datetime(lib):
    """every VALID string of year >= 1 among the named, the replaced and the fuzz seeds' strings, at every unit -- the reference's
    value and the word the passes give are both compared with datetime arithmetic"""
    texts = list(TC.NAMED) + TC.replaced_strings()
    for seed in list(TC.FUZZ_SEEDS)[:60]:
        rng = np.random.default_rng(seed)
        texts += [c for c in TC.random_cells(rng, 40) if isinstance(c, bytes)]
    case = TC.make_case("against datetime", [(0, unit, "naive_utc") for unit in TC.UNITS], [texts], pad=0)
    words = run_sim(lib, case, lib.sim_timecol_chunk_rows())[0][TC.FRONT:TC.FRONT + 4 * len(texts)].reshape(4, len(texts)).tolist()
    checked = 0
    for r, text in enumerate(texts):
        for f, unit in enumerate(TC.UNITS):
            got = TC.string_value(text, unit, True)
            if got is not None and int(text[:4]) >= 1:
                assert got[0] == TC.datetime_value(text, unit), (text, unit)
                assert words[f][r] == (got[0] & TC.MASK if got[1] else 0), (text, unit)
                checked += 1
    assert checked > 4000
    epoch = datetime.datetime(1970, 1, 1, tzinfo=datetime.timezone.utc)
    assert (datetime.datetime.fromisoformat("2015-01-01T15:00:00+05:30") - epoch).total_seconds() == TC.string_value(b"2015-01-01T15:00:00+05:30", "s", False)[0]


# ---------------------------------------------------------------------------------------------------------------------
# the passes against the reference
# ---------------------------------------------------------------------------------------------------------------------
@CHUNKS
def test_named_strings(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    case = TC.named_case()
    ref = check_all(lib, case, R)
    rec = dict(zip(case.fields, ref.records))
    n = len(TC.NAMED)
    assert all(r[0] == n and r[2] == 0 and r[1] + r[3] + r[4] == n for r in ref.records)
    # at NANO the two edges past int64, the four strings of year 0000, 0001-01-01 and 9999-12-31 are range errors: nowhere else
    assert rec[(0, "ns")][4] == 8 and all(r[4] == (8 if f[1] == "ns" else 0) for f, r in rec.items())
    assert rec[(0, "s", "naive_utc")][1] > rec[(0, "s")][1] > 40 and rec[(0, "s")][5] > rec[(0, "ms")][5] > rec[(0, "us")][5] > rec[(0, "ns")][5] == 0


@CHUNKS
def test_every_position_replaced(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    case = TC.replaced_case()
    ref = check_all(lib, case, R, forms=FORMS[:2])
    # VALID: ':' where the grammar wants it (13, 16, 32) -- nothing else of the 105
    assert ref.records[0] == (105, 3, 0, 102, 0, 0) and ref.records[1] == (105, 3, 0, 102, 0, 3)


@CHUNKS
def test_every_type_under_the_field(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    case = TC.type_table_case()
    ref = check_all(lib, case, R)
    n = case.n_rows
    assert ref.records[0] == (n, 2, n - 5, 1, 0, 1) and ref.records[4] == (n, 2, n - 5, 1, 0, 0)  # MISSING and 'n' are counted nowhere


@CHUNKS
def test_the_last_bytes_of_the_string_buffer(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    for case in TC.last_bytes_case():
        ref = check_all(lib, case, R, forms=FORMS[:1])
        assert ref.records[1][1] >= 3 and ref.records[1][3] >= 7, ref.records


@CHUNKS
def test_row_counts_and_live_counts(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    valid = 0
    for n in sorted(set(TC.ROW_COUNTS) | {R - 1, R, R + 1, 2 * R + 1}):
        for case in TC.row_count_cases(n):
            valid += sum(r[1] for r in check_all(lib, case, R, forms=(FORMS[0], FORMS[3]) if n > 300 else FORMS, shift=n % 16).records)
    assert valid > 5000


@CHUNKS
def test_the_types_at_every_shift(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    case = TC.type_shift_case()
    for shift in range(16):
        TC.check("shift %d" % shift, *run_sim(lib, case, R, type_shift=shift, words=shift % 2), case, reference(case))


@CHUNKS
def test_schemas(lib, chunk):
    R = chunk or lib.sim_timecol_chunk_rows()
    for case in TC.schema_cases():
        ref = check_all(lib, case, R, forms=(FORMS[0], FORMS[2]))
        assert any(0 < r[1] < r[0] for r in ref.records), case.name


def test_fuzz(lib):
    """200 seeded cases at every chunk size and both fetch forms.  The generator's condition is asserted from the REFERENCE's
    counts alone: at least a quarter of all fields each have a VALID, a malformed, an other-typed and a MISSING / null row"""
    R = lib.sim_timecol_chunk_rows()
    fields = full = ranged = inexact = 0
    for seed in TC.FUZZ_SEEDS:
        case = TC.fuzz_case(seed)
        ref = TC.reference(case)
        fields += len(ref.records)
        full += sum(r[1] > 0 and r[3] > 0 and r[2] > 0 and r[0] - r[1] - r[2] - r[3] - r[4] > 0 for r in ref.records)
        ranged += sum(r[4] > 0 for r in ref.records)
        inexact += sum(r[5] > 0 for r in ref.records)
        for k, chunk in enumerate(sorted({64, 128, 1024, R})):
            data, validity = FORMS[(seed + k) % 4] if seed % 4 == 0 else FORMS[0]
            got = run_sim(lib, case, chunk, data, validity, type_shift=(seed + k) % 16, words=(seed + k) % 2)
            TC.check("%s, chunk %d, data %s, validity %s" % (case.name, chunk, data, validity), *got, case, ref)
    print("fuzz: %d fields, %d with all four kinds of row, %d with a range error, %d with an inexact value" % (fields, full, ranged, inexact))
    assert 4 * full >= fields and ranged >= 20 and inexact >= 100, (fields, full, ranged, inexact)


def test_argument_errors(lib):
    case = TC.row_count_cases(65)[0]
    assert len(case.fields) == 4
    bad_field = lambda **kw: np.array([tuple(dict(dict(column=0, unit=2, flags=0, reserved=0), **kw).values())], dtype=TC.FIELD)
    one = case._replace(fields=[(0, "us")])
    run_sim(lib, case, 100, expect=-2)                                                     # a chunk that is no multiple of 64
    run_sim(lib, case, 192, expect=-2)                                                     # ... or none the simulation has
    run_sim(lib, case, 64, fields=np.zeros(0, dtype=TC.FIELD), expect=-2)                  # no field
    run_sim(lib, case._replace(fields=[(0, "s")] * 65), 64, expect=-2)                     # more than 64
    for f in (dict(unit=4), dict(unit=1 << 31), dict(flags=2), dict(flags=3), dict(reserved=1), dict(column=3)):
        run_sim(lib, one, 64, fields=bad_field(**f), expect=-2)
    run_sim(lib, one, 64, fields=bad_field(flags=1, unit=3))                               # (legal: NAIVE_UTC at NANO)
    run_sim(lib, case, 64, col_stride=64, readable=0, expect=-2)                           # col_stride < n_rows
    run_sim(lib, case, 64, data_stride=64, expect=-2)                                      # data_stride < n_rows
    run_sim(lib, case, 64, data=False, data_stride=65, expect=-2)                          # a stride without d_data
    run_sim(lib, case, 64, validity_stride=1, expect=-2)                                   # validity_stride < ceil(n_rows / 64)
    run_sim(lib, case, 64, results=None, expect=-2)
    run_sim(lib, case, 64, sb=None, expect=-2)                                             # no string buffer with rows


def test_the_layout_is_arrows(lib):
    """pyarrow.Array.from_buffers(timestamp(unit, tz="UTC")) over the reference's buffers -- which are the passes', word for word --
    for each unit: to_pylist() gives the datetime objects of the strings that both can represent (datetime: years 1..9999,
    microseconds)"""
    pa = pytest.importorskip("pyarrow")
    utc = datetime.timezone.utc
    texts = [b"2015-01-01T15:00:00Z", b"1969-12-31T23:59:59.5Z", b"not a time", b"2015-01-01T15:00:00.125+05:30", b"0001-01-01T00:00:00Z",
             b"9999-12-31T23:59:59.999999Z", b"2024-02-29 12:34:56.789012-08:00", b"1677-09-21T00:12:43.145225Z", b"2262-04-11T23:47:16.854775Z"]
    want = [datetime.datetime(2015, 1, 1, 15, tzinfo=utc), datetime.datetime(1969, 12, 31, 23, 59, 59, 500000, tzinfo=utc), None,
            datetime.datetime(2015, 1, 1, 9, 30, 0, 125000, tzinfo=utc), datetime.datetime(1, 1, 1, tzinfo=utc),
            datetime.datetime(9999, 12, 31, 23, 59, 59, 999999, tzinfo=utc), datetime.datetime(2024, 2, 29, 20, 34, 56, 789012, tzinfo=utc),
            datetime.datetime(1677, 9, 21, 0, 12, 43, 145225, tzinfo=utc), datetime.datetime(2262, 4, 11, 23, 47, 16, 854775, tzinfo=utc)]
    rows = 70  # (a second word of the bitmap)
    cells = [texts[k % 9] if k % 10 != 9 else (TC.NULL, 0) for k in range(rows)]
    expect = [want[k % 9] if k % 10 != 9 else None for k in range(rows)]
    case = TC.make_case("pyarrow", [(0, u) for u in TC.UNITS], [cells])
    ref = TC.reference(case)
    TC.check("pyarrow", *run_sim(lib, case, 64), case, ref)
    for f, unit in enumerate(TC.UNITS):
        buffers = [pa.py_buffer(np.array(ref.validity[f], dtype="<u8").tobytes()), pa.py_buffer(np.array(ref.data[f], dtype="<u8").tobytes())]
        got = pa.Array.from_buffers(pa.timestamp(unit, tz="UTC"), rows, buffers, null_count=rows - ref.records[f][1])
        got.validate(full=True)
        drop = {"s": 1000000, "ms": 1000, "us": 1, "ns": 1}[unit]
        cut = lambda d: d.replace(microsecond=d.microsecond // drop * drop)
        in_unit = lambda k: unit != "ns" or texts[k % 9][:4] not in (b"0001", b"9999")  # (NANO: a range error, NULL)
        assert got.to_pylist() == [cut(e) if e is not None and in_unit(k) else None for k, e in enumerate(expect)], (unit, got)
