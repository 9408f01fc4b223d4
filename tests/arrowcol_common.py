"""What the Arrow column export must give (include/sjmi.h, sjmi_arrow_columns_device), in Python alone: shares no code with the
product.  reference() works cell by cell on Python int / float objects -- float(int) is correctly rounded (to nearest, ties to
even) and int(float(v)) != v is an exact comparison of integers; numpy's casts are not to be trusted at 2^63.  check() compares
everything a call owns word for word and, against CANARY-filled buffers, everything it must not touch (both are
tests/fieldcol_common.py's, with the live rows and the stride rule of a case).  The *_cases() generators
are seeded -- a name is a case -- and shared by the host simulation's tests (tests/test_host_arrowcol.py) and the GPU tests
(tests/test_gpu_arrowcol.py).  A field is the tuple of binding.arrow_fields: (column, kind[, "integral_doubles"])."""
import math
import struct
from collections import namedtuple

import numpy as np

from tests import fieldcol_common as F
from tests.fieldcol_common import (ALL_TYPES, BACK, CANARY_WORD, DOUBLE, FALSE, FRONT, INT64_MAX, INT64_MIN, LONG, MASK, MISSING, NULL, STRING, TRUE,
                                   check, live_counts, live_rows, pack_bits)
from tests.strcol_common import WILD

KINDS = {"int64": 1, "float64": 2, "bool": 3}           # SJMI_ARROW_<KIND>
FLAGS = {"integral_doubles": 1}                         # SJMI_ARROW_F_*
FIELD = np.dtype([("column", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])  # sjmi_arrow_field
RECORD_WORDS = 4                                        # n_rows, n_valid, n_other, n_inexact

# types uint8 / values uint64 [n_cols, col_stride], n_rows <= col_stride; row_count None or what *d_row_count holds;
# data_stride >= n_rows, validity_stride >= ceil(n_rows / 64)
Case = namedtuple("Case", "name fields types values n_rows row_count data_stride validity_stride")
Ref = namedtuple("Ref", "live data validity records")  # data / validity: per field the words the call owns; records: per field 4 ints


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


def encode(fields):
    """tuples -> the sjmi_arrow_field array: the C form, for the host simulation"""
    return F.encode(fields, FIELD, KINDS, FLAGS)


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def cell(kind, flags, ty, word):
    """one cell under one field -> (data word, valid, other, inexact); word is read only behind 'l' / 'd'"""
    ty = int(ty)
    data, valid, inexact = 0, False, False
    if kind == "bool":
        valid, data = ty in (TRUE, FALSE), int(ty == TRUE)
    elif ty == LONG:
        v = int(word)
        v = v - (1 << 64) if v >> 63 else v
        valid = True
        if kind == "int64":
            data = v & MASK
        else:
            x = float(v)                # correctly rounded: to nearest, ties to even
            data, inexact = bits_of(x), int(x) != v
    elif ty == DOUBLE:
        if kind == "float64":
            data, valid = int(word), True
        elif "integral_doubles" in flags:
            x = double_of(word)
            if math.isfinite(x) and x == math.floor(x) and INT64_MIN <= int(x) <= INT64_MAX:
                data, valid = int(x) & MASK, True
    return data, valid, (not valid) and ty not in (MISSING, NULL), inexact


def reference_cells(fields, get, live):
    """get(column, row) -> (type byte, value word or anything for a cell that is neither 'l' nor 'd') -> Ref"""
    data, validity, records = [], [], []
    for field in fields:
        column, kind, flags = field[0], field[1], field[2:]
        cells = [cell(kind, flags, *get(column, r)) for r in range(live)]
        words = [c[0] for c in cells]
        data.append(pack_bits(words) if kind == "bool" else words)
        validity.append(pack_bits([c[1] for c in cells]))
        records.append((live, sum(c[1] for c in cells), sum(c[2] for c in cells), sum(c[3] for c in cells)))
    return Ref(live, data, validity, records)


def reference(case):
    t, v = case.types.tolist(), case.values.tolist()
    return reference_cells(case.fields, lambda c, r: (t[c][r], v[c][r]), live_rows(case))


def reference_from_cells(fields, want, live):
    """the same from the cells of tests/select_common.expected_columns / explode_common.expected_explode: want[column][row] =
    (type byte, payload), the payload of a number its value word (a string's is its bytes: never looked at)"""
    return reference_cells(fields, lambda c, r: want[c][r], live)


def out_buffers(case, data=True, validity=True):
    return F.out_buffers(case, RECORD_WORDS, data, validity)


# ---------------------------------------------------------------------------------------------------------------------
# builders of synthetic column sets
# ---------------------------------------------------------------------------------------------------------------------
EDGE_LONGS = [INT64_MIN, INT64_MAX, 1 << 53, -(1 << 53), (1 << 53) + 1, (1 << 53) - 1, -(1 << 53) + 1, -(1 << 53) - 1, (1 << 53) + 3,
              (1 << 62) + (1 << 9), (1 << 62) + (1 << 10), 0, 1, -1]
EDGE_DOUBLES = [-0.0, 2.0 ** 63, -2.0 ** 63, math.nextafter(2.0 ** 63, 0.0), math.inf, -math.inf, math.nan, 0.5, 1e300, 5e-324, 0.0, 1.0, -7.0, 2.0 ** 53]
LONGS = EDGE_LONGS + [5, 1000, -123456789] + [w - (1 << 64) if w >> 63 else w for w in WILD]
DOUBLES = EDGE_DOUBLES + [5.0, 1000.0, -1.5, 1e19, -1e19, 4503599627370497.0, 3.0e9]
DEFAULT_POOL = ALL_TYPES + [LONG, DOUBLE] * 3 + [TRUE, FALSE]


def columns(rng, n_cols, n_rows, stride, pool=None):
    """random cells of every type: numbers from LONGS / DOUBLES, every other cell -- the booleans among them -- with a WILD value
    word, and so the cells between n_rows and the stride, whatever their type -> (types, values) [n_cols, stride]"""
    pool = np.array(DEFAULT_POOL if pool is None else pool, dtype=np.uint8)
    t = pool[rng.integers(0, pool.size, size=(n_cols, stride))]
    v = np.array(WILD, dtype=np.uint64)[rng.integers(0, len(WILD), size=(n_cols, stride))]
    longs = np.array([x & MASK for x in LONGS], dtype=np.uint64)[rng.integers(0, len(LONGS), size=(n_cols, stride))]
    doubles = np.array([bits_of(x) for x in DOUBLES], dtype=np.uint64)[rng.integers(0, len(DOUBLES), size=(n_cols, stride))]
    live = np.arange(stride)[None, :] < n_rows
    v = np.where(live & (t == LONG), longs, v)
    v = np.where(live & (t == DOUBLE), doubles, v)
    return t, v


def make_case(name, fields, t, v, n_rows, row_count=None, slack=0):
    """slack: how far the output strides lie above their minimum (0: the minimum)"""
    return Case(name, list(fields), np.ascontiguousarray(t, dtype=np.uint8), np.ascontiguousarray(v, dtype=np.uint64), n_rows, row_count,
                *F.strides(n_rows, slack))


def one_column(cells, pad=3):
    """[(type byte, value word)] -> one column with `pad` cells of stride behind it"""
    t = np.array([c[0] for c in cells] + [LONG] * pad, dtype=np.uint8)[None, :]
    v = np.array([c[1] & MASK for c in cells] + [WILD[3]] * pad, dtype=np.uint64)[None, :]
    return t, v


ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 1023, 1024, 1025, 2049)
MIXED_FIELDS = [(0, "int64", "integral_doubles"), (1, "float64"), (2, "bool"), (1, "int64")]


def row_count_cases(n):
    rng = np.random.default_rng(1000 + n)
    t, v = columns(rng, 3, n, n + 7)
    return [make_case("%d rows, row count %s, strides %s" % (n, rc, "above the minimum" if k % 2 else "at the minimum"), MIXED_FIELDS, t, v, n, rc, k % 2)
            for k, rc in enumerate(live_counts(n))]


def kind_table_case():
    """every kind on a cell of every type: one column with cells of all nine types, several numbers among them, every value word
    that must not matter WILD -- those of the 't' / 'f' cells included"""
    cells = [(ty, WILD[k % len(WILD)]) for k, ty in enumerate(ALL_TYPES) if ty not in (LONG, DOUBLE)]
    cells += [(TRUE, WILD[1]), (FALSE, WILD[0]), (TRUE, 0), (FALSE, 1)]
    cells += [(LONG, x) for x in (0, 5, -7, (1 << 60) + 1)] + [(DOUBLE, bits_of(x)) for x in (0.0, 5.0, 5.5, -7.0, math.inf)]
    t, v = one_column(cells)
    fields = [(0, "int64"), (0, "int64", "integral_doubles"), (0, "float64"), (0, "bool")]
    return make_case("every kind on every type", fields, t, v, len(cells), None, 1)


def numeric_edge_case():
    """the integer edges in column 0 and the double edges in column 1, each under INT64 with and without the flag and under
    FLOAT64"""
    n = max(len(EDGE_LONGS), len(EDGE_DOUBLES))
    t = np.zeros((2, n + 2), dtype=np.uint8)
    v = np.full((2, n + 2), WILD[0], dtype=np.uint64)
    t[0, :len(EDGE_LONGS)], v[0, :len(EDGE_LONGS)] = LONG, [x & MASK for x in EDGE_LONGS]
    t[1, :len(EDGE_DOUBLES)], v[1, :len(EDGE_DOUBLES)] = DOUBLE, [bits_of(x) for x in EDGE_DOUBLES]
    fields = [(c, kind) + flag for c in (0, 1) for kind, flag in (("int64", ()), ("int64", ("integral_doubles",)), ("float64", ()))]
    return make_case("numeric edges", fields, t, v, n, None, 0)


def schema_cases():
    """1 field and 64 fields, one column under three kinds, fields in descending column order"""
    rng = np.random.default_rng(4000)
    n = 150
    t, v = columns(rng, 5, n, n + 11)
    kinds = [("int64",), ("float64",), ("bool",), ("int64", "integral_doubles")]
    return [make_case("one field", [(4, "float64")], t, v, n, None, 0),
            make_case("64 fields", [((7 * k) % 5,) + kinds[k % 4] for k in range(64)], t, v, n, None, 1),
            make_case("one column under three kinds", [(2, "int64"), (2, "float64"), (2, "bool")], t, v, n, n - 3, 0),
            make_case("descending columns", [(c,) + kinds[c % 4] for c in (4, 3, 2, 1, 0)], t, v, n, None, 1)]


def type_shift_case():
    rng = np.random.default_rng(4100)
    t, v = columns(rng, 3, 200, 203)
    return make_case("type shifts", MIXED_FIELDS, t, v, 200, 197, 0)


def fuzz_case(seed, max_rows=300):
    """random mixed-type columns under a random schema of 1 to 8 fields; one case in two takes its rows from a row count"""
    rng = np.random.default_rng(seed)
    n_cols, n = int(rng.integers(1, 7)), int(rng.integers(1, max_rows + 1))
    pools = [DEFAULT_POOL, [LONG] * 6 + [DOUBLE, NULL, MISSING], [DOUBLE] * 6 + [LONG, NULL], [TRUE, FALSE, NULL, MISSING, STRING], [LONG, DOUBLE]]
    t, v = columns(rng, n_cols, n, n + int(rng.integers(0, 8)), pool=pools[int(rng.integers(0, len(pools)))])
    kinds = [("int64",), ("int64", "integral_doubles"), ("float64",), ("float64",), ("bool",)]
    fields = [(int(rng.integers(0, n_cols)),) + kinds[int(rng.integers(0, len(kinds)))] for _ in range(int(rng.integers(1, 9)))]
    rc = int(rng.integers(0, n + 4)) if seed % 2 else None
    return make_case("fuzz case %d (%d columns, %d rows, %d fields, row count %s)" % (seed, n_cols, n, len(fields), rc), fields, t, v, n, rc, seed % 3 == 0)


FUZZ_SEEDS = range(5000, 5200)


def past_one_grid_trip_case():
    """3 fields x 70,001 rows: 69 chunks per field"""
    n = 70001
    rng = np.random.default_rng(31)
    t, v = columns(rng, 3, n, n + 3)
    return make_case("%d rows" % n, [(0, "int64", "integral_doubles"), (1, "float64"), (2, "bool")], t, v, n, None, 0)
