"""What filtering the rows of typed columns must give (include/sjmi.h, sjmi_filter_columns_device), in Python and numpy alone:
shares no code with the product.  reference() decides every term on Python int / float / bytes objects, whose mixed comparison
is exact (numpy would convert an int64 to float64 first); reference_same_kind() is the vectorised form for terms that compare
like with like only.  check() compares everything a call wrote -- and that it wrote nothing else --, the builders make column
sets whose cells that are neither strings nor numbers carry value words that would be wild offsets, and the *_cases()
generators are the cases of the issue, shared by the host simulation's tests (tests/test_host_filter.py) and the GPU tests
(tests/test_gpu_filter.py).  A term is the tuple of binding.FilterPlan: (column, "<kind>_<cmp>", constant)."""
import math
import operator
import struct
from collections import namedtuple

import numpy as np

from tests.strcol_common import WILD

STRING, LONG, DOUBLE, MISSING = ord('"'), ord("l"), ord("d"), 0
ALL_TYPES = [MISSING] + [ord(c) for c in 'ntfld"[{']
OVERFLOW = 1                                           # SJMI_FILTER_OVERFLOW
CANARY = 0xC5
CANARY_WORD = 0xC5C5C5C5C5C5C5C5
CANARY_ENTRIES = 4
CANARY_BYTES = 37
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
KINDS = {"type": 0, "long": 1, "double": 2, "string": 3}                               # SJMI_F_<KIND>_<CMP> = kind << 4 | cmp
CMPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5, "prefix": 6}
NUM_CMPS = {"eq": operator.eq, "ne": operator.ne, "lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge}
ALL_OPS = ["type_eq", "type_ne"] + ["%s_%s" % (k, c) for k in ("long", "double") for c in NUM_CMPS] + ["string_eq", "string_ne", "string_prefix"]
TERM = np.dtype([("column", "<u4"), ("op", "<u4"), ("operand", "<u8")])                # sjmi_filter_term

Case = namedtuple("Case", "name terms types values n_rows sb")  # types uint8 / values uint64 [n_cols, col_stride], n_rows <= col_stride


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


def encode(terms):
    """tuples -> (sjmi_filter_term array, the constants' bytes): the C form, for the host simulation"""
    enc = np.zeros(len(terms), dtype=TERM)
    blob = b""
    for k, (column, op, const) in enumerate(terms):
        kind, cmp = op.split("_")
        if kind == "type":
            operand = int(const)
        elif kind == "long":
            operand = int(const) & 0xFFFFFFFFFFFFFFFF
        elif kind == "double":
            operand = bits_of(float(const))
        else:
            operand = (len(const) << 32) | len(blob)
            blob += bytes(const)
        enc[k] = (column, (KINDS[kind] << 4) | CMPS[cmp], operand)
    return enc, blob


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def cell_object(ty, value, sb):
    """the cell as a Python object: an int, a float, bytes, or None for a cell of another type"""
    value = int(value)
    if ty == LONG:
        return value - (1 << 64) if value >> 63 else value
    if ty == DOUBLE:
        return double_of(value)
    if ty == STRING:
        off, ln = value & 0xFFFFFFFF, value >> 32
        assert off + ln <= len(sb)
        return bytes(sb[off:off + ln])
    return None


def term_holds(term, ty, obj):
    """one term on a cell of type ty whose Python object is obj (an int, a float or bytes; anything for another type)"""
    _, op, const = term
    kind, cmp = op.split("_")
    ty = int(ty)
    if kind == "type":
        return (ty == int(const)) == (cmp == "eq")
    if kind == "string":
        if ty != STRING:
            return False
        return obj == bytes(const) if cmp == "eq" else obj != bytes(const) if cmp == "ne" else obj.startswith(bytes(const))
    if ty not in (LONG, DOUBLE):
        return False
    const = int(const) if kind == "long" else float(const)
    return bool(NUM_CMPS[cmp](obj, const))  # (Python compares an int with a float exactly)


def term_true(term, ty, value, sb):
    return term_holds(term, ty, cell_object(int(ty), value, sb))


def reference_from_cells(terms, want, n_rows=None):
    """the same from the cells of tests/select_common.expected_columns / explode_common.expected_explode: want[column][row] =
    (type byte, payload), the payload of a string its bytes, else the value word -> keep, bool [n_rows]"""
    n_rows = len(want[0]) if n_rows is None else n_rows
    obj = lambda t, p: p if t == STRING else cell_object(t, p, b"")
    return np.array([all(term_holds(term, want[term[0]][r][0], obj(*want[term[0]][r])) for term in terms) for r in range(n_rows)], dtype=bool).reshape(n_rows)


def reference(case):
    """-> keep, bool [n_rows]: row r is kept iff every term is true on it"""
    keep = np.ones(case.n_rows, dtype=bool)
    for term in case.terms:
        t, v = case.types[term[0]], case.values[term[0]]
        for r in np.flatnonzero(keep):
            keep[r] = term_true(term, t[r], v[r], case.sb)
    return keep


def reference_same_kind(case):
    """the same in numpy, for LONG terms whose constant a double holds exactly: an 'l' cell compares int64 with int64, a 'd' cell
    float64 with float64 -- like with like, so nothing is rounded on the way"""
    keep = np.ones(case.n_rows, dtype=bool)
    for column, op, const in case.terms:
        kind, cmp = op.split("_")
        assert kind == "long" and abs(const) <= 1 << 53 and int(float(const)) == const
        t, v = case.types[column, :case.n_rows], case.values[column, :case.n_rows]
        as_long = NUM_CMPS[cmp](v.view(np.int64), np.int64(const))
        as_double = NUM_CMPS[cmp](v.view(np.float64), np.float64(const))
        keep &= np.where(t == LONG, as_long, (t == DOUBLE) & as_double)
    return keep


def words_of(keep):
    bits = np.zeros((keep.size + 63) // 64 * 64, dtype=np.uint8)
    bits[:keep.size] = keep
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def out_buffers(n_rows, n_cols, capacity, keep=True, outs=True):
    """the output arrays of one call, canaries all over: (keep words or None, rows or None, out_types or None, out_values or
    None, result uint64 [2]); the columns flat, column c at c * capacity"""
    assert outs or not capacity
    words = np.full((n_rows + 63) // 64 + CANARY_ENTRIES, CANARY_WORD, dtype=np.uint64) if keep else None
    rows = np.full(capacity + CANARY_ENTRIES, CANARY_WORD, dtype=np.uint64) if outs else None
    otypes = np.full(n_cols * capacity + CANARY_BYTES, CANARY, dtype=np.uint8) if outs else None
    ovalues = np.full(n_cols * capacity + CANARY_ENTRIES, CANARY_WORD, dtype=np.uint64) if outs else None
    return words, rows, otypes, ovalues, np.full(2, CANARY_WORD, dtype=np.uint64)


def check(what, got_words, got_rows, got_types, got_values, got_result, case, keep, capacity, canaries=True):
    """got_*: what a call left in out_buffers() (None: called without it); keep = reference(case).  canaries=False: the arrays
    end where their contents end and were not filled with canaries (tensors a wrapper allocated exactly)."""
    n_cols = case.types.shape[0]
    want_rows = np.flatnonzero(keep).astype(np.int64)
    n_kept = want_rows.size
    m = min(n_kept, capacity)
    r = np.asarray(got_result).view(np.uint64)
    got = (int(r[0]), int(r[1]) & 0xFFFFFFFF, int(r[1]) >> 32)
    assert got == (n_kept, OVERFLOW if n_kept > capacity else 0, 0), (what, got, n_kept, capacity)
    if got_words is not None:
        want = words_of(keep)
        got_words = np.asarray(got_words).view(np.uint64)
        assert np.array_equal(got_words[:want.size], want), "%s: keep differs first in word %d" % (what, int(np.flatnonzero(got_words[:want.size] != want)[0]))
        if canaries:
            assert got_words.size == want.size + CANARY_ENTRIES and np.all(got_words[want.size:] == CANARY_WORD), "%s: written behind the last keep word" % what
    if got_rows is None:
        return
    got_rows = np.asarray(got_rows).view(np.uint64)
    got_types = np.asarray(got_types, dtype=np.uint8).reshape(-1)
    got_values = np.asarray(got_values).view(np.uint64).reshape(-1)
    assert np.array_equal(got_rows[:m].view(np.int64), want_rows[:m]), "%s: rows differ first at %d" % (what, int(np.flatnonzero(got_rows[:m].view(np.int64) != want_rows[:m])[0]))
    for c in range(n_cols):
        at = c * capacity
        assert np.array_equal(got_types[at:at + m], case.types[c][want_rows[:m]]), "%s: the types of column %d differ" % (what, c)
        assert np.array_equal(got_values[at:at + m], case.values[c][want_rows[:m]]), "%s: the values of column %d differ" % (what, c)
    if canaries:
        assert got_rows.size == capacity + CANARY_ENTRIES and np.all(got_rows[m:] == CANARY_WORD), "%s: rows written behind n_kept or the capacity" % what
        assert got_types.size == n_cols * capacity + CANARY_BYTES and got_values.size == n_cols * capacity + CANARY_ENTRIES
        for c in range(n_cols):  # entries between n_kept and the capacity stay as they were: behind each column's last entry
            assert np.all(got_types[c * capacity + m:(c + 1) * capacity] == CANARY), "%s: types of column %d written behind its last entry" % (what, c)
            assert np.all(got_values[c * capacity + m:(c + 1) * capacity] == CANARY_WORD), "%s: values of column %d written behind its last entry" % (what, c)
        assert np.all(got_types[n_cols * capacity:] == CANARY) and np.all(got_values[n_cols * capacity:] == CANARY_WORD), "%s: written behind the columns" % what


def capacities(n_kept):
    """the capacities of the issue: n_kept + 3, n_kept, n_kept - 1, half, 1 and the sizing call"""
    return sorted({n_kept + 3, n_kept, max(n_kept - 1, 0), n_kept // 2, 1, 0}, reverse=True)


# ---------------------------------------------------------------------------------------------------------------------
# builders of synthetic column sets
# ---------------------------------------------------------------------------------------------------------------------
LONGS = [0, 1, -1, 5, 1000, 1 << 53, (1 << 53) + 1, (1 << 53) - 1, -(1 << 53) - 1, INT64_MIN, INT64_MAX] + [w - (1 << 64) if w >> 63 else w for w in WILD]
DOUBLES = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 5.0, 1000.0, 2.0 ** 53, 2.0 ** 63, -2.0 ** 63, math.inf, -math.inf, 1e19, -1e19]


def string_buffer(rng, size):
    """two letters only, so that short strings at random places are often equal or prefixes of each other"""
    return rng.integers(97, 99, size=size, dtype=np.uint8)


def columns(rng, n_cols, n_rows, stride, sb_size, max_len=3, types=None):
    """random cells of every type: strings at random places of the buffer, numbers from LONGS / DOUBLES, every other cell with a
    WILD value word (so do the cells between n_rows and the stride, whatever their type) -> (types, values) [n_cols, stride]"""
    pool = np.array(ALL_TYPES if types is None else types, dtype=np.uint8)
    t = pool[rng.integers(0, pool.size, size=(n_cols, stride))]
    v = np.array(WILD, dtype=np.uint64)[rng.integers(0, len(WILD), size=(n_cols, stride))]
    longs = np.array([x & 0xFFFFFFFFFFFFFFFF for x in LONGS], dtype=np.uint64)[rng.integers(0, len(LONGS), size=(n_cols, stride))]
    doubles = np.array([bits_of(x) for x in DOUBLES], dtype=np.uint64)[rng.integers(0, len(DOUBLES), size=(n_cols, stride))]
    lens = rng.integers(0, max_len + 1, size=(n_cols, stride)).astype(np.uint64)
    offs = rng.integers(0, sb_size - max_len + 1, size=(n_cols, stride)).astype(np.uint64)
    live = np.arange(stride)[None, :] < n_rows
    v = np.where(live & (t == LONG), longs, v)
    v = np.where(live & (t == DOUBLE), doubles, v)
    v = np.where(live & (t == STRING), (lens << np.uint64(32)) | offs, v)
    return t, v


def marked(rng, kept_rows, n_rows, n_cols=3, stride=None, sb_size=512):
    """a column set whose column 0 is 'l' with 1 in kept_rows and 0 elsewhere, and the term that keeps exactly those rows"""
    stride = n_rows + 5 if stride is None else stride
    t, v = columns(rng, n_cols, n_rows, stride, sb_size)
    t[0, :n_rows] = LONG
    v[0, :n_rows] = 0
    v[0, np.asarray(kept_rows, dtype=np.int64)] = 1
    return [(0, "long_eq", 1)], t, v


ROW_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)


def row_count_case(n):
    rng = np.random.default_rng(1000 + n)
    sb = string_buffer(rng, 512)
    t, v = columns(rng, 3, n, n + 7, sb.size)
    return Case("%d rows" % n, [(0, "type_ne", MISSING), (2, "long_ge", 0)], t, v, n, sb)


def keep_pattern_cases():
    """none, all, only the first row, only the last, every 64th, every 65th, bit 0 and bit 63 of every word -- at row counts that
    end inside a word, at a word's end and inside a second chunk of the kernels"""
    out = []
    for n in (64, 200, 1024, 2049):
        rng = np.random.default_rng(2000 + n)
        sb = string_buffer(rng, 512)
        for name, rows in (("none", []), ("all", range(n)), ("only the first row", [0]), ("only the last row", [n - 1]),
                           ("every 64th row", range(0, n, 64)), ("every 65th row", range(0, n, 65)),
                           ("bit 0 of each word", range(0, n, 64)), ("bit 63 of each word", range(63, n, 64)),
                           ("bits 0 and 63 of each word", sorted(set(range(0, n, 64)) | set(range(63, n, 64))))):
            terms, t, v = marked(rng, list(rows), n)
            out.append(Case("%s of %d" % (name, n), terms, t, v, n, sb))
    return out


def _one_column(cells, sb, pad=3):
    """[(type byte, value word)] -> one column with `pad` cells of stride behind it"""
    t = np.array([c[0] for c in cells] + [STRING] * pad, dtype=np.uint8)[None, :]
    v = np.array([c[1] & 0xFFFFFFFFFFFFFFFF for c in cells] + [WILD[3]] * pad, dtype=np.uint64)[None, :]
    return t, v


def op_table_cases():
    """every op against a cell of every type: one column with cells of all nine types (several numbers and strings among
    them), one plan per op and constant"""
    sb = np.frombuffer(b"abcabxab", dtype=np.uint8)
    cells = [(ty, WILD[k % len(WILD)]) for k, ty in enumerate(ALL_TYPES) if ty not in (LONG, DOUBLE, STRING)]
    cells += [(LONG, x) for x in (0, 5, -7, 97)] + [(DOUBLE, bits_of(x)) for x in (0.0, 5.0, 5.5, -7.0, math.inf)]
    cells += [(STRING, (ln << 32) | off) for off, ln in ((0, 3), (3, 3), (0, 2), (6, 2), (0, 0), (8, 0), (0, 1))]
    t, v = _one_column(cells, sb)
    consts = {"type": ALL_TYPES + [ord("x"), 255], "long": [5, -7, 6], "double": [5.0, 5.5, -7.0, -math.inf], "string": [b"ab", b"abc", b"", b"abx", b"b"]}
    return [Case("op table: %s %r" % (op, k), [(0, op, k)], t, v, len(cells), sb) for op in ALL_OPS for k in consts[op.split("_")[0]]]


NUMERIC_EDGE_LONGS = [INT64_MIN, INT64_MIN + 1, INT64_MAX, INT64_MAX - 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, -(1 << 53) - 1, -(1 << 53), 0, 1, -1]
NUMERIC_EDGE_DOUBLES = [2.0 ** 63, -2.0 ** 63, math.nextafter(2.0 ** 63, 0.0), math.nextafter(-2.0 ** 63, -math.inf), 2.0 ** 53, -2.0 ** 53, 0.0, -0.0,
                        0.5, -0.5, 1.0, -1.0, math.inf, -math.inf, 1e19, -1e19]


def numeric_edge_cases():
    """INT64_MIN / INT64_MAX and +-2^63 as doubles, 2^53 +- 1 against 2^53, +-0.0, +-0.5 against 0 and +-1, +-inf as a cell and as a
    constant, 1e19: every edge as a cell, every edge as a constant, under all six comparisons of both kinds"""
    sb = np.zeros(1, dtype=np.uint8)
    cells = [(LONG, x) for x in NUMERIC_EDGE_LONGS] + [(DOUBLE, bits_of(x)) for x in NUMERIC_EDGE_DOUBLES] + [(MISSING, WILD[0]), (ord("n"), WILD[1])]
    t, v = _one_column(cells, sb)
    out = []
    for cmp in NUM_CMPS:
        out += [Case("numeric edge: long_%s %d" % (cmp, k), [(0, "long_" + cmp, k)], t, v, len(cells), sb) for k in NUMERIC_EDGE_LONGS]
        out += [Case("numeric edge: double_%s %r" % (cmp, k), [(0, "double_" + cmp, k)], t, v, len(cells), sb) for k in NUMERIC_EDGE_DOUBLES]
    return out


STRING_EDGE_LENGTHS = (0, 1, 7, 8, 9, 255, 256)


def string_edge_cases():
    """for every constant length and every source alignment 0 .. 15: cells one byte shorter than the constant (a prefix of it),
    equal to it, one byte longer (the constant a prefix of the cell), different in the first byte only and in the last byte only
    -- under EQ, NE and PREFIX.  The last cell of every case ENDS the string buffer."""
    out = []
    rng = np.random.default_rng(3000)
    for ln in STRING_EDGE_LENGTHS:
        const = bytes(rng.integers(1, 255, size=ln, dtype=np.uint8))
        variants = [const, const + b"!"]
        if ln:
            variants += [const[:-1], bytes([const[0] ^ 0x80]) + const[1:], const[:-1] + bytes([const[-1] ^ 1])]
        for align in range(16):
            buf = bytearray(b"\xEE" * align)
            cells = [(MISSING, WILD[0])]
            for s in variants + [const]:  # (the constant once more, so that a cell equal to it ends the buffer)
                buf += b"\xEE" * ((align - len(buf)) % 16)
                cells.append((STRING, (len(s) << 32) | len(buf)))
                buf += s
            t, v = _one_column(cells, buf)
            sb = np.frombuffer(bytes(buf), dtype=np.uint8)
            assert int(v[0, len(cells) - 1] & 0xFFFFFFFF) + ln == sb.size
            out += [Case("string_%s, %d bytes at alignment %d" % (cmp, ln, align), [(0, "string_" + cmp, const)], t, v, len(cells), sb)
                    for cmp in ("eq", "ne", "prefix")]
    return out


def layout_cases():
    """n_cols 1, 3 and 64 with col_stride > n_rows; two terms on the same column; terms on the first and the last column"""
    out = []
    for n_cols in (1, 3, 64):
        rng = np.random.default_rng(4000 + n_cols)
        sb = string_buffer(rng, 256)
        n = 150
        t, v = columns(rng, n_cols, n, n + 11, sb.size, types=[LONG, LONG, DOUBLE, STRING, MISSING])
        last = n_cols - 1
        out.append(Case("%d columns, two terms on the last" % n_cols, [(last, "long_ge", 0), (last, "long_lt", 1 << 53)], t, v, n, sb))
        out.append(Case("%d columns, the first and the last" % n_cols, [(0, "type_ne", MISSING), (last, "type_ne", STRING)], t, v, n, sb))
        out.append(Case("%d columns, no term" % n_cols, [], t, v, n, sb))
    return out


def _true_term(rng, column, ty, value, sb):
    """a random term that is TRUE on the cell (ty, value): its constant from the cell or from the pools, its comparison among
    those that hold"""
    cell = cell_object(ty, value, sb)
    pick = int(rng.integers(0, 4))
    if cell is None or pick == 0:
        other = ALL_TYPES[int(rng.integers(0, len(ALL_TYPES)))]
        return (column, "type_eq", int(ty)) if other == ty or rng.random() < 0.5 else (column, "type_ne", other)
    if isinstance(cell, bytes):
        if pick == 1:
            return (column, "string_eq", cell)
        if pick == 2:
            return (column, "string_prefix", cell[:int(rng.integers(0, len(cell) + 1))])
        return (column, "string_ne", cell + b"a")
    kind = "long" if rng.random() < 0.5 else "double"
    if kind == "long":
        const = cell if isinstance(cell, int) and rng.random() < 0.5 else LONGS[int(rng.integers(0, len(LONGS)))]
    else:
        const = DOUBLES[int(rng.integers(0, len(DOUBLES)))]
        if not math.isinf(cell) and abs(cell) < 2 ** 1000 and rng.random() < 0.5:
            const = float(cell)  # (rounded, when the cell is a long above 2^53)
    holding = [c for c, f in NUM_CMPS.items() if f(cell, const)]
    return (column, "%s_%s" % (kind, holding[int(rng.integers(0, len(holding)))]), const)


def fuzz_case(seed, max_rows=300):
    """a random column set and a random plan of 0 to 16 terms: three plans in four are built so that every term is true on one
    row of the set (constants taken from its cells or the pools), in the fourth each term is true on a row of its own"""
    rng = np.random.default_rng(seed)
    sb = string_buffer(rng, 300)
    n_cols, n = int(rng.integers(1, 7)), int(rng.integers(1, max_rows + 1))
    t, v = columns(rng, n_cols, n, n + int(rng.integers(0, 8)), sb.size, types=ALL_TYPES + [LONG, DOUBLE, STRING] * 2)
    n_terms = int(rng.integers(0, 17))
    witness = int(rng.integers(0, n))
    terms = []
    for _ in range(n_terms):
        c = int(rng.integers(0, n_cols))
        if seed % 4:
            terms.append(_true_term(rng, c, int(t[c, witness]), v[c, witness], sb))
        else:
            r = int(rng.integers(0, n))
            term = _true_term(rng, c, int(t[c, r]), v[c, r], sb)
            terms.append(term)
    return Case("fuzz case %d (%d columns, %d rows, %d terms)" % (seed, n_cols, n, n_terms), terms, t, v, n, sb)
