"""A seeded corpus of tables and whole queries for the column operators, with Python's json as the only truth: shared by the corpus's
own test (tests/test_query_fuzz_corpus.py), the host simulations' chain (tests/test_host_query_fuzz.py) and the GPU's
(tests/test_gpu_query_fuzz.py).  Imports nothing from the product and nothing from the oracle.

case(name) -> Case: one JSON object per document (members id, grp, val, flag, ts, meta, tags, attrs: shuffled, whitespace varied,
each now and then missing, null or of another type; no duplicate keys), two per cent of them failing documents of FAILING.
queries(name) -> the query shapes that apply to the case, their parameters drawn from the case's seed and its data; every constant
of a filter comes from the rows.  expected(name, query) -> what the query must answer, from rows = json.loads per document (FAILED
for a failing one) and Python values alone: an int that is no bool is a long, a float a double, str.encode("utf-8") a string's
bytes, dict order member order.  run_query(B, name, query) runs a query through a backend B -- the host simulations or the device
-- that keeps every operator's outputs where they are made; the chain and every comparison are written once, here, and every
comparison is an equality but sum_double's, which takes groupstats_common.check_stats' bound around math.fsum.

A filter term is true only on a cell of a type its kind compares (a numeric term on 'l' and 'd' cells, an int against a float
exactly, as Python does); an order is by (value, row) with the doubles in totalOrder (-0.0 below +0.0), longs under kind "double"
through float(v) with n_inexact counting int(float(v)) != v; a dictionary lists its entries in the order of first occurrence
among the live rows; group statistics are the exact sum() of ints, math.fsum of floats, minima and maxima in totalOrder.

A filter applies to a case only where one of its candidate terms keeps a row and drops a row: the one-document case runs no
shape that filters its one row.  A vocabulary of V < 11 keys is a sample of SPECIAL_KEYS; one of 40 or 600 holds them all."""
import collections
import datetime
import functools
import json
import math
import random
import struct

import numpy as np

from tests import arrowcol_common as AC
from tests import dictcol_common as DC
from tests import filter_common as FC
from tests import groupstats_common as GC
from tests import strcol_common as STC
from tests import timecol_common as TC

SEED = 20261020
MASK = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
MISSING, NULL, LONG, DOUBLE, STRING, TRUE, FALSE, ARRAY, OBJECT = 0, ord("n"), ord("l"), ord("d"), ord('"'), ord("t"), ord("f"), ord("["), ord("{")
FAILED = ("a failing document",)
LDS_KEYS = 512  # SJMI_GROUP_LDS_KEYS (tests/test_query_fuzz_corpus.py holds it against include/sjmi.h)
TOP_MAX_K = 2048
FILTER_OVERFLOW = 1

# name, documents, val profile, V, with failing documents, through from_ndjson
_CASES = [
    ("d1_longs_v1", 1, "longs", 1, False, False),
    ("d63_doubles_v3", 63, "doubles", 3, True, False),
    ("d64_mixed_v40", 64, "mixed", 40, True, False),
    ("d65_ties_v3", 65, "ties", 3, True, False),
    ("d65_mixed_v40_clean", 65, "mixed", 40, False, False),
    ("d1023_longs_v40", 1023, "longs", 40, True, False),
    ("d1023_mixed_v40_ndjson", 1023, "mixed", 40, False, True),
    ("d1024_mixed_v40", 1024, "mixed", 40, True, False),
    ("d1024_ties_v1", 1024, "ties", 1, True, False),
    ("d1025_doubles_v40", 1025, "doubles", 40, True, False),
    ("d1025_longs_v3", 1025, "longs", 3, True, False),
    ("d2500_mixed_v600", 2500, "mixed", 600, True, False),
    ("d2500_ties_v600", 2500, "ties", 600, True, False),
    ("d2500_doubles_v40", 2500, "doubles", 40, True, False),
]
CASE_IDS = [c[0] for c in _CASES]
LARGEST_CASES = [c[0] for c in _CASES if c[1] == 2500]
N_PAIRS = 147  # (case, query) pairs of the corpus: the host and the GPU tests assert that they ran exactly as many

FAILING = [b'{"id":1,"grp":"unterminated', b'{"id":2,"grp":"\xff\xfe","val":1}', b'{"a":1,}', b"[1 1]"]  # stage 1, stage 1, stage 2, stage 2

SPECIAL_KEYS = ["", "k", "seven_7", "eight_88", "nine__999", ("long300_" * 38)[:300], "twin-key-00A", "twin-key-00B", "é€\U0001F600 key",
                'q"uo\\te', "line\nfeed/"]
TAG_NAMES = ["red", "green", "blue", "röd", "", "a longer tag name of thirty bytes"]
ATTR_KEYS = ["a%02d" % k for k in range(14)] + ["", "kéy", "twelve_bytes", "eight_88", 'q"', "seventeen__bytes_"]

LONG_SMALL = ["0", "1", "-1", "7", "42", "1000"]
LONG_HARD = ["9223372036854775807", "-9223372036854775808", "9007199254740993", "9007199254740991", "-9007199254740993", "-9007199254740991",
             "123456789012", "-987654321098"]
DOUBLES = ["-0.0", "0.5", "-1.5", "1e300", "5e-324", "1.0", "123456789.125", "0.0", "2.5", "-1E+300", "7.0", "42.0", "1000.0"]
TIES = ["2", "2.0", "9007199254740993", "9007199254740992.0", "9007199254740993", "9007199254740992.0", "-1.5"]  # (the median is 2^53)
MALFORMED_TS = ["2015-01-01", "2015-13-10T00:00:00Z", "not a time", "", "2015-01-01T15:00:00", "2015-01-01T15:00:00.1234567890Z"]

Case = collections.namedtuple("Case", "name n_docs profile V ndjson docs failing vocabulary rows")


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- documents -----------------------------------------------------------------------------------------------------------------
def string_text(s, rng, escaped=False):
    """the string as JSON text: plainly, or with escapes (\\uXXXX, \\n, \\", \\/, a surrogate pair), one at the least"""
    if not escaped or not s:
        return json.dumps(s, ensure_ascii=False)
    out, made = [], False
    for n, ch in enumerate(s):
        o = ord(ch)
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "/":
            out.append("\\/")
        elif o > 0xFFFF:
            out.append("\\u%04X\\u%04x" % (0xD800 + ((o - 0x10000) >> 10), 0xDC00 + ((o - 0x10000) & 0x3FF)))
        elif o < 0x20 or rng.random() < 0.4 or (n == len(s) - 1 and not made):
            out.append("\\u%04x" % o)
            made = True
        else:
            out.append(ch)
            continue
        made = made or ch in "\n/" or o > 0xFFFF
    return '"' + "".join(out) + '"'


def _number(rng, profile):
    if profile == "ties":
        return rng.choice(TIES)
    if profile == "mixed":
        profile = rng.choice(["longs", "doubles"])
    if profile == "longs":
        return rng.choice(LONG_SMALL if rng.random() < 0.6 else LONG_HARD + LONG_SMALL)
    return rng.choice(DOUBLES)


_OTHER = {"number": ['"text"', "true", "[1]", "{}"], "string": ["5", "false", "[]", '{"x":1}', "1.5"], "atom": ["0", '"true"', "[true]"],
          "object": ["7", '"meta"', "[]"], "array": ["3", '"tags"', '{"name":"red","w":1}']}


def _mutated(rng, text, kind, p=0.03):
    """-> the member's text, None (missing), null, or a value of another type"""
    r = rng.random()
    if r < p:
        return None
    if r < 2 * p:
        return "null"
    if r < 3 * p:
        return rng.choice(_OTHER[kind])
    return text


def _timestamp(rng):
    if rng.random() < 0.06:
        return rng.choice(MALFORMED_TS)
    moment = datetime.datetime(2024, 2, 27) + datetime.timedelta(seconds=rng.randrange(0, 4 * 86400, 3600 if rng.random() < 0.5 else 1))
    fraction = rng.choice(["", ".%03d" % rng.choice([0, 5, 999]), ".%06d" % rng.choice([0, 1, 999999]), ".%09d" % rng.choice([0, 1, 123456789])])
    zone = rng.choice(["Z", "Z", "+00:00", "+05:30", "-08:00", "-00:00"])
    return moment.strftime("%Y-%m-%dT%H:%M:%S") + fraction + zone


def _object(rng, members, ws):
    """members [(key text, value text)] -> the object's text with whitespace of the document's style"""
    w = lambda: rng.choice(ws)
    return "{" + ",".join(w() + k + w() + ":" + w() + v + w() for k, v in members) + ("}" if members else w() + "}")


def _document(rng, k, profile, vocabulary, hot, forced, ws, planted=None):
    draw = lambda: rng.choice(hot) if rng.random() < 0.45 else rng.choice(vocabulary)
    grp = planted if planted is not None else draw()
    val = _number(rng, profile)
    if grp in forced:
        val = {"long": rng.choice(LONG_SMALL + LONG_HARD), "double": rng.choice(DOUBLES), "negzero": "-0.0", "neither": '"no number"'}[forced[grp]]
    tags = []
    for _ in range(rng.choice([0, 1, 2, 2, 3, 5])):
        if rng.random() < 0.04:
            tags.append(rng.choice(["4", '"tag"', "null", "[]"]))  # (an element that is no object: a row of MISSING cells)
            continue
        pair = [('"name"', _mutated(rng, string_text(rng.choice(TAG_NAMES), rng, rng.random() < 0.2), "string")),
                ('"w"', _mutated(rng, _number(rng, profile), "number"))]
        rng.shuffle(pair)
        tags.append(_object(rng, [m for m in pair if m[1] is not None], ws))
    attrs = []
    for key in rng.sample(ATTR_KEYS, rng.choice([0, 1, 2, 3, 4, 6])):
        value = rng.choice([_number(rng, profile), _number(rng, "mixed"), '"s"', string_text(rng.choice(TAG_NAMES), rng), "true", "false", "null", "[]",
                            "[1,2]", "{}", '{"x":null}'])
        attrs.append((string_text(key, rng, rng.random() < 0.15), value))
    src = [('"name"', _mutated(rng, string_text(rng.choice(TAG_NAMES[:3]) + "-%d" % rng.randrange(4), rng), "string")),
           ('"n"', _mutated(rng, _number(rng, "ties" if profile == "ties" else "mixed"), "number"))]
    meta = _object(rng, [('"src"', _object(rng, [m for m in src if m[1] is not None], ws))], ws)
    members = [('"id"', _mutated(rng, "%d" % k, "number", 0.005)),
               ('"grp"', string_text(grp, rng, rng.random() < 0.2) if planted is not None else _mutated(rng, string_text(grp, rng, rng.random() < 0.2), "string")),
               ('"val"', _mutated(rng, val, "number")),
               ('"flag"', _mutated(rng, rng.choice(["true", "false", "null"]), "atom", 0.02)),
               ('"ts"', _mutated(rng, string_text(_timestamp(rng), rng), "string", 0.02)),
               ('"meta"', _mutated(rng, meta, "object", 0.02)),
               ('"tags"', _mutated(rng, "[" + ",".join(tags) + "]", "array", 0.03)),
               ('"attrs"', _mutated(rng, _object(rng, attrs, ws), "object", 0.02))]
    members = [m for m in members if m[1] is not None]
    rng.shuffle(members)
    return _object(rng, members, ws).encode("utf-8")


def vocabulary(V, rng):
    """-> (the case's group keys, the hot ones, {key: what its val is forced to be})"""
    if V < len(SPECIAL_KEYS):
        keys = rng.sample(SPECIAL_KEYS, V)
        return keys, keys[:1], {}
    fill = ["key%d" % i + "x" * (i % 11) for i in range(V - len(SPECIAL_KEYS))]
    keys = SPECIAL_KEYS + fill
    hot = [fill[0], "twin-key-00A", "twin-key-00B", ""]
    forced = dict(zip(fill[1:5], ("long", "double", "negzero", "neither")))
    return keys, hot, forced


@functools.lru_cache(maxsize=None)
def case(name):
    index = CASE_IDS.index(name)
    _, n_docs, profile, V, with_failing, ndjson = _CASES[index]
    rng = random.Random(SEED * 100 + index)
    keys, hot, forced = vocabulary(V, rng)
    if profile != "mixed":
        forced = {k: v for k, v in forced.items() if v == "neither"}
    run = range(64, 128) if n_docs >= 128 else range(0)  # one aligned run of 64 rows with one key
    free = [k for k in range(n_docs) if k not in run]
    failing = set(rng.sample(free, max(1, round(0.02 * n_docs)))) if with_failing else set()
    once = [k for k in keys if k not in hot and k not in forced and len(k) < 100][-1] if V >= 40 else None  # a key that occurs once
    once_at = rng.choice([k for k in free if k not in failing]) if once is not None else None
    draw_from = [k for k in keys if k != once]
    docs = []
    for k in range(n_docs):
        style = rng.choice([[""], ["", " "], ["", "", " ", "  ", "\t"]] + ([] if ndjson else [["", " ", "\n", " \r\n", "\t"]]))
        if k in failing:
            docs.append(rng.choice(FAILING))
        else:
            docs.append(_document(rng, k, profile, draw_from, hot, forced, style, hot[0] if k in run else once if k == once_at else None))
    rows = []
    for d in docs:
        try:
            rows.append(json.loads(d))
        except ValueError:
            rows.append(FAILED)
    return Case(name, n_docs, profile, V, ndjson, docs, sorted(failing), keys, rows)


# ---- Python values as cells ------------------------------------------------------------------------------------------------------
_ABSENT = ("absent",)


def resolve(value, pointer):
    """the value at an RFC 6901 pointer of plain tokens, or _ABSENT"""
    for token in pointer.split("/")[1:]:
        if isinstance(value, dict) and token in value:
            value = value[token]
        elif isinstance(value, list) and token.isdigit() and int(token) < len(value):
            value = value[int(token)]
        else:
            return _ABSENT
    return value


def cell_of(v):
    """a Python value -> (type byte, payload): a string's bytes, a long's or a double's value word, 1 for true; a container's
    payload (its size and tape index) is not json's to know and is never compared"""
    if v is _ABSENT or v is FAILED:
        return (MISSING, 0)
    if v is None:
        return (NULL, 0)
    if v is True or v is False:
        return (TRUE, 1) if v else (FALSE, 0)
    if isinstance(v, int):
        return (LONG, v & MASK)
    if isinstance(v, float):
        return (DOUBLE, bits_of(v))
    if isinstance(v, str):
        return (STRING, v.encode("utf-8"))
    return (ARRAY if isinstance(v, list) else OBJECT, 0)


def number_of(cell):
    """the cell's exact Python number, or None"""
    t, p = cell
    if t == LONG:
        return p - (1 << 64) if p >> 63 else p
    if t == DOUBLE:
        return FC.double_of(p)
    return None


def select_cells(rows, pointers):
    return [[cell_of(r if r is FAILED else resolve(r, p)) for r in rows] for p in pointers]


def explode_cells(rows, base, pointers, members=False):
    """-> (row offsets [n + 1], [column][row] of cells): an array's elements, or an object's members with the key column last"""
    offs, cols = [0], [[] for _ in range(len(pointers) + members)]
    for r in rows:
        at = _ABSENT if r is FAILED else resolve(r, base)
        elems = list(at.items()) if members and isinstance(at, dict) else at if not members and isinstance(at, list) else []
        for e in elems:
            value = e[1] if members else e
            for q, p in enumerate(pointers):
                cols[q].append(cell_of(resolve(value, p)))
            if members:
                cols[-1].append(cell_of(e[0]))
        offs.append(offs[-1] + len(elems))
    return offs, cols


# ---- references --------------------------------------------------------------------------------------------------------------------
def filter_expected(terms, cols, n_rows, capacity=None):
    keep = FC.reference_from_cells(terms, cols, n_rows) if n_rows else np.zeros(0, dtype=bool)
    kept = [int(r) for r in np.flatnonzero(keep)]
    capacity = n_rows if capacity is None else capacity
    m = min(len(kept), capacity)
    return {"terms": terms, "n_rows": n_rows, "capacity": capacity, "keep_words": FC.words_of(keep), "kept": kept, "n_kept": len(kept), "live": m,
            "record": [len(kept), FILTER_OVERFLOW if len(kept) > capacity else 0], "cols": [[c[r] for r in kept[:m]] for c in cols],
            "cell_types": [{t for t, _ in cols[term[0]][:n_rows]} for term in terms],
            # a long cell that is not the double constant but rounds onto it: compared as doubles, the two would be equal
            "rounds_onto_the_constant": sum(1 for term in terms if term[1].startswith("double_") for t, p in cols[term[0]][:n_rows]
                                            if t == LONG and number_of((t, p)) != term[2] and float(number_of((t, p))) == term[2])}


def _total_order(x):
    return (x, math.copysign(1.0, x))


def top_expected(cells, live, kind, largest, k, words=None):
    """cells: the key column's cells; words: instead, [(valid, data word)] of an Arrow data row without types -> rows, record [9]"""
    cand, n_null, n_other, n_inexact = [], 0, 0, 0
    for r in range(live):
        if words is not None:
            valid, w = words[r]
            if not valid:
                n_null += 1
            elif kind == "long":
                cand.append(((w - (1 << 64) if w >> 63 else w, 0), r, w))
            else:
                cand.append((_total_order(FC.double_of(w)), r, w))
            continue
        t, p = cells[r]
        if t in (MISSING, NULL):
            n_null += 1
        elif t == LONG and kind == "long":
            cand.append(((number_of((t, p)), 0), r, p))
        elif t == LONG:
            v = number_of((t, p))
            n_inexact += int(float(v)) != v
            cand.append((_total_order(float(v)), r, bits_of(float(v))))
        elif t == DOUBLE and kind == "double":
            cand.append((_total_order(FC.double_of(p)), r, p))
        else:
            n_other += 1
    sign = -1 if largest else 1
    cand.sort(key=lambda e: (sign * e[0][0], sign * e[0][1], e[1]))
    top = cand[:k]
    tie = 0 < k < len(cand) and cand[k - 1][0] == cand[k][0]
    mixed = words is None and kind == "double" and bool({e[2] for e in cand if cells[e[1]][0] == LONG} & {e[2] for e in cand if cells[e[1]][0] == DOUBLE})
    return {"kind": kind, "largest": largest, "k": k, "rows": [e[1] for e in top], "tie_at_the_cut": tie, "n_candidates": len(cand),
            "a_long_and_a_double_tie": mixed,
            "record": [live, len(cand), n_null, n_other, 0, n_inexact, len(top), top[-1][2] if top else 0, 0]}


def _entry(longs, doubles, n_other):
    lo = hi = None
    if doubles:
        lo, hi = min(doubles, key=_total_order), max(doubles, key=_total_order)
    return {"n_long": len(longs), "n_double": len(doubles), "n_other": n_other, "sum_long": sum(longs), "sum_double": math.fsum(doubles),
            "abs_double": math.fsum(abs(x) for x in doubles), "min_long": min(longs) if longs else None, "max_long": max(longs) if longs else None,
            "min_double": lo, "max_double": hi}


_CLASS = {LONG: 0, DOUBLE: 1, STRING: 2, TRUE: 3, FALSE: 3, NULL: 4, ARRAY: 5, OBJECT: 6}


def groups_expected(key_cells, val_cells, live, n_keys):
    """the dictionary of the key column's live rows, and per entry (n_keys of them: the ones at or above n_distinct are empty) the
    statistics and the type census of the value column"""
    ref = DC.reference_from_cells(key_cells[:live])
    longs, doubles, others = [[] for _ in range(n_keys)], [[] for _ in range(n_keys)], [0] * n_keys
    counts = [[0] * 8 for _ in range(n_keys)]
    grouped = 0
    for r in range(live):
        if key_cells[r][0] != STRING:
            continue
        ix = int(ref.indices[r])
        t, _ = val_cells[r]
        counts[ix][_CLASS.get(t, 7)] += 1
        grouped += 1
        if t == LONG:
            longs[ix].append(number_of(val_cells[r]))
        elif t == DOUBLE:
            doubles[ix].append(number_of(val_cells[r]))
        else:
            others[ix] += 1
    return {"dict": ref, "dict_record": [live, ref.n_valid, ref.n_other, ref.n_distinct, len(ref.dict_bytes), 0], "n_keys": n_keys,
            "entries": [_entry(longs[j], doubles[j], others[j]) for j in range(n_keys)], "group_record": [live, grouped, 0, 0, 0],
            "counts": counts, "census_record": [live, grouped, 0, 0], "live": live}


# ---- queries -----------------------------------------------------------------------------------------------------------------------
NUM_OPS = ["%s_%s" % (kind, cmp) for cmp in ("eq", "ne", "lt", "le", "gt", "ge") for kind in ("long", "double")]
ORDER_POINTERS = ["/val", "/id", "/grp", "/flag"]
GROUP_POINTERS = ["/grp", "/val"]
FGROUP_POINTERS = ["/grp", "/val", "/flag", "/meta/src/n", "/meta/src/name"]
ARROW_POINTERS = ["/val", "/flag", "/id"]
ARROW_FIELDS = [(0, "int64"), (0, "float64"), (1, "bool")]
LATEST_POINTERS = ["/ts", "/id"]
TIME_FIELDS = [(0, "ms")]


def _median_constants(cells):
    numbers = sorted(x for x in (number_of(c) for c in cells) if x is not None)
    if not numbers:
        return None
    m = numbers[len(numbers) // 2]
    as_long = m if isinstance(m, int) else max(INT64_MIN, min(INT64_MAX, int(math.floor(m)))) if abs(m) < 2.0 ** 63 else (INT64_MAX if m > 0 else INT64_MIN)
    return as_long, float(as_long) + 0.5


def _splits(terms, cols, n_rows, least=1):
    kept = int(FC.reference_from_cells(terms, cols, n_rows).sum()) if n_rows else 0
    return least <= kept < n_rows


def numeric_term(cols, column, n_rows, start, front=()):
    """the first of the twelve numeric comparisons from `start` on, against the column's median long or that median as a double
    with .5 added, that -- behind the terms `front` -- keeps a row and drops a row (two rows kept, where one does)"""
    consts = _median_constants(cols[column][:n_rows])
    if consts is None:
        return None
    for least in (2, 1):
        for j in range(len(NUM_OPS)):
            op = NUM_OPS[(start + j) % len(NUM_OPS)]
            term = (column, op, consts[0] if op.startswith("long") else consts[1])
            if _splits(list(front) + [term], cols, n_rows, least):
                return term
    return None


def string_term(cols, column, n_rows, which):
    """string_eq / string_ne on the key that occurs most often, string_prefix on a proper prefix of one that occurs"""
    seen = collections.Counter(p for t, p in cols[column][:n_rows] if t == STRING)
    if not seen:
        return None
    if which == "prefix":
        long_enough = [k for k, _ in seen.most_common() if len(k) >= 2]
        if not long_enough:
            return None
        twin = [k for k in long_enough if k.startswith(b"twin-key-00")]
        return (column, "string_prefix", (twin or long_enough)[0][:-1])
    return (column, "string_" + which, seen.most_common(1)[0][0])


def _group_terms(cols, n_rows, index):
    """two or three terms for a filtered group by: a string term on /grp, type_eq on /flag, a numeric term on /meta/src/n"""
    for shift in range(3):
        which = ("eq", "ne", "prefix")[(index + shift) % 3]
        s = string_term(cols, 0, n_rows, which)
        if s is None:
            continue
        for flag in (TRUE, FALSE, NULL):
            two = [s, (2, "type_eq", flag)]
            third = numeric_term(cols, 3, n_rows, index * 5 + 3, two)
            if third is not None and index % 2 == 0:
                return two + [third]
            if _splits(two, cols, n_rows, 2):
                return two
            if third is not None:
                return two + [third]
    return None


@functools.lru_cache(maxsize=None)
def queries(name):
    """-> [query]: a dict with its "shape", its "name" and its parameters"""
    c = case(name)
    index, n = CASE_IDS.index(name), c.n_docs
    rng = random.Random(SEED * 1000 + index)
    out = []
    order = select_cells(c.rows, ORDER_POINTERS)
    term = numeric_term(order, 0, n, index * 7)
    if term is not None:
        out.append({"shape": "order_by", "terms": [term], "capacity": None})
    out.append({"shape": "group_by", "pointers": GROUP_POINTERS, "terms": None, "capacity": None})
    fgroup = select_cells(c.rows, FGROUP_POINTERS)
    gterms = _group_terms(fgroup, n, index)
    if gterms is not None:
        out.append({"shape": "group_by", "pointers": FGROUP_POINTERS, "terms": gterms, "capacity": None})
    _, tags = explode_cells(c.rows, "/tags", ["/name", "/w"])
    out.append({"shape": "exploded", "terms": [t for t in [numeric_term(tags, 1, len(tags[0]), index * 7 + 5)] if t is not None] or None})
    out.append({"shape": "members"})
    arrow = select_cells(c.rows, ARROW_POINTERS)
    aterm = numeric_term(arrow, 0, n, index * 7 + 6)
    if aterm is not None:
        front = [t for t in [(1, "type_ne", NULL)] if index % 2 and _splits([t, aterm], arrow, n)]
        out.append({"shape": "arrow", "terms": front + [aterm]})
    out.append({"shape": "latest", "terms": None})
    latest = select_cells(c.rows, LATEST_POINTERS)
    lterm = numeric_term(latest, 1, n, index * 7 + 9)
    if lterm is not None:
        out.append({"shape": "latest", "terms": [(0, "type_eq", STRING), lterm] if _splits([(0, "type_eq", STRING), lterm], latest, n) else [lterm]})
    if term is not None and filter_expected([term], order, n)["n_kept"] >= 2:
        half = filter_expected([term], order, n)["n_kept"] // 2
        out.append({"shape": "order_by", "terms": [term], "capacity": half})
    if gterms is not None and filter_expected(gterms, fgroup, n)["n_kept"] >= 2:
        out.append({"shape": "group_by", "pointers": FGROUP_POINTERS, "terms": gterms, "capacity": filter_expected(gterms, fgroup, n)["n_kept"] // 2})
    if term is not None:
        first = filter_expected([term], order, n)
        seconds = [[(3, "type_eq", rng.choice([TRUE, FALSE]))], [t for t in [string_term(first["cols"], 2, first["n_kept"], "ne")] if t is not None],
                   [(3, "type_ne", MISSING), (2, "type_eq", STRING)]]
        second = next((s for s in seconds if s and _splits(s, first["cols"], first["n_kept"])), None)
        if second is not None:
            out.append({"shape": "filter_of_filter", "terms": [term], "second": second})
    for q in out:
        q["name"] = ("filtered_" if q["shape"] == "group_by" and q["terms"] else "") + q["shape"] + \
            (" behind a filter" if q["shape"] == "latest" and q["terms"] else "") + ("" if q.get("capacity") is None else " at half the capacity")
    assert len({q["name"] for q in out}) == len(out)
    return out


def _top_variants(cells, live):
    """shape 1's top_rows calls: both kinds, both directions, k from {0, 1, 10, the number of candidates, 2048}"""
    out = []
    for kind in ("long", "double"):
        n_cand = top_expected(cells, live, kind, True, 0)["n_candidates"]
        for largest in (True, False):
            for k in sorted({0, 1, 10, min(n_cand, TOP_MAX_K), TOP_MAX_K}):
                out.append(top_expected(cells, live, kind, largest, k))
    return out


def _group_capacities(c, extra=7):
    """upper bounds from the generator: every string under /grp is a key of the vocabulary"""
    return len(c.vocabulary) + extra, sum(len(k.encode("utf-8")) for k in c.vocabulary) + 16


@functools.lru_cache(maxsize=None)
def _expected(name, at):
    c = case(name)
    q = queries(name)[at]
    n, shape = c.n_docs, q["shape"]
    E = {"filters": [], "tops": [], "groups": [], "row_counts": [], "n_rows": [n]}
    if shape in ("order_by", "filter_of_filter"):
        cols = select_cells(c.rows, ORDER_POINTERS)
        f = filter_expected(q["terms"], cols, n, q.get("capacity"))
        E["filter"] = f
        if shape == "order_by":
            E["tops"] = _top_variants(f["cols"][0], f["live"])
            at_ten = next(t for t in E["tops"] if t["k"] == 10 and t["kind"] == "double" and t["largest"])
            E["strings"] = STC.reference_from_cells([f["cols"][2][r] for r in at_ten["rows"]])
        else:
            g = filter_expected(q["second"], f["cols"], f["n_kept"])
            E["second"] = g
            E["filters"].append(g)
            E["row_counts"].append(g["n_kept"])
            E["tops"] = [top_expected(g["cols"][0], g["live"], "double", True, 10)]
    elif shape == "group_by":
        cols = select_cells(c.rows, q["pointers"])
        live = n
        if q["terms"]:
            f = E["filter"] = filter_expected(q["terms"], cols, n, q["capacity"])
            cols, live = f["cols"], f["live"]
        C, B = _group_capacities(c)
        E["capacities"] = (C, B)
        E["groups"] = [groups_expected(cols[0], cols[1], live, C)]
    elif shape == "exploded":
        offs, cols = explode_cells(c.rows, "/tags", ["/name", "/w"])
        total = offs[-1]
        E.update(offsets=offs, total=total, capacity=total + 9, cols=cols, capacities=(len(TAG_NAMES) + 3, sum(len(t.encode("utf-8")) for t in TAG_NAMES) + 8))
        E["n_rows"].append(total)
        E["row_counts"].append(total)
        E["groups"] = [groups_expected(cols[0], cols[1], total, E["capacities"][0])]
        E["tops"] = [top_expected(cols[1], total, "double", True, 10)]
        if q["terms"]:
            f = E["filter"] = filter_expected(q["terms"], cols, total)
            E["groups"].append(groups_expected(f["cols"][0], f["cols"][1], f["live"], E["capacities"][0]))
            E["tops"].append(top_expected(f["cols"][1], f["live"], "long", False, 10))
    elif shape == "members":
        offs, cols = explode_cells(c.rows, "/attrs", [""], members=True)
        total = offs[-1]
        E.update(offsets=offs, total=total, capacity=total + 9, cols=cols, capacities=(len(ATTR_KEYS) + 3, sum(len(t.encode("utf-8")) for t in ATTR_KEYS) + 8))
        E["n_rows"].append(total)
        E["row_counts"].append(total)
        E["groups"] = [groups_expected(cols[1], cols[0], total, E["capacities"][0])]
    elif shape == "arrow":
        cols = select_cells(c.rows, ARROW_POINTERS)
        f = E["filter"] = filter_expected(q["terms"], cols, n)
        ref = E["arrow"] = AC.reference_from_cells(ARROW_FIELDS, f["cols"], f["live"])
        bit = lambda words, r: (words[r // 64] >> (r % 64)) & 1
        E["tops"] = [top_expected(None, f["live"], kind, largest, 10, [(bit(ref.validity[fi], r), ref.data[fi][r]) for r in range(f["live"])])
                     for fi, kind, largest in ((0, "long", True), (1, "double", False))]
    elif shape == "latest":
        cols = select_cells(c.rows, LATEST_POINTERS)
        live = n
        if q["terms"]:
            f = E["filter"] = filter_expected(q["terms"], cols, n)
            cols, live = f["cols"], f["live"]
        ref = E["time"] = TC.reference_from_cells(TIME_FIELDS, cols, live)
        bit = lambda words, r: (words[r // 64] >> (r % 64)) & 1
        E["cols"] = cols
        E["tops"] = [top_expected(None, live, "long", largest, 10, [(bit(ref.validity[0], r), ref.data[0][r]) for r in range(live)]) for largest in (True, False)]
    if "filter" in E:
        E["filters"].append(E["filter"])
        E["row_counts"].append(E["filter"]["n_kept"])
    return E


def expected(name, query):
    return _expected(name, queries(name).index(query))


# ---- running a query through a backend -------------------------------------------------------------------------------------------
# A backend keeps every output where its operator made it (numpy arrays of the host simulations, tensors on the device): select,
# explode, filter, top_rows, string_column, dictionary_column, group_stats, key_census, arrow_columns, timestamp_columns take and
# return such handles (a handle takes [i] and [a:b]); group_by_string and discover_keys return Python values; sync() waits for
# everything queued; host(handle) -> numpy (uint64 for words, uint8 for bytes, int32 for indices); string_buffer() -> bytes.
def same_cells(what, types, values, want, sb):
    """one column's first len(want) cells against the reference's"""
    types, values = np.asarray(types), np.asarray(values)
    assert types.size >= len(want) and values.size >= len(want), what
    for r, (t, p) in enumerate(want):
        where = "%s, row %d" % (what, r)
        assert int(types[r]) == t, (where, int(types[r]), t)
        v = int(values[r]) & MASK
        if t == STRING:
            off, ln = v & 0xFFFFFFFF, v >> 32
            assert bytes(sb[off:off + ln]) == p, (where, bytes(sb[off:off + ln]), p)
        elif t not in (ARRAY, OBJECT, MISSING):
            assert v == p, (where, v, p)


def _words(x):
    return [int(w) & MASK for w in np.asarray(x).reshape(-1)]


class _Run:
    def __init__(self, B, what):
        self.B, self.what, self.outputs, self.sb = B, what, [], None

    def own(self, label, array, sum_double=False):
        """a word the call owns: kept for the comparison of two runs"""
        self.outputs.append((label, np.array(array).copy(), sum_double))

    def filter(self, label, got, f):
        rows, oT, oV, keep, res = got
        H, what = self.B.host, "%s: %s" % (self.what, label)
        assert _words(H(res)) == f["record"], (what, _words(H(res)), f["record"])
        assert _words(H(keep))[:len(f["keep_words"])] == _words(f["keep_words"]), (what, "keep")
        m = f["live"]
        assert _words(H(rows[:m])) == f["kept"][:m], (what, "rows")
        for c, col in enumerate(f["cols"]):
            same_cells("%s column %d" % (what, c), H(oT[c][:m]), H(oV[c][:m]), col, self.sb)
        self.own(label + " record", H(res))
        self.own(label + " rows", H(rows[:m]))
        self.own(label + " values", np.stack([H(oV[c][:m]) for c in range(len(f["cols"]))]) if m else np.zeros(0))

    def top(self, label, got, t, carried):
        rows, oT, oV, res = got
        H, what = self.B.host, "%s: %s %s %s k=%d" % (self.what, label, t["kind"], "largest" if t["largest"] else "smallest", t["k"])
        assert _words(H(res)) == t["record"], (what, _words(H(res)), t["record"])
        n_out = len(t["rows"])
        assert _words(H(rows[:n_out])) == t["rows"], (what, _words(H(rows[:n_out])), t["rows"])
        for c, col in enumerate(carried or []):
            same_cells("%s carried column %d" % (what, c), H(oT[c][:n_out]), H(oV[c][:n_out]), [col[r] for r in t["rows"]], self.sb)
        self.own(label + " top record", H(res))
        self.own(label + " top rows", H(rows[:n_out]))

    def groups(self, label, dct, stats, census, g):
        H, what = self.B.host, "%s: %s" % (self.what, label)
        indices, validity, dict_rows, dict_offsets, dict_bytes, dres = dct
        ref, live = g["dict"], g["live"]
        assert _words(H(dres)) == g["dict_record"], (what, _words(H(dres)), g["dict_record"])
        nd = ref.n_distinct
        assert np.array_equal(np.asarray(H(indices[:live])).astype(np.int64), ref.indices), (what, "indices")
        words = (live + 63) // 64
        assert _words(H(validity[:words])) == _words(ref.validity[:words]), (what, "validity")
        assert _words(H(dict_rows[:nd])) == _words(ref.dict_rows), (what, "dict_rows")
        assert _words(H(dict_offsets[:nd + 1])) == _words(ref.dict_offsets), (what, "dict_offsets")
        assert bytes(np.asarray(H(dict_bytes[:len(ref.dict_bytes)]), dtype=np.uint8)) == ref.dict_bytes, (what, "dict_bytes")
        self.own(label + " dictionary", H(dres))
        self.own(label + " dictionary offsets", H(dict_offsets[:nd + 1]))
        if stats is not None:
            table, gres = stats
            assert _words(H(gres)) == g["group_record"], (what, _words(H(gres)), g["group_record"])
            GC.check_stats(H(table), g["entries"], what=what)
            self.own(label + " statistics", np.asarray(H(table)).reshape(-1, GC.WORDS), sum_double=True)
        if census is not None:
            counts, cres = census
            assert _words(H(cres)) == g["census_record"], (what, _words(H(cres)), g["census_record"])
            assert np.asarray(H(counts)).reshape(-1, 8).astype(np.int64).tolist() == g["counts"], (what, "census")
            self.own(label + " census", H(counts))

    def keyed(self, label, got, g):
        """group_by_string's list against the same entries"""
        what = "%s: %s" % (self.what, label)
        ref = g["dict"]
        assert [k for k, _ in got] == ref.values, (what, "keys")
        for j, (_, d) in enumerate(got):
            w = g["entries"][j]
            for field in ("n_long", "n_double", "n_other", "sum_long", "min_long", "max_long"):
                assert d[field] == w[field], (what, j, field, d[field], w[field])
            for field in ("min_double", "max_double"):
                assert (d[field] is None) == (w[field] is None) and (w[field] is None or bits_of(d[field]) == bits_of(w[field])), (what, j, field)
            assert abs(d["sum_double"] - w["sum_double"]) <= GC.gamma(w["n_double"]) * w["abs_double"], (what, j, d["sum_double"], w["sum_double"])


def run_query(B, name, query):
    """the query, queued whole and read behind one sync() (but for the wrappers that read a size back themselves) -> the words the
    calls own, for the comparison of two runs: [(label, numpy array, holds sum_double)]"""
    c = case(name)
    E = expected(name, query)
    R = _Run(B, "%s, %s" % (name, query["name"]))
    n, shape, H = c.n_docs, query["shape"], B.host
    R.sb = B.string_buffer()
    if shape in ("order_by", "filter_of_filter"):
        T, V = B.select(ORDER_POINTERS)
        f = E["filter"]
        got = B.filter(f["terms"], T, V, None, query.get("capacity"))
        rows, oT, oV, keep, res = got
        stride = f["capacity"]
        if shape == "order_by":
            tops = [B.top_rows(oT[0], oV[0], t["k"], t["kind"], t["largest"], None, oT, oV, stride, res[0:1]) for t in E["tops"]]
            B.sync()
            R.filter("filter", got, f)
            for t, g in zip(E["tops"], tops):
                R.top("order by /val", g, t, f["cols"])
            at = next(i for i, t in enumerate(E["tops"]) if t["k"] == 10 and t["kind"] == "double" and t["largest"])
            n_out = len(E["tops"][at]["rows"])
            soffs, svalid, sdata, sres = B.string_column(tops[at][1][2][:n_out], tops[at][2][2][:n_out])
            B.sync()
            STC.check(R.what + ": the carried /grp as a string column", H(soffs), H(svalid), H(sdata), H(sres), E["strings"], len(E["strings"][2]), canaries=False)
        else:
            g = E["second"]
            got2 = B.filter(g["terms"], oT, oV, f["n_kept"], None)
            top = B.top_rows(got2[1][0], got2[2][0], 10, "double", True, None, got2[1], got2[2], g["capacity"], got2[4][0:1])
            B.sync()
            R.filter("the first filter", got, f)
            R.filter("the second filter", got2, g)
            R.top("behind two filters", top, E["tops"][0], g["cols"])
    elif shape == "group_by":
        T, V = B.select(query["pointers"])
        rc, got = None, None
        if query["terms"]:
            f = E["filter"]
            got = B.filter(f["terms"], T, V, None, query["capacity"])
            T, V, rc = got[1], got[2], got[4][0:1]
        C, Bc = E["capacities"]
        g = E["groups"][0]
        dct = B.dictionary_column(T[0], V[0], C, Bc, rc)
        stats = B.group_stats(dct[0], dct[1], T[1], V[1], C, rc)
        census = B.key_census(dct[0], dct[1], T[1], C, rc)
        B.sync()
        if got is not None:
            R.filter("filter", got, E["filter"])
        R.groups("group /val by /grp", dct, stats, census, g)
        R.keyed("group_by_string", B.group_by_string(T[0], V[0], T[1], V[1], C, rc)[0], g)
    elif shape == "exploded":
        offs, T, V = B.explode("/tags", ["/name", "/w"], E["capacity"], False)
        rc = offs[n:n + 1]
        C, Bc = E["capacities"]
        dct = B.dictionary_column(T[0], V[0], C, Bc, rc)
        stats = B.group_stats(dct[0], dct[1], T[1], V[1], C, rc)
        top = B.top_rows(T[1], V[1], 10, "double", True, None, T, V, E["capacity"], rc)
        if query["terms"]:
            f = E["filter"]
            got = B.filter(f["terms"], T, V, E["total"], None)
            krc = got[4][0:1]
            dct2 = B.dictionary_column(got[1][0], got[2][0], C, Bc, krc)
            stats2 = B.group_stats(dct2[0], dct2[1], got[1][1], got[2][1], C, krc)
            top2 = B.top_rows(got[1][1], got[2][1], 10, "long", False, None, got[1], got[2], f["capacity"], krc)
        B.sync()
        assert _words(H(offs[:n + 1])) == E["offsets"], (R.what, "row offsets")
        for col in range(2):
            same_cells("%s: exploded column %d" % (R.what, col), H(T[col][:E["total"]]), H(V[col][:E["total"]]), E["cols"][col], R.sb)
        R.groups("group /w by /name", dct, stats, None, E["groups"][0])
        R.top("order by /w", top, E["tops"][0], E["cols"])
        if query["terms"]:
            R.filter("filter on /w", got, f)
            R.groups("group /w by /name behind the filter", dct2, stats2, None, E["groups"][1])
            R.top("order by /w behind the filter", top2, E["tops"][1], f["cols"])
    elif shape == "members":
        offs, T, V = B.explode("/attrs", [""], E["capacity"], True)
        rc = offs[n:n + 1]
        C, Bc = E["capacities"]
        g = E["groups"][0]
        dct = B.dictionary_column(T[1], V[1], C, Bc, rc)
        census = B.key_census(dct[0], dct[1], T[0], C, rc)
        stats = B.group_stats(dct[0], dct[1], T[0], V[0], C, rc)
        B.sync()
        assert _words(H(offs[:n + 1])) == E["offsets"], (R.what, "row offsets")
        for col in range(2):
            same_cells("%s: members column %d" % (R.what, col), H(T[col][:E["total"]]), H(V[col][:E["total"]]), E["cols"][col], R.sb)
        R.groups("the members of /attrs by key", dct, stats, census, g)
        keys, koffs, _, cres = B.discover_keys("/attrs", C)
        nd = g["dict"].n_distinct
        assert keys == [(g["dict"].values[j], g["counts"][j]) for j in range(nd)], (R.what, "discover_keys")
        assert _words(koffs) == E["offsets"] and _words(cres) == g["census_record"], (R.what, "discover_keys")
    elif shape == "arrow":
        T, V = B.select(ARROW_POINTERS)
        f, ref = E["filter"], E["arrow"]
        got = B.filter(f["terms"], T, V, None, None)
        rc = got[4][0:1]
        data, validity, results = B.arrow_columns(ARROW_FIELDS, got[1], got[2], n, rc)
        tops = [B.top_rows(None, data[fi], 10, t["kind"], t["largest"], validity[fi], got[1], got[2], n, rc) for fi, t in zip((0, 1), E["tops"])]
        B.sync()
        R.filter("filter", got, f)
        live, words = ref.live, (ref.live + 63) // 64
        assert [tuple(r) for r in np.asarray(H(results)).reshape(len(ARROW_FIELDS), 4).tolist()] == ref.records, (R.what, "arrow records")
        for fi, field in enumerate(ARROW_FIELDS):
            owned = words if field[1] == "bool" else live
            assert _words(H(data[fi][:owned])) == ref.data[fi], (R.what, "arrow data of field %d" % fi)
            assert _words(H(validity[fi][:words])) == ref.validity[fi], (R.what, "arrow validity of field %d" % fi)
        for t, g in zip(E["tops"], tops):
            R.top("order by the Arrow field", g, t, f["cols"])
    elif shape == "latest":
        T, V = B.select(LATEST_POINTERS)
        rc, got = None, None
        if query["terms"]:
            got = B.filter(E["filter"]["terms"], T, V, None, None)
            T, V, rc = got[1], got[2], got[4][0:1]
        ref = E["time"]
        data, validity, results = B.timestamp_columns(TIME_FIELDS, T, V, n, rc)
        tops = [B.top_rows(None, data[0], 10, "long", t["largest"], validity[0], T, V, n, rc) for t in E["tops"]]
        B.sync()
        if got is not None:
            R.filter("filter", got, E["filter"])
        live, words = ref.live, (ref.live + 63) // 64
        assert [tuple(r) for r in np.asarray(H(results)).reshape(1, 6).tolist()] == ref.records, (R.what, "time records", H(results), ref.records)
        assert _words(H(data[0][:live])) == ref.data[0] and _words(H(validity[0][:words])) == ref.validity[0], (R.what, "timestamps")
        for t, g in zip(E["tops"], tops):
            R.top("latest", g, t, E["cols"])
    else:
        raise AssertionError(shape)
    return R.outputs


def same_runs(a, b):
    """two runs of one query: every word the calls own identical, sum_double aside"""
    assert [x[0] for x in a] == [x[0] for x in b]
    for (label, x, sums), (_, y, _) in zip(a, b):
        if sums:
            assert GC.same_but_sum_double(x, y), label
        else:
            assert x.shape == y.shape and np.array_equal(x, y), label
    return True


# ---- what the corpus contains ------------------------------------------------------------------------------------------------------
def pairs():
    return [(name, q) for name in CASE_IDS for q in queries(name)]


def _aligned_run_of_one_key(g):
    """a key that fills an aligned run of 64 live rows of the grouped column"""
    ref, live = g["dict"], g["live"]
    for at in range(0, live - 63, 64):
        if int(ref.validity[at // 64]) & MASK == MASK and len(set(ref.indices[at:at + 64].tolist())) == 1:
            return True
    return False


def source_texts(name):
    """{key: the source texts of its occurrences under "grp"} of the documents that are not failing"""
    import re
    c = case(name)
    out = collections.defaultdict(set)
    for k, d in enumerate(c.docs):
        if c.rows[k] is not FAILED:
            m = re.search(rb'"grp"\s*:\s*("(?:[^"\\]|\\.)*")', d)
            if m:
                out[json.loads(m.group(1))].add(m.group(1))
    return out


@functools.lru_cache(maxsize=None)
def statistics():
    """what tests/test_query_fuzz_corpus.py asserts, counted from expected() alone"""
    st = {"pairs": 0, "filters": 0, "filters_that_do_not_split": [], "ops": set(), "long_cell_double_constant": 0, "double_cell_long_constant": 0, "rounds_onto_the_constant": 0,
          "order_by_cuts": 0, "order_by_ties_at_the_cut": 0, "a_long_and_a_double_tie": 0, "n_inexact": 0, "n_null": 0, "n_other": 0, "fewer_than_k": 0,
          "only_longs": 0, "only_doubles": 0, "both": 0, "neither": 0, "all_negative_zero": 0, "once": 0, "aligned_runs": 0, "empty_groups": 0,
          "n_rows": set(), "row_counts": set(), "distinct_of_the_600": 0, "overflows": 0}
    for name, q in pairs():
        E = expected(name, q)
        st["pairs"] += 1
        st["n_rows"].update(E["n_rows"])
        st["row_counts"].update(E["row_counts"])
        for f in E["filters"]:
            st["filters"] += 1
            st["overflows"] += f["record"][1]
            st["rounds_onto_the_constant"] += f["rounds_onto_the_constant"] > 0
            if not 1 <= f["n_kept"] < f["n_rows"]:
                st["filters_that_do_not_split"].append((name, q["name"], f["terms"], f["n_kept"], f["n_rows"]))
            for term, types in zip(f["terms"], f["cell_types"]):
                st["ops"].add(term[1])
                st["long_cell_double_constant"] += term[1].startswith("double_") and LONG in types
                st["double_cell_long_constant"] += term[1].startswith("long_") and DOUBLE in types
        for t in E["tops"]:
            if q["shape"] == "order_by" and 0 < t["k"] < t["n_candidates"]:
                st["order_by_cuts"] += 1
                st["order_by_ties_at_the_cut"] += t["tie_at_the_cut"]
            st["a_long_and_a_double_tie"] += t["a_long_and_a_double_tie"]
            st["n_inexact"] += t["record"][5] > 0
            st["n_null"] += t["record"][2] > 0
            st["n_other"] += t["record"][3] > 0
            st["fewer_than_k"] += t["record"][6] < t["k"]
        for g in E["groups"]:
            nd = g["dict"].n_distinct
            st["aligned_runs"] += _aligned_run_of_one_key(g)
            st["empty_groups"] += g["n_keys"] - nd
            if q["shape"] == "group_by" and not q["terms"] and case(name).V == 600:
                st["distinct_of_the_600"] = max(st["distinct_of_the_600"], nd)
            for e in g["entries"][:nd]:
                st["only_longs"] += e["n_long"] > 0 and e["n_double"] == 0
                st["only_doubles"] += e["n_long"] == 0 and e["n_double"] > 0
                st["both"] += e["n_long"] > 0 and e["n_double"] > 0
                st["neither"] += e["n_long"] == 0 and e["n_double"] == 0
                st["all_negative_zero"] += e["n_double"] > 0 and bits_of(e["max_double"]) == bits_of(-0.0)
                st["once"] += e["n_long"] + e["n_double"] + e["n_other"] == 1
    st["keys_with_two_source_texts"] = max(sum(len(texts) >= 2 for texts in source_texts(name).values()) for name in CASE_IDS)
    return st
