"""What the timestamp column export must give (include/sjmi.h, sjmi_time_columns_device), in Python alone: shares no code with the
product.  reference() works cell by cell on Python ints: an explicit, state-free test of the RFC 3339 grammar position by
position, Hinnant's days_from_civil, and exact integer arithmetic for the value, the range and the dropped digits -- no datetime
in the value path, because datetime has no year 0 (datetime_value() is the cross-check the tests run for years >= 1).  check()
compares everything a call owns word for word and, against CANARY-filled buffers, everything it must not touch (both are
tests/fieldcol_common.py's, with the live rows and the stride rule of a case).  The *_case()
generators are seeded -- a name is a case -- and shared by the host simulation's tests (tests/test_host_timecol.py) and the GPU
tests (tests/test_gpu_timecol.py).  A field is the tuple of binding.time_fields: (column, unit[, "naive_utc"])."""
import datetime
from collections import namedtuple

import numpy as np

from tests import fieldcol_common as F
from tests.fieldcol_common import (ALL_TYPES, BACK, CANARY_WORD, DOUBLE, FALSE, FRONT, INT64_MAX, INT64_MIN, LONG, MASK, MISSING, NULL, STRING, TRUE,
                                   check, live_counts, live_rows, pack_bits)
from tests.strcol_common import WILD

UNITS = {"s": 0, "ms": 1, "us": 2, "ns": 3}             # SJMI_TIME_<UNIT>
UNIT_DIGITS = {"s": 0, "ms": 3, "us": 6, "ns": 9}
FLAGS = {"naive_utc": 1}                                # SJMI_TIME_F_*
FIELD = np.dtype([("column", "<u4"), ("unit", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])  # sjmi_time_field
RECORD_WORDS = 6                                        # n_rows, n_valid, n_other, n_malformed, n_range, n_inexact

# types uint8 / values uint64 [n_cols, col_stride], n_rows <= col_stride; sb: the string buffer (uint8) the '"' cells point into;
# row_count None or what *d_row_count holds; data_stride >= n_rows, validity_stride >= ceil(n_rows / 64)
Case = namedtuple("Case", "name fields types values sb n_rows row_count data_stride validity_stride")
Ref = namedtuple("Ref", "live data validity records")  # data / validity: per field the words the call owns; records: per field 6 ints


def encode(fields):
    """tuples -> the sjmi_time_field array: the C form, for the host simulation"""
    return F.encode(fields, FIELD, UNITS, FLAGS)


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def days_from_civil(y, m, d):
    """days since 1970-01-01 in the proleptic Gregorian calendar (H. Hinnant, chrono-Compatible Low-Level Date Algorithms)"""
    y -= m <= 2
    era = (y if y >= 0 else y - 399) // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def _digits(b, at, n):
    """the n ASCII digits at b[at:] as a number, or None"""
    part = b[at:at + n]
    if len(part) != n or any(not 0x30 <= c <= 0x39 for c in part):
        return None
    return int(bytes(part))


def parse(b, naive_utc):
    """the bytes of a string -> (epoch seconds, fraction digits as bytes) when they are the WHOLE of
    YYYY-MM-DD sep hh:mm:ss ['.' 1 to 9 digits] zone, else None.  Position by position: no state, no regular expression."""
    b = bytes(b)
    if not (19 if naive_utc else 20) <= len(b) <= 35:
        return None
    y, m, d, hh, mi, ss = _digits(b, 0, 4), _digits(b, 5, 2), _digits(b, 8, 2), _digits(b, 11, 2), _digits(b, 14, 2), _digits(b, 17, 2)
    if None in (y, m, d, hh, mi, ss) or b[4] != 0x2D or b[7] != 0x2D or b[10] not in b"Tt " or b[13] != 0x3A or b[16] != 0x3A:
        return None
    leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    if not 1 <= m <= 12 or not 1 <= d <= (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]:
        return None
    if hh > 23 or mi > 59 or ss > 59:
        return None
    at, fraction = 19, b""
    if b[at:at + 1] == b".":
        end = at + 1
        while end < len(b) and 0x30 <= b[end] <= 0x39:
            end += 1
        fraction = b[at + 1:end]
        if not 1 <= len(fraction) <= 9:
            return None
        at = end
    zone = b[at:]
    if zone == b"":
        if not naive_utc:
            return None
        offset = 0
    elif zone in (b"Z", b"z"):
        offset = 0
    elif len(zone) == 6 and zone[0:1] in (b"+", b"-") and zone[3] == 0x3A:
        zh, zm = _digits(zone, 1, 2), _digits(zone, 4, 2)
        if zh is None or zm is None or zh > 23 or zm > 59:
            return None
        offset = (zh * 3600 + zm * 60) * (-1 if zone[0:1] == b"-" else 1)
    else:
        return None
    return days_from_civil(y, m, d) * 86400 + hh * 3600 + mi * 60 + ss - offset, fraction


def string_value(b, unit, naive_utc):
    """-> None (malformed), or (value, in_range, inexact): the exact integer at the unit, surplus digits dropped"""
    got = parse(b, naive_utc)
    if got is None:
        return None
    secs, fraction = got
    k = UNIT_DIGITS[unit]
    kept, dropped = fraction[:k], fraction[k:]
    value = secs * 10 ** k + int((kept + b"0" * k)[:k] or b"0")
    return value, INT64_MIN <= value <= INT64_MAX, any(c != 0x30 for c in dropped)


def cell(unit, flags, ty, word, sb):
    """one cell under one field -> (data word, valid, other, malformed, range, inexact); word is looked at only behind '"'"""
    ty = int(ty)
    if ty != STRING:
        return 0, False, ty not in (MISSING, NULL), False, False, False
    offset, length = int(word) & 0xFFFFFFFF, int(word) >> 32
    return cell_of_bytes(unit, flags, ty, sb[offset:offset + length] if length <= 35 else None)  # (a longer one: not sliced at all)


def cell_of_bytes(unit, flags, ty, text):
    """the same for a cell given as its type byte and, for a string, its bytes (None: too long to be looked at)"""
    if int(ty) != STRING:
        return 0, False, int(ty) not in (MISSING, NULL), False, False, False
    got = string_value(text, unit, "naive_utc" in flags) if text is not None else None
    if got is None:
        return 0, False, False, True, False, False
    value, in_range, inexact = got
    if not in_range:
        return 0, False, False, False, True, False
    return value & MASK, True, False, False, False, inexact


def datetime_value(b, unit):
    """the same value by datetime arithmetic, for a VALID string of year >= 1 -- the cross-check of the reference.  Only the
    calendar is datetime's: the fields are cut out by position, as the grammar fixes them"""
    b = bytes(b)
    text = b.decode("ascii")
    moment = datetime.datetime(int(text[0:4]), int(text[5:7]), int(text[8:10]), int(text[11:13]), int(text[14:16]), int(text[17:19]))
    rest = text[19:]
    fraction = ""
    if rest.startswith("."):
        fraction = rest[1:].rstrip("Zz").split("+")[0].split("-")[0]
        rest = rest[1 + len(fraction):]
    offset = 0
    if rest[:1] in ("+", "-"):
        offset = (int(rest[1:3]) * 3600 + int(rest[4:6]) * 60) * (-1 if rest[0] == "-" else 1)
    delta = moment - datetime.datetime(1970, 1, 1)
    secs = delta.days * 86400 + delta.seconds - offset
    k = UNIT_DIGITS[unit]
    return secs * 10 ** k + int((fraction + "0" * 9)[:k] or "0")


def reference_cells(fields, get, live, sb):
    """get(column, row) -> (type byte, value word or anything for a cell that is no string) -> Ref"""
    sb = bytes(np.asarray(sb, dtype=np.uint8).tobytes())
    data, validity, records = [], [], []
    memo = {}
    for field in fields:
        column, unit, flags = field[0], field[1], tuple(field[2:])
        cells = []
        for r in range(live):
            ty, word = get(column, r)
            key = (unit, flags, int(ty), int(word) if int(ty) == STRING else 0)
            if key not in memo:
                memo[key] = cell(unit, flags, ty, word, sb)
            cells.append(memo[key])
        data.append([c[0] for c in cells])
        validity.append(pack_bits([c[1] for c in cells]))
        records.append((live,) + tuple(sum(c[j] for c in cells) for j in range(1, 6)))
    return Ref(live, data, validity, records)


def reference_from_cells(fields, want, live):
    """the same from the cells of tests/select_common.expected_columns / explode_common.expected_explode: want[column][row] =
    (type byte, payload), a string's payload its unescaped bytes"""
    data, validity, records = [], [], []
    for field in fields:
        cells = [cell_of_bytes(field[1], tuple(field[2:]), *want[field[0]][r]) for r in range(live)]
        data.append([c[0] for c in cells])
        validity.append(pack_bits([c[1] for c in cells]))
        records.append((live,) + tuple(sum(c[j] for c in cells) for j in range(1, 6)))
    return Ref(live, data, validity, records)


def reference(case):
    t, v = case.types.tolist(), case.values.tolist()
    return reference_cells(case.fields, lambda c, r: (t[c][r], v[c][r]), live_rows(case), case.sb)


def out_buffers(case, data=True, validity=True):
    return F.out_buffers(case, RECORD_WORDS, data, validity)


# ---------------------------------------------------------------------------------------------------------------------
# builders of synthetic column sets.  A cell is bytes (a string cell with these bytes) or (type byte, value word).
# ---------------------------------------------------------------------------------------------------------------------
FILLER = np.frombuffer(b"0123456789-:TZ+. \xb0\x00\"", dtype=np.uint8)  # what lies between the strings looks like their neighbours


def make_case(name, fields, columns, n_rows=None, row_count=None, slack=0, pad=3, rng=None):
    """columns: per column its cells.  The strings go into one buffer, the first at offset 0 and the last ending at the buffer's
    last byte, 0 to 9 FILLER bytes between two so that every alignment occurs; the `pad` cells between n_rows and the stride are
    string cells with WILD value words -- a row that is not live must not be looked at.  slack: output strides above the minimum"""
    rng = np.random.default_rng(len(name)) if rng is None else rng
    n = max(len(c) for c in columns) if n_rows is None else n_rows
    stride = n + pad
    t = np.full((len(columns), stride), STRING, dtype=np.uint8)
    v = np.array(WILD, dtype=np.uint64)[rng.integers(0, len(WILD), size=(len(columns), stride))]
    parts, at = [], 0
    where = [(c, r) for c, col in enumerate(columns) for r, x in enumerate(col) if isinstance(x, (bytes, bytearray))]
    for k, (c, r) in enumerate(where):
        text = bytes(columns[c][r])
        if k:
            gap = FILLER[rng.integers(0, FILLER.size, size=int(rng.integers(0, 10)))].tobytes()
            parts.append(gap)
            at += len(gap)
        v[c, r] = (len(text) << 32) | at
        parts.append(text)
        at += len(text)
    for c, col in enumerate(columns):
        assert len(col) <= n
        for r, x in enumerate(col):
            if not isinstance(x, (bytes, bytearray)):
                t[c, r], v[c, r] = x[0], x[1] & MASK
        for r in range(len(col), n):
            t[c, r], v[c, r] = MISSING, WILD[r % len(WILD)]
    sb = np.frombuffer(b"".join(parts) or b"\x00", dtype=np.uint8).copy()
    return Case(name, list(fields), t, v, sb, n, row_count, *F.strides(n, slack))


EVERY_FIELD = [(0, unit) + flag for unit in ("s", "ms", "us", "ns") for flag in ((), ("naive_utc",))]
CANONICAL = b"2024-02-29T23:59:58.123456789+05:30"  # 35 bytes: every part of the grammar at its longest

NANO_EDGES = [b"2262-04-11T23:47:16.854775807Z", b"2262-04-11T23:47:16.854775808Z", b"1677-09-21T00:12:43.145224192Z", b"1677-09-21T00:12:43.145224191Z"]
NAMED = NANO_EDGES + [
    b"2015-01-01T15:00:00Z", b"2015-01-01t15:00:00z", b"2015-01-01 15:00:00Z", b"2015-01-01T15:00:00+00:00", b"2015-01-01T15:00:00-00:00",
    b"2015-01-01T15:00:00+00:01", b"2015-01-01T15:00:00-23:59", b"2015-01-01T15:00:00+23:59", b"2015-01-01T15:00:00+05:30",
    # fractions of 1, 3, 6 and 9 digits, above and below the epoch: the floor and n_inexact
    b"2015-01-01T15:00:00.5Z", b"2015-01-01T15:00:00.125Z", b"2015-01-01T15:00:00.125000Z", b"2015-01-01T15:00:00.000001Z", b"2015-01-01T15:00:00.123456789Z",
    b"2015-01-01T15:00:00.000000001Z", b"2015-01-01T15:00:00.100000000Z", b"2015-01-01T15:00:00.000Z",
    b"1969-12-31T23:59:59.5Z", b"1969-12-31T23:59:59.999Z", b"1969-12-31T23:59:59.999999Z", b"1969-12-31T23:59:59.999999999Z", b"1969-12-31T23:59:59.000000001+00:00",
    b"1970-01-01T00:00:00Z", b"1969-12-31T23:59:59Z", b"1970-01-01T00:00:00.000000000-00:00",
    b"0000-01-01T00:00:00Z", b"9999-12-31T23:59:59.999999999-23:59", b"0000-01-01T00:00:00+23:59", b"0000-02-29T12:00:00Z", b"0001-01-01T00:00:00Z",
    # the calendar
    b"2015-01-00T00:00:00Z", b"2015-01-32T00:00:00Z", b"2015-04-31T00:00:00Z", b"2015-04-30T00:00:00Z", b"2015-01-31T00:00:00Z", b"2015-12-31T00:00:00Z",
    b"1900-02-29T00:00:00Z", b"2000-02-29T00:00:00Z", b"2023-02-29T00:00:00Z", b"2024-02-29T00:00:00Z", b"0000-02-29T00:00:00Z", b"2100-02-29T00:00:00Z",
    b"1900-02-28T00:00:00Z", b"2015-00-10T00:00:00Z", b"2015-13-10T00:00:00Z", b"2015-01-01T24:00:00Z", b"2015-01-01T23:60:00Z", b"2015-01-01T23:59:60Z",
    b"2015-01-01T23:59:59Z", b"2015-01-01T00:00:00+24:00", b"2015-01-01T00:00:00+00:60", b"2015-01-01T00:00:00-24:00",
    # shapes: lengths 18, 19, 20, 35 and 36, a 10-digit fraction, '.' without a digit, a trailing byte, a leading '+', no zone
    b"2015-01-01T15:00:0Z", b"2015-01-01T15:00:00", b"2015-01-01T15:00:00Z", CANONICAL, CANONICAL + b"0", b"2015-01-01T15:00:00.1234567890Z",
    b"2015-01-01T15:00:00.Z", b"2015-01-01T15:00:00.", b"2015-01-01T15:00:00.+01:00", b"2015-01-01T15:00:00Z ", b"2015-01-01T15:00:00ZZ", b"+2015-01-01T15:00:00Z",
    b"2015-01-01T15:00:00.123456789", b"2015-01-01T15:00:00.5", b"2015-01-01", b"2015-01-01T", b"", b"2015-01-01T15:00:00+01:0", b"2015-01-01T15:00:00+0100Z",
    b"2015-01-01T15:00:00+01:000", b"2015-01-01T15:00:00 01:00", b"2015-01-01T15:00:00.1234567890", b"2015-01-01T15:00:00.12345678901234Z",
    b"2015-01-01T15:00:00,5Z", b"2015-01-01TT15:00:00Z", b"2015-01-01  15:00:00Z", b"2015-1-1T15:00:00.000Z", b"Sun Aug 31 00:29:15 +0000 2014",
]


def named_case():
    """every named string in one column under every unit with and without the flag"""
    return make_case("named strings", EVERY_FIELD, [list(NAMED)], slack=1)


def replaced_strings():
    return [CANONICAL[:at] + bytes([c]) + CANONICAL[at + 1:] for at in range(len(CANONICAL)) for c in (0x2F, 0x3A, 0xB0)]


def replaced_case():
    """from the canonical 35-byte string every position in turn replaced by '/', by ':' (the bytes next to the digits) and by
    0xB0 (a digit with its top bit set: a signed-char slip)"""
    return make_case("every position replaced", [(0, "ns"), (0, "s", "naive_utc")], [replaced_strings()])


def type_table_case():
    """every cell type under the field, wild value words in all cells that are no strings, and three strings among them"""
    cells = [(ty, WILD[k % len(WILD)]) for k, ty in enumerate(ALL_TYPES) if ty != STRING] + [(LONG, 1420124400), (DOUBLE, 0x41D5A9364C000000)]
    cells += [b"2015-01-01T15:00:00Z", b"not a time at all...", b"2015-01-01T15:00:00.25+01:00"]
    return make_case("every type", EVERY_FIELD, [cells], slack=0)


def last_bytes_case():
    """string cells whose value words point at the LAST bytes of the string buffer: strings that end with it, and cells of
    lengths the grammar cannot have -- with offsets that reach to the end and past it, which must not be followed"""
    texts = [b"2015-01-01T15:00:00Z", b"2015-01-01T15:00:00.123456789+05:30", b"2015-01-01T15:00:00", b"2015-01-01T15:00:00.5Z"]
    cases = []
    for k, last in enumerate(texts):
        col = [texts[(k + 1) % 4], (LONG, 5), last]
        case = make_case("the last bytes of the buffer %d" % k, EVERY_FIELD[2 * (k % 4):2 * (k % 4) + 2], [col], pad=0)
        size = case.sb.size
        assert int(case.values[0, 2]) == (len(last) << 32) | (size - len(last))
        extra_t = np.full((1, 8), STRING, dtype=np.uint8)
        extra_v = np.array([[(36 << 32) | (size - 5), (18 << 32) | (size - 18), (0xFFFFFFFF << 32) | (size - 1), (5 << 32) | 0xFFFFFFF0,
                             (36 << 32) | size, (0 << 32) | size, (1 << 63) | (size - 1), (len(last) << 32) | (size - len(last))]], dtype=np.uint64)
        t, v = np.concatenate([case.types, extra_t], axis=1), np.concatenate([case.values, extra_v], axis=1)
        n = t.shape[1]
        cases.append(case._replace(types=t, values=v, n_rows=n, data_stride=n, validity_stride=(n + 63) // 64))
    return cases


# ---- seeded random cells ----
_SEPS, _ZONES = (b"T", b"T", b"t", b" "), (b"Z", b"Z", b"z", b"+00:00", b"-00:00", b"+05:30", b"-08:00", b"+23:59", b"-23:59", b"+00:01", b"")
_YEARS = (0, 1, 1600, 1677, 1678, 1900, 1969, 1970, 1999, 2000, 2015, 2023, 2024, 2100, 2262, 2263, 9999)


def random_timestamp(rng):
    """a string that is mostly well-formed: days up to 31 in every month, hours up to 24, 0 to 10 digits of fraction, one zone in
    eleven absent -- the reference says which"""
    y = int(_YEARS[rng.integers(0, len(_YEARS))]) if rng.integers(0, 3) else int(rng.integers(0, 10000))
    m, d = int(rng.integers(1, 13)), int(rng.integers(1, 32)) if rng.integers(0, 4) == 0 else int(rng.integers(1, 29))
    hh, mi, ss = int(rng.integers(0, 25)) if rng.integers(0, 8) == 0 else int(rng.integers(0, 24)), int(rng.integers(0, 60)), int(rng.integers(0, 60))
    nd = int((0, 0, 0, 1, 3, 3, 6, 6, 9, 9, 2, 7, 10)[rng.integers(0, 13)])
    frac = b"." + b"".join(b"%d" % int(rng.integers(0, 10)) for _ in range(nd)) if nd else b""
    if nd and rng.integers(0, 3) == 0:
        frac = b"." + b"0" * nd
    return b"%04d-%02d-%02d%s%02d:%02d:%02d%s%s" % (y, m, d, _SEPS[rng.integers(0, 4)], hh, mi, ss, frac, _ZONES[rng.integers(0, len(_ZONES))])


def mutated(rng, text):
    kind = int(rng.integers(0, 5))
    if kind == 0 and text:
        at = int(rng.integers(0, len(text)))
        pool = b"/:09TZz+-. \xb0\x00"
        return text[:at] + bytes([pool[int(rng.integers(0, len(pool)))]]) + text[at + 1:]
    if kind == 1:
        return text[:int(rng.integers(0, len(text) + 1))]
    if kind == 2:
        return text + bytes([b"Z0 +"[int(rng.integers(0, 4))]])
    if kind == 3 and text:
        at = int(rng.integers(0, len(text)))
        return text[:at] + text[at + 1:]
    return b"x" * int(rng.integers(0, 50))


def random_cells(rng, n, p=(0.5, 0.2, 0.15, 0.15)):
    """n cells: a (mostly) well-formed string, a mutated one, a cell of another type, MISSING / null"""
    others = [ty for ty in ALL_TYPES if ty not in (STRING, MISSING, NULL)]
    cells = []
    for kind in rng.choice(4, size=n, p=p):
        if kind == 0:
            cells.append(random_timestamp(rng))
        elif kind == 1:
            cells.append(mutated(rng, random_timestamp(rng)))
        elif kind == 2:
            cells.append((others[rng.integers(0, len(others))], WILD[rng.integers(0, len(WILD))]))
        else:
            cells.append(((MISSING, NULL)[rng.integers(0, 2)], WILD[rng.integers(0, len(WILD))]))
    return cells


ROW_COUNTS = (0, 1, 63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024, 1025, 2049)
MIXED_FIELDS = [(0, "us"), (1, "ns", "naive_utc"), (2, "s"), (1, "ms")]


def row_count_cases(n):
    rng = np.random.default_rng(1000 + n)
    columns = [random_cells(rng, n) for _ in range(3)]
    base = make_case("%d rows" % n, MIXED_FIELDS, columns, n_rows=n, pad=7, rng=rng)
    return [base._replace(name="%d rows, row count %s, strides %s" % (n, rc, "above the minimum" if k % 2 else "at the minimum"), row_count=rc,
                          data_stride=F.strides(n, k % 2)[0], validity_stride=F.strides(n, k % 2)[1]) for k, rc in enumerate(live_counts(n))]


def schema_cases():
    """1 field and 64 fields, one column under every unit, fields in descending column order"""
    rng = np.random.default_rng(4000)
    n = 150
    columns = [random_cells(rng, n) for _ in range(5)]
    kinds = [("s",), ("ms", "naive_utc"), ("us",), ("ns", "naive_utc"), ("ns",)]
    make = lambda name, fields, rc, slack: make_case(name, fields, columns, n_rows=n, row_count=rc, slack=slack, pad=11, rng=np.random.default_rng(4001))
    return [make("one field", [(4, "us")], None, 0), make("64 fields", [((7 * k) % 5,) + kinds[k % 5] for k in range(64)], None, 1),
            make("one column under every unit", [(2, u) for u in ("s", "ms", "us", "ns")], n - 3, 0),
            make("descending columns", [(c,) + kinds[c] for c in (4, 3, 2, 1, 0)], None, 1)]


def type_shift_case():
    rng = np.random.default_rng(4100)
    return make_case("type shifts", MIXED_FIELDS, [random_cells(rng, 200) for _ in range(3)], n_rows=200, row_count=197, rng=rng)


def fuzz_case(seed, max_rows=300):
    """random cells in 1 to 4 columns under a random schema of 1 to 6 fields; one case in two takes its rows from a row count"""
    rng = np.random.default_rng(seed)
    n_cols, n = int(rng.integers(1, 5)), int(rng.integers(1, max_rows + 1))
    mixes = [(0.5, 0.2, 0.15, 0.15), (0.8, 0.1, 0.05, 0.05), (0.25, 0.25, 0.25, 0.25), (0.1, 0.6, 0.2, 0.1)]
    columns = [random_cells(rng, n, mixes[int(rng.integers(0, 4))]) for _ in range(n_cols)]
    kinds = [(u,) + f for u in ("s", "ms", "us", "ns") for f in ((), ("naive_utc",))]
    fields = [(int(rng.integers(0, n_cols)),) + kinds[int(rng.integers(0, 8))] for _ in range(int(rng.integers(1, 7)))]
    rc = int(rng.integers(0, n + 4)) if seed % 2 else None
    return make_case("fuzz case %d (%d columns, %d rows, %d fields, row count %s)" % (seed, n_cols, n, len(fields), rc), fields, columns, n_rows=n,
                     row_count=rc, slack=seed % 3 == 0, pad=int(rng.integers(0, 8)), rng=rng)


FUZZ_SEEDS = range(7000, 7200)


def past_one_grid_trip_case():
    """2 fields x 70,001 rows: 274 chunks of 256 rows per field.  The strings are drawn from 500 and shared, so that the case is cheap to make"""
    n = 70001
    rng = np.random.default_rng(31)
    pool = random_cells(rng, 500)
    small = make_case("pool", [(0, "us")], [pool], pad=0, rng=rng)
    pick = rng.integers(0, 500, size=n + 3)
    t, v = small.types[:, pick].copy(), small.values[:, pick].copy()
    return Case("%d rows" % n, [(0, "us"), (0, "ns", "naive_utc")], t, v, small.sb, n, None, n, (n + 63) // 64)
