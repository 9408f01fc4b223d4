"""What sjmi_sort_rows_device must give, from Python and numpy alone: every live position classified (candidate, NaN, other, null,
bad) with the classes and keys of tests/toprows_common.py, the candidates ordered by (value ascending -- descending under the
flag --, position ascending), then the NaN, OTHER and NULL + BAD positions by ascending position, and the record of nine words.
Position i stands for source row rows_in[i] (or i); an entry at or above n_source_rows is BAD.  Shares no code with the product.
Used by the host simulation's tests, the GPU tests and tools/bench_sortrows.py.

Everything is an integer and exact: there is no tolerance anywhere."""
import math

import numpy as np

from tests.toprows_common import DOUBLE, LONG, _order_key, bits_of, classify, double_of  # noqa: F401 (LONG, DOUBLE: the kinds)

DESCENDING, BAD_ROW, RESULT_WORDS = 1, 1, 9
BAD_ENTRIES = ((1 << 32) - 1, 1 << 63)  # with n_source_rows itself: the entries of rows_in that name no row


def n_digits(keys):
    """the 8-bit digit passes that the keys (uint64, the order keys of the candidates) need: ceil((msb(min ^ max) + 1) / 8)"""
    if keys.size == 0:
        return 0
    differ = int(keys.min()) ^ int(keys.max())
    return (differ.bit_length() + 7) // 8


def _source(rows_in, n_rows, live, n_source_rows):
    """-> (the source row of every live position as uint64, the mask of the BAD ones)"""
    live = min(int(live), int(n_rows))
    src = np.arange(live, dtype=np.uint64) if rows_in is None else np.asarray(rows_in[:live], dtype=np.uint64)
    return live, src, src >= np.uint64(n_source_rows)


def expected(key_types, validity_bits, key_values, rows_in, n_rows, live, kind, descending):
    """-> (rows uint64 [live]: the source row at every output place, record [9] of ints, positions int64 [live])"""
    n_source = len(key_values)
    live, src, bad = _source(rows_in, n_rows, live, n_source)
    good = np.nonzero(~bad)[0]
    at = src[good].astype(np.int64)
    # the classes of the source rows that the good positions name, by the reference of the top rows on the gathered column
    g_types = None if key_types is None else np.asarray(key_types)[at]
    g_valid = None if validity_bits is None else np.asarray(validity_bits)[at]
    g_values = np.asarray(key_values, dtype=np.uint64)[at]
    cand, bits, n_null, n_other, n_nan, n_inexact = classify(g_types, g_valid, g_values, good.size, kind)
    valid = np.ones(good.size, dtype=bool) if g_valid is None else np.asarray(g_valid, dtype=bool)
    if g_types is None:
        number, null = np.ones(good.size, dtype=bool), ~valid
    else:
        number = (g_types == ord("l")) | ((g_types == ord("d")) & (kind == DOUBLE))
        null = ~valid | (g_types == 0) | (g_types == ord("n"))
    nan = valid & number & ~cand  # (classify took the NaNs out of the candidates and counted them)
    other = ~cand & ~nan & ~null
    assert int(nan.sum()) == n_nan and int(null.sum()) == n_null and int(other.sum()) == n_other
    key = _order_key(bits[cand], kind)
    pos_c = good[cand]
    order = np.lexsort((pos_c, ~key if descending else key))  # (the last key is the primary one)
    tail = np.concatenate([np.nonzero(bad)[0], good[null]])
    tail.sort()
    positions = np.concatenate([pos_c[order], good[nan], good[other], tail]).astype(np.int64)
    n_bad = int(bad.sum())
    record = [live, int(cand.sum()), n_null, n_other, n_nan, n_inexact, n_bad, n_digits(key), BAD_ROW if n_bad else 0]
    return src[positions], record, positions


def expected_by_python_sort(key_types, validity_bits, key_values, rows_in, n_rows, live, kind, descending):
    """expected() by the plain loop and Python's sorted on (class, value, sign of zero, position) tuples: holds the numpy form"""
    n_source = len(key_values)
    live = min(int(live), int(n_rows))
    out, counts, lo, hi = [], {"null": 0, "other": 0, "nan": 0, "inexact": 0, "bad": 0, "cand": 0}, None, None
    sign = -1 if descending else 1
    for i in range(live):
        r = i if rows_in is None else int(rows_in[i])
        if r >= n_source:
            counts["bad"] += 1
            out.append((3, 0, 0, i, r))
            continue
        t = None if key_types is None else int(key_types[r])
        v = int(key_values[r])
        if validity_bits is not None and not validity_bits[r]:
            counts["null"] += 1
            out.append((3, 0, 0, i, r))
        elif t is not None and t in (0, ord("n")):
            counts["null"] += 1
            out.append((3, 0, 0, i, r))
        elif t is not None and not (t == ord("l") or (t == ord("d") and kind == DOUBLE)):
            counts["other"] += 1
            out.append((2, 0, 0, i, r))
        else:
            if kind == LONG:
                x, z, word = (v - (1 << 64) if v >> 63 else v), 0, v ^ (1 << 63)
            else:
                if t == ord("l"):
                    n = v - (1 << 64) if v >> 63 else v
                    x = float(n)
                    counts["inexact"] += int(x) != n
                else:
                    x = double_of(v)
                if math.isnan(x):
                    counts["nan"] += 1
                    out.append((1, 0, 0, i, r))
                    continue
                z, b = math.copysign(1, x), bits_of(x)
                word = (b ^ 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b ^ (1 << 63))
            counts["cand"] += 1
            word = word ^ 0xFFFFFFFFFFFFFFFF if descending else word
            lo, hi = (word, word) if lo is None else (min(lo, word), max(hi, word))
            out.append((0, sign * x, sign * z, i, r))
    ordered = sorted(out)
    passes = 0 if lo is None else ((lo ^ hi).bit_length() + 7) // 8
    record = [live, counts["cand"], counts["null"], counts["other"], counts["nan"], counts["inexact"], counts["bad"], passes,
              BAD_ROW if counts["bad"] else 0]
    return (np.array([e[4] for e in ordered], dtype=np.uint64), record, np.array([e[3] for e in ordered], dtype=np.int64))


def chain(keys, n_source_rows, rows_in=None, n_rows=None, live=None):
    """a sort by several keys, most significant first, as repeated expected() calls from the last key to the first ->
    (rows uint64 [live], the records in the order of `keys`).  keys: (key_types, validity_bits, key_values, kind, descending)"""
    n_rows = (n_source_rows if rows_in is None else len(rows_in)) if n_rows is None else n_rows
    live = n_rows if live is None else live
    rows, records = rows_in, []
    for key_types, validity_bits, key_values, kind, descending in reversed(keys):
        rows, record, _ = expected(key_types, validity_bits, key_values, rows, n_rows, live, kind, descending)
        records.append(record)
    return rows, records[::-1]
