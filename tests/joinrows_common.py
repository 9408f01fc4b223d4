"""What sjmi_join_rows_device must give, from Python and numpy alone: the left positions classified with classify() of
tests/toprows_common.py (kind LONG; an entry of rows_in at or above the source rows is BAD), the build set taken from the reference
of the sort (tests/sortrows_common.py: the right side's candidates by ascending key, equal keys by ascending position), a
dictionary from key to the ascending build places, the four hows, the record of nine words and the pair offsets.  A second form,
by np.searchsorted on the sorted build keys, holds the first.  Shares no code with the product.  Used by the host simulation's
tests, the GPU tests and tools/bench_joinrows.py.

Everything is an integer and exact: there is no tolerance anywhere."""
import numpy as np

from tests import sortrows_common as SO
from tests.toprows_common import LONG, classify

INNER, LEFT, SEMI, ANTI = 0, 1, 2, 3
HOWS = {"inner": INNER, "left": LEFT, "semi": SEMI, "anti": ANTI}
OVERFLOW, BAD_ROW, BAD_ORDER, RESULT_WORDS = 1, 2, 4, 9
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)


def left_classes(key_types, validity_bits, key_values, rows_in, n_left, live):
    """-> (live, src uint64 [live]: the source row of every live position, cand bool [live], keys int64 [live] (0 where no
    candidate), n_null, n_other, n_bad)"""
    live, src, bad = SO._source(rows_in, n_left, live, len(key_values))
    good = np.nonzero(~bad)[0]
    at = src[good].astype(np.int64)
    g_types = None if key_types is None else np.asarray(key_types)[at]
    g_valid = None if validity_bits is None else np.asarray(validity_bits)[at]
    c, bits, n_null, n_other, _, _ = classify(g_types, g_valid, np.asarray(key_values, dtype=np.uint64)[at], good.size, LONG)
    cand, keys = np.zeros(live, dtype=bool), np.zeros(live, dtype=np.int64)
    cand[good], keys[good] = c, bits.view(np.int64)
    return live, src, cand, keys, n_null, n_other, int(bad.sum())


def build_set(key_types, validity_bits, key_values, rows_in=None, n_right=None, live=None):
    """the sort of the right side as the caller makes it -> (order uint64 [n_right]: the sort's d_rows, entries at or behind its
    live positions 0, the sort's record [9], the build keys int64 [n_build])"""
    n_right = (len(key_values) if rows_in is None else len(rows_in)) if n_right is None else n_right
    live = n_right if live is None else min(live, n_right)
    rows, record, _ = SO.expected(key_types, validity_bits, key_values, rows_in, n_right, live, LONG, False)
    order = np.zeros(n_right, dtype=np.uint64)
    order[:live] = rows
    n_build = record[1]
    return order, record, np.asarray(key_values, dtype=np.uint64)[rows[:n_build].astype(np.int64)].view(np.int64)


def _counts(how, m):
    return m if how == INNER else np.maximum(m, 1) if how == LEFT else (m > 0).astype(np.int64) if how == SEMI else (m == 0).astype(np.int64)


def _finish(how, live, src, order, starts, m, e, n_build, n_null, n_other, n_bad, pair_capacity, n_right_bad=0, bad_order=False):
    offsets = np.zeros(live + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(e, dtype=np.uint64)
    n_pairs = int(offsets[-1])
    owner = np.repeat(np.arange(live, dtype=np.int64), e)
    t = np.arange(n_pairs, dtype=np.int64) - offsets[:-1].astype(np.int64)[owner]
    right = np.full(n_pairs, NO_ROW, dtype=np.uint64)
    hit = (m[owner] > 0) & (how != ANTI)
    right[hit] = order[(starts[owner] + t)[hit]]
    flags = (OVERFLOW if n_pairs > pair_capacity else 0) | (BAD_ROW if n_bad else 0) | (BAD_ORDER if bad_order else 0)
    record = [live, n_build, n_pairs, int((m > 0).sum()), n_null, n_other, n_bad, n_right_bad, flags]
    return src[owner], right, offsets, record


def expected(how, left, right_order, n_build, build_keys, pair_capacity=1 << 62):
    """left = left_classes(...); right_order / n_build / build_keys = build_set(...)'s.  By a dictionary from key to the ascending
    build places -> (left_rows uint64 [n_pairs], right_rows uint64 [n_pairs], offsets uint64 [live + 1], record [9] of ints): ALL
    pairs; the call writes the first min(n_pairs, pair_capacity) of them"""
    live, src, cand, keys, n_null, n_other, n_bad = left
    places = {}
    for p, k in enumerate(build_keys.tolist()):
        places.setdefault(k, []).append(p)
    assert all(v == list(range(v[0], v[0] + len(v))) for v in places.values()), "the build keys are not sorted"
    starts, m = np.zeros(live, dtype=np.int64), np.zeros(live, dtype=np.int64)
    for i in np.nonzero(cand)[0].tolist():
        run = places.get(int(keys[i]))
        if run:
            starts[i], m[i] = run[0], len(run)
    return _finish(how, live, src, right_order, starts, m, _counts(how, m), n_build, n_null, n_other, n_bad, pair_capacity)


def expected_by_searchsorted(how, left, right_order, n_build, build_keys, pair_capacity=1 << 62):
    """expected() by two np.searchsorted on the stably sorted build keys"""
    live, src, cand, keys, n_null, n_other, n_bad = left
    lo, hi = np.searchsorted(build_keys, keys, "left"), np.searchsorted(build_keys, keys, "right")
    m = np.where(cand, hi - lo, 0).astype(np.int64)
    return _finish(how, live, src, right_order, lo.astype(np.int64), m, _counts(how, m), n_build, n_null, n_other, n_bad, pair_capacity)


def carried_cells(carry, rows, n_source):
    """the cells of the carried columns (types [n_cols, stride], values [n_cols, stride]) at the expected rows: type byte 0 and
    value 0 for a BAD entry and for NO_ROW"""
    good = rows < np.uint64(n_source)
    at = np.where(good, rows, 0).astype(np.int64)
    return np.where(good, carry[0][:, at], 0).astype(np.uint8), np.where(good, carry[1][:, at], 0).astype(np.uint64)
