"""What sjmi_top_rows_device must give, from Python and numpy alone: every live row classified (candidate, null, other, NaN), the
candidates ordered by (value descending -- ascending for the smallest --, row ascending), cut at k, and the record of nine words.
Doubles are ordered by IEEE totalOrder on the non-NaN values (-0.0 < +0.0); a long under the DOUBLE kind is converted with round
to nearest even first, and counted in n_inexact when that rounded.  Shares no code with the product.  Used by the host
simulation's tests, the GPU tests and tools/bench_toprows.py.

Everything is an integer and exact: there is no tolerance anywhere."""
import struct

import numpy as np

from tests.members_common import pack_bits

LONG, DOUBLE, SMALLEST, MAX_K, RESULT_WORDS = 1, 2, 1, 2048, 9
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SIGN = np.uint64(1 << 63)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
POISON = (0x7FF8DEADBEEF0001, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x7FF0000000000000, 0x0123456789ABCDEF)  # behind non-numbers
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001)
OTHER_TYPES = b'"tf[{x'  # OTHER under both kinds
NULL_TYPES = b"n\0"      # NULL: a JSON null, a MISSING cell
DIGIT_EDGES = (10, 11, 21, 22, 32, 33, 43, 44, 54, 55)


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


# ---- generators: each -> a uint64 array of value words --------------------------------------------------------------------------
def longs_full(n, seed):
    """int64 over the whole range, INT64_MIN and INT64_MAX among them (a twentieth of the rows, so they tie)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    edge = rng.random(n) < 0.05
    v[edge] = rng.choice(np.array([INT64_MIN, INT64_MAX], dtype=np.int64), int(edge.sum()))
    return v.view(np.uint64)


def counters(n, seed):
    """small counters 0 .. 10^4, half of them below 10: heavy ties"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 10001, n, dtype=np.int64)
    low = rng.random(n) < 0.5
    v[low] = rng.integers(0, 10, int(low.sum()))
    return v.view(np.uint64)


def doubles_wide(n, seed):
    """doubles of both signs from 1e-300 to 1e100, with both zeros, both infinities and denormals of both signs"""
    rng = np.random.default_rng(seed)
    d = np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.random(n) * 10.0 ** rng.integers(-300, 101, n)
    special = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4])
    hit = rng.random(n) < 0.15
    d[hit] = rng.choice(special, int(hit.sum()))
    return d.view(np.uint64)


def longs_above_2_53(n, seed):
    """longs around and above 2^53 in magnitude: half of them are not exact as doubles, and many round to the same double"""
    rng = np.random.default_rng(seed)
    v = (1 << 53) + rng.integers(-3, 40, n, dtype=np.int64)
    v[rng.random(n) < 0.3] *= -1
    far = rng.random(n) < 0.2
    v[far] = rng.choice(np.array([INT64_MAX, INT64_MIN, INT64_MAX - 1, (1 << 62) + 1], dtype=np.int64), int(far.sum()))
    return v.view(np.uint64)


def typed_column(n, seed, what):
    """ONE (types uint8, values uint64) key column, about 80 % of whose cells are numbers:
    longs / counters / equal: 'l' cells of longs_full() / counters() / the one value 7, a tenth 'd' cells;
    doubles: 'd' cells of doubles_wide(), a tenth 'l' cells of longs_above_2_53(), a twentieth NaNs of NAN_BITS;
    the rest OTHER_TYPES and NULL_TYPES over POISON words."""
    rng = np.random.default_rng(seed ^ 0x70B)
    pick = rng.random(n)
    types = rng.choice(np.frombuffer(OTHER_TYPES + NULL_TYPES, dtype=np.uint8), n)
    values = rng.choice(np.array(POISON, dtype=np.uint64), n)
    is_l, is_d = (pick < 0.7, (pick >= 0.7) & (pick < 0.8)) if what != "doubles" else ((pick >= 0.7) & (pick < 0.8), pick < 0.7)
    types[is_l], types[is_d] = ord("l"), ord("d")
    if what == "doubles":
        longs, dbl = longs_above_2_53(n, seed), doubles_wide(n, seed)
        nan = is_d & (rng.random(n) < 0.07)
        dbl[nan] = rng.choice(np.array(NAN_BITS, dtype=np.uint64), int(nan.sum()))
    else:
        longs = {"longs": longs_full, "counters": counters, "equal": lambda n, s: np.full(n, 7, dtype=np.uint64)}[what](n, seed)
        dbl = doubles_wide(n, seed)
    values[is_l], values[is_d] = longs[is_l], dbl[is_d]
    return types, values


def validity(n, seed, p=0.8):
    """-> (words uint64, bits bool)"""
    bits = np.random.default_rng(seed ^ 0xB175).random(n) < p
    return pack_bits(bits), bits


def carried(n_cols, n, stride, seed):
    """n_cols carried columns of `stride` cells, all cells distinct: (types uint8 [n_cols, stride], values uint64 [n_cols, stride])"""
    rng = np.random.default_rng(seed ^ 0xCA22)
    types = rng.integers(1, 255, (n_cols, stride), dtype=np.uint8)
    values = (np.arange(n_cols * stride, dtype=np.uint64).reshape(n_cols, stride) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(seed)
    return types, values


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _order_key(bits, kind):
    """value words -> unsigned keys with the order of the values: a long's sign bit flipped; a double's bits with the sign bit
    flipped when it is clear and all bits flipped when it is set (totalOrder)"""
    if kind == LONG:
        return bits ^ SIGN
    return np.where((bits >> np.uint64(63)) != 0, ~bits, bits ^ SIGN)


def classify(key_types, validity_bits, key_values, live, kind):
    """-> (candidate mask, the candidates' value words AS THE KIND (uint64 [live], 0 elsewhere), n_null, n_other, n_nan, n_inexact)"""
    v = np.asarray(key_values[:live], dtype=np.uint64)
    valid = np.ones(live, dtype=bool) if validity_bits is None else np.asarray(validity_bits[:live], dtype=bool)
    bits = np.zeros(live, dtype=np.uint64)
    n_inexact = 0
    if key_types is None:
        cand = valid.copy()
        bits[cand] = v[cand]
        null, other = ~valid, np.zeros(live, dtype=bool)
    else:
        t = np.asarray(key_types[:live], dtype=np.uint8)
        is_l, is_d = valid & (t == ord("l")), valid & (t == ord("d")) & (kind == DOUBLE)
        null = ~valid | (t == 0) | (t == ord("n"))
        cand = is_l | is_d
        other = ~null & ~cand
        bits[is_d] = v[is_d]
        if kind == LONG:
            bits[is_l] = v[is_l]
        else:
            longs = v[is_l].view(np.int64)
            as_double = longs.astype(np.float64)  # (round to nearest, ties to even)
            big = np.abs(longs.astype(np.float64)) >= 2.0 ** 53
            n_inexact = sum(1 for x, d in zip(longs[big].tolist(), as_double[big].tolist()) if int(d) != x)
            bits[is_l] = as_double.view(np.uint64)
    nan = np.zeros(live, dtype=bool)
    if kind == DOUBLE:
        nan = cand & ((bits & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000))
        cand &= ~nan
        bits[nan] = 0
    return cand, bits, int(null.sum()), int(other.sum()), int(nan.sum()), n_inexact


def expected(key_types, validity_bits, key_values, live, kind, largest, k):
    """-> (rows int64 [n_out] in rank order, record [9] of ints)"""
    live = min(int(live), len(key_values))
    cand, bits, n_null, n_other, n_nan, n_inexact = classify(key_types, validity_bits, key_values, live, kind)
    rows = np.nonzero(cand)[0]
    key = _order_key(bits[rows], kind)
    order = np.lexsort((rows, ~key if largest else key))  # (the last key is the primary one: ascending ~key = descending key)
    top = rows[order][:k]
    n_out = int(top.size)
    kth = int(bits[top[-1]]) if n_out else 0
    return top.astype(np.int64), [live, int(rows.size), n_null, n_other, n_nan, n_inexact, n_out, kth, 0]


def expected_by_python_sort(key_types, validity_bits, key_values, live, kind, largest, k):
    """expected() by the plain loop and Python's sort on (float or int, sign of zero, row) tuples: holds the numpy form in the tests"""
    import math
    live = min(int(live), len(key_values))
    out, counts = [], {"null": 0, "other": 0, "nan": 0, "inexact": 0}
    for r in range(live):
        t = None if key_types is None else int(key_types[r])
        v = int(key_values[r])
        if validity_bits is not None and not validity_bits[r]:
            counts["null"] += 1
        elif t is not None and t in (0, ord("n")):
            counts["null"] += 1
        elif t is not None and not (t == ord("l") or (t == ord("d") and kind == DOUBLE)):
            counts["other"] += 1
        elif kind == LONG:
            out.append(((v - (1 << 64) if v >> 63 else v, 0), r, v))
        else:
            if t == ord("l"):
                x = v - (1 << 64) if v >> 63 else v
                d = float(x)
                counts["inexact"] += int(d) != x
            else:
                d = double_of(v)
            if math.isnan(d):
                counts["nan"] += 1
            else:
                out.append(((d, math.copysign(1, d)), r, bits_of(d)))
    sign = -1 if largest else 1
    out.sort(key=lambda e: (sign * e[0][0], sign * e[0][1], e[1]))
    top = out[:k]
    return (np.array([e[1] for e in top], dtype=np.int64),
            [live, len(out), counts["null"], counts["other"], counts["nan"], counts["inexact"], len(top), top[-1][2] if top else 0, 0])
