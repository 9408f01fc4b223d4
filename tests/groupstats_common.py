"""What sjmi_group_stats_device must give, from Python and numpy alone: per key Counters of the three classes, exact int sums, min /
max, math.fsum of the doubles; IEEE totalOrder on the zeros (-0.0 < +0.0); a NaN 'd' cell goes to n_nan and nowhere else; a row
whose index is outside [0, n_keys) to n_out_of_range.  Shares no code with the product.  Used by the host simulation's tests, the
GPU tests and tools/bench_groupstats.py.

The tolerance of sum_double is derived, not measured: any order of n floating-point additions satisfies |computed - sum x| <=
gamma(n - 1) * sum|x|, gamma(k) = k u / (1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2) -- partial
sums per workgroup and their flush included, because adding an exact zero is exact.  Against math.fsum (the exact sum rounded
once, another u * |sum| <= u * sum|x|) the tests require |got - fsum| <= gamma(n) * sum|x|, n = the key's n_double."""
import math
import struct

import numpy as np

from tests.members_common import pack_bits

WORDS = 10
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
POISON = (0x7FF8DEADBEEF0001, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x7FF0000000000000, 0x0123456789ABCDEF)  # behind non-numbers
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FFFFFFFFFFFFFFF, 0xFFF0000000000001)
OTHER_TYPES = b'"tfn[{\0x'
SCALES = (2.0 ** -1074, 2.0 ** -1040, 1.0, 2.0 ** 970)  # of value_column's kind "scaled"
SCALE_IDS = ("2^-1074", "2^-1040", "1", "2^970")
U = 2.0 ** -53


def gamma(k):
    return k * U / (1 - k * U)


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", int(bits)))[0]


def is_nan_bits(b):
    return (int(b) & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000


# ---- generators ------------------------------------------------------------------------------------------------------------------
def keys_column(n_rows, n_keys, seed, kind="uniform"):
    """-> (indices int32, validity words uint64, bits bool): uniform = every index in range; wild = a quarter of the indices out
    of range (negatives, n_keys, INT32_MIN, INT32_MAX); skewed = wild, with half the rows in three keys; one_bin = every row in
    key n_keys // 2.  80 % of the rows are valid."""
    rng = np.random.default_rng(seed)
    if kind == "one_bin":
        indices = np.full(n_rows, n_keys // 2, dtype=np.int32)
    else:
        indices = rng.integers(0, max(n_keys, 1), n_rows).astype(np.int32)
        if kind == "skewed":
            hot = rng.random(n_rows) < 0.5
            indices[hot] = rng.choice(np.array([0, n_keys // 3, n_keys - 1], dtype=np.int32), int(hot.sum()))
        if kind in ("wild", "skewed"):
            wild = np.array([-1, n_keys, INT32_MIN, INT32_MAX, n_keys + 7, -n_keys - 1], dtype=np.int64).astype(np.int32)
            hit = rng.random(n_rows) < 0.25
            indices[hit] = rng.choice(wild, int(hit.sum()))
    bits = rng.random(n_rows) < 0.8
    return indices, pack_bits(bits), bits


def value_column(n_rows, seed, kind="mixed", scale=1.0):
    """-> (types uint8, values uint64), ONE (type, value) column.
    mixed: 40 % 'l' cells -- small ones, the whole int64 range, INT64_MIN and INT64_MAX, and a run of 70 of each --, 30 % 'd' cells of
        both signs with magnitudes from 1e-300 to 1e100 and +-0.0 among them, 30 % other type bytes whose value words are POISON;
    exact: the same classes, the doubles integers below 2^20 in magnitude (every partial sum of fewer than 2^20 of them is exact);
    scaled: exact, every double times `scale`, a power of two: m * scale with |m| < 2^20.  While m * scale is representable for every
        |m| < 2^50 -- from 2^-1074, where every cell and every sum is subnormal, up to 2^970 -- every partial sum of fewer than 2^30
        cells is exact in any order, so sum_double must be EQUAL to math.fsum;
    all_long: only 'l', the whole range;  half_double: 'l' and 'd' half and half."""
    rng = np.random.default_rng(seed ^ 0x5EED)
    pick = rng.random(n_rows)
    if kind == "all_long":
        is_l, is_d = np.ones(n_rows, dtype=bool), np.zeros(n_rows, dtype=bool)
    elif kind == "half_double":
        is_l = pick < 0.5
        is_d = ~is_l
    else:
        is_l, is_d = pick < 0.4, (pick >= 0.4) & (pick < 0.7)
    types = rng.choice(np.frombuffer(OTHER_TYPES, dtype=np.uint8), n_rows)
    types[is_l], types[is_d] = ord("l"), ord("d")
    values = rng.choice(np.array(POISON, dtype=np.uint64), n_rows)
    # the longs
    longs = rng.integers(INT64_MIN, INT64_MAX, n_rows, dtype=np.int64, endpoint=True)
    small = rng.random(n_rows) < 0.5
    longs[small] = rng.integers(-1000, 1000, int(small.sum()))
    edge = rng.random(n_rows) < 0.05
    longs[edge] = rng.choice(np.array([INT64_MIN, INT64_MAX], dtype=np.int64), int(edge.sum()))
    if kind in ("exact", "scaled"):
        longs = rng.integers(-(1 << 40), 1 << 40, n_rows, dtype=np.int64)
    if n_rows >= 400 and kind == "mixed":  # runs of the extremes: more of them than a wave has lanes
        types[100:170], longs[100:170] = ord("l"), INT64_MAX
        types[200:270], longs[200:270] = ord("l"), INT64_MIN
        is_l, is_d = types == ord("l"), types == ord("d")
    values[is_l] = longs[is_l].view(np.uint64)
    # the doubles
    if kind in ("exact", "scaled"):
        doubles = rng.integers(-(1 << 20) + 1, 1 << 20, n_rows).astype(np.float64)
        if kind == "scaled":
            power = int(math.log2(scale))  # (ldexp: exact, whatever floating-point mode numpy's multiply runs in)
            doubles = np.array([math.ldexp(m, power) for m in doubles.tolist()], dtype=np.float64)
    else:
        doubles = np.where(rng.random(n_rows) < 0.5, -1.0, 1.0) * rng.random(n_rows) * 10.0 ** rng.integers(-300, 101, n_rows)
        zero = rng.random(n_rows) < 0.1
        doubles[zero] = rng.choice(np.array([0.0, -0.0]), int(zero.sum()))
    values[is_d] = doubles[is_d].view(np.uint64)
    return types, values


def infinity_case():
    """a hand-made column: key 0 only +inf among finite doubles, key 1 both infinities, key 2 only -inf, key 3 finite only, key 4
    nothing -> (indices, types, values, n_keys)"""
    inf = float("inf")
    rows = [(0, 1.5), (0, inf), (0, -2.0), (0, inf), (1, inf), (1, 3.0), (1, -inf), (2, -inf), (2, -inf), (2, 1e300), (3, 1e300), (3, -0.0), (3, 2.5)] * 67
    indices = np.array([k for k, _ in rows], dtype=np.int32)
    values = np.array([x for _, x in rows], dtype=np.float64).view(np.uint64)
    return indices, np.full(indices.size, ord("d"), dtype=np.uint8), values, 5


def nan_case(n_rows, n_keys, seed):
    """a mixed column in which a fifth of the rows are 'd' cells holding a NaN of NAN_BITS -> (indices, words, bits, types, values)"""
    indices, words, bits = keys_column(n_rows, n_keys, seed, "wild")
    types, values = value_column(n_rows, seed, "mixed")
    rng = np.random.default_rng(seed + 99)
    hit = rng.random(n_rows) < 0.2
    types[hit] = ord("d")
    values[hit] = rng.choice(np.array(NAN_BITS, dtype=np.uint64), int(hit.sum()))
    return indices, words, bits, types, values


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _min_max_total_order(xs):
    """min / max of non-NaN floats under totalOrder: among zeros -0.0 is the smaller"""
    lo, hi = min(xs), max(xs)
    if lo == 0 and any(x == 0 and math.copysign(1, x) < 0 for x in xs):
        lo = -0.0
    elif lo == 0:
        lo = 0.0
    if hi == 0 and any(x == 0 and math.copysign(1, x) > 0 for x in xs):
        hi = 0.0
    elif hi == 0:
        hi = -0.0
    return lo, hi


def _sum_doubles(xs):
    """-> (the reference sum, sum|x|): math.fsum; with infinities what IEEE addition gives in any order (inf, or NaN for both)"""
    pos, neg = any(x == math.inf for x in xs), any(x == -math.inf for x in xs)
    if pos or neg:
        return (math.nan if pos and neg else math.inf if pos else -math.inf), math.inf
    return math.fsum(xs), math.fsum(abs(x) for x in xs)


def _key_entry(longs, doubles, n_other):
    lo, hi = _min_max_total_order(doubles) if doubles else (None, None)
    total, abs_total = _sum_doubles(doubles)
    return {"n_long": len(longs), "n_double": len(doubles), "n_other": n_other, "sum_long": sum(longs), "sum_double": total, "abs_double": abs_total,
            "min_long": min(longs) if longs else None, "max_long": max(longs) if longs else None, "min_double": lo, "max_double": hi}


def expected(indices, validity_bits, types, values, n_keys, live):
    """the plain loop -> ([dict per key], (n_grouped, n_out_of_range, n_nan)).  values: uint64 words"""
    longs, doubles, others = [[] for _ in range(n_keys)], [[] for _ in range(n_keys)], [0] * n_keys
    grouped = outside = nan = 0
    for r in range(live):
        if validity_bits is not None and not validity_bits[r]:
            continue
        ix = int(indices[r])
        if not 0 <= ix < n_keys:
            outside += 1
            continue
        t, v = int(types[r]), int(values[r])
        if t == ord("l"):
            longs[ix].append(v - (1 << 64) if v >> 63 else v)
        elif t == ord("d"):
            if is_nan_bits(v):
                nan += 1
                continue
            doubles[ix].append(double_of(v))
        else:
            others[ix] += 1
        grouped += 1
    return [_key_entry(longs[k], doubles[k], others[k]) for k in range(n_keys)], (grouped, outside, nan)


def expected_large(indices, validity_bits, types, values, n_keys, live):
    """expected() for columns of a million rows: the rows sorted by key with numpy, then the same Python sums, minima and maxima
    per key (tests/test_host_groupstats.py holds the two against each other)"""
    ix = np.asarray(indices[:live], dtype=np.int64)
    t, v = np.asarray(types[:live], dtype=np.uint8), np.asarray(values[:live], dtype=np.uint64)
    valid = np.ones(live, dtype=bool) if validity_bits is None else np.asarray(validity_bits[:live], dtype=bool)
    inside = valid & (ix >= 0) & (ix < n_keys)
    is_l, is_d = inside & (t == ord("l")), inside & (t == ord("d"))
    is_nan = is_d & ((v & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000))
    is_d &= ~is_nan
    n_other = np.bincount(ix[inside & ~is_l & ~is_d & ~is_nan], minlength=n_keys)

    def by_key(mask, column):
        order = np.argsort(ix[mask], kind="stable")
        keys, col = ix[mask][order], column[mask][order]
        cuts = np.searchsorted(keys, np.arange(n_keys + 1))
        return [col[cuts[k]:cuts[k + 1]].tolist() for k in range(n_keys)]

    longs, doubles = by_key(is_l, v.view(np.int64)), by_key(is_d, v.view(np.float64))
    out = [_key_entry(longs[k], doubles[k], int(n_other[k])) for k in range(n_keys)]
    return out, (int((inside & ~is_nan).sum()), int((valid & ~inside).sum()), int(is_nan.sum()))


# ---- comparing -------------------------------------------------------------------------------------------------------------------
def check_stats(stats, want, exact_sum=False, what=""):
    """stats: the call's words, uint64 [n_keys, 10], read here word by word.  Every word but sum_double must be EQUAL to the
    reference (doubles by their bits: -0.0 is not +0.0; the empty classes' minima and maxima are the contract's constants);
    sum_double within gamma(n_double) * sum|x| of math.fsum, equal to it with exact_sum (a column whose partial sums are all
    exact) and to the infinity or NaN that IEEE addition gives."""
    stats = np.asarray(stats).view(np.uint64).reshape(-1, WORDS)
    assert stats.shape[0] == len(want), what
    for k, w in enumerate(want):
        got = [int(x) for x in stats[k]]
        where = "%s key %d" % (what, k)
        assert got[:3] == [w["n_long"], w["n_double"], w["n_other"]], where
        total = ((got[4] - (1 << 64) if got[4] >> 63 else got[4]) << 64) + got[3]
        assert total == w["sum_long"], where
        signed = lambda x: x - (1 << 64) if x >> 63 else x
        assert signed(got[6]) == (INT64_MAX if w["min_long"] is None else w["min_long"]), where
        assert signed(got[7]) == (INT64_MIN if w["max_long"] is None else w["max_long"]), where
        assert got[8] == bits_of(math.inf if w["min_double"] is None else w["min_double"]), where
        assert got[9] == bits_of(-math.inf if w["max_double"] is None else w["max_double"]), where
        s, ref = double_of(got[5]), w["sum_double"]
        if math.isnan(ref):
            assert math.isnan(s), where
        elif math.isinf(ref) or exact_sum:
            assert s == ref, (where, s, ref)
        else:
            assert abs(s - ref) <= gamma(w["n_double"]) * w["abs_double"], (where, s, ref, w["n_double"], w["abs_double"])


def same_but_sum_double(a, b):
    """two runs' stats: every word but sum_double equal"""
    a, b = np.asarray(a).view(np.uint64).reshape(-1, WORDS), np.asarray(b).view(np.uint64).reshape(-1, WORDS)
    keep = [w for w in range(WORDS) if w != 5]
    return a.shape == b.shape and bool((a[:, keep] == b[:, keep]).all())
