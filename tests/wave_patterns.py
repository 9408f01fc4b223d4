"""Directed wave patterns for the device-only lane-group forms: GsGroup::merge and CsGroup::merge (the combine of a wave's equal
keys / bins, csrc/groupstats.hip and csrc/census.hip), TrGroup::all (csrc/toprows.hip) and PaGroup::scan_max (csrc/parents.hip).
These members run on the GPU only -- the host simulation has a one-lane form of them --, so the columns here PLACE what a random
column meets by chance: exactly eight sets and a ninth, a ninth set with duplicates, a leader that is not lane 0, an extreme in a
non-leader lane, inactive lanes among the members.  Pure numpy, no GPU; tests/test_wave_patterns.py holds every builder to its
claims and tests/test_gpu_wave_combine.py runs the cases.

A WAVE is 64 consecutive rows; a pattern says lane -> local key (0 .. 63, or one of the OUT_* indices outside the keys), validity,
type byte and value word.  materialize() lays a case out as 18 waves -- two chunks of 1024 rows, the second one short:
    wave 0    the pattern                  the first wave of the first workgroup
    wave 9    the pattern again            a later wave of the first workgroup
    wave 16   the pattern again            the second workgroup
    wave 17   the pattern, 37 lanes of it  the last, partial wave (with a row count: all 64 lanes, the count ending inside it)
each with 64 keys of its own (wave i: keys 64 i ...), so that no two waves share a key; the waves between them hold nothing (validity
clear, index -1).  A case `every_wave` puts the pattern into all 18 waves with the SAME keys: one key across waves, workgroups and
the atomics.  Every key is below 512, so the same rows run at any n_keys >= 512.

A case's CLAIMS are about its pattern wave as the operator's merge sees it -- the sets of equal merge keys among the active
lanes, lowest lane first: their number, whether an active lane lies outside the first MERGE_ROUNDS sets, the lowest active lane
(the first leader), and where it is easy to say the lowest lane and the size of the largest set.  The merge key of group_stats
is the index, that of the census the bin index * 8 + class.

Doubles are integers below 2^20 in magnitude (every partial sum is exact, in any order), the infinities and the zeros; value words
behind a type byte that is no number are POISON, as in groupstats_common.value_column."""
import numpy as np

from tests.groupstats_common import INT32_MIN, INT64_MAX, INT64_MIN, NAN_BITS, OTHER_TYPES, POISON, bits_of
from tests.members_common import census_class, pack_bits

WAVE = 64
MERGE_ROUNDS = 8  # GS_MERGE_ROUNDS and CS_MERGE_ROUNDS (tests/test_wave_patterns.py reads them from the headers)
D_VALUES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 32, 63, 64)
LEADER_LANES = (0, 1, 31, 32, 62)
ROW_COUNT_LANES = (1, 32, 63)
PLACEMENTS = (0, 9, 16, 17)
N_WAVES, TAIL = 18, 37
MAX_KEY = 512  # every key of every case is below it
OUT_NEG, OUT_N_KEYS, OUT_INT32_MIN = -1, -2, -3  # local keys that become the indices -1, n_keys, INT32_MIN
INACTIVE_KINDS = ("invalid", "index_minus_1", "index_n_keys", "index_int32_min", "nan")
INACTIVE_WHERE = ("lane_0", "every_second", "all_but_one", "all")
CLASS_MIXES = ("other_leader_long_members", "long_leader_double_members", "all_three", "only_other", "only_long_in_highest",
               "only_double_in_highest")
VALUE_KINDS = ("min_last_max_middle", "low_halves_full", "all_negative", "zeros_negative_first", "zeros_positive_first", "plus_inf_in_a_member",
               "minus_inf_in_a_member", "both_infs_in_members")
CLASS_BYTES = b'ld"tn[{x'  # one type byte of every census class, in the order of the classes


class Pattern:
    """one wave: key int64 [64] (local, or OUT_*), valid bool [64], types uint8 [64], values uint64 [64]"""

    def __init__(self, key, valid=None, types=None, values=None):
        self.key = np.array(key, dtype=np.int64)
        assert self.key.shape == (WAVE,) and self.key.max() < WAVE
        self.valid = np.ones(WAVE, dtype=bool) if valid is None else np.array(valid, dtype=bool)
        t, v = default_cells()
        self.types = t if types is None else np.array(types, dtype=np.uint8)
        self.values = v if values is None else np.array(values, dtype=np.uint64)
        other = (self.types != ord("l")) & (self.types != ord("d"))
        self.values[other] = np.array(POISON, dtype=np.uint64)[np.arange(WAVE)[other] % len(POISON)]

    def copy(self):
        return Pattern(self.key, self.valid, self.types, self.values)


class Case:
    def __init__(self, name, pattern, tags, n_sets, leftover, leader, largest=None, every_wave=False, row_count_lane=None):
        self.name, self.pattern, self.tags = name, pattern, frozenset(tags)
        self.n_sets, self.leftover, self.leader, self.largest = n_sets, leftover, leader, largest
        self.every_wave, self.row_count_lane = every_wave, row_count_lane
        self.claim_wave = N_WAVES - 1 if row_count_lane is not None else 0  # the wave the claims are about

    def __repr__(self):
        return self.name


def default_cells():
    """the cells of a key pattern, the same in every case: about two fifths longs (small ones and the whole range), two fifths
    doubles, a fifth other type bytes, drawn once from a fixed seed"""
    rng = np.random.default_rng(64)
    cls = rng.integers(0, 5, WAVE)
    types = np.frombuffer(OTHER_TYPES, dtype=np.uint8)[np.arange(WAVE) % len(OTHER_TYPES)].copy()
    types[cls < 2], types[(cls >= 2) & (cls < 4)] = ord("l"), ord("d")
    longs = rng.integers(INT64_MIN, INT64_MAX, WAVE, dtype=np.int64, endpoint=True)
    small = rng.random(WAVE) < 0.5
    longs[small] = rng.integers(-1000, 1000, int(small.sum()))
    doubles = rng.integers(-(1 << 20) + 1, 1 << 20, WAVE).astype(np.float64)
    values = np.zeros(WAVE, dtype=np.uint64)
    values[types == ord("l")] = longs[types == ord("l")].view(np.uint64)
    values[types == ord("d")] = doubles[types == ord("d")].view(np.uint64)
    return types, values


# ---- the sets of a wave, as a merge takes them ---------------------------------------------------------------------------------
def sets_of(merge_keys, active):
    """-> the sets of equal merge keys among the active lanes, each a list of lanes, in the order of their lowest lanes"""
    sets, todo = [], [t for t in range(len(merge_keys)) if active[t]]
    while todo:
        k = merge_keys[todo[0]]
        sets.append([t for t in todo if merge_keys[t] == k])
        todo = [t for t in todo if merge_keys[t] != k]
    return sets


def describe(sets):
    """-> (n_sets, leftover, leader, largest) of sets_of()'s result, in the form of a case's claims"""
    left = any(len(s) for s in sets[MERGE_ROUNDS:])
    biggest = max(sets, key=lambda s: (len(s), -s[0])) if sets else None
    return len(sets), left, sets[0][0] if sets else None, (biggest[0], len(biggest)) if sets else None


# ---- key patterns ---------------------------------------------------------------------------------------------------------------
def round_robin(d):
    lanes = np.arange(WAVE)
    return Case("round_robin_%d" % d, Pattern(lanes % d), [("round_robin", d)], d, d > MERGE_ROUNDS, 0, (0, (WAVE + d - 1) // d))


def blocks(d):
    lanes = np.arange(WAVE)
    key = lanes * d // WAVE
    first = max(range(d), key=lambda k: (int((key == k).sum()), -k))
    return Case("blocks_%d" % d, Pattern(key), [("blocks", d)], d, d > MERGE_ROUNDS, 0, (int(np.argmax(key == first)), int((key == first).sum())))


def leader_position(lane, alone):
    """one multi-lane set whose lowest lane is `lane` (its members: lane + 5, lane + 20 and 61 where they lie above it; lane 62
    pairs with 63), every other lane a key of its own, so lane 63 is a one-lane set unless lane is 62.  alone: the lanes below
    `lane` are not valid, so the set is the FIRST one and its leader is not lane 0; otherwise the lanes in front of it use up the
    eight rounds and the set stays unmerged"""
    members = [lane] + ([63] if lane == 62 else sorted({m for m in (lane + 5, lane + 20, 61) if lane < m <= 62}))
    key = np.zeros(WAVE, dtype=np.int64)
    key[members] = 0
    rest = [t for t in range(WAVE) if t not in members]
    key[rest] = 1 + np.arange(len(rest))
    valid = np.ones(WAVE, dtype=bool)
    if alone:
        valid[:lane] = False
    n_sets = int(valid.sum()) - len(members) + 1
    return Case("leader_at_%d%s" % (lane, "_alone" if alone else ""), Pattern(key, valid), [("leader", lane, "alone" if alone else "behind")], n_sets,
                n_sets > MERGE_ROUNDS, lane if alone else 0, (lane, len(members)))


def late_big_set():
    """eight one-lane sets in lanes 0 .. 7 and one 56-lane set behind them: the big set is never merged"""
    key = np.concatenate([np.arange(8), np.full(56, 8)])
    return Case("eight_singles_then_56", Pattern(key), ["late_big_set"], 9, True, 0, (8, 56))


def early_big_set():
    """the reverse: a big set first, then eight singles, then one more pair -- 54 + 8 + 2 lanes: the pair is the tenth set"""
    key = np.concatenate([np.full(54, 0), 1 + np.arange(8), np.full(2, 9)])
    return Case("54_then_eight_singles_then_a_pair", Pattern(key), ["early_big_set"], 10, True, 0, (0, 54))


def one_key_across_waves(d):
    """every wave of both chunks, the SAME d keys round robin"""
    c = round_robin(d)
    return Case("every_wave_%d" % d, c.pattern, [("every_wave", d)], c.n_sets, c.leftover, c.leader, c.largest, every_wave=True)


# ---- inactive lanes -------------------------------------------------------------------------------------------------------------
def _knock_out(pattern, lanes, kind):
    p = pattern.copy()
    if kind == "invalid":
        p.valid[lanes] = False
    elif kind == "nan":
        p.types[lanes] = ord("d")
        p.values[lanes] = np.array(NAN_BITS, dtype=np.uint64)[np.array(lanes) % len(NAN_BITS)]
    else:
        p.key[lanes] = {"index_minus_1": OUT_NEG, "index_n_keys": OUT_N_KEYS, "index_int32_min": OUT_INT32_MIN}[kind]
    return p


def with_inactive(base, d, kind, where):
    """base: round_robin or blocks with d keys, each of which has a lane among 1, 3, 5, ...; the lanes `where` made inactive in
    the way `kind`"""
    lanes = {"lane_0": [0], "every_second": list(range(0, WAVE, 2)), "all_but_one": [t for t in range(WAVE) if t != 37], "all": list(range(WAVE))}[where]
    c = base(d)
    n_sets = {"lane_0": d, "every_second": d, "all_but_one": 1, "all": 0}[where]
    leader = {"lane_0": 1, "every_second": 1, "all_but_one": 37, "all": None}[where]
    return Case("%s_%s_%s" % (c.name, kind, where), _knock_out(c.pattern, lanes, kind), [("inactive", kind, where)], n_sets, n_sets > MERGE_ROUNDS, leader)


def with_row_count(base, d, lane):
    """the live rows end inside the last wave, in front of `lane`"""
    c = base(d)
    n_sets = len(set(c.pattern.key[:lane].tolist()))
    return Case("%s_row_count_%d" % (c.name, lane), c.pattern, [("row_count", lane)], n_sets, n_sets > MERGE_ROUNDS, 0, row_count_lane=lane)


# ---- the classes and the values inside one set (group_stats) -------------------------------------------------------------------
def _one_set(name, tag, lanes, types, values):
    """one key in `lanes`, the other lanes not valid"""
    valid = np.zeros(WAVE, dtype=bool)
    valid[lanes] = True
    t, v = np.full(WAVE, ord("n"), dtype=np.uint8), np.zeros(WAVE, dtype=np.uint64)
    t[lanes], v[lanes] = types, values
    return Case(name, Pattern(np.zeros(WAVE, dtype=np.int64), valid, t, v), [tag], 1, False, lanes[0], (lanes[0], len(lanes)))


def class_mix(mix, strided):
    """strided: the set is the lanes 1, 4, 7, ... (its leader is lane 1, inactive lanes lie among its members)"""
    lanes = list(range(1, WAVE, 3)) if strided else list(range(WAVE))
    n = len(lanes)
    at = np.arange(n)
    longs = ((at + 1) * 0x100000003 * np.where(at % 2, -1, 1)).astype(np.int64).view(np.uint64)
    doubles = ((at * 9973 % (1 << 20)) * np.where(at % 3, 1.0, -1.0)).astype(np.float64).view(np.uint64)
    others = np.frombuffer(OTHER_TYPES, dtype=np.uint8)[at % len(OTHER_TYPES)]
    L, D = ord("l"), ord("d")
    if mix == "other_leader_long_members":
        types = np.where(at == 0, others, L)
    elif mix == "long_leader_double_members":
        types = np.where(at == 0, L, D)
    elif mix == "all_three":
        types = np.where(at % 3 == 0, L, np.where(at % 3 == 1, D, others))
    elif mix == "only_other":
        types = others
    elif mix == "only_long_in_highest":
        types = np.where(at == n - 1, L, np.where(at % 2, D, others))
    else:
        assert mix == "only_double_in_highest"
        types = np.where(at == n - 1, D, np.where(at % 2, L, others))
    types = types.astype(np.uint8)
    values = np.where(types == L, longs, doubles)
    return _one_set("%s%s" % (mix, "_strided" if strided else ""), ("class", mix, "strided" if strided else "whole"), lanes, types, values)


def value_case(kind, strided):
    lanes = list(range(1, WAVE, 3)) if strided else list(range(WAVE))
    n = len(lanes)
    at = np.arange(n)
    as_bits = lambda doubles: np.array([bits_of(float(x)) for x in doubles], dtype=np.uint64)
    ints = ((at * 7919 + 11) % (1 << 20) * np.where(at % 2, -1.0, 1.0)).astype(np.float64)
    t = ord("d")
    if kind == "min_last_max_middle":  # INT64_MIN only in the set's last lane, INT64_MAX only in a middle one
        v = (at * 1000 - 20000).astype(np.int64)
        v[n - 1], v[n // 2] = INT64_MIN, INT64_MAX
        t, values = ord("l"), v.view(np.uint64)
    elif kind == "low_halves_full":  # every low half 0xFFFFFFFF: the sum of the low halves carries far; high halves of both signs
        t, values = ord("l"), (((at * 7919 - 200000).astype(np.int64) << 32) | 0xFFFFFFFF).view(np.uint64)
    elif kind == "all_negative":  # the sum of the high halves is signed
        t, values = ord("l"), (-(at + 1) * (1 << 40) - 1).astype(np.int64).view(np.uint64)
    elif kind == "zeros_negative_first":
        values = as_bits(np.where(at % 2 == 0, -0.0, 0.0))
    elif kind == "zeros_positive_first":
        values = as_bits(np.where(at % 2 == 0, 0.0, -0.0))
    else:
        if kind in ("plus_inf_in_a_member", "both_infs_in_members"):
            ints[n // 4] = np.inf
        if kind in ("minus_inf_in_a_member", "both_infs_in_members"):
            ints[n - 2] = -np.inf
        values = as_bits(ints)
    return _one_set("%s%s" % (kind, "_strided" if strided else ""), ("value", kind, "strided" if strided else "whole"), lanes,
                    np.full(n, t, dtype=np.uint8), values)


# ---- the census: the pattern is on the bin -------------------------------------------------------------------------------------
def one_type(case, t=ord("{")):
    """the case with one type byte in every lane: its bins are its keys"""
    p = case.pattern.copy()
    p.types[:] = t
    c = Case(case.name + "_bins", Pattern(p.key, p.valid, p.types), case.tags, case.n_sets, case.leftover, case.leader, case.largest,
             case.every_wave, case.row_count_lane)
    return c


def one_index_two_classes():
    """one index under two classes in the same wave: two sets, not one"""
    types = np.where(np.arange(WAVE) % 2 == 0, ord("l"), ord('"')).astype(np.uint8)
    return Case("one_index_two_classes", Pattern(np.zeros(WAVE, dtype=np.int64), None, types), ["one_index_two_classes"], 2, False, 0, (0, 32))


def eight_classes_then_a_ninth_index():
    """the eight classes of one index as exactly eight sets, a ninth index (eight lanes of it) behind them"""
    lanes = np.arange(WAVE)
    types = np.frombuffer(CLASS_BYTES, dtype=np.uint8)[lanes % 8].copy()
    types[56:] = ord("l")
    return Case("eight_classes_then_a_ninth_index", Pattern(np.where(lanes < 56, 0, 1), None, types), ["eight_classes_then_a_ninth_index"], 9, True, 0)


# ---- the lists -----------------------------------------------------------------------------------------------------------------
def _key_cases(with_nan):
    out = [round_robin(d) for d in D_VALUES] + [blocks(d) for d in D_VALUES]
    out += [leader_position(lane, alone) for lane in LEADER_LANES for alone in (False, True)]
    out += [late_big_set(), early_big_set(), one_key_across_waves(1), one_key_across_waves(9)]
    for base, d in ((round_robin, 9), (blocks, 3)):
        out += [with_inactive(base, d, kind, where) for kind in INACTIVE_KINDS if with_nan or kind != "nan" for where in INACTIVE_WHERE]
        out += [with_row_count(base, d, lane) for lane in ROW_COUNT_LANES]
    return out


def groupstats_cases():
    out = _key_cases(True)
    out += [class_mix(mix, strided) for mix in CLASS_MIXES for strided in (False, True)]
    out += [value_case(kind, strided) for kind in VALUE_KINDS for strided in (False, True)]
    return out


def census_cases():
    """(a 'd' cell that holds a NaN counts in the census like any other: that kind of inactive lane is group_stats' alone)"""
    return [one_type(c) for c in _key_cases(False)] + [one_index_two_classes(), eight_classes_then_a_ninth_index()]


REQUIRED_KEY_TAGS = ({("round_robin", d) for d in D_VALUES} | {("blocks", d) for d in D_VALUES}
                     | {("leader", lane, how) for lane in LEADER_LANES for how in ("alone", "behind")}
                     | {"late_big_set", "early_big_set", ("every_wave", 1), ("every_wave", 9)} | {("row_count", lane) for lane in ROW_COUNT_LANES})
REQUIRED_GROUPSTATS_TAGS = (REQUIRED_KEY_TAGS | {("inactive", kind, where) for kind in INACTIVE_KINDS for where in INACTIVE_WHERE}
                            | {("class", mix, how) for mix in CLASS_MIXES for how in ("whole", "strided")}
                            | {("value", kind, how) for kind in VALUE_KINDS for how in ("whole", "strided")})
REQUIRED_CENSUS_TAGS = (REQUIRED_KEY_TAGS | {("inactive", kind, where) for kind in INACTIVE_KINDS if kind != "nan" for where in INACTIVE_WHERE}
                        | {"one_index_two_classes", "eight_classes_then_a_ninth_index"})


# ---- a case as columns ---------------------------------------------------------------------------------------------------------
def materialize(case, n_keys):
    """-> dict(indices int32, words uint64, bits bool, types uint8, values uint64, row_count None or int, n_rows)"""
    assert n_keys >= MAX_KEY
    with_count = case.row_count_lane is not None
    n_rows = N_WAVES * WAVE if with_count else (N_WAVES - 1) * WAVE + TAIL
    indices = np.full(N_WAVES * WAVE, -1, dtype=np.int64)
    bits = np.zeros(N_WAVES * WAVE, dtype=bool)
    types = np.full(N_WAVES * WAVE, ord("l"), dtype=np.uint8)
    values = np.full(N_WAVES * WAVE, POISON[0], dtype=np.uint64)
    p = case.pattern
    for i, w in enumerate(range(N_WAVES) if case.every_wave else PLACEMENTS):
        base = 0 if case.every_wave else WAVE * i
        key = np.where(p.key >= 0, p.key + base, 0)
        key[p.key == OUT_NEG], key[p.key == OUT_N_KEYS], key[p.key == OUT_INT32_MIN] = -1, n_keys, INT32_MIN
        rows = slice(w * WAVE, (w + 1) * WAVE)
        indices[rows], bits[rows], types[rows], values[rows] = key, p.valid, p.types, p.values
    assert indices.max() < MAX_KEY or indices.max() == n_keys
    bits = bits[:n_rows]
    return dict(indices=indices[:n_rows].astype(np.int32), words=pack_bits(bits), bits=bits, types=types[:n_rows].copy(), values=values[:n_rows].copy(),
                row_count=(N_WAVES - 1) * WAVE + case.row_count_lane if with_count else None, n_rows=n_rows)


def wave_sets(case, column, n_keys, census):
    """the sets of the case's claim wave as the operator's merge meets them in the materialized column"""
    first = case.claim_wave * WAVE
    live = column["n_rows"] if column["row_count"] is None else min(column["n_rows"], column["row_count"])
    keys, active = [], []
    for r in range(first, first + WAVE):
        inside = r < live and bool(column["bits"][r]) and 0 <= int(column["indices"][r]) < n_keys
        t, v = int(column["types"][r]) if r < live else 0, int(column["values"][r]) if r < live else 0
        if inside and not census and t == ord("d") and (v & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000:
            inside = False
        active.append(inside)
        keys.append((int(column["indices"][r]) * 8 + census_class(t) if census else int(column["indices"][r])) if inside else None)
    return sets_of(keys, active)


# ---- top_rows: TrGroup::all -----------------------------------------------------------------------------------------------------
TOP_ROWS = 1024 + 70
TOP_POSITIONS = (0, 1, 63, 64, 65, 959, 960, 1023, 1024, 1093)


def top_rows_column(v, p, q, double):
    """1024 + 70 rows in which every candidate holds v, but row p holds v - 1 and row q holds v + 1; around p and q and at every
    seventh row lie non-candidates (a JSON null, a string, a cleared validity bit) -> (types, words, bits, values uint64)"""
    assert p != q
    rows = np.arange(TOP_ROWS)
    types = np.full(TOP_ROWS, ord("d") if double else ord("l"), dtype=np.uint8)
    bits = np.ones(TOP_ROWS, dtype=bool)
    around = {r for c in (p, q) for r in (c - 2, c - 1, c + 1, c + 2) if 0 <= r < TOP_ROWS} | set(range(3, TOP_ROWS, 7))
    for r in sorted(around - {p, q}):
        if r % 3 == 0:
            types[r] = ord("n")
        elif r % 3 == 1:
            types[r] = ord('"')
        else:
            bits[r] = False
    cells = np.full(TOP_ROWS, v, dtype=np.float64 if double else np.int64)
    cells[~bits] = v + 1  # (a row that is not valid would win if it were read)
    cells[p], cells[q] = v - 1, v + 1
    values = cells.view(np.uint64).copy()
    dead = (types != types[p]) & (rows >= 0)
    values[dead] = np.array(POISON, dtype=np.uint64)[rows[dead] % len(POISON)]
    return types, pack_bits(bits), bits, values


# ---- parent_columns: PaGroup::scan_max ------------------------------------------------------------------------------------------
PARENT_ROWS = 2 * 1024 + 5
PARENT_POSITIONS = (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 767, 768, 1022, 1023)


def parent_counts(p):
    """rows per document for 2 x 1024 + 5 dense rows: one document begins in each chunk at position p (rows p, 1024 + p and, where
    it lies below the end, 2048 + p) and owns the rows up to the next one, so the rows of a chunk in front of p belong to the
    document that began in the chunk before (in the first chunk: to a document that begins at row 0); documents without rows in
    front, between and behind"""
    starts = sorted({0, p, 1024 + p} | ({2048 + p} if 2048 + p < PARENT_ROWS else set()))
    counts = [0, 0]
    for a, b in zip(starts, starts[1:] + [PARENT_ROWS]):
        counts += [b - a] + [0] * (3 + a % 5)
    assert sum(counts) == PARENT_ROWS
    return counts
