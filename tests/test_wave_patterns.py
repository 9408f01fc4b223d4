"""The builders of tests/wave_patterns.py yield what they claim, cover what they are meant to cover, and the references agree on
every case -- so a failure of tests/test_gpu_wave_combine.py is the device form's and not the column's.  Also the arithmetic fact
under the scaled columns of tests/test_gpu_groupstats.py: their doubles add up exactly in any order.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

from tests import groupstats_common as GC
from tests import members_common as MC
from tests import parents_common as PC
from tests import toprows_common as TC
from tests import wave_patterns as WP

N_KEYS = WP.MAX_KEY + 1
GS_CASES, CS_CASES = WP.groupstats_cases(), WP.census_cases()


def test_the_merge_rounds_are_the_headers():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "simdjson-java_amd", "csrc")
    for header, name in (("sj_groupstats.h", "GS_MERGE_ROUNDS"), ("sj_census.h", "CS_MERGE_ROUNDS")):
        with open(os.path.join(csrc, header)) as f:
            assert int(re.search(r"constexpr uint32_t %s = (\d+);" % name, f.read()).group(1)) == WP.MERGE_ROUNDS
    assert MC.header_constant("SJMI_GROUP_LDS_KEYS") == WP.MAX_KEY <= MC.header_constant("SJMI_CENSUS_LDS_KEYS")


def test_sets_of_counts_lowest_lane_first():
    sets = WP.sets_of([5, 7, 5, None, 7, 9, 5], [True, True, True, False, True, True, False])
    assert sets == [[0, 2], [1, 4], [5]] and WP.describe(sets) == (3, False, 0, (0, 2))
    assert WP.describe(WP.sets_of(list(range(10)), [False] + [True] * 9)) == (9, True, 1, (1, 1))
    assert WP.describe(WP.sets_of([1, 2], [False, False])) == (0, False, None, None)


@pytest.mark.parametrize("census,cases", [(False, GS_CASES), (True, CS_CASES)], ids=["group_stats", "census"])
def test_every_builder_yields_what_it_claims(census, cases):
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        column = WP.materialize(c, N_KEYS)
        assert column["n_rows"] <= 2048 and column["n_rows"] > 1024 and column["indices"].size == column["n_rows"]
        n_sets, leftover, leader, largest = WP.describe(WP.wave_sets(c, column, N_KEYS, census))
        assert (n_sets, leftover, leader) == (c.n_sets, c.leftover, c.leader), c
        assert c.largest is None or largest == c.largest, c
        # the pattern stands, whole, in the second workgroup too, and the last wave is a partial one
        assert c.claim_wave != 0 or WP.describe(WP.wave_sets(c, dict(column, row_count=None), N_KEYS, census))[:3] == (n_sets, leftover, leader)
        live = column["n_rows"] if column["row_count"] is None else column["row_count"]
        assert live % 64 and live > 1024 + 64
        a, b = slice(0, 64), slice(16 * 64, 17 * 64)
        assert (column["types"][a] == column["types"][b]).all() and (column["bits"][a] == column["bits"][b]).all()
        if not c.every_wave:  # no two waves share a key
            ix, ok = column["indices"].astype(np.int64), column["bits"] & (column["indices"] >= 0) & (column["indices"] < N_KEYS)
            waves = [set(ix[w * 64:(w + 1) * 64][ok[w * 64:(w + 1) * 64]].tolist()) for w in range(WP.N_WAVES)]
            assert all(not (waves[i] & waves[j]) for i in range(len(waves)) for j in range(i))
        # value words behind type bytes that are no numbers are POISON
        other = (column["types"] != ord("l")) & (column["types"] != ord("d"))
        assert np.isin(column["values"][other], np.array(GC.POISON, dtype=np.uint64)).all()


def test_the_cases_cover_what_they_are_meant_to():
    gs = set().union(*(c.tags for c in GS_CASES))
    cs = set().union(*(c.tags for c in CS_CASES))
    assert gs == WP.REQUIRED_GROUPSTATS_TAGS and cs == WP.REQUIRED_CENSUS_TAGS
    # ... and said once more without the module's own lists: every d, every kind of inactive lane at lane 0, every class mix
    for d in (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 32, 63, 64):
        assert {("round_robin", d), ("blocks", d)} <= gs & cs
    for kind in ("invalid", "index_minus_1", "index_n_keys", "index_int32_min", "nan"):
        for where in ("lane_0", "every_second", "all_but_one", "all"):
            assert ("inactive", kind, where) in gs and (kind == "nan" or ("inactive", kind, where) in cs)
    for lane in (1, 32, 63):
        assert ("row_count", lane) in gs & cs
    for mix in ("other_leader_long_members", "long_leader_double_members", "all_three", "only_other", "only_long_in_highest", "only_double_in_highest"):
        assert {("class", mix, "whole"), ("class", mix, "strided")} <= gs
    # by what the waves hold: fewer than, exactly and more than the rounds; a ninth set with duplicates; a first leader that is
    # not lane 0; a set whose leader is an "other" cell and whose members are longs
    for cases, census in ((GS_CASES, False), (CS_CASES, True)):
        seen = [WP.wave_sets(c, WP.materialize(c, N_KEYS), N_KEYS, census) for c in cases]
        assert {len(s) for s in seen} >= {0, 1, 7, 8, 9, 10, 64}
        assert any(len(s) > 8 and len(s[8]) > 1 for s in seen) and any(s and s[0][0] not in (0,) and len(s[0]) > 1 for s in seen)
    c = next(c for c in GS_CASES if c.name == "other_leader_long_members")
    assert chr(c.pattern.types[0]) not in "ld" and (c.pattern.types[1:] == ord("l")).all()


@pytest.mark.parametrize("at", range(0, len(GS_CASES), 16))
def test_the_two_references_of_group_stats_agree_on_every_case(at):
    for c in GS_CASES[at:at + 16]:
        for n_keys in (WP.MAX_KEY, N_KEYS):
            k = WP.materialize(c, n_keys)
            live = k["n_rows"] if k["row_count"] is None else k["row_count"]
            a = GC.expected(k["indices"], k["bits"], k["types"], k["values"], n_keys, live)
            b = GC.expected_large(k["indices"], k["bits"], k["types"], k["values"], n_keys, live)
            same = lambda x, y: x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y))
            assert a[1] == b[1] and all(same(x[w], y[w]) for x, y in zip(a[0], b[0]) for w in x), c
            assert a[1][0] + a[1][1] + a[1][2] == int(k["bits"][:live].sum())


def test_the_two_references_of_the_census_agree_on_every_case():
    for c in CS_CASES + GS_CASES:
        k = WP.materialize(c, N_KEYS)
        live = k["n_rows"] if k["row_count"] is None else k["row_count"]
        a = MC.expected_census(k["indices"], k["bits"], k["types"], N_KEYS, live)
        assert a == MC.expected_census_large(k["indices"], k["bits"], k["types"], N_KEYS, live), c
        assert a[1] + a[2] == int(k["bits"][:live].sum())


def test_the_top_rows_columns_hold_what_they_say():
    for v, double in ((1000, False), (GC.INT64_MAX - 1, False), (GC.INT64_MIN + 1, False), (0.0, True)):
        kind = TC.DOUBLE if double else TC.LONG
        for p in WP.TOP_POSITIONS:
            for q in WP.TOP_POSITIONS:
                if p == q:
                    continue
                types, words, bits, values = WP.top_rows_column(v, p, q, double)
                cell = lambda x: int(np.array([x], dtype=np.float64 if double else np.int64).view(np.uint64)[0])
                assert values.size == WP.TOP_ROWS == 1024 + 70
                rows, rec = TC.expected(types, bits, values, WP.TOP_ROWS, kind, True, 1)
                assert rows.tolist() == [q] and rec[7] == cell(v + 1) and 800 < rec[1] < WP.TOP_ROWS and rec[2] > 100 and rec[3] > 50
                assert TC.expected(types, bits, values, WP.TOP_ROWS, kind, False, 1)[0].tolist() == [p]
                rows, rec = TC.expected(types, bits, values, WP.TOP_ROWS, kind, True, 3)
                holds_v = [r for r in range(WP.TOP_ROWS) if bits[r] and types[r] == types[p] and int(values[r]) == cell(v)]
                assert rows.tolist() == [q] + holds_v[:2] and rec[7] == cell(v)
                assert rows.tolist() == TC.expected_by_python_sort(types, bits, values, WP.TOP_ROWS, kind, True, 3)[0].tolist()
                near = [r for c in (p, q) for r in (c - 1, c + 1) if 0 <= r < WP.TOP_ROWS and r not in (p, q)]
                assert not any(bits[r] and types[r] == types[p] for r in near)  # (non-candidates sit around them)


def test_the_parent_columns_hold_what_they_say():
    for p in WP.PARENT_POSITIONS:
        counts = WP.parent_counts(p)
        offsets = PC.offsets_of(counts)
        want = PC.expected_parents(offsets, np.arange(WP.PARENT_ROWS))
        assert int(offsets[-1]) == WP.PARENT_ROWS == 2 * 1024 + 5 and (want >= 0).all()
        starts = np.flatnonzero(np.diff(want)) + 1
        assert p in [0] + starts.tolist() and 1024 + p in starts.tolist()
        assert (np.diff(want)[np.diff(want) > 0] > 1).all() and counts[0] == 0 and counts[-1] == 0  # (empty documents between, in front, behind)
        if p:
            assert want[1024 + p - 1] == want[1024] == want[p] and want[1024 + p] > want[p]  # (in front of p: the document of the chunk before)


# ---- the scaled columns are exact in any order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", GC.SCALES, ids=GC.SCALE_IDS)
def test_a_scaled_column_sums_exactly_in_any_order(scale):
    types, values = GC.value_column(70000, 5, "scaled", scale=scale)
    cells = values[types == ord("d")].view(np.float64)
    assert cells.size > 15000 and (np.abs(cells) < 2.0 ** 20 * scale).all() and (cells / scale == np.round(cells / scale)).all()
    if scale < 2.0 ** -1022 / 2.0 ** 20:
        assert (np.abs(cells) < 2.0 ** -1022).all()  # (every cell subnormal)
    exact = math.fsum(cells.tolist())
    rng = np.random.default_rng(1)
    for _ in range(5):
        x = cells[rng.permutation(cells.size)]
        total = 0.0
        for c in x.tolist():
            total += c
        assert total == exact
        while x.size > 1:  # a pairwise tree
            if x.size % 2:
                x = np.concatenate([x, [0.0]])
            x = x[0::2] + x[1::2]
        assert float(x[0]) == exact
    # the same cells as value_column's kind "exact", times the scale
    assert (GC.value_column(70000, 5, "exact")[1][types == ord("d")].view(np.float64) == cells / scale).all()
