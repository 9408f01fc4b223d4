"""The device-only lane-group forms on the directed wave patterns of tests/wave_patterns.py: the combine of a wave's equal keys
(GsGroup::merge, csrc/groupstats.hip) and bins (CsGroup::merge, csrc/census.hip), the minimum / maximum over a workgroup
(TrGroup::all, csrc/toprows.hip) and the running maximum over a workgroup (PaGroup::scan_max, csrc/parents.hip).  The host
simulation runs a one-lane form of these members, so this file is their test: every case against the plain-loop reference, on the
global path (where the merge runs) at two key counts, on the LDS path with the same rows as the control, twice.  All doubles of
the cases add up exactly in any order: every comparison is an equality.  The calls and their canaries are those of
tests/test_gpu_groupstats.py, test_gpu_census.py, test_gpu_toprows.py and test_gpu_parents.py."""
import numpy as np
import pytest

from tests import groupstats_common as GC
from tests import members_common as MC
from tests import parents_common as PC
from tests import test_gpu_census as CENSUS
from tests import test_gpu_groupstats as GROUPS
from tests import test_gpu_parents as PARENTS
from tests import test_gpu_toprows as TOP
from tests import toprows_common as TC
from tests import wave_patterns as WP

pytestmark = pytest.mark.gpu

MANY_KEYS = 1 << 18
GS_CASES, CS_CASES = WP.groupstats_cases(), WP.census_cases()
PER_TEST = 16  # cases per test function: a few seconds each
EMPTY_KEY = np.array([0, 0, 0, 0, 0, 0, GC.INT64_MAX, 1 << 63, GC.bits_of(float("inf")), GC.bits_of(float("-inf"))], dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def live_of(column):
    return column["n_rows"] if column["row_count"] is None else min(column["n_rows"], column["row_count"])


def nan_as_one(stats):
    """a sum that is a NaN (both infinities in one key) has no bits that two paths must share"""
    stats = stats.copy()
    sums = stats[:, 5]
    sums[(sums & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)] = np.uint64(0x7FF8000000000000)
    return stats


def group_stats_twice(ctx, case, n_keys):
    """the case at n_keys, twice -> (stats, result) of the first run.  Every word and the record equal to groupstats_common.expected
    (above the cases' keys, where that reference has only empty keys, the words of an empty key), sum_double included; the second
    run equal to the first word for word"""
    column = WP.materialize(case, n_keys)
    head = min(n_keys, WP.MAX_KEY + 1)  # (every index at or above it is outside n_keys too)
    want, counts = GC.expected(column["indices"], column["bits"], column["types"], column["values"], head, live_of(column))
    runs = []
    for shift in (0, 5):
        stats, result = GROUPS.group_stats(ctx, column["indices"], column["words"], column["types"], column["values"], n_keys, column["row_count"],
                                           types_shift=shift)
        assert [int(x) for x in result] == [live_of(column), *counts, 0], (case, n_keys)
        GC.check_stats(stats[:head], want, exact_sum=True, what="%s at %d keys" % (case, n_keys))
        assert (stats[head:] == EMPTY_KEY).all(), (case, n_keys, "a key that no row has")
        runs.append((stats, result))
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all(), (case, n_keys, "two runs differ")
    return runs[0]


@pytest.mark.parametrize("at", range(0, len(GS_CASES), PER_TEST))
def test_group_stats_combines_a_waves_equal_keys(ctx, at):
    for case in GS_CASES[at:at + PER_TEST]:
        control = group_stats_twice(ctx, case, GROUPS.LDS_KEYS)  # the LDS path: no merge
        for n_keys in (GROUPS.LDS_KEYS + 1, MANY_KEYS):
            stats, result = group_stats_twice(ctx, case, n_keys)
            assert (nan_as_one(stats[:GROUPS.LDS_KEYS]) == nan_as_one(control[0])).all() and (result == control[1]).all(), (case, n_keys, "against the LDS path")


def census_twice(ctx, case, n_keys):
    column = WP.materialize(case, n_keys)
    head = min(n_keys, WP.MAX_KEY + 1)
    want, counted, outside = MC.expected_census(column["indices"], column["bits"], column["types"], head, live_of(column))
    runs = []
    for shift in (0, 3):
        counts, result = CENSUS.census(ctx, column["indices"], column["words"], column["types"], n_keys, column["row_count"], types_shift=shift)
        assert [int(x) for x in result] == [live_of(column), counted, outside, 0], (case, n_keys)
        assert counts[:head].tolist() == want, (case, n_keys)
        assert not counts[head:].any(), (case, n_keys, "a key that no row has")
        runs.append((counts.copy(), result))
    assert (runs[0][0] == runs[1][0]).all() and (runs[0][1] == runs[1][1]).all(), (case, n_keys, "two runs differ")
    return runs[0]


@pytest.mark.parametrize("at", range(0, len(CS_CASES), PER_TEST))
def test_the_census_merges_a_waves_equal_bins(ctx, at):
    for case in CS_CASES[at:at + PER_TEST]:
        control = census_twice(ctx, case, CENSUS.LDS_KEYS)
        for n_keys in (CENSUS.LDS_KEYS + 1, MANY_KEYS):
            counts, result = census_twice(ctx, case, n_keys)
            assert (counts[:CENSUS.LDS_KEYS] == control[0]).all() and (result == control[1]).all(), (case, n_keys, "against the LDS path")


def test_the_census_of_the_group_stats_cases(ctx):
    """their class mixes are bins too: one key's lanes fall into up to eight sets"""
    for case in GS_CASES[::3]:
        census_twice(ctx, case, CENSUS.LDS_KEYS + 1)


# ---- TrGroup::all ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v,double", [(1000, False), (GC.INT64_MAX - 1, False), (GC.INT64_MIN + 1, False), (0.0, True)],
                         ids=["1000", "int64_max_less_1", "int64_min_plus_1", "double_0"])
def test_top_rows_minimum_and_maximum_over_the_workgroup(ctx, v, double):
    """every candidate holds v but row p (v - 1) and row q (v + 1), p and q at the wave and chunk edges: a wave dropped from the
    reduction narrows [min, max] and changes the answer.  v - 1, v, v + 1 straddle the sign at the ends of int64 and at 0.0"""
    kind = TC.DOUBLE if double else TC.LONG
    cell = lambda x: int(np.array([x], dtype=np.float64 if double else np.int64).view(np.uint64)[0])
    for p in WP.TOP_POSITIONS:
        for q in WP.TOP_POSITIONS:
            if p == q:
                continue
            types, words, bits, values = WP.top_rows_column(v, p, q, double)
            (rows, _, _, result), _, _ = TOP.check(ctx, types, words, bits, values, kind, True, 1, what=(v, p, q, "largest"))
            assert rows.tolist() == [q] and int(result[7]) == cell(v + 1), (v, p, q)
            (rows, _, _, result), _, _ = TOP.check(ctx, types, words, bits, values, kind, False, 1, what=(v, p, q, "smallest"))
            assert rows.tolist() == [p] and int(result[7]) == cell(v - 1), (v, p, q)
            (rows, _, _, result), _, _ = TOP.check(ctx, types, words, bits, values, kind, True, 3, what=(v, p, q, "three"))
            holds_v = np.flatnonzero(bits & (types == types[p]) & (values == np.uint64(cell(v))))
            assert rows.tolist() == [q] + holds_v[:2].tolist() and int(result[7]) == cell(v), (v, p, q)


# ---- PaGroup::scan_max ----------------------------------------------------------------------------------------------------------
def test_parents_running_maximum_at_the_wave_and_trip_edges(ctx):
    """2 x 1024 + 5 dense rows; a document begins in each chunk at position p and the rows in front of it belong to the document of
    the chunk before; the block is 256 lanes and a chunk four trips, so the positions are the wave and trip edges of scan_max and
    of the carry between the trips"""
    for p in WP.PARENT_POSITIONS:
        counts = WP.parent_counts(p)
        offsets = PC.offsets_of(counts)
        cols = PC.doc_columns(2, len(counts), len(counts) + 1, p)
        want, result = PC.check(PARENTS.device_call(ctx), offsets, WP.PARENT_ROWS, cols=cols, what=p)
        assert result == [WP.PARENT_ROWS, 0, 0] and len(set(want.tolist())) >= 3
        PC.check(PARENTS.device_call(ctx), offsets, WP.PARENT_ROWS + 70, row_count=WP.PARENT_ROWS - 3, cols=cols, out_stride=WP.PARENT_ROWS + 75, what=(p, "count"))
