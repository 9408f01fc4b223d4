"""CPU check of the join's passes (simdjson-java_amd/csrc/sj_joinrows.h, which csrc/joinrows.hip compiles verbatim) against the
reference of tests/joinrows_common.py: tests/host_sim/joinrows_sim.cpp runs the clear, the key gather, the count / scan / offsets
and the emit with a sequential workgroup, the chunks of all three kinds in three orders; a stand-alone program runs them under
ASan and UBSan.  All results are integers: every comparison is an equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import host_sim_lib
from tests import joinrows_common as JO
from tests import sortrows_common as SO
from tests import toprows_common as TC
from tests.members_common import header_constant, pack_bits

CANARY = 0xC0FFEE0DDF00D5
LEFT_POSITIONS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
BUILD_SIZES = [0, 1, 2, 63, 64, 65, 1023, 1025]
HOWS = (JO.INNER, JO.LEFT, JO.SEMI, JO.ANTI)
SIDE = np.dtype([("key_types", "<u8"), ("key_validity", "<u8"), ("key_values", "<u8"), ("n_source_rows", "<u8"), ("types", "<u8"),
                 ("values", "<u8"), ("n_cols", "<u8"), ("col_stride", "<u8")])  # sjmi_join_side


def load_sim():
    """tests/host_sim/joinrows_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("joinrows", ("sj_joinrows.h", "sj_parents.h", "sj_sortrows.h", "sj_toprows.h", "sj_filter.h", "sj_okey.h",
                                         "sj_arrowcol.h", "sj_fieldcol.h"))
    P, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
    lib.sim_join_rows.restype = C.c_int
    lib.sim_join_rows.argtypes = [P, P, U64, P, P, P, U64, P, U32, U64, P, P, P, P, P, P, U64, P, P, U32, U32]
    lib.sim_join_chunk_rows.restype = U32
    lib.sim_join_workspace_words.restype, lib.sim_join_workspace_words.argtypes = U64, [U64, U64]
    return lib


@pytest.fixture(scope="module")
def lib():
    lib = load_sim()
    assert lib.sim_join_chunk_rows() == 1024
    assert [header_constant("SJMI_JOIN_" + n) for n in ("INNER", "LEFT", "SEMI", "ANTI")] == list(HOWS)
    assert [header_constant("SJMI_JOIN_" + n) for n in ("OVERFLOW", "BAD_ROW", "BAD_ORDER", "RESULT_WORDS")] == [
        JO.OVERFLOW, JO.BAD_ROW, JO.BAD_ORDER, JO.RESULT_WORDS]
    return lib


class Key:
    """one side's key column on the host: types uint8 or None, the validity bits (bool) or None, values uint64"""

    def __init__(self, types, bits, values):
        self.types, self.bits, self.values = types, bits, np.ascontiguousarray(values, dtype=np.uint64)
        self.words = None if bits is None else pack_bits(bits)
        self.n = self.values.size


def longs(vals):
    v = np.array(vals, dtype=np.int64).view(np.uint64)
    return Key(np.full(v.size, ord("l"), dtype=np.uint8), None, v)


def mixed(n, seed, with_types=True, with_validity=True):
    """counters with heavy ties among 'd', string, null and MISSING cells over poison words, and a validity bitmap"""
    types, values = TC.typed_column(n, seed, "counters")
    if not with_types:
        values = TC.counters(n, seed)
    return Key(types if with_types else None, TC.validity(n, seed)[1] if with_validity else None, values)


def side_struct(key, carry, shift, keep):
    """-> the C struct as a numpy record; `keep` collects the arrays it points into.  The types columns begin at the odd offset `shift`"""
    moved = lambda a: None if a is None else np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])
    kt, ct = moved(key.types), moved(None if carry is None else carry[0])
    cv = None if carry is None else np.ascontiguousarray(carry[1])
    keep += [kt, ct, cv, key.words, key.values]
    ptr = lambda a, off=0: a.ctypes.data + off if a is not None and a.size > off else 0
    s = np.zeros(1, dtype=SIDE)
    s[0] = (ptr(kt, shift), ptr(key.words), ptr(key.values), key.n, ptr(ct, shift), ptr(cv), 0 if carry is None else carry[0].shape[0],
            0 if carry is None else carry[0].shape[1])
    return s


def run(lib, how, left, right, order, sort_record, rows_in=None, n_left=None, left_count=None, n_right=None, lcarry=None, rcarry=None,
        capacity=0, with_offsets=True, with_right_rows=True, chunk=0, sched=0, shift=1, pad=3):
    """-> (left_rows [capacity], right_rows [capacity] or None, (left types, left values, right types, right values) each [n_cols,
    stride], offsets [n_left + 1] or None, result [9]).  Canaries in front of and behind every output are checked here, and the
    entries at or behind min(n_pairs, capacity) and behind off[live] must still hold them"""
    n_left = (left.n if rows_in is None else rows_in.size) if n_left is None else n_left
    n_right = order.size if n_right is None else n_right
    keep = []
    ls, rs = side_struct(left, lcarry, shift, keep), side_struct(right, rcarry, shift, keep)
    stride = capacity + pad if lcarry is not None or rcarry is not None else 0
    cols = [0 if c is None else c[0].shape[0] for c in (lcarry, rcarry)]
    out_rows = [np.full(capacity + 16, CANARY, dtype=np.uint64) for _ in range(2)]
    out_values = [np.full(n * stride + 16, CANARY, dtype=np.uint64) for n in cols]
    out_types = [np.full(n * stride + 16 + shift, 0xC5, dtype=np.uint8) for n in cols]
    offsets = np.full(n_left + 1 + 16, CANARY, dtype=np.uint64)
    result = np.full(JO.RESULT_WORDS + 2, CANARY, dtype=np.uint64)
    lc = None if left_count is None else np.array([left_count], dtype=np.uint64)
    rec = None if sort_record is None else np.array(sort_record, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None
    got = lib.sim_join_rows(ls.ctypes.data, ptr(rows_in), n_left, ptr(lc), rs.ctypes.data, ptr(order), n_right, ptr(rec), how, capacity,
                            out_rows[0][8:].ctypes.data if capacity else None, out_rows[1][8:].ctypes.data if capacity and with_right_rows else None,
                            out_types[0][8 + shift:].ctypes.data if cols[0] * stride else None, out_values[0][8:].ctypes.data if cols[0] * stride else None,
                            out_types[1][8 + shift:].ctypes.data if cols[1] * stride else None, out_values[1][8:].ctypes.data if cols[1] * stride else None,
                            stride, offsets[8:].ctypes.data if with_offsets else None, result[1:].ctypes.data, chunk, sched)
    assert got == 0
    return outputs(out_rows, out_types, out_values, offsets, result, cols, stride, capacity, n_left, with_offsets, with_right_rows, shift)


def outputs(out_rows, out_types, out_values, offsets, result, cols, stride, capacity, n_left, with_offsets, with_right_rows, shift):
    """the canaries around and behind what a call wrote (numpy arrays as run() lays them out) -> run()'s result"""
    assert result[0] == CANARY and result[-1] == CANARY
    live, n_pairs = int(result[1]), int(result[3])
    written = min(n_pairs, capacity)
    assert live <= n_left
    for k, rows in enumerate(out_rows):
        upto = written if k == 0 or with_right_rows else 0
        assert (rows[:8] == CANARY).all() and (rows[8 + upto:] == CANARY).all(), "a word outside rows[0, written) was written"
    cells = []
    for n, ot, ov in zip(cols, out_types, out_values):
        v, t = ov[8:8 + n * stride].reshape(n, stride), ot[8 + shift:8 + shift + n * stride].reshape(n, stride)
        assert (ov[:8] == CANARY).all() and (ov[8 + n * stride:] == CANARY).all() and (v[:, written:] == CANARY).all()
        assert (ot[:8 + shift] == 0xC5).all() and (ot[8 + shift + n * stride:] == 0xC5).all() and (t[:, written:] == 0xC5).all()
        cells += [t, v]
    upto = live + 1 if with_offsets else 0
    assert (offsets[:8] == CANARY).all() and (offsets[8 + upto:] == CANARY).all(), "an offset behind off[live] was written"
    return (out_rows[0][8:8 + capacity], out_rows[1][8:8 + capacity] if with_right_rows else None, cells, offsets[8:8 + n_left + 1] if with_offsets else None,
            result[1:-1])


def check(join, how, left, right, rows_in=None, n_left=None, left_count=None, right_rows_in=None, n_right=None, right_live=None, lcarry=None,
          rcarry=None, capacity=None, n_candidates=None, what="", **kw):
    """join = a function with run()'s arguments behind the library: the host simulation here, the GPU in tests/test_gpu_joinrows.py.
    capacity None: the pairs the reference counts.  n_candidates: what the sort record claims instead of the truth (the build set
    follows it).  -> (the expected pairs, the record)"""
    n_l = (left.n if rows_in is None else rows_in.size) if n_left is None else n_left
    lref = JO.left_classes(left.types, left.bits, left.values, rows_in, n_l, n_l if left_count is None else left_count)
    order, sort_record, build_keys = JO.build_set(right.types, right.bits, right.values, right_rows_in, n_right, right_live)
    if n_candidates is not None:
        assert n_candidates <= sort_record[1] or sort_record[1] == order.size, "the claim would put non-candidates into the build set"
        sort_record = list(sort_record)
        sort_record[1] = n_candidates
        build_keys = build_keys[:min(n_candidates, order.size)]
    n_build = build_keys.size
    if how in (JO.SEMI, JO.ANTI):
        rcarry = None
    want_l, want_r, want_off, want = JO.expected(how, lref, order, n_build, build_keys, 1 << 62)
    capacity = want[2] if capacity is None else capacity
    want[8] |= JO.OVERFLOW if want[2] > capacity else 0
    left_rows, right_rows, cells, offsets, result = join(how, left, right, order, sort_record, rows_in=rows_in, n_left=n_left, left_count=left_count,
                                                         lcarry=lcarry, rcarry=rcarry, capacity=capacity, **kw)
    assert [int(x) for x in result] == want, (what, [int(x) for x in result], want)
    n = min(want[2], capacity)
    assert (left_rows[:n] == want_l[:n]).all(), what
    if right_rows is not None:
        assert (right_rows[:n] == want_r[:n]).all(), what  # (under SEMI the first match, under ANTI NO_ROW: the reference's too)
    if offsets is not None:
        assert (offsets[:lref[0] + 1] == want_off).all(), what
    for carry, rows, n_source, got in ((lcarry, want_l, left.n, cells[0:2]), (rcarry, want_r, right.n, cells[2:4])):
        if carry is not None:
            ct, cv = JO.carried_cells(carry, rows[:n], n_source)
            assert (got[0][:, :n] == ct).all() and (got[1][:, :n] == cv).all(), what
    return (want_l, want_r, want_off), want


@pytest.fixture(scope="module")
def sim(lib):
    return lambda *a, **kw: run(lib, *a, **kw)


def shaped(ms):
    """left position i has key i and exactly ms[i] matches -> (left, right); the build side is shuffled"""
    ms = np.asarray(ms, dtype=np.int64)
    keys = np.repeat(np.arange(ms.size, dtype=np.int64), ms)
    keys = np.concatenate([keys, np.array([-5, ms.size + 7], dtype=np.int64)])  # (two build keys that nobody asks for)
    np.random.default_rng(ms.size).shuffle(keys)
    return longs(np.arange(ms.size)), longs(keys)


def test_the_two_forms_of_the_reference_agree():
    for seed, (n_l, n_r) in enumerate(((1500, 700), (300, 2000), (0, 5), (5, 0))):
        left, right = mixed(n_l, seed), mixed(n_r, seed + 50)
        rows_in = np.random.default_rng(seed).integers(0, n_l + 3, n_l + 9).astype(np.uint64)
        for ri in (None, rows_in):
            lref = JO.left_classes(left.types, left.bits, left.values, ri, n_l if ri is None else ri.size, 1 << 40)
            order, record, build_keys = JO.build_set(right.types, right.bits, right.values)
            for how in HOWS:
                a = JO.expected(how, lref, order, record[1], build_keys)
                b = JO.expected_by_searchsorted(how, lref, order, record[1], build_keys)
                assert all((x == y).all() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
                assert a[3][2] == a[0].size == int(a[2][-1]) and (n_l == 0 or n_r == 0 or how == JO.ANTI or a[3][3] > 0)


def test_the_scratch(lib):
    for n_left, n_right in ((0, 0), (1, 0), (0, 1), (1024, 7), (1025, 1025), (8 << 20, 1 << 20), ((1 << 32) - 1, (1 << 32) - 1)):
        # the build keys, a sum per left chunk, n_left + 1 offsets, n_left 32-bit lower bounds and counts
        assert lib.sim_join_workspace_words(n_left, n_right) == n_right + (n_left + 1023) // 1024 + n_left + 1 + 2 * ((n_left + 1) // 2)


@pytest.mark.parametrize("n_left", LEFT_POSITIONS)
def test_left_positions_against_build_sizes(sim, n_left):
    left = mixed(n_left, 300 + n_left)
    lcarry = TC.carried(2, n_left, n_left + 5, n_left)
    for n_right in BUILD_SIZES:
        right = mixed(n_right, 900 + n_right)
        rcarry = TC.carried(1, n_right, n_right, n_right) if n_right else None  # (a column set without a cell has no pointer to give)
        for how in HOWS:
            check(sim, how, left, right, lcarry=lcarry, rcarry=rcarry, what=(n_left, n_right, how), shift=1 + 2 * (how & 1))


@pytest.mark.parametrize("ms", [[], [0], [1], [500, 523], [500, 524], [1000, 25], [1023], [1024], [1025], [3, 0, 1021, 0, 0, 1, 0]],
                         ids=lambda ms: "pairs%d_%d" % (sum(ms), len(ms)))
def test_pair_counts_at_the_output_chunk_edge(sim, ms):
    left, right = shaped(ms)
    for how in HOWS:
        _, want = check(sim, how, left, right, lcarry=TC.carried(1, left.n, left.n, 3), rcarry=TC.carried(1, right.n, right.n + 2, 4), what=(ms, how))
        if how == JO.INNER:
            assert want[2] == sum(ms)


@pytest.mark.parametrize("ms", [[2049], [2049, 2049, 2049], [0, 0, 1024, 0, 0, 0, 1, 0, 2049, 0, 0, 1023, 0, 1, 0],
                                [1023, 0, 1, 0, 0, 1024, 0, 3 * 1024 + 1, 0, 0]], ids=lambda ms: "hot%d_%d" % (max(ms), len(ms)))
def test_hot_keys_fill_output_chunks_that_begin_no_position(sim, ms):
    left, right = shaped(ms)
    for how in (JO.INNER, JO.LEFT):
        for sched in (0, 1, 2):
            check(sim, how, left, right, lcarry=TC.carried(1, left.n, left.n, 3), rcarry=TC.carried(1, right.n, right.n, 4), sched=sched, what=(ms, how))


def test_unique_keys_duplicates_no_match_and_all_match(sim):
    rng = np.random.default_rng(5)
    perm = lambda n: rng.permutation(n).astype(np.int64)
    cases = {"permutation": (longs(perm(1500) * 3), longs(perm(1500) * 3)),
             "m_x_n": (longs(rng.integers(0, 9, 700)), longs(rng.integers(0, 9, 400))),
             "no_match": (longs(perm(1100) * 2), longs(perm(900) * 2 + 1)),
             "all_match_all": (longs([7] * 130), longs([7] * 90))}
    for name, (left, right) in cases.items():
        for how in HOWS:
            _, want = check(sim, how, left, right, lcarry=TC.carried(1, left.n, left.n, 1), rcarry=TC.carried(1, right.n, right.n, 2), what=(name, how))
            if how == JO.INNER:
                assert want[2] == {"permutation": 1500, "no_match": 0, "all_match_all": 130 * 90}.get(name, want[2])


def test_the_ends_of_the_key_range(sim):
    """INT64_MAX's sort key is all ones: a sentinel in the searches would show here"""
    ends = [TC.INT64_MIN, -1, 0, 1, TC.INT64_MAX]
    left = longs(ends * 3 + [TC.INT64_MAX - 1, TC.INT64_MIN + 1, 2])
    for right_vals in (ends * 2, [TC.INT64_MAX] * 70, [TC.INT64_MIN] * 70, [TC.INT64_MAX - 1], [TC.INT64_MIN + 1, 0]):
        for how in HOWS:
            check(sim, how, left, longs(right_vals), what=(right_vals[:2], how))


@pytest.mark.parametrize("with_types,with_validity", [(True, True), (True, False), (False, True), (False, False)])
def test_null_other_and_bad_positions_under_every_how(sim, with_types, with_validity):
    n = 2100
    left, right = mixed(n, 1, with_types, with_validity), mixed(800, 2, with_types, with_validity)
    rows_in = np.random.default_rng(1).permutation(n).astype(np.uint64)
    for k, i in enumerate((0, 63, 64, 700, 1024, 2099)):
        rows_in[i] = ((n,) + SO.BAD_ENTRIES)[k % 3]
    lcarry = TC.carried(2, n, n, 8)  # (the source columns end exactly at n_source_rows)
    for how in HOWS:
        _, want = check(sim, how, left, right, rows_in=rows_in, lcarry=lcarry, rcarry=TC.carried(1, 800, 800, 9), what=how)
        assert want[6] == 6 and want[8] & JO.BAD_ROW and (with_types or with_validity or want[4] == want[5] == 0)
        if with_types:
            assert want[4] > 100 and want[5] > 100  # (NULL and OTHER -- 'd' and '"' cells -- are there)
        if how in (JO.LEFT, JO.ANTI):
            assert want[2] >= want[4] + want[5] + want[6]  # (every NULL, OTHER and BAD position comes out)


def test_rows_in_forms_and_live_positions(sim):
    n = 1300
    left, right = mixed(n, 11), mixed(500, 12)
    rng = np.random.default_rng(11)
    subset = np.nonzero(rng.random(n) < 0.4)[0].astype(np.uint64)
    forms = {"identity": np.arange(n, dtype=np.uint64), "permutation": rng.permutation(n).astype(np.uint64),
             "doubled_subset": np.concatenate([subset, subset]), "bad": np.array([n, 5, (1 << 32) - 1, 7, 1 << 63, n - 1] * 20, dtype=np.uint64)}
    for name, rows_in in forms.items():
        for how in HOWS:
            check(sim, how, left, right, rows_in=rows_in, lcarry=TC.carried(1, n, n + 1, 2), what=(name, how))
    rows_in = forms["permutation"]
    for left_count in (0, 1, 64, 1024, 1299, 1300, 1301, 1 << 50):
        poisoned = rows_in.copy()
        poisoned[min(n, left_count):] = SO.BAD_ENTRIES[1]  # (would be counted if it were read)
        for how in (JO.INNER, JO.ANTI):
            check(sim, how, left, right, rows_in=poisoned, left_count=left_count, what=(left_count, how))
            check(sim, how, left, right, left_count=left_count, what=(left_count, how))
    check(sim, JO.LEFT, left, right, n_left=700)
    check(sim, JO.LEFT, left, right, rows_in=rows_in, n_left=700)


def test_the_right_side_behind_a_selection_a_row_count_and_the_records_claim(sim):
    left, right = mixed(900, 21), mixed(1100, 22)
    rng = np.random.default_rng(21)
    sel = np.nonzero(rng.random(1100) < 0.5)[0].astype(np.uint64)
    for how in HOWS:
        check(sim, how, left, right, right_rows_in=sel, what=("selection", how))
        check(sim, how, left, right, right_rows_in=sel, right_live=200, what=("row count", how))
        check(sim, how, left, right, n_right=600, what=("n_right", how))
    # the record's n_candidates below, at and above n_right (every right row a candidate: the build set is min(n_right, the claim))
    right = longs(rng.integers(0, 50, 300))
    left = longs(rng.integers(0, 60, 400))
    for claim in (0, 1, 299, 300, 301, 1 << 40):
        for how in HOWS:
            _, want = check(sim, how, left, right, n_candidates=claim, what=(claim, how))
            assert want[1] == min(300, claim)


def test_the_pair_capacity(sim):
    left, right = mixed(1500, 31), mixed(700, 32)
    lcarry, rcarry = TC.carried(1, 1500, 1500, 1), TC.carried(1, 700, 700, 2)
    for how in HOWS:
        _, want = check(sim, how, left, right)
        n_pairs = want[2]
        assert n_pairs > (1100 if how in (JO.INNER, JO.LEFT) else 300)
        for capacity in (n_pairs, n_pairs - 1, 1025, 1024, n_pairs // 2, 1, 0, n_pairs + 1000):
            _, got = check(sim, how, left, right, lcarry=lcarry, rcarry=rcarry, capacity=capacity, what=(how, capacity))
            assert got[2] == n_pairs and bool(got[8] & JO.OVERFLOW) == (capacity < n_pairs)


@pytest.mark.parametrize("n_cols", [0, 1, 5])
def test_carried_columns(sim, n_cols):
    left, right = mixed(1200, 41), mixed(600, 42)
    lcarry = TC.carried(n_cols, 1200, 1203, 1) if n_cols else None
    for other in (0, 1, 5):
        rcarry = TC.carried(other, 600, 600, 2) if other else None
        for how in HOWS:
            check(sim, how, left, right, lcarry=lcarry, rcarry=rcarry, what=(n_cols, other, how), with_right_rows=how in (JO.INNER, JO.LEFT))


def test_outputs_that_may_be_left_out(sim):
    left, right = mixed(700, 51), mixed(300, 52)
    for how in HOWS:
        check(sim, how, left, right, with_offsets=False, with_right_rows=how in (JO.INNER, JO.LEFT), what=how)


def test_schedules_and_chunk_sizes_do_not_matter(sim):
    left, right = mixed(2 * 1024 + 77, 61), mixed(1024 + 300, 62)
    lcarry, rcarry = TC.carried(1, left.n, left.n, 1), TC.carried(1, right.n, right.n, 2)
    order, record, _ = JO.build_set(right.types, right.bits, right.values)
    for how in HOWS:
        first = None
        for chunk in (64, 256, 0):
            for sched in (0, 1, 2):
                _, want = check(sim, how, left, right, lcarry=lcarry, rcarry=rcarry if how < 2 else None, chunk=chunk, sched=sched, what=(how, chunk, sched))
                got = sim(how, left, right, order, record, lcarry=lcarry, capacity=want[2], chunk=chunk, sched=sched)
                flat = [got[0], got[1], got[3], got[4]] + got[2]
                first = flat if first is None else first
                assert all((x == y).all() for x, y in zip(first, flat))


def wild_orders(right, seed):
    """-> [(name, order, the sort record's claim, the n_right_bad the record must hold)]: every load must stay inside its buffer"""
    rng = np.random.default_rng(seed)
    n = right.n
    order, record, _ = JO.build_set(right.types, right.bits, right.values)
    n_cand = record[1]
    cand_rows = order[:n_cand]
    unsorted = cand_rows.copy()[::-1].copy()
    above = cand_rows.copy()
    above[::7] = np.array([n, (1 << 32) - 1, 1 << 63, n + 1] * n, dtype=np.uint64)[:above[::7].size]
    off_cells = np.arange(n, dtype=np.uint64)  # (the identity: null, other and 'd' cells inside the build set, keys in no order)
    bad_cells = n - n_cand
    noise = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2)
    return [("unsorted", unsorted, n_cand, 0), ("above", above, n_cand, above[::7].size), ("non_candidates", off_cells, n, bad_cells),
            ("noise", noise, n, None)]


def test_wild_right_sides_set_the_flag_and_stay_in_bounds(sim):
    left, right = mixed(1500, 71), mixed(1400, 72)
    rcarry = TC.carried(2, right.n, right.n, 7)
    for name, order, claim, n_right_bad in wild_orders(right, 7):
        for how in HOWS:
            for capacity in (0, 5000, 1 << 16):
                got = sim(how, left, right, order, [order.size, claim, 0, 0, 0, 0, 0, 0, 0], lcarry=TC.carried(1, left.n, left.n, 3),
                          rcarry=rcarry if how < 2 else None, capacity=capacity)
                result = [int(x) for x in got[4]]
                assert result[8] & JO.BAD_ORDER, (name, how)
                assert result[0] == left.n and result[1] == min(order.size, claim) and (n_right_bad is None or result[7] == n_right_bad), (name, how, result)
                assert bool(result[8] & JO.OVERFLOW) == (result[2] > capacity) and int(got[3][-1]) == result[2]
                if got[1] is not None:  # (every right row written is an entry of the order, or NO_ROW)
                    written = got[1][:min(result[2], capacity)]
                    assert np.isin(written, np.concatenate([order, [JO.NO_ROW]])).all()
    # a sorted build set sets nothing
    _, want = check(sim, JO.INNER, left, right)
    assert want[7] == 0 and not want[8] & JO.BAD_ORDER


def test_argument_errors(lib):
    ok = np.zeros(96, dtype=np.uint64)
    ty, va = np.zeros(16, dtype=np.uint8), np.zeros(9, dtype=np.uint64)
    p = lambda a, off=0: a.ctypes.data + off
    LR, RR, LT, LV, RT, RV, OFF, RES, RI, ORD, REC = (p(ok, 64 * k) for k in range(11))

    def side(kt=p(ty), kv=0, kval=p(va), ns=4, t=p(ty), v=p(va), n_cols=1, stride=4):
        s = np.zeros(1, dtype=SIDE)
        s[0] = (kt, kv, kval, ns, t, v, n_cols, stride)
        return s

    def f(left=None, right=None, ri=None, n=4, lc=None, order=ORD, nr=4, rec=REC, how=0, cap=4, lrows=LR, rrows=RR, lt=LT, lv=LV, rt=RT, rv=RV,
          ostride=4, off=OFF, res=RES, no_left=False, no_right=False):
        left, right = side() if left is None else left, side() if right is None else right
        return lib.sim_join_rows(None if no_left else left.ctypes.data, ri, n, lc, None if no_right else right.ctypes.data, order, nr, rec, how, cap,
                                 lrows, rrows, lt, lv, rt, rv, ostride, off, res, 0, 0)

    none = dict(t=0, v=0, n_cols=0, stride=0)
    assert f() == 0
    assert f(left=side(kt=0), right=side(kt=0, kv=p(ok, 8))) == 0  # (types and validity NULL is legal: every row is a candidate)
    assert f(left=side(kt=p(ty, 3), t=p(ty, 5)), lt=LT + 1, rt=RT + 3) == 0  # (types: any alignment)
    assert f(no_left=True) == -2 and f(no_right=True) == -2 and f(res=None) == -2
    assert f(how=4) == -2 and f(how=1) == 0 and f(how=2, right=side(**none)) == 0 and f(how=3, right=side(**none)) == 0
    assert f(how=2) == -2 and f(how=3) == -2  # (right carried columns under SEMI and ANTI)
    assert f(how=2, right=side(**none), rrows=None) == 0 and f(how=3, right=side(**none), rrows=None) == 0
    assert f(rrows=None) == -2 and f(how=1, rrows=None) == -2 and f(lrows=None) == -2 and f(lrows=None, rrows=None, cap=0, ostride=0) == 0
    assert f(n=1 << 32, ri=RI) == -2 and f(nr=1 << 32) == -2 and f(left=side(ns=1 << 32, stride=1 << 32)) == -2 and f(right=side(ns=1 << 32, stride=1 << 32)) == -2
    assert f(cap=1 << 40, ostride=1 << 40) == -2
    assert f(n=5) == -2 and f(n=5, ri=RI) == 0  # (without rows_in the positions are rows)
    assert f(nr=5) == 0  # (the order may name more positions than the right side has rows)
    assert f(left=side(kval=0)) == -2 and f(left=side(kval=0), n=0) == 0 and f(right=side(kval=0)) == -2 and f(right=side(kval=0), nr=0) == 0
    assert f(order=None) == -2 and f(rec=None) == -2 and f(order=None, rec=None, nr=0) == 0
    assert f(left=side(t=0)) == -2 and f(left=side(v=0)) == -2 and f(lt=None) == -2 and f(lv=None) == -2 and f(rt=None) == -2 and f(rv=None) == -2
    assert f(left=side(**none), right=side(**none), lt=None, lv=None, rt=None, rv=None, ostride=0) == 0
    assert f(left=side(stride=3)) == -2 and f(right=side(stride=3)) == -2 and f(ostride=3) == -2 and f(cap=3, ostride=3) == 0
    assert f(off=None) == 0 and f(lc=p(ok, 8)) == 0
    for bad in (dict(left=side(kv=p(ok, 4))), dict(left=side(kval=p(va, 4))), dict(right=side(v=p(va, 4))), dict(ri=RI + 4), dict(lc=p(ok, 4)),
                dict(order=ORD + 4), dict(rec=REC + 4), dict(lrows=LR + 4), dict(rrows=RR + 4), dict(lv=LV + 4), dict(rv=RV + 4), dict(off=OFF + 4),
                dict(res=RES + 4)):
        assert f(**bad) == -2, bad


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/joinrows_asan_main.cpp: random adversarial sides, wild orders included, in heap blocks of exactly their size,
    every schedule, the runs on sorted sides compared with a std::multimap join.  Run as a child process."""
    exe = str(tmp_path / "joinrows_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "joinrows_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "60"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
