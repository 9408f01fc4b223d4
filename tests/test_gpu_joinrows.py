"""Two row sets joined on a long key on the GPU (sjmi_join_rows_device through Context.join_rows_device / BatchShard.join_rows):
the pairs, the carried cells of both sides, the pair offsets and the record against the reference of tests/joinrows_common.py,
with canaries in front of and behind every output and the types columns at odd alignments; the shapes of the host simulation's
tests; a million left positions against 2^16 build rows under every how, twice (several workgroups per kernel run only here);
the hot-key shape; live positions from a filter's n_kept and an explode's last offset; the right side behind a filter; the pair
offsets read by parent_columns; and BatchShard.join_rows end to end on the committed fixtures against Python's json.  All results
are integers: every comparison is an equality.  Every input is legal, or is answered by SJMI_ERR_ARG before any launch."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import joinrows_common as JO
from tests import select_common as SC
from tests import sortrows_common as SO
from tests import toprows_common as TC
from tests.test_gpu_explode import parse
from tests.test_host_joinrows import BUILD_SIZES, CANARY, HOWS, LEFT_POSITIONS, check, longs, mixed, outputs, shaped, wild_orders

pytestmark = pytest.mark.gpu

MILLION = 1024 * 1024 + 1


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def _up(a):
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def device_side(key, carry, shift, keep):
    """-> the tuple Context.join_rows_device takes for a side; `keep` collects the tensors it points into"""
    moved = lambda a: _up(np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])) if a is not None and a.size else None
    kt, ct = moved(key.types), moved(None if carry is None else carry[0])
    kw = _up(key.words) if key.words is not None and key.words.size else None
    kv = _up(key.values) if key.n else None
    cv = _up(np.ascontiguousarray(carry[1])) if carry is not None and carry[1].size else None
    keep += [kt, ct, kw, kv, cv]
    ptr = lambda t, off=0: t.data_ptr() + off if t is not None else 0
    return (ptr(kt, shift), ptr(kw), ptr(kv), key.n, ptr(ct, shift), ptr(cv), 0 if carry is None else carry[0].shape[0],
            0 if carry is None else carry[0].shape[1])


def join_rows(ctx, how, left, right, order, sort_record, rows_in=None, n_left=None, left_count=None, n_right=None, lcarry=None, rcarry=None,
              capacity=0, with_offsets=True, with_right_rows=True, shift=1, pad=3):
    """Context.join_rows_device on numpy columns, with the arguments and the result of tests/test_host_joinrows.run; every output
    lies between canaries, the types columns `shift` bytes into their buffers"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    n_left = (left.n if rows_in is None else rows_in.size) if n_left is None else n_left
    n_right = order.size if n_right is None else n_right
    keep = []
    ls, rs = device_side(left, lcarry, shift, keep), device_side(right, rcarry, shift, keep)
    stride = capacity + pad if lcarry is not None or rcarry is not None else 0
    cols = [0 if c is None else c[0].shape[0] for c in (lcarry, rcarry)]
    d_rows = [_up(np.full(capacity + 16, CANARY, dtype=np.uint64)) for _ in range(2)]
    d_values = [_up(np.full(n * stride + 16, CANARY, dtype=np.uint64)) for n in cols]
    d_types = [_up(np.full(n * stride + 16 + shift, 0xC5, dtype=np.uint8)) for n in cols]
    d_off = _up(np.full(n_left + 1 + 16, CANARY, dtype=np.uint64))
    d_res = _up(np.full(JO.RESULT_WORDS + 2, CANARY, dtype=np.uint64))
    d_in = _up(rows_in) if rows_in is not None and rows_in.size else None
    d_lc = None if left_count is None else _up(np.array([left_count], dtype=np.uint64))
    d_order = _up(order) if order.size else None
    d_rec = _up(np.array(sort_record, dtype=np.uint64))
    ptr = lambda t, off=0: t.data_ptr() + off if t is not None else 0
    ctx.join_rows_device(ls, ptr(d_in), n_left, ptr(d_lc), rs, ptr(d_order), n_right, ptr(d_rec), how, capacity,
                         ptr(d_rows[0], 64) if capacity else 0, ptr(d_rows[1], 64) if capacity and with_right_rows else 0,
                         ptr(d_types[0], 8 + shift) if cols[0] * stride else 0, ptr(d_values[0], 64) if cols[0] * stride else 0,
                         ptr(d_types[1], 8 + shift) if cols[1] * stride else 0, ptr(d_values[1], 64) if cols[1] * stride else 0, stride,
                         ptr(d_off, 64) if with_offsets else 0, ptr(d_res, 8), stream)
    torch.cuda.synchronize()
    down = lambda t: t.cpu().numpy().view(np.uint64) if t.dtype == torch.int64 else t.cpu().numpy()
    return outputs([down(t) for t in d_rows], [down(t) for t in d_types], [down(t) for t in d_values], down(d_off), down(d_res), cols, stride,
                   capacity, n_left, with_offsets, with_right_rows, shift)


@pytest.fixture(scope="module")
def gpu(ctx):
    return lambda *a, **kw: join_rows(ctx, *a, **kw)


@pytest.mark.parametrize("n_left", LEFT_POSITIONS)
def test_left_positions_against_build_sizes(gpu, n_left):
    left = mixed(n_left, 300 + n_left)
    lcarry = TC.carried(2, n_left, n_left + 5, n_left)
    for n_right in BUILD_SIZES[n_left % 2::2] + [1025]:
        right = mixed(n_right, 900 + n_right)
        rcarry = TC.carried(1, n_right, n_right, n_right) if n_right else None
        for how in HOWS:
            check(gpu, how, left, right, lcarry=lcarry, rcarry=rcarry, what=(n_left, n_right, how), shift=(n_left + how) % 8)


@pytest.mark.parametrize("ms", [[], [1], [500, 523], [500, 524], [1000, 25], [1025], [3, 0, 1021, 0, 0, 1, 0]], ids=lambda ms: "pairs%d_%d" % (sum(ms), len(ms)))
def test_pair_counts_at_the_output_chunk_edge(gpu, ms):
    left, right = shaped(ms)
    for how in HOWS:
        check(gpu, how, left, right, lcarry=TC.carried(1, left.n, left.n, 3), rcarry=TC.carried(1, right.n, right.n + 2, 4), what=(ms, how))


@pytest.mark.parametrize("ms", [[3 * 1024 + 1], [2049, 2049, 2049], [0, 0, 1024, 0, 0, 0, 1, 0, 2049, 0, 0, 1023, 0, 1, 0],
                                [1023, 0, 1, 0, 0, 1024, 0, 3 * 1024 + 1, 0, 0]], ids=lambda ms: "hot%d_%d" % (max(ms), len(ms)))
def test_hot_keys_fill_output_chunks_that_begin_no_position(gpu, ms):
    """one position with 3 x 1024 + 1 matches: output chunks that begin no position find their owner by the two searches alone.  A
    rank that depended on wave timing would show here: both runs equal the reference"""
    left, right = shaped(ms)
    for how in (JO.INNER, JO.LEFT):
        for _ in range(2):
            check(gpu, how, left, right, lcarry=TC.carried(1, left.n, left.n, 3), rcarry=TC.carried(1, right.n, right.n, 4), what=(ms, how))


def test_unique_keys_duplicates_no_match_all_match_and_the_ends_of_the_range(gpu):
    rng = np.random.default_rng(5)
    perm = lambda n: rng.permutation(n).astype(np.int64)
    ends = [TC.INT64_MIN, -1, 0, 1, TC.INT64_MAX]
    cases = {"permutation": (longs(perm(1500) * 3), longs(perm(1500) * 3)), "m_x_n": (longs(rng.integers(0, 9, 700)), longs(rng.integers(0, 9, 400))),
             "no_match": (longs(perm(1100) * 2), longs(perm(900) * 2 + 1)), "all_match_all": (longs([7] * 130), longs([7] * 90)),
             "ends": (longs(ends * 3 + [TC.INT64_MAX - 1, TC.INT64_MIN + 1, 2]), longs(ends * 2)),
             "max_only": (longs(ends * 3), longs([TC.INT64_MAX] * 70)), "below_max": (longs(ends * 3), longs([TC.INT64_MAX - 1]))}
    for name, (left, right) in cases.items():
        for how in HOWS:
            check(gpu, how, left, right, lcarry=TC.carried(1, left.n, left.n, 1), rcarry=TC.carried(1, right.n, right.n, 2), what=(name, how))


@pytest.mark.parametrize("with_types,with_validity", [(True, True), (True, False), (False, True)])
def test_null_other_and_bad_positions_under_every_how(gpu, with_types, with_validity):
    n = 2100
    left, right = mixed(n, 1, with_types, with_validity), mixed(800, 2, with_types, with_validity)
    rows_in = np.random.default_rng(1).permutation(n).astype(np.uint64)
    for k, i in enumerate((0, 63, 64, 700, 1024, 2099)):
        rows_in[i] = ((n,) + SO.BAD_ENTRIES)[k % 3]
    for how in HOWS:
        _, want = check(gpu, how, left, right, rows_in=rows_in, lcarry=TC.carried(2, n, n, 8), rcarry=TC.carried(1, 800, 800, 9), what=how)
        assert want[6] == 6 and want[8] & JO.BAD_ROW


def test_rows_in_forms_live_positions_and_the_records_claim(gpu):
    n = 1300
    left, right = mixed(n, 11), mixed(500, 12)
    rng = np.random.default_rng(11)
    subset = np.nonzero(rng.random(n) < 0.4)[0].astype(np.uint64)
    for rows_in in (rng.permutation(n).astype(np.uint64), np.concatenate([subset, subset])):
        for how in HOWS:
            check(gpu, how, left, right, rows_in=rows_in, lcarry=TC.carried(1, n, n + 1, 2), what=how)
    rows_in = rng.permutation(n).astype(np.uint64)
    for left_count in (0, 1, 1024, 1299, 1300, 1 << 50):
        poisoned = rows_in.copy()
        poisoned[min(n, left_count):] = SO.BAD_ENTRIES[1]  # (would be counted if it were read)
        check(gpu, JO.LEFT, left, right, rows_in=poisoned, left_count=left_count, what=left_count)
    sel = np.nonzero(rng.random(500) < 0.5)[0].astype(np.uint64)
    check(gpu, JO.INNER, left, right, right_rows_in=sel, right_live=200)
    right, left = longs(rng.integers(0, 50, 300)), longs(rng.integers(0, 60, 400))
    for claim in (0, 1, 299, 300, 301, 1 << 40):
        check(gpu, JO.LEFT, left, right, n_candidates=claim, what=claim)


def test_the_pair_capacity_and_the_carried_columns(gpu):
    left, right = mixed(1500, 31), mixed(700, 32)
    for how in HOWS:
        _, want = check(gpu, how, left, right, with_offsets=False, with_right_rows=how < 2)
        n_pairs = want[2]
        for capacity, n_cols in ((n_pairs, 5), (n_pairs - 1, 1), (1024, 0), (0, 1), (n_pairs + 1000, 1)):
            lcarry = TC.carried(n_cols, 1500, 1500, 1) if n_cols else None
            _, got = check(gpu, how, left, right, lcarry=lcarry, rcarry=TC.carried(5 - n_cols, 700, 700, 2) if n_cols < 5 else None, capacity=capacity,
                           what=(how, capacity))
            assert got[2] == n_pairs and bool(got[8] & JO.OVERFLOW) == (capacity < n_pairs)


def test_wild_right_sides_set_the_flag_and_stay_in_bounds(gpu):
    """an unsorted order, entries at or above the source rows, entries on non-candidate cells, noise: the flag, n_right_bad, and
    every store between its canaries; the source columns end exactly at their last row"""
    left, right = mixed(1500, 71), mixed(1400, 72)
    for name, order, claim, n_right_bad in wild_orders(right, 7):
        for how in HOWS:
            got = gpu(how, left, right, order, [order.size, claim, 0, 0, 0, 0, 0, 0, 0], lcarry=TC.carried(1, left.n, left.n, 3),
                      rcarry=TC.carried(2, right.n, right.n, 7) if how < 2 else None, capacity=5000)
            result = [int(x) for x in got[4]]
            assert result[8] & JO.BAD_ORDER and result[1] == min(order.size, claim) and (n_right_bad is None or result[7] == n_right_bad), (name, how, result)
            assert bool(result[8] & JO.OVERFLOW) == (result[2] > 5000) and int(got[3][-1]) == result[2]
            assert np.isin(got[1][:min(result[2], 5000)], np.concatenate([order, [JO.NO_ROW]])).all()


def test_a_million_left_positions_under_every_how_twice(ctx):
    """2^20 + 1 left positions against 2^16 build rows with 2^12 distinct keys: 1025 left chunks, 64 build chunks and, under INNER
    and LEFT, more than 14 Mi pairs.  Both runs equal to the reference and byte-equal to each other"""
    import torch
    rng = np.random.default_rng(17)
    lk = rng.integers(0, 4096 + 256, MILLION)  # (a sixteenth of the keys is not on the build side)
    lt = np.full(MILLION, ord("l"), dtype=np.uint8)
    lt[rng.random(MILLION) < 0.05] = ord("n")
    left, right = longs(lk), longs(rng.integers(0, 4096, 1 << 16))
    left.types = lt
    lref = JO.left_classes(left.types, None, left.values, None, MILLION, MILLION)
    order, record, build_keys = JO.build_set(right.types, None, right.values)
    lcarry = TC.carried(1, MILLION, MILLION, 17)
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    ls, rs = device_side(left, lcarry, 3, keep), device_side(right, None, 3, keep)
    d_order, d_rec = _up(order), _up(np.array(record, dtype=np.uint64))
    for how in HOWS:
        want_l, want_r, want_off, want = JO.expected_by_searchsorted(how, lref, order, record[1], build_keys)
        n_pairs = want[2]
        assert how >= 2 or n_pairs > 14 << 20
        runs = []
        for _ in range(2):
            out = [torch.full((n_pairs + 8,), -2, dtype=torch.int64, device="cuda") for _ in range(3)]
            ot = torch.full((n_pairs + 8,), 0xC5, dtype=torch.uint8, device="cuda")
            off, res = torch.full((MILLION + 2,), -2, dtype=torch.int64, device="cuda"), torch.full((9,), -2, dtype=torch.int64, device="cuda")
            ctx.join_rows_device(ls, 0, MILLION, 0, rs, d_order.data_ptr(), order.size, d_rec.data_ptr(), how, n_pairs, out[0].data_ptr(),
                                 out[1].data_ptr(), ot.data_ptr(), out[2].data_ptr(), 0, 0, n_pairs, off.data_ptr(), res.data_ptr(), stream)
            runs.append(out + [ot, off, res])
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        a = runs[0]
        assert a[5].cpu().tolist() == want
        assert torch.equal(a[0][:n_pairs], _up(want_l)) and torch.equal(a[1][:n_pairs], _up(want_r)) and torch.equal(a[4][:MILLION + 1], _up(want_off))
        ct, cv = JO.carried_cells(lcarry, want_l, MILLION)
        assert torch.equal(a[2][:n_pairs], _up(cv[0])) and torch.equal(a[3][:n_pairs], _up(ct[0]))
        assert all(int(t[n_pairs:].min()) == int(t[n_pairs:].max()) == -2 for t in a[:3]) and int(a[4][-1]) == -2 and (a[3][n_pairs:] == 0xC5).all()
        del runs, a


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ty = torch.zeros(96, dtype=torch.uint8, device=dev)
    w = torch.zeros(64 * 12, dtype=torch.int64, device=dev)
    T, Wp = ty.data_ptr(), w.data_ptr()
    at = lambda k: Wp + 512 * k
    side = lambda **kw: tuple(dict(dict(kt=T, kv=at(0), kval=at(1), ns=4, t=T + 16, v=at(2), n_cols=1, stride=4), **kw).values())
    none = dict(t=0, v=0, n_cols=0, stride=0)
    good = dict(left=side(), d_left_rows_in=at(3), n_left=4, d_left_count=at(4), right=side(), d_right_order=at(5), n_right=4, d_right_sort_result=at(6),
                how=0, pair_capacity=4, d_left_rows=at(7), d_right_rows=at(8), d_left_out_types=T + 32, d_left_out_values=at(9), d_right_out_types=T + 48,
                d_right_out_values=at(10), out_stride=4, d_pair_offsets=at(11), d_result=at(11) + 64)
    ctx.join_rows_device(**good)
    ctx.join_rows_device(**dict(good, left=side(kt=T + 3, t=T + 17), d_left_out_types=T + 33))  # (types: any alignment)
    ctx.join_rows_device(**dict(good, left=side(kt=0, kv=0), d_left_rows_in=0, d_left_count=0, d_pair_offsets=0, how=1))
    ctx.join_rows_device(**dict(good, how=2, right=side(**none), d_right_rows=0))
    ctx.join_rows_device(**dict(good, how=3, right=side(**none)))
    ctx.join_rows_device(**dict(good, n_right=0, d_right_order=0, d_right_sort_result=0))
    ctx.join_rows_device(**dict(good, pair_capacity=0, out_stride=0, d_left_rows=0, d_right_rows=0))
    ctx.join_rows_device(**dict(good, n_left=5))  # (with rows_in there may be more positions than rows)
    ctx.join_rows_device(**dict(good, n_left=0, n_right=0, d_right_order=0, d_right_sort_result=0))  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[64 * 11 + 8:64 * 11 + 17].tolist() == [0] * 9
    bad = [dict(d_result=0), dict(how=4), dict(how=2), dict(how=3), dict(n_left=1 << 32), dict(n_right=1 << 32), dict(pair_capacity=1 << 40, out_stride=1 << 40),
           dict(left=side(ns=1 << 32, stride=1 << 32)), dict(right=side(ns=1 << 32, stride=1 << 32)), dict(d_left_rows_in=0, n_left=5),
           dict(left=side(kval=0)), dict(right=side(kval=0)), dict(d_right_order=0), dict(d_right_sort_result=0), dict(d_left_rows=0), dict(d_right_rows=0),
           dict(how=1, d_right_rows=0), dict(left=side(t=0)), dict(right=side(v=0)), dict(d_left_out_types=0), dict(d_left_out_values=0),
           dict(d_right_out_types=0), dict(d_right_out_values=0), dict(left=side(stride=3)), dict(right=side(stride=3)), dict(out_stride=3),
           dict(left=side(kv=at(0) + 4)), dict(right=side(kval=at(1) + 4)), dict(left=side(v=at(2) + 4)), dict(d_left_rows_in=at(3) + 4),
           dict(d_left_count=at(4) + 4), dict(d_right_order=at(5) + 4), dict(d_right_sort_result=at(6) + 4), dict(d_left_rows=at(7) + 4),
           dict(d_right_rows=at(8) + 4), dict(d_left_out_values=at(9) + 4), dict(d_right_out_values=at(10) + 4), dict(d_pair_offsets=at(11) + 4),
           dict(d_result=at(11) + 68)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.join_rows_device(**dict(good, **change))
    lib = C.CDLL(S.lib_path())
    l = S.binding.join_side(*side())
    lib.sjmi_join_rows_device.restype = C.c_int
    args = [C.c_void_p(l.ctypes.data), None, C.c_uint64(4), None, C.c_void_p(l.ctypes.data), C.c_void_p(at(5)), C.c_uint64(4), C.c_void_p(at(6)), C.c_uint32(0),
            C.c_uint64(0), None, None, None, None, None, None, C.c_uint64(0), None, C.c_void_p(at(11) + 64), None]
    assert lib.sjmi_join_rows_device(None, *args) == -2  # (no context)
    assert S.binding.lib().sjmi_join_rows_device(ctx._h, None, *args[1:]) == -2 and S.binding.lib().sjmi_join_rows_device(ctx._h, *args[:4], None, *args[5:]) == -2


# ---- chained with the other operators, and end to end on the committed fixtures against Python's json -------------------------
def test_twitter_retweeted_users_against_the_mentions(ctx):
    """LEFT and INNER through BatchShard.join_rows, a status a document.  Left: the 100 statuses' /retweeted_status/user/id, 27 of
    them missing.  Right: the 87 exploded /entities/user_mentions/*/id, the live rows the explode's last offset read on the
    device, sorted once and probed twice.  3382 inner pairs, one key with 58 x 58 of them: more than three output chunks from a
    real document.  The pair offsets then go to parent_columns as row offsets ("left position = document, pair = row"), which
    must carry the same left cells onto the pairs as the join itself.  Last, the sides exchanged: the mentions as the left side
    behind the same device count"""
    import torch
    import simdjson_java_amd as S
    docs = SC.reserialised("twitter.json", lambda d: d["statuses"])
    statuses = [json.loads(d) for d in docs]
    n = len(statuses)
    keys = [s["retweeted_status"]["user"]["id"] if "retweeted_status" in s else None for s in statuses]
    mentions = [(r, m["id"]) for r, s in enumerate(statuses) for m in s["entities"]["user_mentions"]]
    by_id = {}
    for place, (_, uid) in enumerate(mentions):
        by_id.setdefault(uid, []).append(place)
    inner = [(r, p) for r in range(n) if keys[r] is not None for p in by_id.get(keys[r], [])]
    left_pairs = [pair for r in range(n) for pair in ([(r, p) for p in by_id.get(keys[r], [])] or [(r, -1)])]
    assert (n, keys.count(None), len(mentions), len(inner)) == (100, 27, 87, 3382) and max(len(v) for v in by_id.values()) == 58
    matched = sum(1 for k in keys if k in by_id)
    shard, _, _ = parse(ctx, docs)
    stream = torch.cuda.current_stream().cuda_stream
    lplan, rplan = S.SelectPlan(["/retweeted_status/user/id", "/id"]), S.ExplodePlan("/entities/user_mentions", ["/id", "/screen_name"])
    ltypes, lvalues = shard.select(lplan, stream)
    capacity = len(mentions) + 9
    roffs, rtypes, rvalues = shard.explode(rplan, capacity, stream)
    count = roffs[shard.n_docs:]
    sorted_right = None
    for how, want in (("inner", inner), ("left", left_pairs)):
        res = shard.join_rows((ltypes[0], lvalues[0]), (rtypes[0], rvalues[0]), how=how, left=(ltypes, lvalues), right=(rtypes, rvalues),
                              right_count=count, right_sorted=sorted_right, pair_capacity=4096, with_offsets=True, stream=stream)
        left_rows, right_rows, lt, lv, rt, rv, offsets, record, sorted_right = res
        _, parents, pt, pv, pres = shard.parent_columns(offsets, ltypes, lvalues, n_rows=4096, row_count=record[2:3], stream=stream)
        torch.cuda.synchronize()
        k = len(want)
        assert record.cpu().tolist() == [n, len(mentions), k, matched, keys.count(None), 0, 0, 0, 0]
        assert list(zip(left_rows.cpu().tolist()[:k], right_rows.cpu().tolist()[:k])) == want
        assert lv[1].cpu().tolist()[:k] == [statuses[r]["id"] for r, _ in want] and lt[1].cpu().tolist()[:k] == [ord("l")] * k
        assert rv[0].cpu().tolist()[:k] == [mentions[p][1] if p >= 0 else 0 for _, p in want]
        assert rt[0].cpu().tolist()[:k] == [ord("l") if p >= 0 else 0 for _, p in want]
        assert offsets.cpu().tolist()[n] == k and pres.cpu().tolist()[:2] == [k, 0] and parents.cpu().tolist()[:k] == [r for r, _ in want]
        assert torch.equal(pt[:, :k], lt[:, :k]) and torch.equal(pv[:, :k], lv[:, :k])
    # the mentions of a retweeted user: the left side is the explode, its live rows the last offset
    got = shard.join_rows((rtypes[0], rvalues[0]), (ltypes[0], lvalues[0]), how="semi", left=(rtypes, rvalues), left_count=count,
                          pair_capacity=capacity, stream=stream)
    torch.cuda.synchronize()
    retweeted = {k for k in keys if k is not None}
    want = [p for p, (_, uid) in enumerate(mentions) if uid in retweeted]
    assert got[7].cpu().tolist() == [len(mentions), n - keys.count(None), len(want), len(want), 0, 0, 0, 0, 0] and len(want) > 50
    assert got[0].cpu().tolist()[:len(want)] == want and got[3][0].cpu().tolist()[:len(want)] == [mentions[p][1] for p in want]
    lplan.close()
    rplan.close()


def test_github_actors_against_themselves_behind_filters(ctx):
    """the events' /actor/id joined with itself: 30 rows, 32 pairs.  Then the left side as a filter's selection with its n_kept
    read on the device, and the right side sorted behind the same filter"""
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    docs = [json.loads(e) for e in events]
    n = len(docs)
    actor = [d["actor"]["id"] for d in docs]
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/actor/id", "/id", "/type"])
    types, values = shard.select(plan, stream)
    key = (types[0], values[0])
    left_rows, right_rows, lt, lv, rt, rv, _, record, _ = shard.join_rows(key, key, left=(types, values), right=(types, values), pair_capacity=64, stream=stream)
    torch.cuda.synchronize()
    want = [(a, b) for a in range(n) for b in range(n) if actor[a] == actor[b]]
    assert (n, len(want)) == (30, 32) and record.cpu().tolist() == [n, n, 32, n, 0, 0, 0, 0, 0]
    assert list(zip(left_rows.cpu().tolist()[:32], right_rows.cpu().tolist()[:32])) == want
    assert lv[0].cpu().tolist()[:32] == [actor[a] for a, _ in want] and torch.equal(lv[:, :32], values[:, left_rows[:32]])
    assert torch.equal(rv[0][:32], lv[0][:32]) and torch.equal(rt[:, :32], types[:, right_rows[:32]]) and torch.equal(rv[:, :32], values[:, right_rows[:32]])
    flt = S.FilterPlan([(2, "string_eq", "PushEvent")])
    kept_rows, _, _, _, fres = shard.filter(flt, types, values, stream=stream)
    kept = [r for r in range(n) if docs[r]["type"] == "PushEvent"]
    for how in ("inner", "left", "semi", "anti"):
        got = shard.join_rows(key, key, how=how, left_rows=kept_rows, left_count=fres[0:1], right_rows=kept_rows, right_count=fres[0:1],
                              pair_capacity=64, stream=stream)
        torch.cuda.synchronize()
        pairs = {"inner": [(a, b) for a in kept for b in kept if actor[a] == actor[b]], "semi": [(a, None) for a in kept], "anti": []}
        pairs["left"] = pairs["inner"]
        rec = got[7].cpu().tolist()
        assert rec == [len(kept), len(kept), len(pairs[how]), len(kept), 0, 0, 0, 0, 0] and 7 < len(kept) < n
        assert got[0].cpu().tolist()[:rec[2]] == [a for a, _ in pairs[how]]
        if how in ("inner", "left"):
            assert got[1].cpu().tolist()[:rec[2]] == [b for _, b in pairs[how]]
        else:
            assert got[1] is None
    flt.close()
    plan.close()
