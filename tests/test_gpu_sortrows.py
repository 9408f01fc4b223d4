"""All rows ordered by a column on the GPU (sjmi_sort_rows_device through Context.sort_rows_device / BatchShard.sort_rows): the
rows, the carried cells and the record against the reference of tests/sortrows_common.py, with canaries in front of and behind
every output and the types columns at odd alignments; the shapes of the host simulation's tests; a million rows per kind twice
(several workgroups per kernel and a scan of more than one trip run only here); live positions from a filter's n_kept and an
explode's last offset; behind timestamp_columns; chained keys on the committed fixtures against Python's json and sorted; and
top_rows with k = live.  All results are integers: every comparison is an equality.  Every input is legal, or is answered by
SJMI_ERR_ARG before any launch."""
import ctypes as C
import datetime
import functools
import json

import numpy as np
import pytest

from tests import select_common as SC
from tests import sortrows_common as SO
from tests import toprows_common as TC
from tests.test_gpu_explode import parse
from tests.test_host_sortrows import POSITIONS, SPREAD_BITS, TILE, check, longs_column, spread_column

pytestmark = pytest.mark.gpu

CANARY = 0x0C0FFEE0DDF00D55
MILLION = 1024 * 1024 + 1
L, D = TC.LONG, TC.DOUBLE


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def sort_rows(ctx, types, words, values, kind, descending, rows_in=None, n_rows=None, carry=None, row_count=None, shift=0, pad=3):
    """Context.sort_rows_device on numpy columns -> (rows uint64 [n_rows], out_types [n_cols, stride], out_values [n_cols, stride],
    result [9]); every output lies between canaries, the types columns `shift` bytes into their buffers (any alignment); the
    canaries and the entries at or behind `live` are checked here"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_source = values.size
    n_rows = (n_source if rows_in is None else rows_in.size) if n_rows is None else n_rows
    n_cols = 0 if carry is None else carry[0].shape[0]
    col_stride = 0 if carry is None else carry[0].shape[1]
    stride = n_rows + pad if n_cols else 0
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    moved = lambda a: up(np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])) if a is not None and a.size else None
    d_kt, d_ct = moved(types), moved(None if carry is None else carry[0])
    d_words = up(words) if words is not None and words.size else None
    d_values = up(values) if values.size else None
    d_in = up(rows_in) if rows_in is not None and rows_in.size else None
    d_cv = up(carry[1]) if carry is not None and carry[1].size else None
    d_rows = up(np.full(n_rows + 16, CANARY, dtype=np.uint64))
    d_ov = up(np.full(n_cols * stride + 16, CANARY, dtype=np.uint64))
    d_ot = up(np.full(n_cols * stride + 16 + shift, 0xC5, dtype=np.uint8))
    d_res = up(np.full(SO.RESULT_WORDS + 2, CANARY, dtype=np.uint64))
    d_rc = None if row_count is None else torch.tensor([row_count], dtype=torch.int64, device=dev)
    ptr = lambda t, off=0: t.data_ptr() + off if t is not None else 0
    ctx.sort_rows_device(ptr(d_kt, shift), ptr(d_words), ptr(d_values), n_source, ptr(d_in), n_rows, ptr(d_rc), kind,
                         SO.DESCENDING if descending else 0, ptr(d_ct, shift), ptr(d_cv), n_cols, col_stride, d_rows.data_ptr() + 64 if n_rows else 0,
                         d_ot.data_ptr() + 8 + shift if n_cols * stride else 0, d_ov.data_ptr() + 64 if n_cols * stride else 0, stride,
                         d_res.data_ptr() + 8, stream)
    torch.cuda.synchronize()
    rows, ov = d_rows.cpu().numpy().view(np.uint64), d_ov.cpu().numpy().view(np.uint64)
    ot, result = d_ot.cpu().numpy(), d_res.cpu().numpy().view(np.uint64)
    live = int(result[1])
    assert live <= n_rows and result[0] == CANARY and result[-1] == CANARY
    assert (rows[:8] == CANARY).all() and (rows[8 + live:] == CANARY).all(), "a word outside rows[0, live) was written"
    cv, ct = ov[8:8 + n_cols * stride].reshape(n_cols, stride), ot[8 + shift:8 + shift + n_cols * stride].reshape(n_cols, stride)
    assert (ov[:8] == CANARY).all() and (ov[8 + n_cols * stride:] == CANARY).all() and (cv[:, live:] == CANARY).all()
    assert (ot[:8 + shift] == 0xC5).all() and (ot[8 + shift + n_cols * stride:] == 0xC5).all() and (ct[:, live:] == 0xC5).all()
    return rows[8:8 + n_rows].copy(), ct.copy(), cv.copy(), result[1:-1].copy()


@pytest.fixture(scope="module")
def gpu(ctx):
    return lambda *a, **kw: sort_rows(ctx, *a, **kw)


@pytest.mark.parametrize("n_rows", POSITIONS)
def test_positions_in_both_kinds_and_directions(gpu, n_rows):
    for what, kind in (("longs", L), ("counters", L), ("doubles", D)):
        types, values = TC.typed_column(n_rows, 100 + n_rows, what)
        words, bits = TC.validity(n_rows, n_rows)
        carry = TC.carried(2, n_rows, n_rows + 5, n_rows)
        for descending in (False, True):
            check(gpu, types, words, bits, values, kind, descending, carry=carry, what=(n_rows, what, descending), shift=(n_rows + descending) % 8)


def test_every_number_of_digit_passes(gpu):
    for bit in SPREAD_BITS:
        types, values = spread_column(TILE + 77, bit, bit)
        _, want = check(gpu, types, None, None, values, L, bit % 2 == 0, what=bit)
        assert want[7] == bit // 8 + 1
    for n in (1, 1025, 2 * TILE + 1):  # (one value only: nothing moves)
        types, values = longs_column([42] * n)
        rows, want = check(gpu, types, None, None, values, L, True)
        assert want[7] == 0 and rows.tolist() == list(range(n))


def test_bins_of_a_tile_and_the_ends_of_the_range(gpu):
    n = 3 * TILE
    one = np.full(n, 7, dtype=np.int64)
    one[TILE:2 * TILE] = 9
    every = np.arange(n, dtype=np.int64) % 256
    straddle = np.repeat(np.arange(6, dtype=np.int64)[::-1], n // 6)
    straddle[TILE - 3:TILE + 3] = 200
    ends = np.array([TC.INT64_MAX, TC.INT64_MIN, 0, -1, TC.INT64_MIN, TC.INT64_MAX, 1] * 30, dtype=np.int64)
    for vals in (one, every, every[::-1].copy(), straddle, (every << 8) | 3, ends):
        types, values = longs_column(vals)
        for descending in (False, True):
            check(gpu, types, None, None, values, L, descending)


def test_zeros_infinities_nans_and_longs_that_round(gpu):
    xs = [0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 5e-324, -5e-324, 2.2e-308 / 4, -2.2e-308 / 4] * 40
    values = np.array(xs, dtype=np.float64).view(np.uint64).copy()
    for k, nan in enumerate(TC.NAN_BITS):
        values[7 + 13 * k] = nan
    types = np.full(values.size, ord("d"), dtype=np.uint8)
    for descending in (False, True):
        rows, want = check(gpu, types, None, None, values, D, descending)
        assert want[4] == len(TC.NAN_BITS) and rows[want[1]:].tolist() == [7 + 13 * k for k in range(len(TC.NAN_BITS))]
    types, values = np.full(200, ord("d"), dtype=np.uint8), np.array([0.0, -0.0] * 100).view(np.uint64)
    rows, _ = check(gpu, types, None, None, values, D, False)
    assert rows.tolist() == list(range(1, 200, 2)) + list(range(0, 200, 2))
    types, values = longs_column([(1 << 53) + 1, 1 << 53, (1 << 53) + 2, 5, (1 << 53) + 3, -(1 << 53) - 1])
    rows, want = check(gpu, types, None, None, values, D, False)
    assert want[5] == 3 and rows.tolist() == [5, 3, 0, 1, 2, 4]
    types, values = TC.typed_column(5000, 77, "doubles")
    _, want = check(gpu, types, None, None, values, D, True)
    assert want[5] > 50


@pytest.mark.parametrize("what", ["counters", "equal"])
def test_equal_values_keep_their_positions(gpu, what):
    """stability: a rank that depended on which wave ran first would fail here"""
    n = 5 * TILE + 500
    types, values = TC.typed_column(n, 31, what)
    rng = np.random.default_rng(31)
    perm = rng.permutation(n).astype(np.uint64)
    subset = np.nonzero(rng.random(n) < 0.4)[0].astype(np.uint64)
    for rows_in in (None, perm, subset):
        for descending in (False, True):
            check(gpu, types, None, None, values, L, descending, rows_in=rows_in, what=(what, descending))


def test_bad_entries_are_counted_and_ordered_with_the_nulls(gpu):
    n = 1500
    types, values = TC.typed_column(n, 8, "longs")
    words, bits = TC.validity(n, 8)
    rows_in = np.random.default_rng(8).permutation(n).astype(np.uint64)
    for k, i in enumerate([0, 63, 64, 700, 1024, 1499]):
        rows_in[i] = ((n,) + SO.BAD_ENTRIES)[k % 3]
    carry = TC.carried(2, n, n, 8)
    for descending in (False, True):
        _, want = check(gpu, types, words, bits, values, L, descending, rows_in=rows_in, carry=carry, shift=1)
        assert want[6] == 6 and want[8] == SO.BAD_ROW
    all_bad = np.array([5, 6, SO.BAD_ENTRIES[1]], dtype=np.uint64)
    _, want = check(gpu, types[:5], None, None, values[:5], L, False, rows_in=all_bad, carry=TC.carried(1, 5, 5, 1))
    assert want == [3, 0, 0, 0, 0, 0, 3, 0, 1]
    _, want = check(gpu, types[:0], None, None, values[:0], L, False, rows_in=all_bad)  # (no source row at all)
    assert want == [3, 0, 0, 0, 0, 0, 3, 0, 1]


@pytest.mark.parametrize("n_keys", [2, 3])
def test_chained_keys_against_lexsort(gpu, n_keys):
    n = TILE + 333
    rng = np.random.default_rng(n_keys)
    cols = [rng.integers(0, m, n, dtype=np.int64) for m in (5, 7, 1000)][:n_keys]
    descending = [False, True, False][:n_keys]
    rows = None
    for vals, desc in list(zip(cols, descending))[::-1]:
        types, values = longs_column(vals)
        rows, _ = check(gpu, types, None, None, values, L, desc, rows_in=rows)
    assert rows.tolist() == np.lexsort(tuple(-v if d else v for v, d in list(zip(cols, descending))[::-1])).tolist()


@functools.lru_cache(maxsize=None)
def million(what):
    """the column of the million-row tests and what it must give, made once: (types, words, bits, values, kind, carried, want)"""
    types, values = TC.typed_column(MILLION, 17, what)
    words, bits = TC.validity(MILLION, 17)
    kind = D if what == "doubles" else L
    return types, words, bits, values, kind, TC.carried(1, MILLION, MILLION, 17), SO.expected(types, bits, values, None, MILLION, MILLION, kind, False)


@pytest.mark.parametrize("what", ["longs", "doubles"])
def test_a_million_rows_twice(gpu, what):
    """1024 x 1024 + 1 positions: 257 tiles and 1025 chunks, several workgroups in every kernel.  Both runs equal to the reference,
    and their complete outputs byte-equal to each other"""
    types, words, bits, values, kind, carry, want = million(what)
    a = gpu(types, words, values, kind, False, None, None, carry, shift=3)
    b = gpu(types, words, values, kind, False, None, None, carry, shift=3)
    assert all((x == y).all() for x, y in zip(a, b))
    live = want[1][0]
    assert [int(x) for x in a[3]] == want[1] and (a[0][:live] == want[0]).all()
    assert (a[2][0, :live] == carry[1][0, want[0].astype(np.int64)]).all() and (a[1][0, :live] == carry[0][0, want[0].astype(np.int64)]).all()
    assert want[1][7] == 8


def test_live_positions_from_the_device(gpu):
    types, values = TC.typed_column(3000, 5, "longs")
    words, bits = TC.validity(3000, 5)
    rows_in = np.random.default_rng(5).permutation(3000).astype(np.uint64)
    for row_count in (0, 1, 64, 1024, 2999, 3000, 5000, 1 << 50):
        live = min(3000, row_count)
        poisoned = rows_in.copy()
        poisoned[live:] = SO.BAD_ENTRIES[1]  # (would be counted if it were read)
        want = SO.expected(types, bits, values, rows_in, 3000, live, L, False)
        check(gpu, types, words, bits, values, L, False, rows_in=poisoned, row_count=row_count, want=want, what=row_count)
    check(gpu, types, words, bits, values, L, True, n_rows=700)
    _, want = check(gpu, types[:0], None, None, values[:0], L, False)
    assert want == [0] * 9
    types[:] = ord("t")
    check(gpu, types, None, None, values, L, False, carry=TC.carried(1, 3000, 3000, 2))  # (no candidate)


def test_the_first_rows_are_top_rows_with_k_live(ctx, gpu):
    """where live <= 2048 the candidates come out as top_rows ranks them, and the other classes follow"""
    from tests.test_gpu_toprows import top_rows
    for n, what, kind in ((2048, "counters", L), (1500, "doubles", D), (65, "longs", L)):
        types, values = TC.typed_column(n, 44, what)
        words, bits = TC.validity(n, 44)
        for descending in (False, True):
            rows, want = check(gpu, types, words, bits, values, kind, descending)
            top, _, _, result = top_rows(ctx, types, words, values, kind, descending, n)
            assert int(result[6]) == want[1] and rows[:want[1]].tolist() == top[:want[1]].tolist()
            assert [int(x) for x in result[:6]] == want[:6]


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ty = torch.zeros(64, dtype=torch.uint8, device=dev)
    w = torch.zeros(160, dtype=torch.int64, device=dev)
    T, Wp = ty.data_ptr(), w.data_ptr()
    good = dict(d_key_types=T, d_key_validity=Wp, d_key_values=Wp + 64, n_source_rows=4, d_rows_in=Wp + 640, n_rows=4, d_row_count=Wp + 8, kind=L,
                flags=0, d_types=T + 16, d_values=Wp + 128, n_cols=1, col_stride=4, d_rows=Wp + 256, d_out_types=T + 32, d_out_values=Wp + 320,
                out_stride=4, d_result=Wp + 512)
    ctx.sort_rows_device(**good)
    ctx.sort_rows_device(**dict(good, d_key_types=T + 3, d_types=T + 17, d_out_types=T + 33))  # (types: any alignment)
    ctx.sort_rows_device(**dict(good, d_key_types=0, d_key_validity=0, d_row_count=0, d_rows_in=0, flags=1))
    ctx.sort_rows_device(**dict(good, n_rows=0, d_rows=0, d_rows_in=0, d_types=0, d_values=0, d_out_types=0, d_out_values=0))
    ctx.sort_rows_device(**dict(good, n_cols=0, col_stride=0, out_stride=0, d_types=0, d_values=0, d_out_types=0, d_out_values=0))
    ctx.sort_rows_device(**dict(good, n_rows=5, out_stride=5))  # (with rows_in there may be more positions than rows)
    ctx.sort_rows_device(0, 0, 0, 0, 0, 0, 0, L, 0, 0, 0, 0, 0, 0, 0, 0, 0, Wp + 512)  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[64:73].tolist() == [0] * 9
    bad = [dict(d_result=0), dict(kind=0), dict(kind=3), dict(flags=2), dict(flags=3), dict(n_rows=1 << 32, out_stride=1 << 32),
           dict(n_source_rows=1 << 32, col_stride=1 << 32), dict(d_rows_in=0, n_rows=5, out_stride=5), dict(d_key_values=0), dict(d_rows=0),
           dict(d_types=0), dict(d_values=0), dict(d_out_types=0), dict(d_out_values=0), dict(col_stride=3), dict(out_stride=3),
           dict(d_key_validity=Wp + 4), dict(d_key_values=Wp + 68), dict(d_rows_in=Wp + 644), dict(d_row_count=Wp + 12), dict(d_values=Wp + 132),
           dict(d_rows=Wp + 260), dict(d_out_values=Wp + 324), dict(d_result=Wp + 516)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.sort_rows_device(**dict(good, **change))
    assert C.CDLL(S.lib_path()).sjmi_sort_rows_device(None, T, Wp, Wp + 64, 4, None, 4, None, L, 0, None, None, 0, 0, Wp + 256, None, None, 0,
                                                      Wp + 512, None) == -2  # (no context)


# ---- end to end on the committed fixtures, against Python's json and sorted (stable) ------------------------------------------
def test_twitter_statuses_by_lang_then_retweets(ctx):
    """/statuses exploded; the live rows are the explode's last offset, read on the device, below the row capacity; the first key
    is the dictionary index of /user/lang (validity, no types), the second /retweet_count descending; /id travels along"""
    import torch
    import simdjson_java_amd as S
    from tests.conftest import load_fixture
    doc = load_fixture("twitter.json")
    statuses = json.loads(doc)["statuses"]
    n = len(statuses)
    first_seen = {}
    for s in statuses:
        first_seen.setdefault(s["user"]["lang"], len(first_seen))
    want = sorted(range(n), key=lambda r: (first_seen[statuses[r]["user"]["lang"]], -statuses[r]["retweet_count"]))  # (stable)
    assert len(first_seen) > 2 and len({(s["user"]["lang"], s["retweet_count"]) for s in statuses}) < n  # (ties are there)
    shard, _, _ = parse(ctx, [doc])
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.ExplodePlan("/statuses", ["/user/lang", "/retweet_count", "/id"])
    capacity = n + 29
    offs, types, values = shard.explode(plan, capacity, stream)
    count = offs[shard.n_docs:]
    indices, validity, _, _, _, dres = shard.dictionary_column(types[0], values[0], 64, byte_capacity=4096, row_count=count, stream=stream)
    lang = torch.zeros(capacity, dtype=torch.int64, device=indices.device)
    lang[:n] = indices[:n]  # (entries at or behind the live rows are not written by the dictionary, and not read by the sort)
    rows, out_types, out_values, records = shard.sort_rows([(None, lang, "long", False, validity), (types[1], values[1], "long", True)],
                                                           types=types[2:], values=values[2:], row_count=count, stream=stream)
    torch.cuda.synchronize()
    assert int(dres.cpu()[3]) == len(first_seen)
    assert rows.cpu().tolist()[:n] == want and rows.shape == (capacity,) and out_values.shape == (1, capacity)
    assert out_values[0].cpu().tolist()[:n] == [statuses[r]["id"] for r in want] and out_types[0].cpu().tolist()[:n] == [ord("l")] * n
    rec = records.cpu().tolist()
    assert rec[0][:7] == [n, n, 0, 0, 0, 0, 0] and rec[1][:7] == [n, n, 0, 0, 0, 0, 0] and rec[0][8] == rec[1][8] == 0
    plan.close()


def test_github_events_by_payload_size_behind_a_filter_and_timestamps(ctx):
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    docs = [json.loads(e) for e in events]
    n = len(docs)

    def size(d):
        v = d.get("payload", {}).get("size")
        return v if isinstance(v, int) and not isinstance(v, bool) else None

    with_size = [r for r in range(n) if size(docs[r]) is not None]
    want = sorted(with_size, key=lambda r: size(docs[r])) + [r for r in range(n) if size(docs[r]) is None]
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/payload/size", "/repo/id", "/type", "/created_at"])
    types, values = shard.select(plan, stream)
    rows, out_types, out_values, records = shard.sort_rows([(types[0], values[0], "long", False)], types=types, values=values, stream=stream)
    torch.cuda.synchronize()
    rec = records.cpu().tolist()[0]
    assert 5 < len(with_size) < n and rows.cpu().tolist() == want and rec[:2] == [n, len(with_size)] and sum(rec[1:5]) + rec[6] == n
    assert out_values[1].cpu().tolist() == [docs[r]["repo"]["id"] for r in want]
    # behind a filter: its selection vector is rows_in, its n_kept the row count, read on the device
    flt = S.FilterPlan([(2, "string_eq", "PushEvent")])
    kept_rows, _, _, _, fres = shard.filter(flt, types, values, stream=stream)
    rows, _, out_values, records = shard.sort_rows([(types[1], values[1], "long", True)], types=types, values=values, rows=kept_rows,
                                                   row_count=fres[0:1], stream=stream)
    torch.cuda.synchronize()
    kept = [r for r in range(n) if docs[r]["type"] == "PushEvent"]
    want = sorted(kept, key=lambda r: -docs[r]["repo"]["id"])
    assert 7 < len(kept) < n and rows.cpu().tolist()[:len(kept)] == want and records.cpu().tolist()[0][:2] == [len(kept)] * 2
    assert out_values[1].cpu().tolist()[:len(kept)] == [docs[r]["repo"]["id"] for r in want]
    # behind timestamp_columns: data plus validity, no types
    stamps = [int(datetime.datetime.fromisoformat(d["created_at"].replace("Z", "+00:00")).timestamp()) for d in docs]
    data, validity, _ = shard.timestamp_columns([(3, "s")], types, values, stream=stream)
    for descending in (False, True):
        rows, _, _, records = shard.sort_rows([(None, data[0], "long", descending, validity[0])], stream=stream)
        torch.cuda.synchronize()
        assert rows.cpu().tolist() == sorted(range(n), key=lambda r: -stamps[r] if descending else stamps[r])
        assert records.cpu().tolist()[0][:7] == [n, n, 0, 0, 0, 0, 0]
    flt.close()
    plan.close()
