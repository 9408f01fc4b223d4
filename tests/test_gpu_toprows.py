"""The top k rows of a column on the GPU (sjmi_top_rows_device through Context.top_rows_device / BatchShard.top_rows): the rows, the
carried cells and the record against the reference of tests/toprows_common.py, with canaries in front of and behind every output
and the types columns at odd alignments; the shapes of the host simulation's tests; a million rows twice (several workgroups per
kernel and more than one trip of the capped grids run only here); live rows from a filter's n_kept and an explode's last offset;
behind timestamp_columns; the committed fixtures against Python's json.  All results are integers: every comparison is an
equality."""
import ctypes as C
import datetime
import functools
import json
import math

import numpy as np
import pytest

from tests import select_common as SC
from tests import toprows_common as TC
from tests.test_gpu_explode import parse
from tests.test_host_toprows import KS, ROWS, longs_column

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


def top_rows(ctx, types, words, values, kind, largest, k, carry=None, row_count=None, n_rows=None, shift=0):
    """Context.top_rows_device on numpy columns -> (rows uint64 [k], out_types [n_cols, k], out_values [n_cols, k], result [9]);
    every output lies between canaries, the types columns `shift` bytes into their buffers (any alignment); the canaries and the
    entries at or behind n_out are checked here"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_rows = values.size if n_rows is None else n_rows
    n_cols = 0 if carry is None else carry[0].shape[0]
    stride = 0 if carry is None else carry[0].shape[1]
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    moved = lambda a: up(np.concatenate([np.zeros(shift, dtype=np.uint8), a.reshape(-1)])) if a is not None and a.size else None
    d_kt, d_ct = moved(types), moved(None if carry is None else carry[0])
    d_words = up(words) if words is not None and words.size else None
    d_values = up(values) if values.size else None
    d_cv = up(carry[1]) if carry is not None and carry[1].size else None
    d_rows = up(np.full(k + 16, CANARY, dtype=np.uint64))
    d_ov = up(np.full(n_cols * k + 16, CANARY, dtype=np.uint64))
    d_ot = up(np.full(n_cols * k + 16 + shift, 0xC5, dtype=np.uint8))
    d_res = up(np.full(TC.RESULT_WORDS + 2, CANARY, dtype=np.uint64))
    d_rc = None if row_count is None else torch.tensor([row_count], dtype=torch.int64, device=dev)
    ptr = lambda t, off=0: t.data_ptr() + off if t is not None else 0
    ctx.top_rows_device(ptr(d_kt, shift), ptr(d_words), ptr(d_values), n_rows, ptr(d_rc), kind, 0 if largest else TC.SMALLEST, k, ptr(d_ct, shift),
                        ptr(d_cv), n_cols, stride, d_rows.data_ptr() + 64 if k else 0, d_ot.data_ptr() + 8 + shift if n_cols * k else 0,
                        d_ov.data_ptr() + 64 if n_cols * k else 0, d_res.data_ptr() + 8, stream)
    torch.cuda.synchronize()
    rows, ov = d_rows.cpu().numpy().view(np.uint64), d_ov.cpu().numpy().view(np.uint64)
    ot, result = d_ot.cpu().numpy(), d_res.cpu().numpy().view(np.uint64)
    n_out = int(result[7])
    assert n_out <= k and result[0] == CANARY and result[-1] == CANARY
    assert (rows[:8] == CANARY).all() and (rows[8 + n_out:] == CANARY).all(), "a word outside rows[0, n_out) was written"
    cv, ct = ov[8:8 + n_cols * k].reshape(n_cols, k), ot[8 + shift:8 + shift + n_cols * k].reshape(n_cols, k)
    assert (ov[:8] == CANARY).all() and (ov[8 + n_cols * k:] == CANARY).all() and (cv[:, n_out:] == CANARY).all()
    assert (ot[:8 + shift] == 0xC5).all() and (ot[8 + shift + n_cols * k:] == 0xC5).all() and (ct[:, n_out:] == 0xC5).all()
    return rows[8:8 + k].copy(), ct.copy(), cv.copy(), result[1:-1].copy()


def check(ctx, types, words, bits, values, kind, largest, k, carry=None, row_count=None, what="", want=None, **kw):
    n_rows = kw.get("n_rows", values.size)
    live = n_rows if row_count is None else min(n_rows, row_count)
    want_rows, want = want or TC.expected(types, bits, values, live, kind, largest, k)
    got = top_rows(ctx, types, words, values, kind, largest, k, carry, row_count, **kw)
    rows, ot, ov, result = got
    assert [int(x) for x in result] == want, (what, [int(x) for x in result], want)
    n_out = want[6]
    assert rows[:n_out].astype(np.int64).tolist() == want_rows.tolist(), what
    if carry is not None:
        assert (ot[:, :n_out] == carry[0][:, want_rows]).all() and (ov[:, :n_out] == carry[1][:, want_rows]).all(), what
    return got, want_rows, want


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_k_in_both_kinds_and_directions(ctx, n_rows):
    for what, kind in (("longs", L), ("counters", L), ("doubles", D)):
        types, values = TC.typed_column(n_rows, 100 + n_rows, what)
        words, bits = TC.validity(n_rows, n_rows)
        carry = TC.carried(2, n_rows, n_rows + 5, n_rows)
        for largest in (True, False):
            for k in KS[::2] if largest else KS[1::2]:
                check(ctx, types, words, bits, values, kind, largest, k, carry, what=(n_rows, what, largest, k), shift=(n_rows + k) % 8)


@pytest.mark.parametrize("kind,what", [(L, "longs"), (D, "doubles")])
def test_the_four_forms_of_the_key_column(ctx, kind, what):
    n = 3000
    types, values = TC.typed_column(n, 3, what)
    words, bits = TC.validity(n, 3)
    plain = TC.longs_full(n, 4) if kind == L else TC.doubles_wide(n, 4)
    plain[::7] = TC.NAN_BITS[0]
    for largest in (True, False):
        for t, w, b, v in ((types, words, bits, values), (types, None, None, values), (None, words, bits, plain), (None, None, None, plain)):
            _, _, want = check(ctx, t, w, b, v, kind, largest, 100, TC.carried(1, n, n, 8), shift=3)
            assert want[6] == 100 and (t is not None or kind == L or want[4] > 0)


def test_shapes_where_the_select_can_go_wrong(ctx):
    rng = np.random.default_rng(2)
    # all equal; one bit; bit 63; every digit boundary
    for lo, hi in [(42, 42), (6, 7), (TC.INT64_MIN, TC.INT64_MAX)] + [(0x2AAAAAAAAAAAAAAA & ~(1 << b), 0x2AAAAAAAAAAAAAAA | (1 << b)) for b in TC.DIGIT_EDGES]:
        types, values = longs_column(np.where(rng.random(2500) < 0.4, lo, hi))
        for largest in (True, False):
            for k in (1, 1100, 2048):
                check(ctx, types, None, None, values, L, largest, k, what=(lo, hi, largest, k))
    # a tie group at the threshold across a wave, a chunk and the end, need_equal of 1 and of all but one
    n = 3 * 1024
    for first, last in ((60, 70), (1000, 1100), (1020, 2100)):
        vals = np.arange(n, dtype=np.int64) % 50
        vals[first:last] = 1000
        vals[5], vals[n - 5] = 5000, 5001
        ties = last - first
        types, values = longs_column(vals)
        for k in (3, 2 + ties - 1, 2 + ties):
            (rows, _, _, _), _, want = check(ctx, types, None, None, values, L, True, k, what=(first, last, k))
            assert rows[:k].tolist() == [n - 5, 5] + list(range(first, first + k - 2)) and want[7] == 1000
    # the threshold bin holds every candidate but one
    vals = (1 << 40) + (np.arange(4000, dtype=np.int64) * 7) % 2000
    vals[0] = (1 << 40) + (1 << 30)
    types, values = longs_column(vals)
    for k in (1, 2, 100):
        check(ctx, types, None, None, values, L, True, k)


def test_zeros_infinities_nans_and_longs_that_round(ctx):
    xs = [0.0, -0.0, math.inf, -math.inf, 1.5, -1.5, 5e-324, -5e-324] * 40
    values = np.array(xs, dtype=np.float64).view(np.uint64).copy()
    values[3::16] = TC.NAN_BITS[1]
    types = np.full(values.size, ord("d"), dtype=np.uint8)
    for largest in (True, False):
        for k in (1, 21, 100, 2048):
            _, _, want = check(ctx, types, None, None, values, D, largest, k)
            assert want[4] == 20
    types, values = np.full(200, ord("d"), dtype=np.uint8), np.array([0.0, -0.0] * 100).view(np.uint64)
    (rows, _, _, _), _, want = check(ctx, types, None, None, values, D, True, 101)
    assert rows.tolist() == list(range(0, 200, 2)) + [1] and want[7] == TC.bits_of(-0.0)
    types, values = longs_column([(1 << 53) + 1, 1 << 53, (1 << 53) + 2, 5, (1 << 53) + 3, -(1 << 53) - 1])
    (rows, _, _, _), _, want = check(ctx, types, None, None, values, D, True, 6)
    assert want[5] == 3 and rows.tolist() == [4, 2, 0, 1, 3, 5]


def test_a_value_word_behind_a_type_that_makes_no_candidate_changes_nothing(ctx):
    for kind, what in ((L, "longs"), (D, "doubles")):
        types, values = TC.typed_column(3000, 21, what)
        dead = (types != ord("l")) & ((types != ord("d")) | (kind == L))
        a = top_rows(ctx, types, None, values, kind, True, 500)
        for poison in (0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000):
            changed = values.copy()
            changed[dead] = poison
            b = top_rows(ctx, types, None, changed, kind, True, 500)
            assert all((x == y).all() for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def million(what):
    """the column of the million-row tests, made once: (types, words, bits, values, kind, carried)"""
    types, values = TC.typed_column(MILLION, 17, "longs" if what == "uniform" else what)
    words, bits = TC.validity(MILLION, 17)
    return types, words, bits, values, D if what == "doubles" else L, TC.carried(1, MILLION, MILLION, 17)


@pytest.mark.parametrize("k", [1, 100, 2048])
@pytest.mark.parametrize("what", ["uniform", "counters", "equal", "doubles"])
def test_a_million_rows_twice(ctx, what, k):
    """1024 x 1024 + 1 rows: more than one trip of the capped grids, 1025 chunks in the mark / scan / emit.  Both runs equal to the
    reference, and their complete outputs equal to each other"""
    types, words, bits, values, kind, carry = million(what)
    want = TC.expected(types, bits, values, MILLION, kind, True, k)
    a, _, _ = check(ctx, types, words, bits, values, kind, True, k, carry, what=(what, k, "first"), want=want, shift=3)
    b, _, _ = check(ctx, types, words, bits, values, kind, True, k, carry, what=(what, k, "second"), want=want, shift=3)
    assert all((x == y).all() for x, y in zip(a, b))
    assert want[1][6] == k and (what != "equal" or want[0].tolist() == np.nonzero(bits & (types == ord("l")))[0][:k].tolist())


def test_live_rows_from_the_device(ctx):
    types, values = TC.typed_column(3000, 5, "longs")
    words, bits = TC.validity(3000, 5)
    for row_count in (0, 1, 64, 1024, 2999, 3000, 5000, 1 << 50):
        live = min(3000, row_count)
        ty, va = types.copy(), values.copy()
        ty[live:], va[live:] = ord("l"), TC.INT64_MAX  # (what lies at or above the live rows would win if it were read)
        want = TC.expected(types, bits, values, live, L, True, 70)
        check(ctx, ty, words, bits, va, L, True, 70, row_count=row_count, want=want, what=row_count)
    check(ctx, types, words, bits, values, L, False, 9, n_rows=700)
    _, _, want = check(ctx, types[:0], None, None, values[:0], L, True, 9)
    assert want == [0] * 9


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ty = torch.zeros(64, dtype=torch.uint8, device=dev)
    w = torch.zeros(128, dtype=torch.int64, device=dev)
    T, Wp = ty.data_ptr(), w.data_ptr()
    good = dict(d_key_types=T, d_key_validity=Wp, d_key_values=Wp + 64, n_rows=4, d_row_count=Wp + 8, kind=L, flags=0, k=2, d_types=T + 16,
                d_values=Wp + 128, n_cols=1, col_stride=4, d_rows=Wp + 256, d_out_types=T + 32, d_out_values=Wp + 320, d_result=Wp + 512)
    ctx.top_rows_device(**good)
    ctx.top_rows_device(**dict(good, d_key_types=T + 3, d_types=T + 17, d_out_types=T + 33))  # (types: any alignment)
    ctx.top_rows_device(**dict(good, d_key_types=0, d_key_validity=0, d_row_count=0, flags=1))  # (both NULL: every live row is a candidate)
    ctx.top_rows_device(**dict(good, k=0, d_rows=0, d_types=0, d_values=0, d_out_types=0, d_out_values=0))
    ctx.top_rows_device(**dict(good, n_cols=0, col_stride=0, d_types=0, d_values=0, d_out_types=0, d_out_values=0))
    ctx.top_rows_device(0, 0, 0, 0, 0, L, 0, 0, 0, 0, 0, 0, 0, 0, 0, Wp + 512)  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[64:73].tolist() == [0] * 9
    bad = [dict(d_result=0), dict(kind=0), dict(kind=3), dict(flags=2), dict(flags=3), dict(k=2049), dict(n_rows=1 << 32, col_stride=1 << 32),
           dict(d_key_values=0), dict(d_rows=0), dict(d_types=0), dict(d_values=0), dict(d_out_types=0), dict(d_out_values=0), dict(col_stride=3),
           dict(d_key_validity=Wp + 4), dict(d_key_values=Wp + 68), dict(d_row_count=Wp + 12), dict(d_values=Wp + 132), dict(d_rows=Wp + 260),
           dict(d_out_values=Wp + 324), dict(d_result=Wp + 516)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.top_rows_device(**dict(good, **change))
    assert C.CDLL(S.lib_path()).sjmi_top_rows_device(None, T, Wp, Wp + 64, 4, None, L, 0, 2, None, None, 0, 0, Wp + 256, None, None, Wp + 512,
                                                     None) == -2  # (no context)


# ---- end to end on the committed fixtures, against Python's json ---------------------------------------------------------------
def python_top(rows, pointer, k, largest=True):
    """rows: json.loads documents -> the indices of the k rows whose value at `pointer` is an int (no bool), by (value, row)"""
    cand = []
    for r, row in enumerate(rows):
        cur = row
        for token in pointer.split("/")[1:]:
            cur = cur.get(token) if isinstance(cur, dict) else None
        if isinstance(cur, int) and not isinstance(cur, bool):
            cand.append((-cur if largest else cur, r))
    return [r for _, r in sorted(cand)[:k]], len(cand)


def test_twitter_statuses_with_the_most_retweets(ctx):
    """/statuses exploded; the live rows are the explode's last offset, read on the device, below the row capacity; /id and
    /user/screen_name travel along, and the carried string cells go through string_column as they are"""
    import torch
    import simdjson_java_amd as S
    from tests.conftest import load_fixture
    doc = load_fixture("twitter.json")
    statuses = json.loads(doc)["statuses"]
    want, n_cand = python_top(statuses, "/retweet_count", 10)
    assert n_cand == len(statuses) and len({s["retweet_count"] for s in statuses}) < len(statuses)  # (ties are there)
    shard, _, _ = parse(ctx, [doc])
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.ExplodePlan("/statuses", ["/retweet_count", "/id", "/user/screen_name"])
    offs, types, values = shard.explode(plan, len(statuses) + 29, stream)
    rows, out_types, out_values, result = shard.top_rows(types[0], values[0], 10, types=types[1:], values=values[1:],
                                                         row_count=offs[shard.n_docs:], stream=stream)
    offsets, _, data, sres = shard.string_column(out_types[1], out_values[1], stream=stream)
    torch.cuda.synchronize()
    n = len(statuses)
    assert rows.cpu().tolist() == want
    assert result.cpu().tolist() == [n, n, 0, 0, 0, 0, 10, statuses[want[-1]]["retweet_count"], 0]
    assert out_types[0].cpu().tolist() == [ord("l")] * 10 and out_values[0].cpu().tolist() == [statuses[r]["id"] for r in want]
    ends, raw = offsets.cpu().numpy(), bytes(data.cpu().numpy())
    assert [raw[int(ends[j]):int(ends[j + 1])].decode() for j in range(10)] == [statuses[r]["user"]["screen_name"] for r in want]
    assert int(sres.cpu()[1]) == 10
    # the ten with the fewest, as doubles: the same order of equal counts, by row
    rows, _, _, result = shard.top_rows(types[0], values[0], 10, kind="double", largest=False, row_count=offs[shard.n_docs:], stream=stream)
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == python_top(statuses, "/retweet_count", 10, largest=False)[0] and int(result.cpu()[5]) == 0
    plan.close()


def test_github_events_by_payload_size_and_behind_a_filter(ctx):
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    docs = [json.loads(e) for e in events]
    want, n_cand = python_top(docs, "/payload/size", 5)
    assert 5 < n_cand < len(docs)
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/payload/size", "/repo/id", "/type"])
    types, values = shard.select(plan, stream)
    rows, out_types, out_values, result = shard.top_rows(types[0], values[0], 5, types=types, values=values, stream=stream)
    torch.cuda.synchronize()
    res = result.cpu().tolist()
    assert rows.cpu().tolist() == want and res[:2] == [len(docs), n_cand] and res[1] + res[2] + res[3] + res[4] == res[0] and res[6] == 5
    assert out_values[1].cpu().tolist() == [d["repo"]["id"] for d in (docs[r] for r in want)]
    # more than there are: all of them, in order
    rows, _, _, result = shard.top_rows(types[0], values[0], 2048, largest=False, stream=stream)
    torch.cuda.synchronize()
    assert rows.cpu().tolist()[:n_cand] == python_top(docs, "/payload/size", 2048, largest=False)[0] and int(result.cpu()[6]) == n_cand
    # behind a filter: its n_kept is the row count, read on the device; the compacted columns are not written behind it
    kept_docs = [d for d in docs if d["type"] == "PushEvent"]
    flt = S.FilterPlan([(2, "string_eq", "PushEvent")])
    _, f_types, f_values, _, fres = shard.filter(flt, types, values, stream=stream)
    rows, out_types, out_values, result = shard.top_rows(f_types[1], f_values[1], 7, types=f_types, values=f_values, row_count=fres[0:1], stream=stream)
    torch.cuda.synchronize()
    want, n_cand = python_top(kept_docs, "/repo/id", 7)
    assert 7 < n_cand == len(kept_docs) < len(docs)
    assert rows.cpu().tolist() == want and result.cpu().tolist()[:2] == [len(kept_docs)] * 2
    assert out_values[1].cpu().tolist() == [kept_docs[r]["repo"]["id"] for r in want] and out_types[2].cpu().tolist() == [ord('"')] * 7
    flt.close()
    plan.close()


def test_the_latest_events_behind_timestamp_columns(ctx):
    """data plus validity, no types: a finished Arrow array"""
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    stamps = [int(datetime.datetime.fromisoformat(json.loads(e)["created_at"].replace("Z", "+00:00")).timestamp()) for e in events]
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/created_at", "/payload/size"])
    types, values = shard.select(plan, stream)
    data, validity, _ = shard.timestamp_columns([(0, "s"), (1, "s")], types, values, stream=stream)
    for largest in (True, False):
        rows, _, _, result = shard.top_rows(None, data[0], 50, largest=largest, key_validity=validity[0], stream=stream)
        torch.cuda.synchronize()
        order = sorted(range(len(stamps)), key=lambda r: (-stamps[r] if largest else stamps[r], r))[:50]
        n = len(stamps)
        assert rows.cpu().tolist()[:min(50, n)] == order and result.cpu().tolist() == [n, n, 0, 0, 0, 0, min(50, n), stamps[order[-1]], 0]
    # a column of no strings: every row is null
    rows, _, _, result = shard.top_rows(None, data[1], 50, key_validity=validity[1], stream=stream)
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [len(stamps), 0, len(stamps), 0, 0, 0, 0, 0, 0]
    plan.close()
