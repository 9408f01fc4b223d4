"""Group statistics per dictionary key on the GPU (sjmi_group_stats_device through Context.group_stats_device /
BatchShard.group_stats / BatchShard.group_by_string): the stats and the record against the reference of
tests/groupstats_common.py, with canaries in front of and behind the stats and the types column at odd alignments; both kernels'
paths; a million rows twice (the wave combine of the global path runs only here); infinities and NaNs; live rows from a filter's
n_kept and an explode's last offset; the whole chain on the committed fixtures against Python's json."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest

from tests import groupstats_common as GC
from tests import select_common as SC
from tests.members_common import header_constant
from tests.test_gpu_explode import parse
from tests.test_host_groupstats import ROWS

pytestmark = pytest.mark.gpu

CANARY = 0x0C0FFEE0DDF00D55
LDS_KEYS = header_constant("SJMI_GROUP_LDS_KEYS")
W = GC.WORDS
MILLION = 1024 * 1024 + 1


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def group_stats(ctx, indices, words, types, values, n_keys, row_count=None, n_rows=None, types_shift=0):
    """Context.group_stats_device on numpy columns -> (stats uint64 [n_keys, 10], result [5]); the stats lie between canaries,
    the types column `types_shift` bytes into its buffer (any alignment), and both are checked here"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_rows = indices.size if n_rows is None else n_rows
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d_ix = up(indices) if indices.size else None
    d_words = up(words) if words is not None and words.size else None
    d_types = up(np.concatenate([np.zeros(types_shift, dtype=np.uint8), types])) if types.size else None
    d_values = up(values) if values.size else None
    block = up(np.full(n_keys * W + 16, CANARY, dtype=np.uint64))
    result = up(np.full(5, CANARY, dtype=np.uint64))
    d_rc = None if row_count is None else torch.tensor([row_count], dtype=torch.int64, device=dev)
    ptr = lambda t, off=0: t.data_ptr() + off if t is not None else 0
    ctx.group_stats_device(ptr(d_ix), ptr(d_words), ptr(d_types, types_shift), ptr(d_values), n_rows, ptr(d_rc), n_keys,
                           block.data_ptr() + 64 if n_keys else 0, result.data_ptr(), stream)
    torch.cuda.synchronize()
    block = block.cpu().numpy().view(np.uint64)
    assert (block[:8] == CANARY).all() and (block[8 + n_keys * W:] == CANARY).all(), "a word outside the stats was written"
    return block[8:8 + n_keys * W].reshape(n_keys, W).copy(), result.cpu().numpy().view(np.uint64)


def check(ctx, indices, words, bits, types, values, n_keys, row_count=None, what="", exact_sum=False, reference=GC.expected, want=None, **kw):
    live = indices.size if row_count is None else min(indices.size, row_count)
    want, counts = want or reference(indices, bits, types, values, n_keys, live)
    stats, result = group_stats(ctx, indices, words, types, values, n_keys, row_count, **kw)
    assert [int(x) for x in result] == [live, *counts, 0], what
    GC.check_stats(stats, want, exact_sum=exact_sum, what=str(what))
    return stats, result


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_key_counts_on_both_paths(ctx, n_rows):
    for n_keys in (0, 1, LDS_KEYS, LDS_KEYS + 1):
        for kind, vkind in (("uniform", "mixed"), ("wild", "mixed"), ("wild", "exact")):
            indices, words, bits = GC.keys_column(n_rows, n_keys, 1000 * n_rows + n_keys, kind)
            types, values = GC.value_column(n_rows, n_rows + n_keys, vkind)
            check(ctx, indices, words, bits, types, values, n_keys, what=(n_rows, n_keys, kind, vkind), exact_sum=vkind == "exact",
                  types_shift=(n_rows + n_keys) % 8)


@functools.lru_cache(maxsize=None)
def million(n_keys, kind):
    """the column of the million-row tests and its reference, made once"""
    indices, words, bits = GC.keys_column(MILLION, n_keys, 17 + n_keys, kind)
    types, values = GC.value_column(MILLION, 17, "mixed")
    return indices, words, bits, types, values, GC.expected_large(indices, bits, types, values, n_keys, MILLION)


@pytest.mark.parametrize("n_keys", [LDS_KEYS, LDS_KEYS + 1], ids=["lds", "global"])
@pytest.mark.parametrize("kind", ["uniform", "skewed", "one_bin"])
def test_a_million_rows_twice(ctx, n_keys, kind):
    """1024 x 1024 + 1 rows: more than one trip of the capped grid on the LDS path, every workgroup and the wave combine on the
    global one.  Both runs: every integer word EQUAL to the reference (on the global path the check of the combine's reduction),
    sum_double within the bound; between the runs every word but sum_double equal"""
    indices, words, bits, types, values, want = million(n_keys, kind)
    a = check(ctx, indices, words, bits, types, values, n_keys, what=(n_keys, kind, "first"), want=want, types_shift=3)
    b = check(ctx, indices, words, bits, types, values, n_keys, what=(n_keys, kind, "second"), want=want, types_shift=5)
    assert GC.same_but_sum_double(a[0], b[0]) and (a[1] == b[1]).all()
    if kind == "one_bin":
        assert int(a[0][n_keys // 2, :3].sum()) == int(a[1][1]) and int(a[0][:, :3].sum()) == int(a[1][1])
        assert int(a[0][n_keys // 2, 6]) == 1 << 63 and int(a[0][n_keys // 2, 7]) == (1 << 63) - 1  # (INT64_MIN, INT64_MAX are among the cells)


@pytest.mark.parametrize("n_keys", [LDS_KEYS, LDS_KEYS + 1], ids=["lds", "global"])
def test_an_exact_column_in_one_key_is_summed_exactly(ctx, n_keys):
    """64 Ki + 1 rows in one key, the doubles integers below 2^20: every partial sum -- a wave's, a workgroup's -- is exact, so
    sum_double equals the reference, twice"""
    indices, words, bits = GC.keys_column(64 * 1024 + 1, n_keys, 3, "one_bin")
    types, values = GC.value_column(indices.size, 3, "exact")
    a = check(ctx, indices, words, bits, types, values, n_keys, exact_sum=True, reference=GC.expected_large)
    b = check(ctx, indices, None, None, types, values, n_keys, exact_sum=True, reference=GC.expected_large)
    assert int(b[1][1]) == indices.size > int(a[1][1])


@pytest.mark.parametrize("scale", GC.SCALES, ids=GC.SCALE_IDS)
@pytest.mark.parametrize("n_keys", [1, LDS_KEYS, LDS_KEYS + 1], ids=["one_key", "lds", "global"])
def test_scaled_columns_go_through_the_f64_atomics_exactly(ctx, n_keys, scale):
    """doubles m * scale, |m| < 2^20 (value_column's kind "scaled"): at 2^-1074 every cell and every partial sum is subnormal, at
    2^-1040 the sums cross into the normal range, at 2^970 they stay below the overflow.  Every partial sum in every order is
    exact (tests/test_wave_patterns.py), so sum_double EQUALS math.fsum, with no tolerance: an LDS add, a flush or an L2 add that
    flushed a subnormal operand or result to zero would show.  One key and 512 keys: the LDS atomic and its flush; 513 keys: the
    wave butterfly and the L2 atomic; one_bin: thousands of adds on one word, uniform: few.  Twice, equal word for word"""
    for n_rows, kind in ((64 * 1024 + 1, "one_bin"), (5 * 1024, "uniform")):
        indices, words, bits = GC.keys_column(n_rows, n_keys, 3, kind)
        types, values = GC.value_column(n_rows, 3, "scaled", scale=scale)
        want = GC.expected_large(indices, bits, types, values, n_keys, n_rows)
        a = check(ctx, indices, words, bits, types, values, n_keys, what=(scale, kind, n_keys, "first"), exact_sum=True, want=want)
        b = check(ctx, indices, words, bits, types, values, n_keys, what=(scale, kind, n_keys, "second"), exact_sum=True, want=want, types_shift=3)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
        sums = a[0][:, 5].view(np.float64)
        assert scale != GC.SCALES[0] or ((np.abs(sums) < 2.0 ** -1022).all() and (sums != 0).any())  # (subnormal sums, and kept)


def test_the_128_bit_sum(ctx):
    n = 1025
    big, small = np.full(n, GC.INT64_MAX, dtype=np.int64), np.full(n, GC.INT64_MIN, dtype=np.int64)
    mix = np.where(np.arange(n) % 2 == 1, GC.INT64_MAX, -GC.INT64_MAX).astype(np.int64)
    mix[0] = 0
    types = np.full(n, ord("l"), dtype=np.uint8)
    for n_keys in (2, LDS_KEYS + 1):
        indices = np.full(n, n_keys - 1, dtype=np.int32)
        for column in (big, small, mix):
            check(ctx, indices, None, None, types, column.view(np.uint64), n_keys, what=(n_keys, int(column[1])))


def test_a_value_word_behind_a_type_that_is_no_number_changes_nothing(ctx):
    for n_keys in (5, LDS_KEYS + 1):
        indices, words, bits = GC.keys_column(3000, n_keys, 21, "wild")
        types, values = GC.value_column(3000, 21, "exact")
        other = (types != ord("l")) & (types != ord("d"))
        a = group_stats(ctx, indices, words, types, values, n_keys)
        for poison in (0, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000000000):
            changed = values.copy()
            changed[other] = poison
            b = group_stats(ctx, indices, words, types, changed, n_keys)
            assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_infinite_cells_follow_ieee_addition(ctx):
    indices, types, values, n_keys = GC.infinity_case()
    for extra in (0, LDS_KEYS + 1):
        stats, _ = check(ctx, indices, None, None, types, values, n_keys + extra, what="infinities")
        f = stats.view(np.float64)
        assert f[0, 5] == math.inf and math.isnan(f[1, 5]) and f[2, 5] == -math.inf and math.isfinite(f[3, 5])  # only +inf; both; only -inf
        assert (f[1, 8], f[1, 9]) == (-math.inf, math.inf) and (f[4, 8], f[4, 9]) == (math.inf, -math.inf)


def test_nan_cells_appear_only_in_n_nan(ctx):
    for n_keys in (4, LDS_KEYS + 1):
        indices, words, bits, types, values = GC.nan_case(5000, n_keys, 31)
        stats, result = check(ctx, indices, words, bits, types, values, n_keys, what=("nan", n_keys), types_shift=1)
        assert int(result[3]) > 100 and int(stats[:, :3].sum()) == int(result[1])


def test_a_null_validity_and_indices_outside_the_keys(ctx):
    for n_keys in (0, 1, 4, LDS_KEYS, LDS_KEYS + 1):
        indices = np.array([-1, n_keys, GC.INT32_MIN, GC.INT32_MAX, 0, n_keys - 1, -n_keys, n_keys + 1] * 33, dtype=np.int64).astype(np.int32)
        types, values = GC.value_column(indices.size, 5, "mixed")
        _, result = check(ctx, indices, None, None, types, values, n_keys)
        assert int(result[2]) >= 4 * 33


def test_live_rows_from_the_device(ctx):
    for n_keys in (3, LDS_KEYS + 1):
        indices, words, bits = GC.keys_column(3000, n_keys, 5, "wild")
        types, values = GC.value_column(3000, 5, "mixed")
        for row_count in (0, 1, 64, 1024, 2999, 3000, 5000, 1 << 50):
            live = min(3000, row_count)
            ix, ty, va = indices.copy(), types.copy(), values.copy()
            ix[live:], ty[live:], va[live:] = 0, ord("l"), 1 << 62  # (what lies at or above the live rows would count if it were read)
            want = GC.expected(indices, bits, types, values, n_keys, live)
            stats, result = group_stats(ctx, ix, words, ty, va, n_keys, row_count)
            assert [int(x) for x in result] == [live, *want[1], 0], (n_keys, row_count)
            GC.check_stats(stats, want[0], what=str((n_keys, row_count)))


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ix = torch.zeros(8, dtype=torch.int32, device=dev)
    ty = torch.zeros(8, dtype=torch.uint8, device=dev)
    w = torch.zeros(40, dtype=torch.int64, device=dev)
    I, T, Wp = ix.data_ptr(), ty.data_ptr(), w.data_ptr()
    good = dict(d_indices=I, d_validity=Wp, d_types=T, d_values=Wp + 16, n_rows=4, d_row_count=Wp + 8, n_keys=1, d_stats=Wp + 64, d_result=Wp + 160)
    ctx.group_stats_device(**good)
    ctx.group_stats_device(**dict(good, d_types=T + 3, d_validity=0, d_row_count=0))  # (types: any alignment; both may be NULL)
    ctx.group_stats_device(0, 0, 0, 0, 0, 0, 0, 0, Wp + 160)  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[20:25].tolist() == [0, 0, 0, 0, 0]
    bad = [dict(d_result=0), dict(d_indices=0), dict(d_types=0), dict(d_values=0), dict(d_stats=0), dict(n_keys=(1 << 20) + 1), dict(n_rows=1 << 32),
           dict(n_rows=1 << 40), dict(d_indices=I + 2), dict(d_validity=Wp + 4), dict(d_values=Wp + 20), dict(d_row_count=Wp + 4), dict(d_stats=Wp + 68),
           dict(d_result=Wp + 164)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.group_stats_device(**dict(good, **change))
    assert C.CDLL(S.lib_path()).sjmi_group_stats_device(None, I, Wp, T, Wp + 16, 4, None, 1, Wp + 64, Wp + 160, None) == -2  # (no context)


# ---- end to end on the committed fixtures, against Python's json ---------------------------------------------------------------
def _resolve(doc, pointer):
    """-> the value at an RFC 6901 pointer of plain keys, or KeyError"""
    cur = doc
    for token in pointer.split("/")[1:]:
        if not isinstance(cur, dict):
            raise KeyError(pointer)
        cur = cur[token]
    return cur


def python_groups(rows, key_pointer, value_pointer):
    """rows: json.loads documents -> [(key bytes, dict as decode_group_stats gives it)] in first-occurrence order, and the number
    of rows whose key is no string: from Python's own types (a bool is no number)"""
    order, cells, no_key = [], {}, 0
    for row in rows:
        try:
            key = _resolve(row, key_pointer)
        except KeyError:
            key = None
        if not isinstance(key, str):
            no_key += 1
            continue
        k = key.encode("utf-8")
        if k not in cells:
            cells[k] = ([], [], [0])
            order.append(k)
        try:
            v = _resolve(row, value_pointer)
        except KeyError:
            v = None
        if isinstance(v, int) and not isinstance(v, bool):
            cells[k][0].append(v)
        elif isinstance(v, float):
            cells[k][1].append(v)
        else:
            cells[k][2][0] += 1
    out = []
    for k in order:
        longs, doubles, (n_other,) = cells[k]
        out.append((k, dict(n_long=len(longs), n_double=len(doubles), n_other=n_other, sum_long=sum(longs), sum_double=math.fsum(doubles),
                            min_long=min(longs) if longs else None, max_long=max(longs) if longs else None,
                            min_double=min(doubles) if doubles else None, max_double=max(doubles) if doubles else None)))
    return out, no_key


@pytest.mark.parametrize("value_pointer", ["/payload/size", "/repo/id"])
def test_github_events_grouped_by_type(ctx, value_pointer):
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    want, no_key = python_groups([json.loads(e) for e in events], "/type", value_pointer)
    assert len(want) > 3 and no_key == 0 and sum(d["n_long"] for _, d in want) > 5
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/type", value_pointer])
    types, values = shard.select(plan, stream)
    got, dres, gres = shard.group_by_string(types[0], values[0], types[1], values[1], 64, stream=stream)
    assert got == want  # (no doubles in these columns: sum_double is 0.0 on both sides)
    n = len(events)
    assert [int(dres[0]), int(dres[1]), int(dres[3])] == [n, n, len(want)] and [int(x) for x in gres] == [n, n, 0, 0, 0]
    assert shard.group_by_string(types[0], values[0], types[1], values[1], len(want), stream=stream)[0] == want  # (exactly enough)
    with pytest.raises(RuntimeError, match=r"dict_capacity = %d" % (len(want) - 1)):
        shard.group_by_string(types[0], values[0], types[1], values[1], len(want) - 1, stream=stream)
    plan.close()


@pytest.mark.parametrize("key_pointer", ["/user/lang", "/lang"])
def test_twitter_statuses_grouped_by_language(ctx, key_pointer):
    """/statuses exploded; the live rows are the explode's last offset, read on the device, below the row capacity"""
    import torch
    import simdjson_java_amd as S
    from tests.conftest import load_fixture
    doc = load_fixture("twitter.json")
    statuses = json.loads(doc)["statuses"]
    want, no_key = python_groups(statuses, key_pointer, "/retweet_count")
    shard, _, _ = parse(ctx, [doc])
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.ExplodePlan("/statuses", [key_pointer, "/retweet_count"])
    offs, types, values = shard.explode(plan, len(statuses) + 29, stream)
    got, dres, gres = shard.group_by_string(types[0], values[0], types[1], values[1], 64, row_count=offs[shard.n_docs:], stream=stream)
    assert got == want and (key_pointer != "/user/lang" or len(want) > 1)
    n = len(statuses)
    assert int(dres[0]) == n and [int(x) for x in gres] == [n, n - no_key, 0, 0, 0]
    assert sum(d["n_long"] for _, d in want) == n - no_key
    plan.close()


def test_live_rows_from_a_filters_n_kept(ctx):
    """the events whose /payload/size is a number, compacted by a filter: the dictionary and the statistics read n_kept on the device;
    the compacted columns are not written behind it"""
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd.sharding import decode_group_stats
    events = SC.reserialised("github_events.json", lambda d: d)
    rows = [r for r in (json.loads(e) for e in events) if isinstance(r.get("payload", {}).get("size"), int)]
    want, _ = python_groups(rows, "/type", "/repo/id")
    assert 0 < len(rows) < len(events)
    shard, _, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.SelectPlan(["/type", "/repo/id", "/payload/size"])
    types, values = shard.select(plan, stream)
    flt = S.FilterPlan([(2, "type_eq", "l")])
    _, out_types, out_values, _, fres = shard.filter(flt, types, values, stream=stream)
    kept = fres[0:1]
    indices, validity, _, dict_offsets, dict_bytes, dres = shard.dictionary_column(out_types[0], out_values[0], 64, row_count=kept, stream=stream)
    torch.cuda.synchronize()
    n_keys = int(dres.cpu()[3])
    stats, gres = shard.group_stats(indices, validity, out_types[1], out_values[1], n_keys, row_count=kept, stream=stream)
    torch.cuda.synchronize()
    ends, raw = dict_offsets.cpu().numpy(), bytes(dict_bytes.cpu().numpy())
    decoded = decode_group_stats(stats.cpu().numpy())
    assert [(raw[int(ends[j]):int(ends[j + 1])], decoded[j]) for j in range(n_keys)] == want
    assert gres.cpu().numpy().tolist() == [len(rows), len(rows), 0, 0, 0] and int(kept.cpu()[0]) == len(rows)
    flt.close()
    plan.close()
