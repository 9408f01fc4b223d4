"""The key census on the GPU (sjmi_key_census_device through Context.key_census_device / BatchShard.key_census /
BatchShard.discover_keys): the counts and the record against the Counter reference of tests/members_common.py, with canaries in
front of and behind the counts; both kernels' paths; live rows from a filter's n_kept and an explode's last offset; the whole
schema-discovery chain against Python's own parse of the fixtures."""
import ctypes as C

import numpy as np
import pytest

from tests import members_common as MC
from tests import select_common as SC
from tests.test_gpu_explode import parse
from tests.test_host_census import INT32_MAX, INT32_MIN, ROWS, column

pytestmark = pytest.mark.gpu

CANARY = 0x0C0FFEE0DDF00D55
LDS_KEYS = MC.header_constant("SJMI_CENSUS_LDS_KEYS")


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def census(ctx, indices, words, types, n_keys, row_count=None, n_rows=None, types_shift=0):
    """Context.key_census_device on numpy columns -> (counts [n_keys, 8], result [4]); the counts lie between canaries, the
    types column `types_shift` bytes into its buffer (any alignment), and both are checked here"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n_rows = indices.size if n_rows is None else n_rows
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d_ix = up(indices) if indices.size else None
    d_words = up(words) if words is not None and words.size else None
    d_types = up(np.concatenate([np.zeros(types_shift, dtype=np.uint8), types])) if types.size else None
    block = up(np.full(n_keys * 8 + 16, CANARY, dtype=np.uint64))
    result = up(np.full(4, CANARY, dtype=np.uint64))
    d_rc = None if row_count is None else torch.tensor([row_count], dtype=torch.int64, device=dev)
    ctx.key_census_device(d_ix.data_ptr() if d_ix is not None else 0, d_words.data_ptr() if d_words is not None else 0,
                          d_types.data_ptr() + types_shift if d_types is not None else 0, n_rows, d_rc.data_ptr() if d_rc is not None else 0, n_keys,
                          block.data_ptr() + 64 if n_keys else 0, result.data_ptr(), stream)
    torch.cuda.synchronize()
    block = block.cpu().numpy().view(np.uint64)
    assert (block[:8] == CANARY).all() and (block[8 + n_keys * 8:] == CANARY).all(), "a word outside the counts was written"
    return block[8:8 + n_keys * 8].reshape(n_keys, 8), result.cpu().numpy().view(np.uint64)


def check(ctx, indices, words, bits, types, n_keys, row_count=None, what="", reference=MC.expected_census, **kw):
    live = indices.size if row_count is None else min(indices.size, row_count)
    want, counted, outside = reference(indices, bits, types, n_keys, live)
    counts, result = census(ctx, indices, words, types, n_keys, row_count, **kw)
    assert [int(x) for x in result] == [live, counted, outside, 0], what
    assert counts.tolist() == want, what
    return counts, result


@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_key_counts_on_both_paths(ctx, n_rows):
    for n_keys in (0, 1, LDS_KEYS, LDS_KEYS + 1):
        for kind in ("uniform", "wild"):
            indices, words, types, bits = column(n_rows, n_keys, 1000 * n_rows + n_keys, kind)
            check(ctx, indices, words, bits, types, n_keys, what=(n_rows, n_keys, kind), types_shift=n_rows % 8)


@pytest.mark.parametrize("n_keys", [8, LDS_KEYS, LDS_KEYS + 1, 1 << 18], ids=["8", "lds", "lds_plus_1", "2_18"])
@pytest.mark.parametrize("kind", ["wild", "skewed", "one_bin"])
def test_a_million_rows_twice(ctx, n_keys, kind):
    """1024 x 1024 + 1 rows: more than one trip of the capped grid on the LDS path, every workgroup of the global one; two runs
    give the same words"""
    indices, words, types, bits = column(1024 * 1024 + 1, n_keys, 17 + n_keys, kind)
    a = check(ctx, indices, words, bits, types, n_keys, what=(n_keys, kind), reference=MC.expected_census_large)
    b = census(ctx, indices, words, types, n_keys)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    if kind == "one_bin":
        assert int(a[0][n_keys // 2][0]) == int(bits.sum()) == int(a[1][1])


def test_a_null_validity_and_every_class_byte(ctx):
    types = np.arange(256, dtype=np.uint8).repeat(5)
    indices = (np.arange(types.size) % 5).astype(np.int32)
    for n_keys in (5, LDS_KEYS + 1):
        counts, result = check(ctx, indices, None, None, types, n_keys, types_shift=3)
        assert int(counts[:, 7].sum()) == 5 * (256 - 8) and int(result[1]) == types.size


def test_indices_outside_the_keys_touch_nothing(ctx):
    for n_keys in (0, 1, 4, LDS_KEYS, LDS_KEYS + 1):
        indices = np.array([-1, n_keys, INT32_MIN, INT32_MAX, 0, n_keys - 1, -n_keys, n_keys + 1] * 33, dtype=np.int64).astype(np.int32)
        types = np.full(indices.size, ord("{"), dtype=np.uint8)
        counts, result = check(ctx, indices, None, None, types, n_keys)
        assert int(result[2]) >= 4 * 33


def test_live_rows_from_the_device(ctx):
    for n_keys in (3, LDS_KEYS + 1):
        indices, words, types, bits = column(3000, n_keys, 5, "wild")
        for row_count in (0, 1, 64, 1024, 2999, 3000, 5000, 1 << 50):
            live = min(3000, row_count)
            ix, ty = indices.copy(), types.copy()
            ix[live:], ty[live:] = 0, ord("l")  # (what lies at or above the live rows would count if it were read)
            want, counted, outside = MC.expected_census(indices, bits, types, n_keys, live)
            counts, result = census(ctx, ix, words, ty, n_keys, row_count)
            assert counts.tolist() == want and [int(x) for x in result] == [live, counted, outside, 0], (n_keys, row_count)


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ix = torch.zeros(8, dtype=torch.int32, device=dev)
    ty = torch.zeros(8, dtype=torch.uint8, device=dev)
    w = torch.zeros(16, dtype=torch.int64, device=dev)
    I, T, W = ix.data_ptr(), ty.data_ptr(), w.data_ptr()
    good = dict(d_indices=I, d_validity=W, d_types=T, n_rows=4, d_row_count=W + 8, n_keys=1, d_counts=W + 16, d_result=W + 96)
    ctx.key_census_device(**good)
    ctx.key_census_device(**dict(good, d_types=T + 3, d_validity=0, d_row_count=0))  # (types: any alignment; both may be NULL)
    ctx.key_census_device(0, 0, 0, 0, 0, 0, 0, W + 96)  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[12:16].tolist() == [0, 0, 0, 0]
    bad = [dict(d_result=0), dict(d_indices=0), dict(d_types=0), dict(d_counts=0), dict(n_keys=(1 << 20) + 1), dict(n_rows=1 << 40),
           dict(d_indices=I + 2), dict(d_validity=W + 4), dict(d_row_count=W + 4), dict(d_counts=W + 20), dict(d_result=W + 100)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.key_census_device(**dict(good, **change))
    assert C.CDLL(S.lib_path()).sjmi_key_census_device(None, I, W, T, 4, None, 1, W + 16, W + 96, None) == -2  # (no context)


def test_row_counts_from_a_filter_and_from_an_explode(ctx):
    """the chain on the device: members of the events' root -> the rows whose value is an object (filter) -> their keys
    dictionary-encoded -> the census, every row count read where the operator in front left it"""
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    pairs = [MC.resolve_pairs(MC.loads_pairs(e), "") for e in events]
    shard, sb, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.ExplodePlan("", [""], members=True)
    total = sum(len(p) for p in pairs)
    capacity = total + 50
    offs, types, values = shard.explode(plan, capacity, stream)
    last = offs[shard.n_docs:]
    # an explode's last offset
    indices, validity, _, dict_offsets, dict_bytes, dres = shard.dictionary_column(types[1], values[1], 64, row_count=last, stream=stream)
    torch.cuda.synchronize()
    n_keys = int(dres.cpu()[3])
    counts, cres = shard.key_census(indices, validity, types[0], n_keys, row_count=last, stream=stream)
    torch.cuda.synchronize()
    want = MC.python_key_census(pairs)
    ends, raw = dict_offsets.cpu().numpy(), bytes(dict_bytes.cpu().numpy())
    assert [(raw[int(ends[j]):int(ends[j + 1])], counts.cpu().numpy()[j].tolist()) for j in range(n_keys)] == want
    assert cres.cpu().numpy().tolist() == [total, total, 0, 0]
    # a filter's n_kept: only the members whose value is an object
    flt = S.FilterPlan([(0, "type_eq", "{")])
    rows, out_types, out_values, keep, fres = shard.filter(flt, types, values, n_rows=total, stream=stream)
    kept = fres[0:1]
    indices, validity, _, dict_offsets, dict_bytes, dres = shard.dictionary_column(out_types[1], out_values[1], 64, row_count=kept, stream=stream)
    torch.cuda.synchronize()
    n_keys = int(dres.cpu()[3])
    counts, cres = shard.key_census(indices, validity, out_types[0], n_keys, row_count=kept, stream=stream)
    torch.cuda.synchronize()
    want = MC.python_key_census([[(k, v) for k, v in p if isinstance(v, MC.Pairs)] for p in pairs])
    ends, raw = dict_offsets.cpu().numpy(), bytes(dict_bytes.cpu().numpy())
    assert [(raw[int(ends[j]):int(ends[j + 1])], counts.cpu().numpy()[j].tolist()) for j in range(n_keys)] == want
    n_objects = sum(c[6] for _, c in want)
    assert cres.cpu().numpy().tolist() == [n_objects, n_objects, 0, 0] and 0 < n_objects < total and int(kept.cpu()[0]) == n_objects
    flt.close()
    plan.close()


@pytest.mark.parametrize("fixture,split,base", [("github_events.json", True, ""), ("github_events.json", True, "/payload"),
                                                 ("twitter.json", False, "/search_metadata")], ids=["github_root", "github_payload", "twitter_metadata"])
def test_discover_keys(ctx, fixture, split, base):
    from tests.conftest import load_fixture
    docs = SC.reserialised(fixture, lambda d: d) if split else [load_fixture(fixture)]
    pairs = [MC.resolve_pairs(MC.loads_pairs(d), base) for d in docs]
    want = MC.python_key_census(pairs)
    total = sum(len(p or []) for p in pairs)
    assert total and len(want) > 3
    shard, sb, _ = parse(ctx, docs)
    keys, offs, dres, cres = shard.discover_keys(base)
    assert keys == want
    assert [int(x) for x in np.diff(offs)] == [len(p or []) for p in pairs]
    assert [int(dres[0]), int(dres[1]), int(dres[3]), int(dres[5])] == [total, total, len(want), 0]
    assert [int(x) for x in cres] == [total, total, 0, 0]
    assert shard.discover_keys(base, dict_capacity=len(want))[0] == want  # (exactly enough)
    with pytest.raises(RuntimeError, match=r"dict_capacity = %d" % (len(want) - 1)):
        shard.discover_keys(base, dict_capacity=len(want) - 1)
    assert shard.discover_keys("/no/such/object")[0] == []
