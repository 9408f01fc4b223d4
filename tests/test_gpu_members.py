"""A members explode on the GPU (sjmi_explode_batch_device with a plan of sjmi_explode_members_plan_compile, through
BatchShard.step() + Context.explode_batch_device / BatchShard.explode): the row offsets and every cell -- the element pointers on
the member's value, the key column behind them -- against tests/members_common.py, which reads the ORACLE's tapes with the
oracle's own walk; the key column through the string gather and the dictionary encoder; an array plan beside it unchanged."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests import explode_common as EC
from tests import members_common as MC
from tests import select_common as SC
from tests import select_fuzz as F
from tests.test_gpu_explode import SLACK, _check_trip_batch, parse, trip_documents

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("exact", [False, True], ids=["optimistic", "exact"])


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def explode(ctx, shard, plan, capacity):
    """Context.explode_batch_device into plan.n_columns columns filled with the sentinels -> (row offsets, types or None, values
    or None).  The columns are the front of buffers that are SLACK cells longer than n_columns * capacity, and the offsets have
    SLACK entries behind n_docs + 1: every element behind what the call owns must still hold the sentinel afterwards."""
    import torch
    dev = shard.tape.device
    stream = torch.cuda.current_stream().cuda_stream
    offs = torch.full((shard.n_docs + 1 + SLACK,), -1, dtype=torch.int64, device=dev)
    cells = plan.n_columns * capacity
    types = torch.full((cells + SLACK,), EC.SENTINEL_T, dtype=torch.uint8, device=dev)
    values = torch.from_numpy(np.full(cells + SLACK, EC.SENTINEL_V, dtype=np.uint64).view(np.int64)).to(dev)
    ctx.explode_batch_device(plan, shard.tape.data_ptr(), shard.tape_offsets.data_ptr(), shard.doc_errors.data_ptr(), shard.sb.data_ptr(),
                             shard.n_docs, offs.data_ptr(), capacity, types.data_ptr() if cells else 0, values.data_ptr() if cells else 0, stream)
    torch.cuda.synchronize()
    offs, types, values = offs.cpu().numpy(), types.cpu().numpy(), values.cpu().numpy().view(np.uint64)
    assert (offs[shard.n_docs + 1:] == -1).all(), "an entry behind row_offsets[n_docs] was written"
    assert (types[cells:] == EC.SENTINEL_T).all() and (values[cells:] == EC.SENTINEL_V).all(), \
        "a cell behind the n_columns * row_capacity elements was written (capacity %d)" % capacity
    if not capacity:
        return offs[:shard.n_docs + 1].view(np.uint64), None, None
    return offs[:shard.n_docs + 1].view(np.uint64), types[:cells].reshape(plan.n_columns, capacity), values[:cells].reshape(plan.n_columns, capacity)


def check(ctx, docs, base, pointers, what="", exact=False, expected=None, parsed=None, capacities=None):
    """every capacity of members_common.capacity_cuts (or the given ones): the offsets, every cell below the capacity, the
    sentinels in the rows behind the total and in the slack behind the columns -> (rows, cells that are not MISSING, rejected)"""
    import simdjson_java_amd as S
    parsed = parsed or [O.parse(d) for d in docs]
    want_offs, want = expected or MC.expected_members(parsed, base, pointers)
    total = want_offs[-1]
    shard, sb, rejected = parse(ctx, docs, exact)
    err = shard.doc_errors.cpu().numpy()[:len(docs)]
    assert [int(e) != 0 for e in err] == [p.error != 0 for p in parsed]
    plan = S.ExplodePlan(base, pointers, members=True)
    assert plan.n_columns == len(pointers) + 1
    present = 0
    for capacity in capacities if capacities is not None else (total, max(total - 1, 0), total // 2, 0, total + 5):
        offs, types, values = explode(ctx, shard, plan, capacity)
        present = max(present, EC.check_explode(offs, types, values, sb, want_offs, want, capacity, "%s, capacity %d of %d" % (what, capacity, total)))
    plan.close()
    return total, present, rejected


@pytest.mark.parametrize("case", MC.size_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_object_sizes_and_column_counts(ctx, case):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    expected = MC.expected_members(parsed, base, ptrs)
    rows, present, _ = check(ctx, docs, base, ptrs, name, expected=expected, parsed=parsed, capacities=MC.capacity_cuts(expected[0]))
    assert rows == sum(MC.MEMBER_COUNTS) and present >= rows


@MODES
@pytest.mark.parametrize("case", MC.base_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_base_cases(ctx, case, exact):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    expected = MC.expected_members(parsed, base, ptrs)
    rows, present, rejected = check(ctx, docs, base, ptrs, name, exact=exact, expected=expected, parsed=parsed,
                                    capacities=MC.capacity_cuts(expected[0]))
    if name == "failed documents between good ones":
        assert rows == 7 and (rejected or exact)  # (the unclosed string fails stage 1: the optimistic step is rejected and repaired)


@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(ctx, n):
    name, docs, parsed, base, eptrs, (want_offs, want) = MC.fuzz_cases()[n]
    order = list(range(len(docs)))
    random.Random(F.SEED + 5 * n).shuffle(order)  # who shares a wave with whom differs from batch to batch
    offs, cols = [0], [[] for _ in want]
    for k in order:
        for q in range(len(want)):
            cols[q] += want[q][want_offs[k]:want_offs[k + 1]]
        offs.append(offs[-1] + want_offs[k + 1] - want_offs[k])
    rows, present, rejected = check(ctx, [docs[k] for k in order], base, eptrs, name, expected=(offs, cols), parsed=[parsed[k] for k in order])
    assert not rejected and rows == want_offs[-1]


def test_members_and_array_plans_alternate_on_one_context(ctx):
    """each call's results are what they are alone, whichever kind of plan the context held before"""
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    parsed = [O.parse(d) for d in events]
    shard, sb, _ = parse(ctx, events)
    array_ptrs, member_ptrs = EC.COMMIT_POINTERS, ["", "/0/sha", "/login"]
    xa, xm, xr = S.ExplodePlan("/payload/commits", array_ptrs), S.ExplodePlan("/payload", member_ptrs, members=True), S.ExplodePlan("", [], members=True)
    xo = S.ExplodePlan("/payload", member_ptrs)  # an ARRAY plan on a base that is an object: no rows, as before
    wa = EC.expected_explode(parsed, "/payload/commits", array_ptrs)
    wm, wr = MC.expected_members(parsed, "/payload", member_ptrs), MC.expected_members(parsed, "", [])
    assert wa[0][-1] > 10 and wm[0][-1] > len(events) and wr[0][-1] > 4 * len(events)
    for turn in range(3):
        for plan, want in ((xa, wa), (xm, wm), (xa, wa), (xr, wr), (xm, wm), (xo, None)):
            if want is None:
                offs, types, values = explode(ctx, shard, plan, 7)
                assert not offs.any() and (types == EC.SENTINEL_T).all() and (values == EC.SENTINEL_V).all()
                continue
            total = want[0][-1]
            offs, types, values = explode(ctx, shard, plan, total)
            EC.check_explode(offs, types, values, sb, want[0], want[1], total, "turn %d" % turn)
    for plan in (xa, xm, xr, xo):
        plan.close()


def test_the_key_column_is_a_string_column(ctx):
    """BatchShard.explode with a members plan -> n_paths + 1 columns; the key column through sjmi_string_column_device, and
    through sjmi_dictionary_column_device with the explode's last row offset as the device row count"""
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    docs = events + [b'{"":1,"\\u0041":2,"A":3,"q\\"r":4}', b'[1]', b'{"a":}', b'{}']
    parsed = [O.parse(d) for d in docs]
    want_offs, want = MC.expected_members(parsed, "", [""])
    total = want_offs[-1]
    keys = [k for _, k in want[1]]
    shard, sb, _ = parse(ctx, docs, exact=True)
    stream = torch.cuda.current_stream().cuda_stream
    plan = S.ExplodePlan("", [""], members=True)
    capacity = total + 100  # (rows behind the total are not live: the device row count says so)
    offs, types, values = shard.explode(plan, capacity, stream)
    assert types.shape == values.shape == (2, capacity)
    torch.cuda.synchronize()
    assert [int(x) for x in offs.cpu().numpy()] == want_offs
    # the string gather over exactly the rows present
    s_offs, s_valid, s_data, s_res = shard.string_column(types[1][:total].contiguous(), values[1][:total].contiguous(), stream=stream)
    torch.cuda.synchronize()
    ends, data = s_offs.cpu().numpy(), bytes(s_data.cpu().numpy())
    assert [data[int(ends[r]):int(ends[r + 1])] for r in range(total)] == keys
    assert [int(x) for x in s_res.cpu().numpy()[:3]] == [sum(len(k) for k in keys), total, 0]
    # the dictionary encoder over the whole capacity, live rows from the device
    order = list(dict.fromkeys(keys))
    indices, validity, dict_rows, dict_offsets, dict_bytes, res = shard.dictionary_column(types[1], values[1], 256, row_count=offs[shard.n_docs:],
                                                                                          stream=stream)
    torch.cuda.synchronize()
    r = res.cpu().numpy()
    assert [int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[5]) & 3] == [total, total, 0, len(order), 0]
    d_ends, d_data = dict_offsets.cpu().numpy(), bytes(dict_bytes.cpu().numpy())
    assert [d_data[int(d_ends[j]):int(d_ends[j + 1])] for j in range(len(order))] == order
    assert indices.cpu().numpy()[:total].tolist() == [order.index(k) for k in keys]
    assert b"" in order and order.count(b"A") == 1
    plan.close()


# ---- more than one trip of the kernels' grid-stride loops --------------------------------------------------------------------
POOL, STRIDE = 1021, 389
TRIP_POINTERS = ["", "/a", "/0"]


def _pool_document(i):
    """document i of the pool: a tiny object of 0..5 members of every kind (keys repeat, one is empty)"""
    n = 0 if i % 5 == 4 else 1 + (i * 3) % 5
    members = []
    for j in range(n):
        kind = (i + j) % 6
        key = [b"k%d" % (i % 7), b"", b"a", b"key_%d_%d" % (i, j), b"k%d" % (i % 7), b"z"][(i + 2 * j) % 6]
        members.append(b'"' + key + b'":' + [b"%d" % (i * 1009 + j), b'"s%d_%d"' % (i, j), b'{"a":%d,"s":"v%d"}' % (i + j, j), b"[%d,[%d]]" % (i, j), b"null",
                                              b"true"][kind])
    if i % 3 == 0:
        members.append(b'"n%d":%d' % (i, i))
    return b"{" + b",".join(members) + b"}"


@pytest.fixture(scope="module")
def pool():
    """-> (documents, rows per document, first pool row per document, per column: types, values, string lengths, string bytes)"""
    docs = [_pool_document(i) for i in range(POOL)]
    offs, want = MC.expected_members([O.parse(d) for d in docs], "", TRIP_POINTERS)
    counts, first = np.diff(np.array(offs, dtype=np.int64)), np.array(offs[:-1], dtype=np.int64)
    cols = []
    for col in want:
        t = np.array([c[0] for c in col], dtype=np.uint8)
        v = np.array([0 if c[0] == ord('"') else c[1] for c in col], dtype=np.uint64)
        ln = np.array([len(c[1]) if c[0] == ord('"') else 0 for c in col], dtype=np.int64)
        text = np.zeros((len(col), max(1, int(ln.max()))), dtype=np.uint8)
        for i, c in enumerate(col):
            if c[0] == ord('"'):
                text[i, :len(c[1])] = np.frombuffer(c[1], dtype=np.uint8)
        cols.append((t, v, ln, text))
    assert 0 in counts and counts.max() >= 5
    return docs, counts, first, cols


def test_more_than_one_trip_of_the_grid(ctx, pool):
    """16384 x 8 + 9 tiny objects: a ragged second trip; at the full capacity, at half of it, and count-only"""
    import simdjson_java_amd as S
    T = trip_documents()
    assert T == 16384 * 8
    n_docs = T + 9
    docs = pool[0]
    idx = (np.arange(n_docs, dtype=np.int64) * STRIDE) % POOL
    shard, sb, rejected = parse(ctx, [docs[i] for i in idx])
    assert not rejected
    plan = S.ExplodePlan("", TRIP_POINTERS, members=True)
    offs0, _, _ = explode(ctx, shard, plan, 0)
    total = int(offs0[-1])
    offs, types, values = explode(ctx, shard, plan, total)
    assert _check_trip_batch(pool, offs, types, values, sb, idx, {}) == total and (offs == offs0).all()
    half = total // 2
    offs, half_t, half_v = explode(ctx, shard, plan, half)
    assert (offs == offs0).all() and (half_t == types[:, :half]).all() and (half_v == values[:, :half]).all()
    plan.close()


# ---- end to end on the GitHub events: Python's own parse says what the members are -----------------------------------------
@pytest.mark.parametrize("base", ["", "/payload"])
def test_github_events_against_pythons_pairs(ctx, base):
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    pairs = [MC.resolve_pairs(MC.loads_pairs(e), base) for e in events]
    shard, sb, _ = parse(ctx, events)
    plan = S.ExplodePlan(base, [""], members=True)
    total = sum(len(p or []) for p in pairs)
    offs, types, values = explode(ctx, shard, plan, total)
    assert [int(x) for x in np.diff(offs.astype(np.int64))] == [len(p or []) for p in pairs] and total >= len(events)
    r = 0
    for p in pairs:
        for key, val in p or []:
            v = int(values[1][r])
            assert types[1][r] == ord('"') and sb[(v & 0xFFFFFFFF):(v & 0xFFFFFFFF) + (v >> 32)] == key.encode("utf-8")
            want_t = (b"t" if val is True else b"f" if val is False else b"n" if val is None else b"l" if isinstance(val, int) else
                      b"d" if isinstance(val, float) else b'"' if isinstance(val, str) else b"{" if isinstance(val, MC.Pairs) else b"[")
            assert types[0][r] == want_t[0], (key, val)
            if isinstance(val, str):
                w = int(values[0][r])
                assert sb[(w & 0xFFFFFFFF):(w & 0xFFFFFFFF) + (w >> 32)] == val.encode("utf-8")
            r += 1
    assert r == total
    plan.close()
