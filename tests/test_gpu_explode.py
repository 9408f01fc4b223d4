"""Explode on the GPU (sjmi_explode_batch_device through BatchShard.step() + Context.explode_batch_device / BatchShard.explode):
the row offsets and every cell against tests/explode_common.py, which reads the ORACLE's tapes with the oracle's own walk; and
every cell against sjmi_select_batch_device with the pointer base + "/" + j + p."""
import os
import random
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import explode_common as EC
from tests import select_common as SC
from tests import select_fuzz as F
from tests.conftest import ROOT
from tests.test_gpu_batch import _pack

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("exact", [False, True], ids=["optimistic", "exact"])


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def parse(ctx, docs, exact=False):
    """the batch parsed on the device and accepted (check() runs a rejected step again) -> (shard, string buffer bytes, rejected)"""
    import torch
    from simdjson_java_amd import sharding
    buf, offs = _pack(docs)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.step(torch.cuda.current_stream().cuda_stream, exact=exact)
    torch.cuda.synchronize()
    rejected = bool(int(shard.result.cpu().numpy()[1]) & 0x800)
    c = shard.check()
    torch.cuda.synchronize()
    return shard, bytes(shard.sb[:c["string_bytes"]].cpu().numpy()), rejected


SLACK = 64  # cells behind the n_paths * capacity the call may write: they must keep the sentinel


def explode(ctx, shard, plan, capacity):
    """Context.explode_batch_device into columns filled with the sentinels -> (row offsets, types or None, values or None).
    The columns are the front of buffers that are SLACK cells longer than n_paths * capacity, and the offsets have SLACK
    entries behind n_docs + 1: every element behind what the call owns must still hold the sentinel afterwards."""
    import torch
    dev = shard.tape.device
    stream = torch.cuda.current_stream().cuda_stream
    offs = torch.full((shard.n_docs + 1 + SLACK,), -1, dtype=torch.int64, device=dev)
    cells = plan.n_paths * capacity
    types = torch.full((cells + SLACK,), EC.SENTINEL_T, dtype=torch.uint8, device=dev)
    values = torch.from_numpy(np.full(cells + SLACK, EC.SENTINEL_V, dtype=np.uint64).view(np.int64)).to(dev)
    ctx.explode_batch_device(plan, shard.tape.data_ptr(), shard.tape_offsets.data_ptr(), shard.doc_errors.data_ptr(), shard.sb.data_ptr(),
                             shard.n_docs, offs.data_ptr(), capacity, types.data_ptr() if cells else 0, values.data_ptr() if cells else 0, stream)
    torch.cuda.synchronize()
    offs, types, values = offs.cpu().numpy(), types.cpu().numpy(), values.cpu().numpy().view(np.uint64)
    assert (offs[shard.n_docs + 1:] == -1).all(), "an entry behind row_offsets[n_docs] was written"
    assert (types[cells:] == EC.SENTINEL_T).all() and (values[cells:] == EC.SENTINEL_V).all(), \
        "a cell behind the n_paths * row_capacity elements was written (capacity %d)" % capacity
    if not capacity:
        return offs[:shard.n_docs + 1].view(np.uint64), None, None
    return offs[:shard.n_docs + 1].view(np.uint64), types[:cells].reshape(plan.n_paths, capacity), values[:cells].reshape(plan.n_paths, capacity)


def select(ctx, shard, pointers):
    import torch
    import simdjson_java_amd as S
    plan = S.SelectPlan(pointers)
    types = torch.zeros((len(pointers), shard.n_docs), dtype=torch.uint8, device=shard.tape.device)
    values = torch.zeros((len(pointers), shard.n_docs), dtype=torch.int64, device=shard.tape.device)
    ctx.select_batch_device(plan, shard.tape.data_ptr(), shard.tape_offsets.data_ptr(), shard.doc_errors.data_ptr(), shard.sb.data_ptr(),
                            shard.n_docs, types.data_ptr(), values.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    return types.cpu().numpy(), values.cpu().numpy().view(np.uint64)


def check(ctx, docs, base, pointers, what="", exact=False, expected=None, parsed=None, metamorphic=True):
    """the four capacities of the issue (the total, one less, half, 0 with NULL columns) and one above the total: every cell,
    the sentinels in the rows behind the total and in the slack behind the columns; then every cell of the first elements
    against the selector -> (rows, cells that are not MISSING, rejected)"""
    import simdjson_java_amd as S
    parsed = parsed or [O.parse(d) for d in docs]
    want_offs, want = expected or EC.expected_explode(parsed, base, pointers)
    total = want_offs[-1]
    shard, sb, rejected = parse(ctx, docs, exact)
    err = shard.doc_errors.cpu().numpy()[:len(docs)]
    assert [int(e) != 0 for e in err] == [p.error != 0 for p in parsed]
    plan = S.ExplodePlan(base, pointers)
    present, full = 0, None
    for capacity in (total, max(total - 1, 0), total // 2, 0, total + 5):  # (the last: rows [total, capacity) keep the sentinel)
        offs, types, values = explode(ctx, shard, plan, capacity)
        got = EC.check_explode(offs, types, values, sb, want_offs, want, capacity, "%s, capacity %d of %d" % (what, capacity, total))
        present = max(present, got)
        if capacity == total and total:
            full = (types, values)
    plan.close()
    if metamorphic and full is not None and pointers:
        # cell (row_offsets[k] + j, p) == what the selector gives document k for base/j/p, for the (j, p) that fit a 64-path plan:
        # taken in the order j = 0, 1, ... as long as the select plan holds them; a pointer whose steps, with the base's and
        # the index, are more than a select path may have cannot be asked of the selector at all and is left out
        base_b = base.encode("utf-8") if isinstance(base, str) else bytes(base)
        ptrs = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in pointers]
        usable = [p for p in range(len(ptrs)) if F.plan_fits([base_b + b"/0" + ptrs[p]])]
        pairs, sel_ptrs = [], []
        for j in range(SC_MAX_PATHS):
            for p in usable:
                cand = base_b + b"/%d" % j + ptrs[p]
                if len(sel_ptrs) < SC_MAX_PATHS and F.plan_fits(sel_ptrs + [cand]):
                    pairs.append((j, p))
                    sel_ptrs.append(cand)
            if len(sel_ptrs) == SC_MAX_PATHS:
                break
        assert sel_ptrs or not usable
        if sel_ptrs:
            st, sv = select(ctx, shard, sel_ptrs)
            compared = 0
            for k in range(len(docs)):
                n = want_offs[k + 1] - want_offs[k]
                # (a base that is an OBJECT has no rows, but the selector reads "/j" there as a key: nothing to compare)
                if not parsed[k].error and SC.expected_one(parsed[k].to_python(), base_b)[0] == ord("{"):
                    assert n == 0
                    continue
                for i, (j, p) in enumerate(pairs):
                    if j < n:
                        r = want_offs[k] + j
                        assert (st[i][k], sv[i][k]) == (full[0][p][r], full[1][p][r]), (what, k, j, p)
                        compared += 1
                    else:
                        assert st[i][k] == 0 and sv[i][k] == 0  # (no such element: the selector says MISSING)
            assert compared >= min(total, 1)
    return total, present, rejected


SC_MAX_PATHS = F.MAX_PATHS


@MODES
def test_twitter_statuses_of_one_document(ctx, exact):
    name, docs, base, ptrs = EC.twitter_case()
    rows, present, _ = check(ctx, docs, base, ptrs, name, exact=exact)
    assert rows == 100 and present > 12 * rows


@MODES
@pytest.mark.parametrize("case", EC.github_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_github_events(ctx, case, exact):
    name, docs, base, ptrs = case
    rows, present, _ = check(ctx, docs, base, ptrs, name, exact=exact)
    assert rows >= 10 and present > 4 * rows


@MODES
@pytest.mark.parametrize("case", EC.base_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_base_cases(ctx, case, exact):
    name, docs, base, ptrs = case
    rows, present, rejected = check(ctx, docs, base, ptrs, name, exact=exact)
    if name == "failed documents between good ones":
        assert rows == 7 and (rejected or exact)  # (the unclosed string fails stage 1: the optimistic step is rejected and repaired)


@MODES
@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(ctx, n, exact):
    name, docs, parsed, base, eptrs, (want_offs, want) = EC.fuzz_cases()[n]
    order = list(range(len(docs)))
    random.Random(F.SEED + 2 * n + exact).shuffle(order)  # who shares a wave with whom differs from batch to batch
    offs, cols = [0], [[] for _ in eptrs]
    for k in order:
        for q in range(len(eptrs)):
            cols[q] += want[q][want_offs[k]:want_offs[k + 1]]
        offs.append(offs[-1] + want_offs[k + 1] - want_offs[k])
    rows, present, rejected = check(ctx, [docs[k] for k in order], base, eptrs, name, exact=exact, expected=(offs, cols),
                                    parsed=[parsed[k] for k in order])
    assert not rejected and rows == want_offs[-1]


# ---------------------------------------------------------------------------------------------------------------------
# more than one trip of the kernels' grid-stride loops
# ---------------------------------------------------------------------------------------------------------------------
def trip_documents():
    """EXP_MAX_GRID x EXP_BLOCK / SEL_GROUP of csrc/explode.hip and csrc/sj_select.h: the documents of one trip of the grid"""
    csrc = os.path.join(ROOT, "simdjson-java_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "explode.hip")).read(), open(os.path.join(csrc, "sj_select.h")).read()
    grid = int(re.search(r"EXP_MAX_GRID\s*=\s*(\d+)", hip).group(1))
    block = int(re.search(r"EXP_BLOCK\s*=\s*(\d+)", hip).group(1))
    group = int(re.search(r"SEL_GROUP\s*=\s*(\d+)", hdr).group(1))
    assert block % group == 0
    return grid * block // group


POOL, STRIDE = 4099, 1237  # a prime number of distinct documents, taken in an order that repeats with no period of 8 or of a trip
TRIP_POINTERS = ["", "/a", "/b/0", "/s"]
STAGE2_FAILS, STAGE1_FAILS = b'{"arr":[1,2,}', b'{"arr":["abc'
NO_ROWS = [b'{"arr":[]}', b'{"zz":[1,2]}', b'{"arr":{"a":1}}', b'"arr"']


def _pool_document(i):
    """document i of the pool: 0..11 elements of every kind under "arr" (three in four documents have rows)"""
    n = 0 if i % 4 == 3 else 1 + (i * 7) % 11
    elems = []
    for j in range(n):
        kind = (i + j) % 6
        elems.append([b"%d" % (i * 1009 + j), b'"s%d_%d"' % (i, j), b'{"a":%d,"s":"v%d"}' % (i + j, j), b'{"b":[%d.5,null],"a":true}' % i, b"[%d,[%d]]" % (i, j),
                      b"null"][kind])
    return b'{"n":%d,"arr":[%s]}' % (i, b",".join(elems))


@pytest.fixture(scope="module")
def pool():
    """-> (documents, rows per document, first pool row per document, per path: types, values, string lengths, string bytes by pool row)"""
    docs = [_pool_document(i) for i in range(POOL)]
    assert len(set(docs)) == POOL
    offs, want = EC.expected_explode([O.parse(d) for d in docs], "/arr", TRIP_POINTERS)
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
    assert POOL // 2 < (counts > 0).sum() < POOL
    return docs, counts, first, cols


def _trip_batch(pool, n_docs, T, plants):
    """n_docs documents of the pool with `plants` (documents without rows) put one trip behind documents that have rows"""
    docs, counts, first, cols = pool
    idx = (np.arange(n_docs, dtype=np.int64) * STRIDE) % POOL
    batch = [docs[i] for i in idx]
    planted = {}
    for trip in (1, 2):
        taken = 0
        for off in tuple(range(12)) + (1000, 65537, T - 1):
            q = trip * T + off
            if q < n_docs and taken < len(plants) and counts[idx[q - T]] > 0 and q - T not in planted:
                planted[q] = plants[taken % len(plants)]
                batch[q] = planted[q]
                taken += 1
        assert taken or n_docs <= trip * T, (n_docs, trip)
    return batch, idx, planted


def _check_trip_batch(pool, offs, types, values, sb, idx, planted, tape_index_shift=0):
    """the offsets and EVERY cell of the batch against the pool's expected rows (numpy does the comparing)"""
    docs, counts, first, cols = pool
    n = counts[idx].copy()
    n[np.array(sorted(planted), dtype=np.int64)] = 0
    want_offs = np.concatenate([[0], np.cumsum(n)])
    assert (offs.astype(np.int64) == want_offs).all(), "row offsets differ, first at %d" % np.nonzero(offs.astype(np.int64) != want_offs)[0][0]
    total = int(want_offs[-1])
    doc_of_row = np.repeat(np.arange(len(idx)), n)
    pool_row = first[idx[doc_of_row]] + (np.arange(total) - want_offs[doc_of_row])
    sbv = np.frombuffer(sb + b"\0" * 16, dtype=np.uint8)
    for p, (t, v, ln, text) in enumerate(cols):
        et, ev, eln = t[pool_row], v[pool_row], ln[pool_row]
        wrong = np.nonzero(types[p][:total] != et)[0]
        assert wrong.size == 0, "path %d: %d types differ, first at row %d" % (p, wrong.size, wrong[0])
        plain = et != ord('"')
        wrong = np.nonzero(plain & (values[p][:total] != ev))[0]
        assert wrong.size == 0, "path %d: %d values differ, first at row %d: 0x%x, want 0x%x" % (p, wrong.size, wrong[0], values[p][wrong[0]], ev[wrong[0]])
        s = np.nonzero(~plain)[0]
        if s.size:
            got_ln, off = (values[p][s] >> np.uint64(32)).astype(np.int64), (values[p][s] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert (got_ln == eln[s]).all() and (off >= 4).all() and (off + got_ln <= len(sb)).all(), "path %d: a string's length or offset" % p
            c = np.arange(text.shape[1])
            assert ((sbv[off[:, None] + c] == text[pool_row[s]]) | (c[None, :] >= got_ln[:, None])).all(), "path %d: a string's bytes" % p
    return total


@pytest.mark.parametrize("over", ["0", "1", "T+5"])
def test_more_than_one_trip_of_the_grid(ctx, pool, over):
    """T, T + 1 and 2T + 5 documents: a ragged last trip, and documents that fail stage 2, hold an empty array or no array in a
    slot that held rows one trip earlier; at the full capacity, at half of it, and count-only"""
    import simdjson_java_amd as S
    T = trip_documents()
    n_docs = T + (T + 5 if over == "T+5" else int(over))
    batch, idx, planted = _trip_batch(pool, n_docs, T, [STAGE2_FAILS] + NO_ROWS)
    assert (n_docs == T) == (not planted)
    shard, sb, rejected = parse(ctx, batch)
    assert not rejected  # (a document that fails stage 2 does not reject the batch)
    failed = np.array(sorted(q for q, d in planted.items() if d == STAGE2_FAILS), dtype=np.int64)
    assert (np.nonzero(shard.doc_errors.cpu().numpy()[:n_docs])[0] == failed).all()
    plan = S.ExplodePlan("/arr", TRIP_POINTERS)
    offs0, _, _ = explode(ctx, shard, plan, 0)
    total = int(offs0[-1])
    offs, types, values = explode(ctx, shard, plan, total)
    assert _check_trip_batch(pool, offs, types, values, sb, idx, planted) == total and (offs == offs0).all()
    half = total // 2
    offs, types, values = explode(ctx, shard, plan, half)
    assert (offs == offs0).all()
    full_t, full_v = explode(ctx, shard, plan, total)[1:]
    assert (types == full_t[:, :half]).all() and (values == full_v[:, :half]).all()
    plan.close()


def test_a_document_that_fails_stage_1_in_a_later_trip(ctx, pool):
    """the repair path behind a rejected batch, with the failed document in the third trip and the second"""
    import simdjson_java_amd as S
    T = trip_documents()
    n_docs = 2 * T + 5
    batch, idx, planted = _trip_batch(pool, n_docs, T, [STAGE1_FAILS])
    assert len(planted) == 2
    shard, sb, rejected = parse(ctx, batch)
    assert rejected
    plan = S.ExplodePlan("/arr", TRIP_POINTERS)
    offs, types, values = explode(ctx, shard, plan, int(explode(ctx, shard, plan, 0)[0][-1]))
    _check_trip_batch(pool, offs, types, values, sb, idx, planted)
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------
# one wide array among tiny ones: one group walks all of its elements
# ---------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("n_docs", [8, 16])
def test_a_wide_array_in_every_position_among_tiny_ones(ctx, n_docs, exact):
    elems = []
    for j in range(1003):
        elems.append([b"%d" % j, b'"s%d"' % j, b'{"a":%d,"b":{"c":"x%d"}}' % (j, j), b"[%d,[%d]]" % (j, j), b"true", b'{"a":[%d.5]}' % j][j % 6])
    wide = b'{"pre":1,"arr":[' + b",".join(elems) + b'],"post":[1]}'
    tiny = [b'{"arr":[1]}', b"[]", b'{"arr":[]}', b'{"arr":[{"a":"t"},[7,[8]]]}', b'{"a":{"x":null}}', b"7", b'{"arr":{"a":1}}', b'{"arr":["s",2.5,null]}']
    tiny = [tiny[k % len(tiny)] if k < len(tiny) else b'{"arr":[%d,{"a":%d}]}' % (k, k) for k in range(n_docs - 1)]
    for at in range(n_docs):
        docs = tiny[:at] + [wide] + tiny[at:]
        rows, present, _ = check(ctx, docs, "/arr", EC.ELEMENT_POINTERS, "the wide array at %d of %d" % (at, n_docs), exact=exact)
        assert rows > 1003 and present > 1003


# ---------------------------------------------------------------------------------------------------------------------
# the plan slots, and BatchShard.explode
# ---------------------------------------------------------------------------------------------------------------------
def test_select_and_explode_plans_alternate_on_one_context(ctx):
    import simdjson_java_amd as S
    name, docs, base, ptrs = EC.github_cases()[1]
    parsed = [O.parse(d) for d in docs]
    shard, sb, _ = parse(ctx, docs)
    xa, xb = S.ExplodePlan(base, ptrs), S.ExplodePlan("/payload/commits", ["/author/name"])
    wa, wb = EC.expected_explode(parsed, base, ptrs), EC.expected_explode(parsed, "/payload/commits", ["/author/name"])
    sa, sb_ptrs = SC.GITHUB_POINTERS, ["/type", "/id"]
    total = wa[0][-1]
    for turn in range(3):
        for plan, want in ((xa, wa), (xb, wb), (xa, wa)):
            offs, types, values = explode(ctx, shard, plan, total)
            EC.check_explode(offs, types, values, sb, want[0], want[1], total, "explode, turn %d" % turn)
            for sel in (sa, sb_ptrs):
                st, sv = select(ctx, shard, sel)
                SC.check_columns(st, sv, sb, SC.expected_columns(parsed, sel), "select, turn %d" % turn)
    xa.close()
    xb.close()


def test_batchshard_explode_behind_a_rejected_step(ctx):
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    docs = [b'{"arr":[1,{"a":2}]}', b'{"arr":["abc', b'{"arr":[]}', b'{"arr":[[3],"s"]}'] * 5
    parsed = [O.parse(d) for d in docs]
    ptrs = ["", "/a", "/0"]
    want_offs, want = EC.expected_explode(parsed, "/arr", ptrs)
    total = want_offs[-1]
    assert total == 20
    buf, offs = _pack(docs)
    plan = S.ExplodePlan("/arr", ptrs)
    for capacity in (total, total - 3, 0):
        shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
        stream = torch.cuda.current_stream().cuda_stream
        shard.step(stream)
        shard.explode(plan, capacity, stream)  # queued behind the step: no synchronisation in between
        torch.cuda.synchronize()
        assert int(shard.result.cpu().numpy()[1]) & 0x800  # rejected: what the explode read was not valid
        c = shard.check()  # runs the call for rejected batches and the explode behind it again
        torch.cuda.synchronize()
        assert c["failed_documents"] == 5
        sb = bytes(shard.sb[:c["string_bytes"]].cpu().numpy())
        got_offs = shard.exp_row_offsets.cpu().numpy().view(np.uint64)
        assert shard.exp_types.shape == (len(ptrs), capacity) and shard.exp_values.shape == (len(ptrs), capacity)
        assert [int(x) for x in got_offs] == want_offs
        if capacity:
            n = min(total, capacity)
            SC.check_columns(shard.exp_types.cpu().numpy()[:, :n], shard.exp_values.cpu().numpy().view(np.uint64)[:, :n], sb,
                             [col[:n] for col in want], "BatchShard.explode, capacity %d" % capacity)
        # an accepted step afterwards: step() forgets the pending explode, explode() queues behind it as usual
        shard.step(stream)
        assert shard._exp_pending is None
        r = shard.explode(plan, capacity, stream)
        torch.cuda.synchronize()
        assert [int(x) for x in r[0].cpu().numpy()] == want_offs
    plan.close()
