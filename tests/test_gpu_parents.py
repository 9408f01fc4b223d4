"""The parent columns on the GPU (sjmi_parent_columns_device through Context.parent_columns_device / BatchShard.parent_columns /
BatchShard.explode_with_parents): the parents, their type bytes, the carried cells and the record against numpy's searchsorted
(tests/parents_common.py), with canaries in front of and behind every output and in every entry the call does not own; the shapes
of the host simulation's tests, the span walk's second and third trip, a document over three chunks, a million rows twice; then a
select joined with an explode on the committed GitHub events and on one corpus of tests/query_fuzz.py, cell by cell against
Python's json, and through filter and group_by_string.  All results are integers: every comparison is an equality."""
import ctypes as C
import json

import numpy as np
import pytest

from tests import parents_common as PC
from tests import query_fuzz as QF
from tests import select_common as SC
from tests.test_gpu_explode import parse

pytestmark = pytest.mark.gpu

MILLION = 1024 * 1024 + 1


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def device_call(ctx):
    """the call of parents_common.check through Context.parent_columns_device: every buffer uploaded whole, the pointer at its
    element, the outputs read back whole into the arrays they came from"""
    import torch
    dev = torch.device("cuda", 0)

    def call(*args):
        stream = torch.cuda.current_stream().cuda_stream
        held, passed = [], []
        for a in args:
            if not isinstance(a, tuple):
                passed.append(0 if a is None else a)
                continue
            whole, at = a
            if whole.size == 0:
                whole = np.zeros(1, dtype=whole.dtype)  # (an empty tensor has no pointer to give)
            t = torch.from_numpy(whole.view(np.int64) if whole.dtype == np.uint64 else whole).to(dev)
            held.append((a[0], t))
            passed.append(t.data_ptr() + at * whole.itemsize)
        ctx.parent_columns_device(*passed, stream)
        torch.cuda.synchronize()
        for whole, t in held:
            if whole.size and whole.flags.writeable:
                back = t.cpu().numpy()
                whole[:] = back.view(np.uint64) if whole.dtype == np.uint64 else back
        return 0
    return call


def counts_with_exactly(live, seed):
    counts = PC.random_counts(max(live // 3, 1), seed)
    counts[-1] += max(live - int(counts.sum()), 0)
    while int(counts.sum()) > live:
        counts[int(np.flatnonzero(counts)[0])] -= 1
    return counts


@pytest.mark.parametrize("live", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1])
def test_dense_rows_at_every_edge(ctx, live):
    counts = counts_with_exactly(live, live)
    offsets = PC.offsets_of(counts)
    cols = PC.doc_columns(2, counts.size, counts.size + 3, live)
    PC.check(device_call(ctx), offsets, live, cols=cols, what=live)
    # n_rows above the total: dense orphans; the row count read on the device; wider strides
    PC.check(device_call(ctx), offsets, live + 70, cols=cols, out_stride=live + 75, what=("orphans", live))
    PC.check(device_call(ctx), offsets, live + 70, cols=cols, row_count=live, out_stride=live + 75, what=("row count", live))
    PC.check(device_call(ctx), offsets, live, rows=np.arange(live)[::-1].copy(), cols=cols, what=("sparse", live))


def test_documents_without_rows_and_the_span_walks_later_trips(ctx):
    """documents without rows in front, behind and between; 3000 of them between two that have rows: the span walk's second and
    third trip"""
    for counts in ([0, 0, 0, 5, 0, 0, 2, 0, 0, 0], [3] + [0] * 3000 + [4], [0] * 200 + [1] * 130 + [0] * 200, [0] * 3000 + [1], [1] + [0] * 3000,
                   [900] + [0] * 3000 + [300, 0, 1]):
        offsets = PC.offsets_of(counts)
        cols = PC.doc_columns(1, len(counts), len(counts), 5)
        want, _ = PC.check(device_call(ctx), offsets, int(offsets[-1]), cols=cols, what=counts[:12])
        assert set(want.tolist()) == {k for k, c in enumerate(counts) if c}


def test_one_document_over_three_chunks_and_starts_at_the_edges(ctx):
    """the middle chunk of a long document has no document start and takes its seed alone; documents that begin exactly at a
    wave edge and at a chunk edge"""
    for counts in ([10, 3 * 1024 + 5, 7], [64, 64, 0, 896, 1024, 1, 1023], [1024, 0, 1024, 2048], [1023, 1, 1, 1023], [0, 3 * 1024, 0],
                   [256, 0, 256, 255, 1, 1, 255, 512, 0, 1]):  # (and at the edges of a workgroup's trips through its chunk)
        offsets = PC.offsets_of(counts)
        PC.check(device_call(ctx), offsets, int(offsets[-1]), cols=PC.doc_columns(3, len(counts), len(counts) + 1, 9), what=counts)


def test_no_row_no_document_one_document(ctx):
    cols1 = PC.doc_columns(2, 1, 4, 1)
    for counts, cols in (([0] * 40, PC.doc_columns(2, 40, 40, 2)), ([], cols1), ([0], cols1), ([5], cols1), ([1500], cols1)):
        offsets = PC.offsets_of(counts)
        for n_rows in (0, 1, 70, 1500, 1601):
            _, result = PC.check(device_call(ctx), offsets, n_rows, cols=cols, what=(counts[:3], n_rows))
            assert result[1] == max(0, n_rows - int(offsets[-1]))
            PC.check(device_call(ctx), offsets, n_rows, rows=np.arange(n_rows)[::-1].copy(), cols=cols, what=("sparse", counts[:3], n_rows))


def test_the_row_count_is_read_on_the_device(ctx):
    offsets = PC.offsets_of(PC.random_counts(900, 4))
    total = int(offsets[-1])
    cols = PC.doc_columns(2, 900, 900, 4)
    for row_count in (0, 1, total - 100, total, total + 5, 1 << 50):
        for n_rows in (total, total + 40, total - 60):
            PC.check(device_call(ctx), offsets, n_rows, row_count=row_count, cols=cols, what=(row_count, n_rows))
        PC.check(device_call(ctx), offsets, total, rows=np.arange(total)[::-1].copy(), row_count=row_count, cols=cols, what=("sparse", row_count))


def test_the_sparse_form(ctx):
    """a filter's ascending selection, a top k's rank-order vector, duplicates, and the indices 0, total - 1, total and 2^40"""
    offsets = PC.offsets_of(PC.random_counts(3000, 8))
    total = int(offsets[-1])
    cols = PC.doc_columns(3, 3000, 3001, 8)
    rng = np.random.default_rng(8)
    ascending = np.flatnonzero(rng.random(total) < 0.1)
    ranked = rng.permutation(total)[:2048]
    duplicates = rng.integers(0, total, size=1500) // 7 * 7
    edges = np.array([0, total - 1, total, 1 << 40, total + 1, (1 << 64) - 1, 0, total - 1], dtype=np.uint64)
    for rows in (ascending, ranked, duplicates, edges):
        want, result = PC.check(device_call(ctx), offsets, rows.size, rows=rows.astype(np.uint64), cols=cols)
    with_rows = np.flatnonzero(np.diff(offsets))
    assert want.tolist() == [with_rows[0], with_rows[-1], -1, -1, -1, -1, with_rows[0], with_rows[-1]] and result[1] == 4


def test_each_output_is_optional_strides_may_be_wider_types_at_any_alignment(ctx):
    offsets = PC.offsets_of(PC.random_counts(700, 6))
    total = int(offsets[-1])
    cols = PC.doc_columns(2, 700, 900, 6)  # (col_stride > n_docs)
    for kw in (dict(cols=None), dict(cols=cols, with_parents=False, with_types=False), dict(cols=cols, with_parents=False),
               dict(cols=cols, with_types=False), dict(cols=cols, out_stride=total + 300), dict(cols=cols, shift=3), dict(cols=cols, shift=1)):
        PC.check(device_call(ctx), offsets, total + 9, **kw)
        PC.check(device_call(ctx), offsets, 300, rows=np.arange(300, dtype=np.uint64) * 3, **kw)


def test_the_type_pointers_three_bytes_into_their_allocations(ctx):
    import torch
    dev = torch.device("cuda", 0)
    counts = PC.random_counts(50, 3)
    offsets = PC.offsets_of(counts)
    n = int(offsets[-1])
    types, values = PC.doc_columns(2, 50, 50, 3)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_t = torch.cat([torch.zeros(3, dtype=torch.uint8), torch.from_numpy(types.reshape(-1))]).to(dev)
    d_v = torch.from_numpy(values.view(np.int64)).to(dev)
    d_pt, d_ot = torch.full((n + 8,), 0xC5, dtype=torch.uint8, device=dev), torch.full((2 * n + 8,), 0xC5, dtype=torch.uint8, device=dev)
    d_p, d_ov, d_res = (torch.zeros(k, dtype=torch.int64, device=dev) for k in (n, 2 * n, 3))
    ptrs = (d_t.data_ptr() + 3, d_pt.data_ptr() + 3, d_ot.data_ptr() + 3)
    assert [p & 7 for p in ptrs] == [3, 3, 3]
    ctx.parent_columns_device(d_off.data_ptr(), 50, 0, n, 0, ptrs[0], d_v.data_ptr(), 2, 50, ptrs[1], d_p.data_ptr(), ptrs[2], d_ov.data_ptr(), n,
                              d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = PC.expected_parents(offsets, np.arange(n))
    pt, ot = d_pt.cpu().numpy(), d_ot.cpu().numpy()
    assert (pt[:3] == 0xC5).all() and (pt[3:3 + n] == ord("l")).all() and (pt[3 + n:] == 0xC5).all()
    assert (ot[:3] == 0xC5).all() and (ot[3:3 + 2 * n].reshape(2, n) == types[:, want]).all() and (ot[3 + 2 * n:] == 0xC5).all()
    assert d_p.cpu().numpy().tolist() == want.tolist() and d_res.cpu().tolist() == [n, 0, 0]


def test_64_carried_columns(ctx):
    offsets = PC.offsets_of(PC.random_counts(300, 2))
    PC.check(device_call(ctx), offsets, int(offsets[-1]) + 3, cols=PC.doc_columns(64, 300, 301, 2))
    for n_cols in (1, 3, 4, 5, 63):
        PC.check(device_call(ctx), offsets, int(offsets[-1]), cols=PC.doc_columns(n_cols, 300, 300, n_cols))


def test_a_million_rows_twice(ctx):
    """1024 x 1024 + 1 dense rows over 100,000 documents: 1025 workgroups.  Both runs equal to the reference and, word for word, to
    each other"""
    import torch
    dev = torch.device("cuda", 0)
    n_docs = 100000
    rng = np.random.default_rng(17)
    counts = rng.integers(0, 21, size=n_docs)
    counts[rng.random(n_docs) < 0.3] = 0
    counts[n_docs // 2] += MILLION - 5 - int(counts.sum())  # (five orphans; one document owns what is left)
    assert counts[n_docs // 2] > 0
    offsets = PC.offsets_of(counts)
    types, values = PC.doc_columns(2, n_docs, n_docs, 17)
    want = PC.expected_parents(offsets, np.arange(MILLION))
    up = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    d_off, d_t, d_v = up(offsets), up(types.reshape(-1)), up(values.reshape(-1))
    runs = []
    for _ in range(2):
        d_pt, d_ot = torch.full((MILLION,), 0xC5, dtype=torch.uint8, device=dev), torch.full((2 * MILLION,), 0xC5, dtype=torch.uint8, device=dev)
        d_p, d_ov, d_res = (torch.full((k,), -7, dtype=torch.int64, device=dev) for k in (MILLION, 2 * MILLION, 3))
        ctx.parent_columns_device(d_off.data_ptr(), n_docs, 0, MILLION, 0, d_t.data_ptr(), d_v.data_ptr(), 2, n_docs, d_pt.data_ptr(), d_p.data_ptr(),
                                  d_ot.data_ptr(), d_ov.data_ptr(), MILLION, d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (d_pt, d_p, d_ot, d_ov, d_res)])
    pt, p, ot, ov, res = runs[0]
    has = want >= 0
    k = np.where(has, want, 0)
    assert res.tolist() == [MILLION, 5, 0] and (p == want).all() and (pt == np.where(has, ord("l"), 0)).all()
    assert (ot.reshape(2, -1) == np.where(has, types[:, k], 0)).all() and (ov.view(np.uint64).reshape(2, -1) == np.where(has, values[:, k], 0)).all()
    assert all((a == b).all() for a, b in zip(*runs))


def test_argument_errors(ctx):
    import torch
    import simdjson_java_amd as S
    dev = torch.device("cuda", 0)
    ty = torch.zeros(64, dtype=torch.uint8, device=dev)
    w = torch.zeros(128, dtype=torch.int64, device=dev)
    w[1], w[2] = 2, 4  # the offsets of two documents
    T, Wp = ty.data_ptr(), w.data_ptr()
    good = dict(d_row_offsets=Wp, n_docs=2, d_rows=0, n_rows=4, d_row_count=0, d_types=T, d_values=Wp + 64, n_cols=1, col_stride=2,
                d_parent_types=T + 16, d_parents=Wp + 128, d_out_types=T + 32, d_out_values=Wp + 256, out_stride=4, d_result=Wp + 512)
    ctx.parent_columns_device(**good)
    ctx.parent_columns_device(**dict(good, d_types=T + 3, d_parent_types=T + 17, d_out_types=T + 33))  # (types: any alignment)
    ctx.parent_columns_device(**dict(good, d_parent_types=0, d_parents=0))
    ctx.parent_columns_device(**dict(good, n_cols=0, d_types=0, d_values=0, d_out_types=0, d_out_values=0, col_stride=0, out_stride=0))
    ctx.parent_columns_device(**dict(good, d_rows=Wp + 64, d_row_count=Wp + 8))
    ctx.parent_columns_device(**dict(good, n_rows=0, n_docs=0, col_stride=0, out_stride=0))  # (nothing at all: a zero record)
    torch.cuda.synchronize()
    assert w.cpu().numpy()[64:67].tolist() == [0, 0, 0]
    bad = [dict(d_row_offsets=0), dict(d_result=0), dict(n_cols=65), dict(d_types=0), dict(d_values=0), dict(d_out_types=0), dict(d_out_values=0),
           dict(col_stride=1), dict(out_stride=3), dict(n_rows=1 << 32, out_stride=1 << 32), dict(n_docs=1 << 32, col_stride=1 << 32),
           dict(d_row_offsets=Wp + 4), dict(d_rows=Wp + 68), dict(d_row_count=Wp + 12), dict(d_values=Wp + 68), dict(d_parents=Wp + 132),
           dict(d_out_values=Wp + 260), dict(d_result=Wp + 516)]
    for change in bad:
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.parent_columns_device(**dict(good, **change))
    assert C.CDLL(S.lib_path()).sjmi_parent_columns_device(None, Wp, 2, None, 4, None, None, None, 0, 0, None, Wp + 128, None, None, 0, Wp + 512,
                                                           None) == -2  # (no context)


# ---- a select joined with an explode, against Python's json ---------------------------------------------------------------------
def joined(shard, doc_pointers, base, pointers, capacity, stream, members=False):
    """select(doc_pointers), then explode_with_parents(base, pointers) -> (plans, row offsets, types, values, result)"""
    import simdjson_java_amd as S
    sel, exp = S.SelectPlan(doc_pointers), S.ExplodePlan(base, pointers, members=members)
    doc_types, doc_values = shard.select(sel, stream)
    return (sel, exp) + shard.explode_with_parents(exp, capacity, doc_types, doc_values, stream)


def check_joined(rows, sb, doc_pointers, base, pointers, offs, types, values, result, capacity, members=False):
    """the joined set cell by cell: the explode's columns, the document's cells on every row, the parent ids -> (live rows, the
    parents)"""
    want_offs, want_cols = QF.explode_cells(rows, base, pointers, members)
    live = want_offs[-1]
    assert 0 < live < capacity and offs.tolist() == want_offs and result.tolist() == [live, 0, 0]
    parents = PC.expected_parents(np.array(want_offs, dtype=np.uint64), np.arange(live))
    docs = QF.select_cells(rows, doc_pointers)
    assert types.shape == (len(want_cols) + len(doc_pointers) + 1, capacity)
    for c, col in enumerate(want_cols):
        QF.same_cells("exploded column %d" % c, types[c], values[c], col, sb)
    for c, col in enumerate(docs):
        at = len(want_cols) + c
        QF.same_cells("carried column %d" % c, types[at], values[at], [col[k] for k in parents], sb)
    assert (types[-1][:live] == ord("l")).all() and values[-1][:live].tolist() == parents.tolist()
    assert not types[:, live:].any() and not values[:, live:].any()  # (zeros as allocated: nothing at or behind the live rows is written)
    return live, parents


def test_github_commits_with_their_events_type_and_login(ctx):
    """/payload/commits of every event with the event's /type and /actor/login on each commit; then only the PushEvents' commits
    (a string_eq on the CARRIED /type), and the commits per /actor/login (group_by_string on the carried login)"""
    import torch
    import simdjson_java_amd as S
    events = SC.reserialised("github_events.json", lambda d: d)
    docs = [json.loads(e) for e in events]
    shard, sb, _ = parse(ctx, events)
    stream = torch.cuda.current_stream().cuda_stream
    doc_pointers, pointers = ["/type", "/actor/login"], ["/sha", "/message"]
    n_commits = sum(len(d["payload"].get("commits", [])) for d in docs)
    capacity = n_commits + 37
    sel, exp, offs, types, values, result = joined(shard, doc_pointers, "/payload/commits", pointers, capacity, stream)
    torch.cuda.synchronize()
    H = lambda t: t.cpu().numpy()
    live, parents = check_joined(docs, sb, doc_pointers, "/payload/commits", pointers, H(offs), H(types), H(values), H(result), capacity)
    assert live == n_commits and len(set(parents.tolist())) < len(docs)  # (events without commits are nobody's parent)
    # a filter on the carried /type.  In this fixture every commit hangs on a PushEvent, so on the commits the term keeps every
    # row; the members of /payload come from events of every type, and there it keeps some rows and drops some
    flt = S.FilterPlan([(2, "string_eq", "PushEvent")])
    _, _, _, _, fres = shard.filter(flt, types, values, n_rows=live, stream=stream)
    torch.cuda.synchronize()
    assert int(fres.cpu()[0]) == sum(1 for r in range(live) if docs[parents[r]]["type"] == "PushEvent") == live
    n_members = sum(len(d["payload"]) for d in docs)
    m_capacity = n_members + 11
    msel, mexp, m_offs, m_types, m_values, m_result = joined(shard, ["/type"], "/payload", [""], m_capacity, stream, members=True)
    torch.cuda.synchronize()
    m_live, m_parents = check_joined(docs, sb, ["/type"], "/payload", [""], H(m_offs), H(m_types), H(m_values), H(m_result), m_capacity, members=True)
    assert m_live == n_members
    frows, f_types, f_values, _, fres = shard.filter(flt, m_types, m_values, n_rows=m_live, stream=stream)  # (column 2: the carried /type)
    torch.cuda.synchronize()
    kept = [r for r in range(m_live) if docs[m_parents[r]]["type"] == "PushEvent"]
    assert 0 < len(kept) < m_live and int(fres.cpu()[0]) == len(kept) and frows.cpu().tolist()[:len(kept)] == kept
    assert f_values[-1].cpu().tolist()[:len(kept)] == [int(m_parents[r]) for r in kept]
    keys = [k for d in docs for k in d["payload"]]
    QF.same_cells("the kept members' keys", H(f_types[1][:len(kept)]), H(f_values[1][:len(kept)]), [QF.cell_of(keys[r]) for r in kept], sb)
    per_login = {}
    for k in parents:
        login = docs[k]["actor"]["login"]
        per_login[login] = per_login.get(login, 0) + 1
    assert len(per_login) > 1
    # commits per login: the carried login is the key, the parent id the value
    groups, dres, gres = shard.group_by_string(types[3, :live].contiguous(), values[3, :live].contiguous(), types[4, :live].contiguous(),
                                               values[4, :live].contiguous(), 4096, stream=stream)
    got = {key.decode(): d["n_long"] for key, d in groups}
    assert got == per_login and int(gres[1]) == live
    sums = {}
    for k in parents:
        sums[docs[k]["actor"]["login"]] = sums.get(docs[k]["actor"]["login"], 0) + int(k)
    assert {key.decode(): d["sum_long"] for key, d in groups} == sums
    # the sparse form behind top_rows: the event of each of the five rows with the highest parent ids, in rank order
    trows, _, _, _ = shard.top_rows(types[4], values[4], 5, row_count=offs[shard.n_docs:], stream=stream)
    pt, p, ot, ov, pres = shard.parent_columns(offs, *shard.select(sel, stream), rows=trows, stream=stream)
    torch.cuda.synchronize()
    order = sorted(range(live), key=lambda r: (-int(parents[r]), r))[:5]
    assert trows.cpu().tolist() == order and p.cpu().tolist() == [int(parents[r]) for r in order] and pres.cpu().tolist() == [5, 0, 0]
    QF.same_cells("the top rows' logins", H(ot[1]), H(ov[1]), [QF.cell_of(docs[parents[r]]["actor"]["login"]) for r in order], sb)
    for plan in (flt, sel, exp, msel, mexp):
        plan.close()


def test_one_corpus_of_the_query_fuzz_joined(ctx):
    """the /tags of every document of a seeded corpus (failing documents, documents without tags, elements that are no objects)
    with the document's /grp, /val and /id on each row"""
    import torch
    from simdjson_java_amd import sharding
    c = QF.case("d1025_longs_v3")
    packed = b"".join(d + b"\n" for d in c.docs)
    offsets = np.cumsum([0] + [len(d) + 1 for d in c.docs]).astype(np.uint64)
    stream = torch.cuda.current_stream().cuda_stream
    shard = sharding.BatchShard(ctx, packed, offsets, torch.device("cuda", 0))
    shard.step(stream)
    torch.cuda.synchronize()
    report = shard.check()
    torch.cuda.synchronize()
    sb = bytes(shard.sb[:report["string_bytes"]].cpu().numpy())
    doc_pointers, pointers = ["/grp", "/val", "/id"], ["/name", "/w"]
    capacity = 5 * c.n_docs
    sel, exp, offs, types, values, result = joined(shard, doc_pointers, "/tags", pointers, capacity, stream)
    torch.cuda.synchronize()
    H = lambda t: t.cpu().numpy()
    live, parents = check_joined(c.rows, sb, doc_pointers, "/tags", pointers, H(offs), H(types), H(values), H(result), capacity)
    assert live > 1024 and c.failing and not set(c.failing) & set(parents.tolist())
    sel.close()
    exp.close()
