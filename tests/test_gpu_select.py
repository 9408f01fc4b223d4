"""The device-resident selector on the GPU (sjmi_select_batch_device through BatchShard.step() + BatchShard.select()):
every (path, document) pair against tests/select_common.py, which reads the ORACLE's tapes with the oracle's own walk."""
import json
import os
import random
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import select_common as SC
from tests import select_fuzz as F
from tests.conftest import ROOT, load_fixture
from tests.golden.vectors import TWITTER_DEFAULT_PROFILE_USERS
from tests.test_gpu_batch import _pack

pytestmark = pytest.mark.gpu

# a dozen paths over the fields tools/docgen.c emits: "k<i>" (a string, an integer, an atom, an array of up to eight small
# integers, or {"x": int, "y": string}) and the filler "z"; "/k1000" and "/nope" are names it never emits
DOCGEN_POINTERS = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


def run_select(ctx, docs, pointers, exact=False, plan=None):
    """-> (types [n_paths, n_docs], values, string buffer bytes, doc_errors, was the optimistic step rejected)"""
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    buf, offs = _pack(docs)
    own = plan is None
    plan = plan or S.SelectPlan(pointers)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    stream = torch.cuda.current_stream().cuda_stream
    shard.step(stream, exact=exact)
    shard.select(plan, stream)  # queued behind the step: no synchronisation in between
    torch.cuda.synchronize()
    rejected = bool(int(shard.result.cpu().numpy()[1]) & 0x800)
    c = shard.check()  # (a rejected step: runs the call for rejected batches and the select behind it again)
    torch.cuda.synchronize()
    out = (shard.sel_types.cpu().numpy().copy(), shard.sel_values.cpu().numpy().view(np.uint64).copy(),
           bytes(shard.sb[:c["string_bytes"]].cpu().numpy()), shard.doc_errors.cpu().numpy()[:len(docs)].copy(), rejected)
    assert out[0].shape == (len(pointers), len(docs)) and out[1].shape == out[0].shape
    if own:
        plan.close()
    return out


def check(ctx, docs, pointers, what="", **kw):
    parsed = [O.parse(d) for d in docs]
    types, values, sb, err, rejected = run_select(ctx, docs, pointers, **kw)
    assert [int(e) != 0 for e in err] == [p.error != 0 for p in parsed]
    present = SC.check_columns(types, values, sb, SC.expected_columns(parsed, pointers), what)
    return present, types, values, sb, rejected


def test_twitter_statuses(ctx):
    docs = SC.reserialised("twitter.json", lambda d: d["statuses"])
    present, types, values, sb, _ = check(ctx, docs, SC.TWITTER_POINTERS, "twitter")
    assert present > 12 * len(docs)
    names = set()
    for k in range(len(docs)):  # BenchmarkCorrectnessTest.java:23-55
        if types[0][k] == ord("t"):
            ln, off = int(values[1][k]) >> 32, int(values[1][k]) & 0xFFFFFFFF
            names.add(sb[off:off + ln])
    assert len(names) == TWITTER_DEFAULT_PROFILE_USERS


def test_github_events(ctx):
    docs = SC.reserialised("github_events.json", lambda d: d)
    present, *_ = check(ctx, docs, SC.GITHUB_POINTERS, "github")
    assert present > 8 * len(docs)


def test_wide_object_every_member_and_every_near_miss(ctx):
    """ONE document of 982 members: its tape does not fit the slice, so the walk reads global memory"""
    doc = load_fixture("wide_bench.json").strip()
    parsed = O.parse(doc)
    keys = [k for k, _ in parsed.to_python()[2]]
    keyset = set(keys)
    assert len(keys) == 982 and len(parsed.tape) > 4 * SC.slice_words()
    for lo in range(0, len(keys), 48):
        part = keys[lo:lo + 48]
        ptrs = [b"/" + SC.escape_token(k) for k in part]
        near = []
        for k in part:
            if k:
                m = bytearray(k)
                m[len(m) // 2] ^= 1
                if bytes(m) not in keyset:
                    near.append(b"/" + SC.escape_token(bytes(m)))
        types, values, sb, err, _ = run_select(ctx, [doc], ptrs)
        assert SC.check_columns(types, values, sb, SC.expected_columns([parsed], ptrs), "wide") == len(part)
        types, values, sb, err, _ = run_select(ctx, [doc], near)
        assert len(near) > len(part) // 2 and not types.any() and not values.any()


def test_rfc6901_examples(ctx):
    ex = json.load(open(os.path.join(ROOT, "tests", "golden", "rfc6901_example.json")))
    present, *_ = check(ctx, [ex["document"].encode()], ex["pointers"], "rfc6901")
    assert present == 12


@pytest.mark.parametrize("case", SC.adversarial_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_adversarial(ctx, case):
    name, docs, pointers = case
    present, types, values, sb, _ = check(ctx, docs, pointers, name)
    assert present > 0
    for p, ptr in enumerate(pointers):  # one path per plan: sharing trie nodes changes nothing
        t1, v1, *_ = run_select(ctx, docs, [ptr])
        assert (t1[0] == types[p]).all() and (v1[0] == values[p]).all(), (name, ptr)


@pytest.mark.parametrize("bad, exact, want_rejected", [(b'{"k0":}', False, False), (b'{"k0":"abc', False, True), (b'{"k0":"abc', True, None),
                                                       (b'{"k0":[1,2}', True, None)],
                         ids=["fails_stage2_accepted", "fails_stage1_repaired", "fails_stage1_exact", "fails_stage2_exact"])
def test_a_failing_document_is_missing_and_its_neighbours_do_not_change(ctx, bad, exact, want_rejected):
    from tools import workloads as W
    data, offs = W.unique_docs(1000, 37)
    good = [bytes(data[int(offs[k]):int(offs[k + 1]) - 1]) for k in range(37)]
    for at in (0, 5, 16, 36, 37):
        docs = good[:at] + [bad] + good[at:]
        present, types, values, sb, rejected = check(ctx, docs, DOCGEN_POINTERS, "one bad document", exact=exact)
        if want_rejected is not None:
            assert rejected == want_rejected  # (which path took the batch: the accepted plain pass, or the repair behind a rejection)
        assert not types[:, at].any() and not values[:, at].any()
        t0, v0, sb0, *_ = run_select(ctx, good, DOCGEN_POINTERS, exact=exact)
        keep = [k for k in range(len(docs)) if k != at]
        assert (types[:, keep] == t0).all()
        for p in range(len(DOCGEN_POINTERS)):
            for j, k in enumerate(keep):
                a, b = int(values[p][k]), int(v0[p][j])
                if t0[p][j] == ord('"'):  # (the records of the neighbours move in the shared buffer; their bytes do not change)
                    assert a >> 32 == b >> 32 and sb[(a & 0xFFFFFFFF):(a & 0xFFFFFFFF) + (a >> 32)] == sb0[(b & 0xFFFFFFFF):(b & 0xFFFFFFFF) + (b >> 32)]
                else:
                    assert a == b


def test_configs3_documents(ctx):
    from tools import workloads as W
    n = 20000
    data, offs = W.unique_docs(0, n)
    docs = [bytes(data[int(offs[k]):int(offs[k + 1]) - 1]) for k in range(n)]
    present, types, values, sb, rejected = check(ctx, docs, DOCGEN_POINTERS, "configs[3]")
    assert not rejected
    assert not types[DOCGEN_POINTERS.index("/nope")].any()
    for ptr in ("/k3/x", "/k5/0", "/k2/7", "/k20/y", "/z", "/k0"):  # nested, array-index and plain paths all find something
        assert types[DOCGEN_POINTERS.index(ptr)].any(), ptr
    assert (types[DOCGEN_POINTERS.index("/z")] == ord('"')).all()


@pytest.mark.parametrize("n_docs", [1, 3, 4, 5, 63, 64, 65])
def test_batch_shapes(ctx, n_docs):
    from tools import workloads as W
    data, offs = W.unique_docs(5000, n_docs)
    docs = [bytes(data[int(offs[k]):int(offs[k + 1]) - 1]) for k in range(n_docs)]
    present, *_ = check(ctx, docs, DOCGEN_POINTERS, "%d documents" % n_docs)
    assert present >= 3 * n_docs


def test_one_plan_on_two_batches_and_two_plans_on_one_context(ctx):
    import simdjson_java_amd as S
    from tools import workloads as W
    plan = S.SelectPlan(DOCGEN_POINTERS)
    other = S.SelectPlan(["/z", "", "/k1"])
    batches = []
    for first, n in ((0, 50), (700, 21)):
        data, offs = W.unique_docs(first, n)
        batches.append([bytes(data[int(offs[k]):int(offs[k + 1]) - 1]) for k in range(n)])
    for docs, (pl, ptrs) in ((batches[0], (plan, DOCGEN_POINTERS)), (batches[1], (plan, DOCGEN_POINTERS)), (batches[1], (other, ["/z", "", "/k1"])),
                             (batches[0], (plan, DOCGEN_POINTERS))):
        parsed = [O.parse(d) for d in docs]
        types, values, sb, err, _ = run_select(ctx, docs, ptrs, plan=pl)
        assert SC.check_columns(types, values, sb, SC.expected_columns(parsed, ptrs), "plan reuse") > len(docs)
    plan.close()
    other.close()


# ---------------------------------------------------------------------------------------------------------------------
# the seeded corpus of tests/select_fuzz.py on the device: four unlike documents to a wave, both entry modes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["optimistic", "exact"])
@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(ctx, n, exact):
    name, docs, ptrs, parsed, want = F.parsed_corpus()[n]
    order = list(range(len(docs)))
    random.Random(F.SEED + 2 * n + exact).shuffle(order)  # who shares a wave with whom differs from batch to batch
    types, values, sb, err, rejected = run_select(ctx, [docs[k] for k in order], ptrs, exact=exact)
    assert not err.any() and not rejected
    present = SC.check_columns(types, values, sb, [[col[k] for k in order] for col in want], name)
    assert present == sum(t != SC.MISSING for col in want for t, _ in col)


# ---------------------------------------------------------------------------------------------------------------------
# more than one trip of k_select's grid-stride loop
# ---------------------------------------------------------------------------------------------------------------------
def trip_documents():
    """SEL_MAX_GRID x SEL_BLOCK / SEL_GROUP of csrc/select.hip and csrc/sj_select.h: the documents of one trip of the grid"""
    csrc = os.path.join(ROOT, "simdjson-java_amd", "csrc")
    hip, hdr = open(os.path.join(csrc, "select.hip")).read(), open(os.path.join(csrc, "sj_select.h")).read()
    grid = int(re.search(r"SEL_MAX_GRID\s*=\s*(\d+)", hip).group(1))
    block = int(re.search(r"SEL_BLOCK\s*=\s*(\d+)", hip).group(1))
    group = int(re.search(r"SEL_GROUP\s*=\s*(\d+)", hdr).group(1))
    assert block % group == 0
    return grid * block // group


POOL, STRIDE = 4099, 1237  # a prime number of distinct documents, taken in an order that repeats with no period of 8 or of a trip
TRIP_POINTERS = ["/a", "/b", "/c/1", "/d/e", "/c", "/f", "/d"]
STAGE2_FAILS, STAGE1_FAILS, NOTHING_SELECTED = b'{"a":}', b'{"a":"abc', [b'{"zz":[1,2],"A":{"a":1}}', b"[]", b'"a"']


def _pool_document(i):
    """document i of the pool; two in three hold a value for every path of TRIP_POINTERS, the others miss some"""
    members = [b'"a":%s' % (b"%d" % (i * 104729 - 7) if i % 2 else b"%d.5" % i), b'"b":"%s%d"' % (b"\\u00e9" if i % 5 == 0 else b"s", i),
               b'"c":[%d,%s,%d]' % (i, (b"true", b'"x%d"' % i, b"-%d" % i)[i % 3], i + 2), b'"d":{"e":%s}' % (b"null", b"true", b"false", b"[%d]" % i)[i % 4],
               b'"f":%s' % (b"false", b"null", b'{"g":%d}' % i)[i % 3]]
    if i % 3 == 1:
        members = [m for j, m in enumerate(members) if (i >> (3 + j)) & 1]
        if i % 2:
            members.append(b'"c":[%d]' % i)  # (an array too short for "/c/1")
    members.append(b'"n":%d' % i)  # (no path names it: it keeps the documents distinct)
    r = i % 5
    return b"{" + b",".join(members[r:] + members[:r]) + b"}"


@pytest.fixture(scope="module")
def pool():
    """-> (documents, per path: expected types [POOL], values [POOL], string lengths [POOL], string bytes [POOL, widest])"""
    docs = [_pool_document(i) for i in range(POOL)]
    assert len(set(docs)) == POOL
    want = SC.expected_columns([O.parse(d) for d in docs], TRIP_POINTERS)
    cols = []
    for col in want:
        t = np.array([c[0] for c in col], dtype=np.uint8)
        v = np.array([0 if c[0] == ord('"') else c[1] for c in col], dtype=np.uint64)
        ln = np.array([len(c[1]) if c[0] == ord('"') else 0 for c in col], dtype=np.uint64)
        text = np.zeros((POOL, max(1, int(ln.max()))), dtype=np.uint8)
        for i, c in enumerate(col):
            if c[0] == ord('"'):
                text[i, :len(c[1])] = np.frombuffer(c[1], dtype=np.uint8)
        cols.append((t, v, ln, text))
    full = np.all([c[0] != SC.MISSING for c in cols], axis=0)
    assert POOL // 2 < full.sum() < POOL
    return docs, cols, full


def _trip_batch(pool, n_docs, T, plants):
    """n_docs documents of the pool with `plants` (documents on which nothing may be selected) put into the second and third
    trip where the document one trip earlier has a value for every path -> (documents, pool index per document, planted positions)"""
    docs, cols, full = pool
    idx = (np.arange(n_docs, dtype=np.int64) * STRIDE) % POOL
    batch = [docs[i] for i in idx]
    planted = {}
    for trip in (1, 2):
        taken = 0
        # (with a third trip, the second trip's plants keep away from its first documents: a plant wants a full document one trip earlier)
        offsets = tuple(range(10)) + (1000, 65537, T - 1) if trip == 2 or n_docs <= 2 * T else tuple(range(1000, 1010)) + (65537, T - 1)
        for off in offsets:
            q = trip * T + off
            if q < n_docs and taken < len(plants) and full[idx[q - T]] and q - T not in planted:
                planted[q] = plants[taken % len(plants)]
                batch[q] = planted[q]
                taken += 1
        assert taken or n_docs <= trip * T, (n_docs, trip)
    return batch, idx, planted


def _check_trip_batch(pool, out, idx, planted):
    """EVERY pair of the batch against the pool's expected columns (numpy does the comparing); the planted documents 0/0"""
    types, values, sb = out[0], out[1], np.frombuffer(out[2] + b"\0" * 16, dtype=np.uint8)
    at = np.array(sorted(planted), dtype=np.int64)
    for p, (t, v, ln, text) in enumerate(pool[1]):
        et, ev, eln = t[idx].copy(), v[idx].copy(), ln[idx].copy()
        et[at], ev[at], eln[at] = 0, 0, 0
        wrong = np.nonzero(types[p] != et)[0]
        assert wrong.size == 0, "path %d: %d types differ, first at document %d: %r, want %r" % (p, wrong.size, wrong[0], types[p][wrong[0]], et[wrong[0]])
        plain = et != ord('"')
        wrong = np.nonzero(plain & (values[p] != ev))[0]
        assert wrong.size == 0, "path %d: %d values differ, first at document %d: 0x%x, want 0x%x" % (p, wrong.size, wrong[0], values[p][wrong[0]], ev[wrong[0]])
        s = np.nonzero(~plain)[0]
        if s.size:
            got_ln, off = (values[p][s] >> np.uint64(32)).astype(np.int64), (values[p][s] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            assert (got_ln == eln[s].astype(np.int64)).all() and (off >= 4).all() and (off + got_ln <= len(out[2])).all(), "path %d: a string's length or offset" % p
            head = sb[off[:, None] - 4 + np.arange(4)].astype(np.int64)  # the record's big-endian length in front of its bytes
            assert ((head[:, 0] << 24 | head[:, 1] << 16 | head[:, 2] << 8 | head[:, 3]) == got_ln).all(), "path %d: a string value does not point at a record" % p
            cols = np.arange(text.shape[1])
            got = sb[off[:, None] + cols]
            assert ((got == text[idx[s]]) | (cols[None, :] >= got_ln[:, None])).all(), "path %d: a string's bytes" % p
        assert not types[p][at].any() and not values[p][at].any()


@pytest.mark.parametrize("over", ["0", "1", "7", "8", "9", "T+5"])
def test_more_than_one_trip_of_the_grid(ctx, pool, over):
    """T, T+1, T+7, T+8, T+9 and 2T+5 documents: the per-trip reset of the group's results, a ragged last trip, and documents that
    fail stage 2 or select nothing in a slot that held a full set of results one trip earlier"""
    T = trip_documents()
    n_docs = T + (T + 5 if over == "T+5" else int(over))
    batch, idx, planted = _trip_batch(pool, n_docs, T, [STAGE2_FAILS] + NOTHING_SELECTED)
    assert (n_docs == T) == (not planted)
    out = run_select(ctx, batch, TRIP_POINTERS)
    assert not out[4]  # (a document that fails stage 2 does not reject the batch: this is the accepted, plain pass)
    failed = np.array([q for q, d in planted.items() if d == STAGE2_FAILS], dtype=np.int64)
    assert (np.nonzero(out[3])[0] == np.sort(failed)).all()
    _check_trip_batch(pool, out, idx, planted)


def test_a_document_that_fails_stage_1_in_a_later_trip(ctx, pool):
    """the repair path behind a rejected batch, with the failed document in the third trip and the second"""
    T = trip_documents()
    n_docs = 2 * T + 5
    batch, idx, planted = _trip_batch(pool, n_docs, T, [STAGE1_FAILS])
    assert len(planted) == 2 and T <= min(planted) < 2 * T <= max(planted)
    out = run_select(ctx, batch, TRIP_POINTERS)
    assert out[4]
    assert (np.nonzero(out[3])[0] == np.array(sorted(planted))).all()
    _check_trip_batch(pool, out, idx, planted)


# ---------------------------------------------------------------------------------------------------------------------
# unlike neighbours in one workgroup: one document of 982 members (walked in global memory, 62 rounds) among tiny ones
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["optimistic", "exact"])
@pytest.mark.parametrize("n_docs", [8, 16])
def test_a_wide_document_in_every_position_among_tiny_ones(ctx, n_docs, exact):
    wide = load_fixture("wide_bench.json").strip()
    keys = [k for k, _ in O.parse(wide).to_python()[2]]
    assert len(keys) == 982
    picked = [keys[i] for i in (0, 1, 15, 16, 17, 31, 32, 33, 500, 980, 981)]
    ptrs = [b"/" + SC.escape_token(k) for k in picked] + [b"/a", b"/b/0", b"", b"/a/x", b"/nope"]
    tiny = [b'{"a":1}', b"[]", b'{"b":["t"]}', b"{" + F.key_text(keys[981]) + b':"tiny"}', b'{"a":{"x":null}}', b"7",
            b"{" + F.key_text(keys[16]) + b":[16]," + F.key_text(keys[0]) + b":0}", b'{"a":"s","b":[2.5]}']
    tiny = [tiny[k % len(tiny)] if k < len(tiny) else b'{"a":%d,"b":[%d]}' % (k, k) for k in range(n_docs - 1)]
    for at in range(n_docs):
        docs = tiny[:at] + [wide] + tiny[at:]
        present, types, *_ = check(ctx, docs, ptrs, "the wide document at %d of %d" % (at, n_docs), exact=exact)
        assert types[:len(picked), at].all() and present > len(picked) + n_docs
