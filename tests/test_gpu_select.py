"""The device-resident selector on the GPU (sjmi_select_batch_device through BatchShard.step() + BatchShard.select()):
every (path, document) pair against tests/select_common.py, which reads the ORACLE's tapes with the oracle's own walk."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import select_common as SC
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
