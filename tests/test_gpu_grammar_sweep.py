"""Every short token sequence through the GPU walkers, against the oracle: WHICH error a document gets, not only whether it fails.

The cooperative walkers (csrc/coop_walk.hip: one wave per document, the chunked single-document form, the token stream walker
k_tok_stream) decide stage 2 with local predicates and scans; a document's error must be the failing predicate at the lowest
position, where JsonIterator.java would have stopped.  The families of tests/grammar_sweep.py (every sequence of up to six tokens of
nine, up to five of thirteen with the deferred literals `-` and `nul`, up to four of twelve with the three stage-1 verdicts, and
single-token edits of documents of 31 .. 151 tokens: 1,031,536 documents, pinned to the oracle by
tests/test_grammar_sweep_corpus.py) go through every entry of the device parse:

  a  the three calls (isolated stage 1, string pass, walk), short9 also at maxDepth 2 and 3
  b  BatchShard.step(), the optimistic entry, on accepted batches: twice, identical; short9 also in product order and at maxDepth 3
  c  the same batches with one document that fails stage 1 in the middle: the repair stage behind SJMI_ST_REJECTED
  d  step(exact=True)
  e  SimdJsonParser.parse_batch: the host walker and the pipeline
  f  single documents (every sequence of up to four tokens of nine) under the three placements of stage 2

Each family is one batch, a '\\n' behind every document, in a seeded shuffled order so that every seam of a run has unrelated
neighbours.  The comparison is the same everywhere (compare()): the error codes as one array against the oracle's, no document
handed back, the record's count of failed documents, every kept document's tape word for word and as a tree, the slots of the
failing ones, a canary behind the tape -- and every test asserts that it compared the family's full count.

Wall time on one MI355X (pytest --durations=0, one process, the oracle's share included): 12.7 s for the module's 26 tests.  The two
parse_batch tests of short13 take 3.0 s each (the call returns one Python slice per document), the first test 2.4 s (1.6 s of it the
context), every other test under 0.9 s; 7,380 single documents take 0.36 s on the host walker and by size, 0.64 s on the GPU walker."""
import os
import time
from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as O
from tests import grammar_sweep as G
from tests.walk_common import NEEDS_HOST, assert_tape_equal

pytestmark = pytest.mark.gpu

Batch = namedtuple("Batch", "docs buf offs errors parsed pred")  # errors / pred per position, parsed {position: oracle.Parsed}
STAGE1_FAILURE = b'["abc'
SEED = 20

_batches = {}


def make_batch(parts, seed=None, max_depth=1024):
    """parts: (family, its first `upto` documents or None for all of them), laid end to end, then shuffled by `seed`"""
    docs, errors, parsed = [], [], {}
    for name, upto in parts:
        d, (e, p) = G.family(name), G.answers(name, max_depth)
        n = len(d) if upto is None else upto
        parsed.update({len(docs) + k: v for k, v in p.items() if k < n})
        docs += d[:n]
        errors.append(e[:n])
    errors = np.concatenate(errors)
    pred = G.predicted_lengths(docs, errors)
    if seed is not None:
        perm, docs = G.shuffled(docs, seed)
        inv = np.argsort(perm)
        errors, pred, parsed = errors[perm], pred[perm], {int(inv[k]): v for k, v in parsed.items()}
    buf, offs = G.pack(docs)
    return Batch(docs, buf, offs, errors, parsed, pred)


def batch(name, order="shuffled", max_depth=1024):
    """one family as one batch, made once per module run (shared: leave it unchanged)"""
    key = (name, order, max_depth)
    if key not in _batches:
        _batches[key] = make_batch([(name, None)], SEED if order == "shuffled" else None, max_depth)
    return _batches[key]


def with_stage1_failure(b):
    """the batch with one unclosed string inserted in the middle: rejected by the plain pass, taken by the repair stage"""
    at = len(b.docs) // 2 + 7
    docs = b.docs[:at] + [STAGE1_FAILURE] + b.docs[at:]
    want = O.parse(STAGE1_FAILURE + b"\n")
    assert want.error == 2
    buf, offs = G.pack(docs)
    return Batch(docs, buf, offs, np.insert(b.errors, at, want.error), {k + (k >= at): v for k, v in b.parsed.items()},
                 np.insert(b.pred, at, -1))


def laid_out(rejected, err, to):
    """tests/test_gpu_pipeline.py's tapes_laid_out without its loop: were the tapes laid out before the walk (True), packed behind
    it (False), or can the outputs not tell (None)?  A document that fails stage 1 tells: two words laid out, none packed."""
    s1 = (err >= 1) & (err <= 3)
    if s1.any():
        sizes = np.unique(np.diff(to.astype(np.int64))[s1]).tolist()
        assert sizes in ([0], [2]), sizes
        assert rejected is not False  # (a batch with a document that fails stage 1 is never the plain pass's)
        return sizes == [2]
    return True if rejected is False else None


def compare(tag, b, err, tape_of, strings, to=None, lo=False, failed=None):
    """The outputs of one entry against the oracle.  err: the per-document codes; tape_of(k): document k's tape; to: the tape
    offsets (None: the entry has checked itself that failing documents are empty); lo: laid_out()'s answer; failed: the result
    record's count of failed documents.  -> the number of documents compared"""
    err = np.asarray(err)
    assert err.size == b.errors.size == len(b.docs), (tag, err.size, len(b.docs))
    wrong = np.nonzero(err != b.errors)[0]
    assert wrong.size == 0, (tag, "%d verdicts differ; (position, document, device, oracle):" % wrong.size,
                             [(int(k), b.docs[k][:80], int(err[k]), int(b.errors[k])) for k in wrong[:5]])
    assert not (err == NEEDS_HOST).any(), tag
    if failed is not None:
        assert failed == int((b.errors != 0).sum()), (tag, failed)
    kept = np.nonzero(err == 0)[0]
    assert kept.size == len(b.parsed), tag
    for k in kept:
        want, got = b.parsed[int(k)], tape_of(int(k))
        assert_tape_equal(got, strings, want, (tag, int(k), b.docs[k][:80]))
        assert O.Parsed(got, strings, 0, 0, 0).to_python() == want.to_python(), (tag, int(k), b.docs[k][:80])
    if to is not None:
        # a failing document's slot (tests/test_gpu_pipeline.py, assert_failing_slots): empty when the tapes are packed behind the
        # walk; when they were laid out in advance, two words if it fails stage 1 and else its predicted length
        size = np.diff(to.astype(np.int64))
        assert size.size == err.size and int(to[0]) == 0, tag
        want = np.where((err >= 1) & (err <= 3), 2, b.pred)
        ok = size == 0 if lo is False else (size == want if lo is True else (size == want) | (size == 0))
        wrong = np.nonzero((err != 0) & ~ok)[0]
        assert wrong.size == 0, (tag, "slots of failing documents, laid out: %s; (position, document, code, slot, predicted):" % lo,
                                 [(int(k), b.docs[k][:80], int(err[k]), int(size[k]), int(want[k])) for k in wrong[:5]])
    return err.size


def three_calls(ctx, b, max_depth=1024, tag="three calls"):
    """entry a (tests/test_gpu_walk.py's gpu_walk: it holds the record's counts to the codes, every failing document to an empty
    slot and the canary behind the tape itself)"""
    from tests.test_gpu_walk import gpu_walk
    tapes, strings, err = gpu_walk(ctx, b.docs, max_depth=max_depth, packed=(b.buf, b.offs))
    return compare(tag, b, err, lambda k: tapes[k], strings)


Step = namedtuple("Step", "rejected err to tape strings counts")


def shard_steps(ctx, b, exact=False, max_depth=1024, steps=1):
    """One BatchShard over the batch, a canary behind its tape; `steps` steps, check() behind the last one (which makes the call
    for rejected batches when the optimistic step says SJMI_ST_REJECTED).  -> one Step per step; the outputs of the steps in front
    of the last are read before check(), so they are valid only if that step was not rejected."""
    import torch
    from simdjson_java_amd import sharding
    from tests.test_gpu_walk import CANARY, CANARY_WORDS
    shard = sharding.BatchShard(ctx, b.buf, b.offs, torch.device("cuda", 0), max_depth=max_depth)
    shard.tape = torch.full((shard.tape_capacity + CANARY_WORDS,), CANARY, dtype=torch.int64, device=shard.device)
    n, out = len(b.docs), []
    for i in range(steps):
        shard.step(torch.cuda.current_stream().cuda_stream, exact=exact)
        torch.cuda.synchronize()
        rejected = None if exact else bool(int(shard.result.cpu().numpy()[1]) & 0x800)
        counts = shard.check() if i == steps - 1 else None
        tape = shard.tape.cpu().numpy().view(np.uint64)
        assert (tape[shard.tape_capacity:] == np.uint64(CANARY)).all(), "a store behind the tape's capacity"
        strings = bytes(shard.sb[:counts["string_bytes"]].cpu().numpy()) if counts else None
        out.append(Step(rejected, shard.doc_errors.cpu().numpy()[:n].copy(), shard.tape_offsets.cpu().numpy()[:n + 1].copy(), tape,
                        strings, counts))
    return out


def compare_step(tag, b, s, lo):
    assert s.counts["documents"] == len(b.docs) and s.counts["host_documents"] == 0, (tag, s.counts)
    return compare(tag, b, s.err, lambda k: s.tape[int(s.to[k]):int(s.to[k + 1])], s.strings, to=s.to, lo=lo,
                   failed=s.counts["failed_documents"])


def optimistic_accepted(ctx, b, max_depth=1024, tag="optimistic"):
    """entry b: two steps of the optimistic entry on a batch the plain pass accepts -- the token walker is what ran, the tapes were
    laid out before the walk, and the second step's codes, offsets and kept documents' words are the first's"""
    first, second = shard_steps(ctx, b, max_depth=max_depth, steps=2)
    assert first.rejected is False and second.rejected is False, (tag, "the batch was rejected: the token walker did not run")
    assert laid_out(False, second.err, second.to) is True
    n = compare_step(tag, b, second, True)
    assert np.array_equal(first.err, second.err) and np.array_equal(first.to, second.to), (tag, "the two steps differ")
    words = np.repeat(second.err == 0, np.diff(second.to.astype(np.int64)))
    assert np.array_equal(first.tape[:words.size][words], second.tape[:words.size][words]), (tag, "the two steps' tapes differ")
    return n


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 16 << 20)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["short9", "short13", "short12s", "edits"])
def test_three_calls(ctx, name):
    assert three_calls(ctx, batch(name)) == G.COUNTS[name]


@pytest.mark.parametrize("max_depth", [2, 3])
def test_three_calls_under_a_depth_limit(ctx, max_depth):
    b = batch("short9", max_depth=max_depth)
    assert (b.errors == 28).any()
    assert three_calls(ctx, b, max_depth=max_depth, tag="three calls, maxDepth %d" % max_depth) == G.COUNTS["short9"]


@pytest.mark.parametrize("name,order", [("short9", "shuffled"), ("short9", "product"), ("short13", "shuffled"), ("edits", "shuffled")])
def test_optimistic_entry(ctx, name, order):
    assert optimistic_accepted(ctx, batch(name, order), tag="optimistic, %s" % order) == G.COUNTS[name]


def test_optimistic_entry_under_a_depth_limit(ctx):
    assert optimistic_accepted(ctx, batch("short9", max_depth=3), max_depth=3, tag="optimistic, maxDepth 3") == G.COUNTS["short9"]


@pytest.mark.parametrize("name", ["short9", "short13", "edits", "short12s"])
def test_repair_stage(ctx, name):
    """entry c: one `["abc` in the middle of an accepted batch -- short12s as it is, a third of it fails stage 1 -- sends the batch
    to the repair stage behind SJMI_ST_REJECTED: the walk runs over the sanitized copy, the failing document blanked inside a run"""
    b = batch(name) if name == "short12s" else with_stage1_failure(batch(name))
    s, = shard_steps(ctx, b)
    lo = laid_out(s.rejected, s.err, s.to)
    assert s.rejected and lo, "the repair stage did not take the batch"
    assert compare_step("repair", b, s, True) == G.COUNTS[name] + (name != "short12s")


@pytest.mark.parametrize("name", ["short9", "short13", "short12s", "edits"])
def test_exact_entry(ctx, name):
    b = batch(name)
    s, = shard_steps(ctx, b, exact=True)
    assert compare_step("exact entry", b, s, laid_out(None, s.err, s.to)) == G.COUNTS[name]


@pytest.mark.parametrize("name", ["short13", "short12s"])
@pytest.mark.parametrize("walk", ["host_walk", "pipeline"])
def test_parse_batch(walk, name):
    """entry e: SimdJsonParser.parse_batch -- the C++ host walker over GPU-made indexes and strings, and (SJMI_PARSE_PIPELINE=1 at
    construction, as tests/test_gpu_walk.py sets it) the device pipeline behind the same call"""
    import simdjson_java_amd as S
    b = batch(name)
    if walk == "pipeline":
        os.environ["SJMI_PARSE_PIPELINE"] = "1"
    try:
        p = S.SimdJsonParser(capacity=len(b.buf) + 64)
    finally:
        os.environ.pop("SJMI_PARSE_PIPELINE", None)
    try:
        tapes, strings, err = p.parse_batch(b.buf, b.offs)
        assert all(t is None for t, e in zip(tapes, err) if e != 0)
        assert compare("parse_batch, %s" % walk, b, err, lambda k: tapes[k], strings) == G.COUNTS[name]
    finally:
        p.close()


SINGLE_TOKENS = {"host_walk": 4, "gpu_walk": 4, "by_size": 4}  # every sequence of 1..4 tokens of T9: 7,380 documents


@pytest.mark.parametrize("placement", ["host_walk", "gpu_walk", "by_size"])
def test_single_documents(placement):
    """entry f: SimdJsonParser.parse under the three placements of tests/test_gpu_parse.py, with that module's _same: the code,
    the message, the tape and the strings of every document"""
    import simdjson_java_amd as S
    from tests.test_gpu_parse import _same
    docs = G.short9(SINGLE_TOKENS[placement])
    p = S.SimdJsonParser(capacity=1 << 20, gpu_walk={"host_walk": False, "gpu_walk": True, "by_size": None}[placement])
    try:
        t0, kept = time.time(), 0
        for d in docs:
            kept += _same(p, d) is not None
        print("single documents, %s: %d documents in %.2f s" % (placement, len(docs), time.time() - t0))
    finally:
        p.close()
    assert len(docs) == G.n_sequences(9, SINGLE_TOKENS[placement]) == 7380
    assert kept == int((G.answers("short9")[0][:len(docs)] == 0).sum()) == 10


def forced_run_sweep(ctx, seed):
    """for tests/test_gpu_tok_stream_runs.py's children, one per forced run size: short9 up to five tokens and the edits as one
    batch, shuffled by `seed`, through the three calls and the optimistic entry.  -> documents compared per entry"""
    b = make_batch([("short9", G.SHORT9_UP_TO_5), ("edits", None)], seed)
    n = three_calls(ctx, b, tag="three calls, sweep")
    assert optimistic_accepted(ctx, b, tag="optimistic, sweep") == n == G.SHORT9_UP_TO_5 + G.COUNTS["edits"]
    return n
