"""One context per host thread, several threads in one process: the deployment include/sjmi.h describes (one sjmi_ctx per
SimdJsonParser, a parser per thread).  Four Python threads (ctypes releases the GIL inside a call) with a context each make the host
calls side by side -- three of them stage1, stage1_unescape, parse_document, stage1_batch and SimdJsonParser.parse_batch on
documents of 0 bytes to 6 MiB, the fourth two cases of tests/query_fuzz.py through the column operators, whose scratch growth and
plan uploads drain the device -- while each creates and destroys one more context every fifth round.  So the process-wide registry
of csrc/sjmi_api.hip (its mutex, the hipEventQuery of another context's event, sjmi_destroy of a context others may be polling,
hipDeviceSynchronize under other threads' launches) runs under a test, and with it the ticketed-first-granule form of k_stage1
where the library itself switches it on.

Every expected value is computed before the threads start; every result of every round must equal it.  A thread records its first
mismatch or exception instead of raising; the main thread asserts after joining.  sjmi_debug_counters of every context is printed:
every context queued launches, and at least one launch of the run was flagged because another context was busy -- with four threads
launching for seconds that is no matter of luck; if it fails, the registry does not work.  Repeats in SAFE mode are printed, not
asserted: on a shared GPU a neighbour can cause them (profiles/r29/README.md has the figures of one run)."""
import os
import random
import sys
import threading
import time
import traceback

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_tickets_shapes as A
from tests import query_fuzz as QF
from tests.conftest import load_fixture
from tests.walk_common import assert_tape_equal

pytestmark = pytest.mark.gpu

N_THREADS, ROUNDS = 4, 25
CAPACITY = 8 << 20
QUERY_CASES = ("d1025_doubles_v40", "d2500_mixed_v600")
JOIN_SECONDS = 240


def _u8(doc):
    return doc if isinstance(doc, np.ndarray) else np.frombuffer(bytes(doc), dtype=np.uint8)


# ---- one call and its expected value -> a function of the context that returns None or what differs ----------------------------------
def stage1_item(name, doc, length=None):
    a = _u8(doc)
    n = a.size if length is None else length
    want_idx, want_st = O.stage1(a, n)

    def run(ctx):
        idx, st = ctx.stage1(a, n)
        if st != want_st or not np.array_equal(idx, want_idx):
            return "stage1(%s): status %d for %d, %d indexes for %d" % (name, st, want_st, idx.size, want_idx.size)
    return run


def unescape_item(name, doc, strings=True):
    """strings=False: a text that passes stage 1 and is no JSON document (a shape of all_tickets_shapes: quotes behind primitives
    open strings without being structurals, which the reference's loop over the '"' structurals does not see -- include/sjmi.h,
    sjmi_unescape_device): only the stage-1 outputs of the fused call are compared"""
    doc = bytes(doc)
    a = _u8(doc)
    want_idx, want_st = O.stage1(a)
    assert want_st == 0, name
    if not strings:
        def stage1_part(ctx):
            idx, st, _sb, _fei, _fec = ctx.stage1_unescape(a)
            if st != 0 or not np.array_equal(idx, want_idx):
                return "stage1_unescape(%s): status %d, %d indexes for %d" % (name, st, idx.size, want_idx.size)
        return stage1_part
    want_sb, _offs, want_feo, want_fec = O.unescape_all(doc + b"\0" * 64, want_idx)
    want_fei = None
    if want_feo >= 0:  # (the oracle counts strings, the engine positions in indexes[])
        want_fei = [i for i in range(want_idx.size) if doc[want_idx[i]] == 0x22][want_feo]

    def run(ctx):
        idx, st, sb, fei, fec = ctx.stage1_unescape(a)
        if st != 0 or not np.array_equal(idx, want_idx):
            return "stage1_unescape(%s): status %d, %d indexes for %d" % (name, st, idx.size, want_idx.size)
        if want_fei is None:
            if fei is not None or fec != 0 or bytes(sb) != want_sb:
                return "stage1_unescape(%s): strings differ (%r, %d, %d bytes for %d)" % (name, fei, fec, sb.size, len(want_sb))
        elif fei != want_fei or fec != want_fec or bytes(sb[:len(want_sb)]) != want_sb:
            return "stage1_unescape(%s): first error (%r, %d) for (%d, %d)" % (name, fei, fec, want_fei, want_fec)
    return run


def parse_document_item(name, doc):
    doc = bytes(doc)
    want = O.parse(doc)

    def run(ctx):
        tape, strings, err, st = ctx.parse_document(doc)
        if st != want.stage1_status or err != want.error:
            return "parse_document(%s): (%d, %d) for (%d, %d)" % (name, err, st, want.error, want.stage1_status)
        if err == 0 and not (np.array_equal(tape, want.tape) and strings == want.strings):
            return "parse_document(%s): tape or strings differ" % name
    return run


def batch_item(name, docs):
    buf = b"".join(d + b"\n" for d in docs)
    offs = np.cumsum([0] + [len(d) + 1 for d in docs]).astype(np.uint64)
    want_idx, want_st = O.stage1(buf)  # (the plain batch is one launch over the packed buffer)
    assert want_st == 0
    want_io = np.searchsorted(want_idx, offs).astype(np.uint64)

    def run(ctx):
        idx, io, st = ctx.stage1_batch(buf, offs)
        if st != 0 or not np.array_equal(idx, want_idx) or not np.array_equal(io, want_io):
            return "stage1_batch(%s): status %d, %d indexes for %d, offsets equal: %s" % (name, st, idx.size, want_idx.size, np.array_equal(io, want_io))
    return run


def parse_batch_item(name, docs, parser):
    buf = b"".join(d + b"\n" for d in docs)
    offs = np.cumsum([0] + [len(d) + 1 for d in docs]).astype(np.uint64)
    wants = [O.parse(d + b"\n") for d in docs]

    def run(_ctx):
        tapes, strings, errors = parser.parse_batch(buf, offs)
        for k, w in enumerate(wants):
            if int(errors[k]) != w.error:
                return "parse_batch(%s): document %d: error %d for %d" % (name, k, int(errors[k]), w.error)
            if not w.error:
                try:
                    assert_tape_equal(tapes[k], strings, w, (name, k))
                except AssertionError as e:
                    return "parse_batch(%s): document %d: %s" % (name, k, e)
    return run


def _work(twitter):
    """-> ({kind: [item]}, the parsers the parse_batch items use) -- every expected value is computed here"""
    import simdjson_java_amd as S
    from tests.test_gpu_batch import _small_docs
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from token_docs import document
    github, wide, malformed = (load_fixture(n) for n in ("github_events.json", "wide_bench.json", "malformed.txt"))
    shapes = {}
    for k, n in enumerate((1, 2, 5, 9, 33, 65, 249, 257, 1025)):
        c = [c for c in A.cases(1) if c.n == n][k % len(A.KINDS)]
        shapes[c.name] = (c, A.text_of(c))
    assert any(c.open for c, _ in shapes.values()) and any(not c.open and c.n >= 33 for c, _ in shapes.values())
    six = (twitter * 10)[:6 << 20]
    items = {"stage1": [stage1_item("empty", b""), stage1_item("twitter", twitter), stage1_item("github_events", github),
                        stage1_item("wide_bench", wide), stage1_item("malformed", malformed), stage1_item("6 MiB", six)] +
                       [stage1_item(name, d, c.length) for name, (c, d) in shapes.items()]}
    closed = [(name, bytes(d[:c.length])) for name, (c, d) in shapes.items() if not c.open and 2 <= c.n <= 257]
    three = b"[" + b",".join([twitter.rstrip()] * 5) + b"]"
    items["unescape"] = [unescape_item("twitter", twitter), unescape_item("github_events", github), unescape_item("wide_bench", wide),
                         unescape_item("3 MiB", three), unescape_item("empty array", b"[]")] + \
                        [unescape_item(name, d, strings=False) for name, d in closed]
    items["parse_document"] = [parse_document_item("twitter", twitter), parse_document_item("github_events", github),
                               parse_document_item("[1 1]", b"[1 1]"), parse_document_item("unclosed", b'{"k": "v'),
                               parse_document_item("3 MiB", three)]
    rng = random.Random(5100)
    items["batch"] = [batch_item("small", _small_docs(rng, 800) + [github.rstrip(), b"[]", b"7"]),
                      batch_item("twitter x 3", [twitter.rstrip()] * 3 + _small_docs(rng, 50))]
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)
    try:
        docs = [document(rng) for _ in range(200)]
    finally:
        sys.setrecursionlimit(limit)
    for b in (b'["abc', bytes([0x5B, 0x22, 0xC3, 0x22, 0x5D]), b'"'):
        docs[rng.randrange(len(docs))] = b
    # a parser per thread, each with ONE engine context (a single sub-batch per call) and two stage-2 threads
    keep = {k: os.environ.get(k) for k in ("SJMI_PARSE_PIPELINE", "SJMI_PARSE_THREADS")}
    os.environ["SJMI_PARSE_PIPELINE"], os.environ["SJMI_PARSE_THREADS"] = "1", "2"
    try:
        parsers = [S.SimdJsonParser(capacity=1 << 20) for _ in range(N_THREADS - 1)]
    finally:
        for k, v in keep.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    items["parse_batch"] = [parse_batch_item("tokens", docs, p) for p in parsers]
    return items, parsers


def _plan(items, t, rng):
    """the calls of thread t < 3, round by round: the five kinds in rotation, mostly on small and medium documents"""
    plan = []
    for r in range(ROUNDS):
        calls = [rng.choice(items["stage1"]) for _ in range(6)] + [rng.choice(items["unescape"]) for _ in range(3)]
        calls += [items["parse_document"][(r + t) % len(items["parse_document"])], items["batch"][(r + t) % len(items["batch"])],
                  items["parse_batch"][t]]
        rng.shuffle(calls)
        plan.append(calls)
    return plan


def test_four_threads_with_a_context_each(twitter):
    import torch
    import simdjson_java_amd as S
    from tests.test_gpu_query_fuzz import run_case
    items, parsers = _work(twitter)
    for name in QUERY_CASES:  # (the answers of thread 3's queries: cached by query_fuzz)
        for q in QF.queries(name):
            QF.expected(name, q)
    plans = [_plan(items, t, random.Random(5200 + t)) for t in range(N_THREADS - 1)]
    small = stage1_item("extra", twitter[:70000])
    ctxs = [S.Context(device=0, capacity=CAPACITY) for _ in range(N_THREADS)]
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    barrier = threading.Barrier(N_THREADS)
    spare = threading.BoundedSemaphore(1)  # one short-lived context at a time: 4 + 3 (the parsers') + 1 = 8 alive at most
    mismatch, failure, counters, calls = [None] * N_THREADS, [None] * N_THREADS, [None] * N_THREADS, [0] * N_THREADS

    def note(t, r, bad):
        calls[t] += 1
        if bad and mismatch[t] is None:
            mismatch[t] = "thread %d, round %d: %s" % (t, r, bad)

    def worker(t):
        ctx = ctxs[t]
        try:
            barrier.wait(timeout=60)
            for r in range(ROUNDS):
                if r % 5 == 4:
                    with spare:
                        extra = S.Context(device=0, capacity=1 << 20)
                        try:
                            note(t, r, small(extra))
                        finally:
                            extra.close()
                if t < N_THREADS - 1:
                    for call in plans[t][r]:
                        note(t, r, call(ctx))
                elif r < len(QUERY_CASES):
                    run_case(ctx, side, QUERY_CASES[r])  # (raises on a mismatch: recorded below)
                    calls[t] += len(QF.queries(QUERY_CASES[r]))
                else:
                    note(t, r, small(ctx))
        except BaseException:
            failure[t] = traceback.format_exc()
        finally:
            try:
                counters[t] = ctx.debug_counters()
            except BaseException:
                failure[t] = (failure[t] or "") + traceback.format_exc()

    threads = [threading.Thread(target=worker, args=(t,), daemon=True, name="sjmi-%d" % t) for t in range(N_THREADS)]
    started = time.perf_counter()
    for th in threads:
        th.start()
    deadline = started + JOIN_SECONDS
    for th in threads:
        th.join(max(0.0, deadline - time.perf_counter()))
    stuck = [th.name for th in threads if th.is_alive()]
    if stuck:
        pytest.fail("threads not joined after %d s: %s (nothing more is started; their contexts stay open)" % (JOIN_SECONDS, stuck))
    elapsed = time.perf_counter() - started
    torch.cuda.synchronize()
    for p in parsers:
        p.close()
    for c in ctxs:
        c.close()
    print("\nfour threads, %d rounds, %.1f s, calls per thread %s" % (ROUNDS, elapsed, calls))
    for t, n in enumerate(counters):
        print("context %d: launches %d, flagged %d, repeats in SAFE mode %d, SAFE mode now %d" % ((t,) + tuple(n)))
    assert failure == [None] * N_THREADS, "\n".join(f for f in failure if f)
    assert mismatch == [None] * N_THREADS, [m for m in mismatch if m]
    assert all(n[0] > 0 for n in counters), counters
    assert any(n[1] > 0 for n in counters), "no launch of any context saw another context busy: %s" % counters
