"""The stream walker (k_tok_stream, coop_walk.hip) on MULTI-DOCUMENT runs, with broken neighbours at every seam.

The launch sizes a run as ceil(n / (W * j)) documents (W resident waves), so every batch below several thousand documents walks one
document per run and never reaches what the kernel does where documents meet inside a step or a run: DOCSTART re-basing, NC (a
document not back at depth 0 where the next one starts), the FL0 / REG / ACT masking of documents that failed earlier, the previous
document's root words written at the next one's start, the string word stored one step late, the primitive queue flushed across
documents.  SJMI_TS_RUN_DOCS forces the run size; it is read once per process, so each size runs in a fresh child process (one after
another, each under its own time limit; the first child that dies by a signal or a timeout ends the test).

In each child the seam layouts of tests/tok_stream_layouts.py go through (a) the three calls -- three times, identical -- and at
maxDepth 4 and 63, (b) the optimistic entry on an accepted batch (tapes laid out before the walk), (c) the same batch plus one
document that fails stage 1 (the repair stage: its blanked document is an empty one inside a run), (d) the exact entry.  Per document:
the oracle's error code, a kept document's tape word for word, the slot of a failing one; a canary behind the tape's capacity.
(e) Every sequence of up to five tokens and the single-token edits of tests/grammar_sweep.py (75,242 documents, shuffled by the run
size) through the three calls and the optimistic entry, compared as tests/test_gpu_grammar_sweep.py compares them."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUN_SIZES = [1, 2, 3, 5, 8, 16]  # 1: what the rest of the suite reaches
N_DOCS = 16000
CHILD_TIMEOUT = 600


def _check(tag, docs, wants, err, tape_of, strings):
    from tests.walk_common import NEEDS_HOST, assert_tape_equal
    for k, d in enumerate(docs):
        e = int(err[k])
        assert e != NEEDS_HOST, (tag, k, d[:40])
        assert e == wants[k].error, (tag, k, d[:60], e, wants[k].error)
        if e == 0:
            assert_tape_equal(tape_of(k), strings, wants[k], (tag, k, d[:40]))


def _shard(ctx, docs, exact):
    """one step of a BatchShard -> (rejected bit of the optimistic step or None, err, to, tape, strings); a canary behind the tape"""
    import torch
    from simdjson_java_amd import sharding
    from tests.test_gpu_walk import CANARY, CANARY_WORDS
    buf = b"".join(d + b"\n" for d in docs)
    offs = np.concatenate([[0], np.cumsum([len(d) + 1 for d in docs])]).astype(np.uint64)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.tape = torch.full((shard.tape_capacity + CANARY_WORDS,), CANARY, dtype=torch.int64, device=shard.device)
    shard.step(torch.cuda.current_stream().cuda_stream, exact=exact)
    torch.cuda.synchronize()
    rejected = None if exact else bool(int(shard.result.cpu().numpy()[1]) & 0x800)
    c = shard.check()
    tape = shard.tape.cpu().numpy().view(np.uint64)
    assert (tape[shard.tape_capacity:] == np.uint64(CANARY)).all(), "a store behind the tape's capacity"
    n = len(docs)
    return rejected, shard.doc_errors.cpu().numpy()[:n], shard.tape_offsets.cpu().numpy()[:n + 1], tape, \
        bytes(shard.sb[:c["string_bytes"]].cpu().numpy()), c


def child():
    """one run size (SJMI_TS_RUN_DOCS): everything in the module docstring"""
    import simdjson_java_amd as S
    from oracle import oracle as O
    from tests import tok_stream_layouts as L
    from tests.test_gpu_pipeline import assert_failing_slots, tapes_laid_out
    from tests.test_gpu_walk import gpu_walk
    run = int(os.environ["SJMI_TS_RUN_DOCS"])
    # the layouts without documents that fail stage 1 (one of those sends its whole run to the exact walker), then all of them
    docs, kinds = L.batch(seed=run, n_docs=N_DOCS, kinds=[k for k in L.BROKEN if k != "s1"])
    all_docs, _ = L.batch(seed=run + 100, n_docs=N_DOCS // 4)
    wants = [O.parse(d + b"\n") for d in docs]
    for d, k, w in zip(docs, kinds, wants):
        assert (w.error == 0) == (k in ("valid", "filler", "scalar", "deep")), (k, d[:40], w.error)
    ctx = S.Context(0, 1 << 20)
    try:
        # (a) the three calls, three times: identical, and against the oracle; at maxDepth 4 and 63; with stage-1 failures in runs
        first = None
        for i in range(3):
            tapes, strings, err = gpu_walk(ctx, docs)
            if first is None:
                _check("three calls", docs, wants, err, lambda k: tapes[k], strings)
                first = (tapes, strings, err)
            else:
                assert np.array_equal(err, first[2]) and strings == first[1], ("three calls, repeat", i)
                assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(tapes, first[0])), ("three calls, repeat", i)
        for md in (4, 63):
            w_md = [O.parse(d + b"\n", max_depth=md) for d in docs]
            tapes, strings, err = gpu_walk(ctx, docs, max_depth=md)
            _check("three calls, maxDepth %d" % md, docs, w_md, err, lambda k: tapes[k], strings)
        tapes, strings, err = gpu_walk(ctx, all_docs)
        _check("three calls, stage-1 failures", all_docs, [O.parse(d + b"\n") for d in all_docs], err, lambda k: tapes[k], strings)
        # (b) the optimistic entry on the accepted batch: tapes laid out before the walk
        rejected_b, err, to, tape, strings, c = _shard(ctx, docs, exact=False)
        _check("optimistic", docs, wants, err, lambda k: tape[int(to[k]):int(to[k + 1])], strings)
        laid_out = tapes_laid_out(rejected_b, docs, err, to)
        assert_failing_slots(docs, err, to, laid_out)
        assert c["failed_documents"] == sum(1 for w in wants if w.error)
        # (c) ... plus one document that fails stage 1: the repair stage, its blanked document an empty one inside a run
        docs_c = list(docs)
        docs_c.insert(len(docs) // 2 + 7, b'["abc')
        wants_c = list(wants)
        wants_c.insert(len(docs) // 2 + 7, O.parse(b'["abc\n'))
        rejected, err, to, tape, strings, c = _shard(ctx, docs_c, exact=False)
        _check("repair", docs_c, wants_c, err, lambda k: tape[int(to[k]):int(to[k + 1])], strings)
        assert rejected and tapes_laid_out(rejected, docs_c, err, to), "the repair stage did not take the batch"
        assert_failing_slots(docs_c, err, to, True)
        # (d) the exact entry
        _, err, to, tape, strings, c = _shard(ctx, docs_c, exact=True)
        _check("exact entry", docs_c, wants_c, err, lambda k: tape[int(to[k]):int(to[k + 1])], strings)
        assert_failing_slots(docs_c, err, to, tapes_laid_out(None, docs_c, err, to))
        assert rejected_b is False, "the layout batch was rejected by the plain pass: (b) did not test the accepted path"
        # (e) every sequence of up to five tokens and the single-token edits of long documents (tests/grammar_sweep.py), shuffled by
        # the run size: which error each document gets, through the three calls and the optimistic entry
        from tests.test_gpu_grammar_sweep import forced_run_sweep
        swept = forced_run_sweep(ctx, seed=run)
    finally:
        ctx.close()
    print("TOK_STREAM_RUNS_OK", run, len(docs), swept)


def test_multi_document_runs_against_the_oracle():
    from tests.conftest import ROOT
    failures = []
    for run in RUN_SIZES:
        env = dict(os.environ, SJMI_TS_RUN_DOCS=str(run))
        cmd = [sys.executable, "-c", "import sys; sys.path.insert(0, %r); from tests.test_gpu_tok_stream_runs import child; child()" % ROOT]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT, env=env, cwd=ROOT)
        except subprocess.TimeoutExpired:
            pytest.fail("run size %d: no result within %d s -- the sizes behind it were not started" % (run, CHILD_TIMEOUT))
        if out.returncode < 0:
            pytest.fail("run size %d: the child died by signal %d -- the sizes behind it were not started\n%s" %
                        (run, -out.returncode, out.stderr[-3000:]))
        if out.returncode != 0 or "TOK_STREAM_RUNS_OK" not in out.stdout:
            failures.append("run size %d (exit %d):\n%s" % (run, out.returncode, out.stderr[-2500:]))
    assert not failures, "\n\n".join(failures)
