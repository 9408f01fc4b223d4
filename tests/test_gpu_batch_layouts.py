"""The accepted batch's layout pass (k_doc_prepare, batch.hip; k_batch_layout / k_tape_offsets, walk.hip) on the layouts of
tests/batch_layouts.py: a document boundary at every offset of a 64-byte block with every count of structurals in front of it,
crowded blocks, blocks entered inside a string, backslash runs up to a block's start, quotes behind primitives, word classes at
the edges, every count of whole blocks from every start block, 2 .. 513 documents, tiny batches, every kind of batch end.  That
the layouts hold these conditions is asserted on the CPU (tests/test_batch_layouts.py).

Every batch goes through BatchShard.step by the optimistic entry (twice: the second step reuses the workspaces) and must not be
rejected, then by the exact entry; then through the repair stage, where k_doc_prepare runs in its relaxed form over the sanitized
copy: with three documents that fail stage 1 put in (an unclosed string, invalid UTF-8, a failing document that ends in an odd
backslash run; one a block ahead of a hazard, one inside a hazard's block, one directly behind a hazard; each 64 bytes long, so
that every offset behind it stays), and once with blank separators and no failing document.
One more batch, backslash_in_front_of_dense, is the one the repair stage must decline (its test says why).

Everything is compared with the oracle directly, nothing with another path of the engine: index_offsets and every document's
indexes (oracle.stage1), doc_errors (oracle.parse), every well-formed document's tape and tree, the slot sizes (a well-formed
document: its tape's length; one that fails stage 2: its predicted length; one that fails stage 1: two words; tape_offsets[0] = 0,
tape_words their sum), doc_string_offsets (cumulative string bytes, where every document is well-formed), canaries behind the
capacities of the tape and of the index array."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import batch_layouts as BL
from tests.walk_common import assert_tape_equal

pytestmark = pytest.mark.gpu

IDX_CANARY, IDX_CANARY_WORDS = 0x7E5A7E5A, 512
_wants = {}


def _oracle(key, docs):
    """the oracle's verdicts of a batch's documents, computed once per batch and never changed"""
    if key not in _wants:
        _wants[key] = [(O.stage1(d), O.parse(d)) for d in docs]
    return _wants[key]


def _run(ctx, buf, offs, exact):
    """two steps of a fresh BatchShard, canaries behind the tape and the index array -> (rejected bit of the optimistic step or
    None, the shard, check()'s record)"""
    import torch
    from simdjson_java_amd import sharding
    from tests.test_gpu_walk import CANARY, CANARY_WORDS
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.tape = torch.full((shard.tape_capacity + CANARY_WORDS,), CANARY, dtype=torch.int64, device=shard.device)
    shard.idx = torch.full((shard.index_capacity + IDX_CANARY_WORDS,), IDX_CANARY, dtype=torch.int32, device=shard.device)
    for _ in range(2):
        shard.step(torch.cuda.current_stream().cuda_stream, exact=exact)
        torch.cuda.synchronize()
    rejected = None if exact else bool(int(shard.result.cpu().numpy()[1]) & 0x800)
    c = shard.check()
    tape = shard.tape.cpu().numpy().view(np.uint64)
    assert (tape[shard.tape_capacity:] == np.uint64(CANARY)).all(), "a store behind the tape's capacity"
    assert (shard.idx[shard.index_capacity:].cpu().numpy() == IDX_CANARY).all(), "a store behind the index array's capacity"
    return rejected, shard, c


def _verify(tag, buf, offs, docs, wants, shard, c, check_dso, laid_out=True):
    """every per-document output of a step against the oracle; a failure names the batch, the document, its boundary's offset
    inside its block and the structurals of that block in front of it (counted on the documents' own structurals, so that it
    holds with failing documents in the batch too).  laid_out=False: the tapes were packed behind the per-document passes, a
    failing document's slot is empty"""
    from tests.tok_stream_layouts import predicted_length
    n = len(docs)
    o, cnt = BL.boundary_profile_per_document(offs, [None if w[0][1] else w[0][0] for w in wants])

    def at(k):
        return "%s: document %d %r, boundary offset %d, structurals of the block in front of it %d" % (
            tag, k, docs[k][:40], int(o[k]), int(cnt[k]))
    to = shard.tape_offsets.cpu().numpy()[:n + 1]
    tape = shard.tape.cpu().numpy().view(np.uint64)
    err = shard.doc_errors.cpu().numpy()[:n]
    io = shard.index_offsets.cpu().numpy()[:n + 1]
    idx = shard.idx.cpu().numpy()[:c["structurals"] + 1].view(np.uint32)
    strings = bytes(shard.sb[:c["string_bytes"]].cpu().numpy())
    dso = shard.doc_string_offsets.cpu().numpy()[:n + 1]
    assert int(to[0]) == 0 and int(io[0]) == 0, tag
    n_io = n_dso = n_bad = 0
    for k, d in enumerate(docs):
        (want_idx, st), want = wants[k]
        # the index range
        n_io += 0 if st else want_idx.size
        assert int(io[k + 1]) == n_io, (at(k), "index_offsets[k + 1]", int(io[k + 1]), n_io)
        got_idx = idx[int(io[k]):int(io[k + 1])].astype(np.int64) - int(offs[k])
        assert np.array_equal(got_idx, want_idx.astype(np.int64) if not st else np.zeros(0, np.int64)), (at(k), "indexes")
        # the verdict
        assert int(err[k]) == want.error, (at(k), "doc_errors", int(err[k]), want.error)
        # the slot
        size = int(to[k + 1]) - int(to[k])
        want_size = want.tape.size if want.error == 0 else (0 if not laid_out else 2 if st else predicted_length(d))
        assert size == want_size, (at(k), "tape slot", size, want_size)
        if check_dso:
            assert int(dso[k]) == n_dso, (at(k), "doc_string_offsets", int(dso[k]), n_dso)
            n_dso += len(want.strings)
        if want.error:
            n_bad += 1
            continue
        got = tape[int(to[k]):int(to[k + 1])]
        assert_tape_equal(got, strings, want, at(k))
        assert O.Parsed(got, strings, 0, 0, 0).to_python() == want.to_python(), at(k)
    if check_dso:
        assert int(dso[n]) == n_dso == c["string_bytes"], (tag, int(dso[n]), n_dso, c["string_bytes"])
    assert c["tape_words"] == int(to[n]), (tag, c["tape_words"], int(to[n]))
    assert c["structurals"] == n_io and c["failed_documents"] == n_bad and c["host_documents"] == 0, (tag, c, n_io, n_bad)


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(BL.FAMILIES))
def test_accepted_batch_layouts_against_the_oracle(ctx, name):
    for L in BL.family(name):
        buf, offs, docs, hz = L.render()
        wants = _oracle((L.name, "plain"), docs)
        rejected, shard, c = _run(ctx, buf, offs, exact=False)
        assert rejected is False and getattr(shard, "rejected_steps", 0) == 0, "%s: the plain pass rejected the batch" % L.name
        assert c["stage1_status"] == 0, (L.name, c)
        _verify(L.name + " (optimistic entry)", buf, offs, docs, wants, shard, c, check_dso=L.wellformed)
        _, shard, c = _run(ctx, buf, offs, exact=True)
        _verify(L.name + " (exact entry)", buf, offs, docs, wants, shard, c, check_dso=L.wellformed)


@pytest.mark.parametrize("name", list(BL.FAMILIES))
def test_batch_layouts_through_the_repair_stage(ctx, name):
    """(with blank separators and only well-formed documents nothing in the outputs tells the repair stage from the per-document
    passes: there the shard's own record says which call took the batch; wherever a document fails, its slot tells)"""
    from tests.test_gpu_pipeline import assert_failing_slots, tapes_laid_out
    for i, L in enumerate(BL.family(name)):
        ins = BL.repair_inserts(L, rotate=i)
        for variant, kw in (("failing documents " + ", ".join("%s %s of %d" % (BL.failing_documents()[(j + i) % 3][0], t[3], t[4])
                                                              for j, t in enumerate(ins)), dict(inserts=[t[:3] for t in ins])),
                            ("blank separators", dict(blank_separators=True))):
            buf, offs, docs, hz = L.render(**kw)
            tag = "%s, repair stage, %s" % (L.name, variant)
            wants = _oracle((L.name, variant), docs)
            rejected, shard, c = _run(ctx, buf, offs, exact=False)
            assert rejected is True and shard.rejected_steps == 1, tag + ": not rejected"
            assert not getattr(shard, "unrepairable", False), tag + ": the repair stage did not take the batch"
            to = shard.tape_offsets.cpu().numpy()[:len(docs) + 1]
            err = shard.doc_errors.cpu().numpy()[:len(docs)]
            laid_out = tapes_laid_out(rejected, docs, err, to)
            assert laid_out is not False and (laid_out or "inserts" not in kw), tag + ": the tapes were not laid out in advance"
            assert_failing_slots(docs, err, to, True)
            _verify(tag, buf, offs, docs, wants, shard, c, check_dso=L.wellformed and "inserts" not in kw)


def test_a_surviving_trailing_backslash_in_front_of_a_dense_boundary_block_is_not_repaired(ctx):
    """The one batch here that the repair stage must decline (as "none, a trailing backslash" of
    test_the_repair_stage_takes_what_it_can_and_only_that): no separators, and `[1]\\` -- it passes stage 1, so it survives the
    sanitizer, and its backslash would escape the quote its neighbour begins with -- directly in front of a dense document whose
    boundary has >= 17 structurals of its block in front.  The optimistic step is rejected, the call for rejected batches says
    REJECTED once more, the exact call decides every document by the per-document passes: tapes packed behind the walk, the slot
    of the document that fails stage 1 (and of every failing one) empty.  Everything against the oracle, every document alone."""
    from tests.test_gpu_pipeline import assert_failing_slots, tapes_laid_out
    L = BL.backslash_in_front_of_dense()
    buf, offs, docs, hz = L.render()
    wants = _oracle((L.name, "plain"), docs)
    for exact in (False, True):
        tag = "%s (%s entry)" % (L.name, "exact" if exact else "optimistic")
        rejected, shard, c = _run(ctx, buf, offs, exact=exact)
        if not exact:
            assert rejected is True and shard.rejected_steps == 1, tag + ": not rejected"
            assert getattr(shard, "unrepairable", False), tag + ": the repair stage took a batch with a surviving trailing backslash"
        to = shard.tape_offsets.cpu().numpy()[:len(docs) + 1]
        err = shard.doc_errors.cpu().numpy()[:len(docs)]
        assert tapes_laid_out(rejected, docs, err, to) is False, tag + ": the tapes were laid out in advance"
        assert_failing_slots(docs, err, to, False)
        _verify(tag, buf, offs, docs, wants, shard, c, check_dso=False, laid_out=False)
