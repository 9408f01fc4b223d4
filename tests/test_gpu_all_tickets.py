"""The stage-1 kernel's third assignment form -- FAST mode with the scanner workgroup and EVERY granule by ticket, a wave's first
one included (FLAG_ALL_TICKETS, csrc/stage1.hip) -- which a launch takes by itself while another context of the process still has
a stage-1 launch running (csrc/sjmi_api.hip: another_context_busy, note_launch), i.e. in the documented deployment of one context
per host thread.  Forced here with debug flag 0x800, alone and on the small grid (0x800 | 32), at the granule counts of
tests/all_tickets_shapes.py; then provoked for real by two contexts of one thread.  Everything is bit-exact against oracle.stage1 /
oracle.parse: indexes, count, the sentinel, the status.

Equality alone would also hold on a context that had tripped its spin bound and latched SAFE mode (another kernel instantiation:
the case would have covered nothing), so sjmi_debug_counters is read behind every case: every launch flagged, no repeat in SAFE
mode, SAFE mode off, no SJMI_ST_INTERNAL in any record.  A case that did latch is repeated once on a fresh context -- foreign work on
a shared GPU can trip the bound -- and the file fails if a case latches twice or if a second case needs the repeat."""
import os
import random
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_tickets_shapes as A
from tests import stream_fuzz as F
from tests.walk_common import assert_tape_equal

pytestmark = pytest.mark.gpu

ST_INTERNAL = 0x200
PATTERN = 0x5A5A5A5A
FRONT, BEHIND = 32, 64  # canary words in front of an index array (its base stays 128-byte aligned) and behind [count]
FLAGS = (A.FLAG_ALL_TICKETS, A.FLAG_ALL_TICKETS | A.FLAG_SMALL_GRID)
SEQUENCE = (1025, 1, 9, 1025, 3, 257, 5, A.BIG_COUNT, 2)  # granule counts of the back-to-back launches
REPEATS = []  # cases that latched SAFE mode and were run again (at most one in the whole file)

flags_param = pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "flags%#x" % f)


class Covered:
    """A FAST context under debug `flags`; run(name, body) is one case: body(ctx) compares what it computes and returns whether a
    device-side record of its own held SJMI_ST_INTERNAL (it then compares nothing); the counters are held to the rule above."""

    def __init__(self, flags, capacity, steps=0):
        self.flags, self.capacity, self.steps, self.ctx = flags, capacity, steps, None
        self.fresh()

    def fresh(self):
        import simdjson_java_amd as S
        self.close()
        self.ctx = S.Context(device=0, capacity=self.capacity)
        self.ctx.debug_set_flags(self.flags)
        self.ctx.set_tile_steps(self.steps)
        assert self.ctx.debug_counters() == [0, 0, 0, 0]

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def run(self, name, body):
        for attempt in (0, 1):
            before = self.ctx.debug_counters()
            internal = bool(body(self.ctx))
            n = self.ctx.debug_counters()
            if not internal and n[2] == 0 and n[3] == 0:
                assert n[0] > before[0], (name, "no stage-1 launch counted", before, n)
                assert n[1] == n[0], (name, "a launch without FLAG_ALL_TICKETS", n)
                return
            assert attempt == 0, "%s tripped the spin bound twice (counters %s)" % (name, n)
            REPEATS.append(name)
            assert len(REPEATS) <= 1, "more than one case latched SAFE mode: %s" % REPEATS
            self.fresh()


def _same(name, got_idx, got_st, want_idx, want_st):
    assert got_st == want_st, (name, got_st, want_st)
    assert got_idx.size == want_idx.size, (name, got_idx.size, want_idx.size)
    if not np.array_equal(got_idx, want_idx):
        bad = int(np.nonzero(got_idx != want_idx)[0][0])
        raise AssertionError("%s: first index mismatch at %d: got %d want %d" % (name, bad, got_idx[bad], want_idx[bad]))


_truth = {}


def truth(steps):
    """[(case, text, reference indexes, reference status)] of one granule size; one granule size is kept at a time"""
    if steps not in _truth:
        _truth.clear()
        _truth[steps] = [(c, d) + O.stage1(d, c.length) for c, d in ((c, A.text_of(c)) for c in A.cases(steps))]
    return _truth[steps]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_references():
    yield
    _truth.clear()


@pytest.fixture(scope="module")
def big(twitter):
    """the 64 MiB input of BIG_COUNT 4 KiB granules and its indexes by the closed form"""
    d, length, copies = A.big_case(twitter)
    idx0, st0 = O.stage1(twitter)
    assert st0 == 0
    return d, length, A.big_expected(idx0, len(twitter), copies)


# ---- the host form on every shape --------------------------------------------------------------------------------------------------
@flags_param
@pytest.mark.parametrize("steps", A.STEPS)
def test_host_form_on_every_shape(flags, steps, big):
    big_text, big_len, big_idx = big
    cov = Covered(flags, big_len + 64, steps)
    try:
        for c, d, want_idx, want_st in truth(steps):
            assert want_st == c.want_status
            cov.run(c.name, lambda ctx: _same(c.name, *ctx.stage1(d, c.length), want_idx, want_st))
        # 16384 granules of 4 KiB (8192 / 4096 of the larger ones): more than twice the waves any grid holds
        assert A.granules_for(big_len, steps) == A.BIG_COUNT // steps
        cov.run("big-s%d" % steps, lambda ctx: _same("big", *ctx.stage1(big_text, big_len), big_idx, 0))
        n = cov.ctx.debug_counters()
        print("\nhost form, flags %#x, steps %d: %d shapes, %.0f MiB, counters %s, repeated: %s" % (
            flags, steps, len(truth(steps)) + 1, (sum(c.length for c, *_x in truth(steps)) + big_len) / 2**20, n, REPEATS))
    finally:
        cov.close()


# ---- the device form, back to back -------------------------------------------------------------------------------------------------
@flags_param
def test_device_form_back_to_back(flags, big):
    """Nine launches on one context and one stream with nothing between them: every launch finds the workspace half the one before
    it cleaned on its way out -- most of whose waves, after a 1025-granule launch in front of a one-granule one, never held a
    granule -- and cleans the other half (zero_next_workspace, ws_dev_clean).  Own index array (capacity count + 1, canaries around
    it) and own record per launch; one synchronisation; nothing outside [0, count] written."""
    import torch
    big_text, big_len, big_idx = big
    by_n = {}
    for c, d, want_idx, want_st in truth(1):
        by_n.setdefault(c.n, []).append((c.name, d, c.length, want_idx, want_st))
    jobs = []
    for k, n in enumerate(SEQUENCE):
        jobs.append(("big", big_text, big_len, big_idx, 0) if n == A.BIG_COUNT else by_n[n][k % len(A.KINDS)])
    assert [A.granules_for(j[2], 1) for j in jobs] == list(SEQUENCE)
    bufs = [torch.from_numpy(np.ascontiguousarray(j[1])).cuda() for j in jobs]
    wants = [torch.from_numpy(j[3].astype(np.int64)).cuda() for j in jobs]

    def body(ctx):
        wholes = [torch.full((FRONT + j[3].size + 1 + BEHIND,), PATTERN, dtype=torch.int32, device="cuda") for j in jobs]
        recs = torch.zeros((len(jobs), 2), dtype=torch.int64, device="cuda")
        assert all(w.data_ptr() % 128 == 0 for w in wholes)
        torch.cuda.synchronize()
        for k, (name, _d, length, want_idx, _st) in enumerate(jobs):
            ctx.stage1_device(bufs[k].data_ptr(), length, wholes[k][FRONT:].data_ptr(), want_idx.size + 1, recs[k].data_ptr(), 0)
        torch.cuda.synchronize()
        r = recs.cpu().numpy()
        if any((int(x[1]) & 0xFFFFFFFF) & ST_INTERNAL for x in r):
            return True
        for k, (name, _d, length, want_idx, want_st) in enumerate(jobs):
            count = int(want_idx.size)
            where = (k, name)
            assert int(r[k][0]) == count and (int(r[k][1]) & 0xFFFFFFFF) == want_st, (where, r[k], count, want_st)
            w = wholes[k]
            assert bool((w[:FRONT] == PATTERN).all()), (where, "written in front of the base")
            assert torch.equal(w[FRONT:FRONT + count].to(torch.int64) & 0xFFFFFFFF, wants[k]), where
            assert int(w[FRONT + count].item()) == 0, (where, "sentinel")
            assert bool((w[FRONT + count + 1:] == PATTERN).all()), (where, "written behind [count]")
        return False

    cov = Covered(flags, 1 << 20, 1)
    try:
        cov.run("back-to-back", body)
        assert cov.ctx.debug_counters()[0] >= len(SEQUENCE)
    finally:
        cov.close()


# ---- the other stage-1 entry points under 0x800 -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    """the same calls without the flag"""
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=8 << 20)
    yield c
    assert c.debug_counters()[1:] == [0, 0, 0]
    c.close()


@pytest.fixture()
def forced():
    cov = Covered(A.FLAG_ALL_TICKETS, 8 << 20)
    yield cov
    cov.close()


def _batch_docs():
    from tests.test_gpu_batch import _small_docs
    from tests.conftest import load_fixture
    rng = random.Random(4100)
    docs = _small_docs(rng, 1500) + [load_fixture("github_events.json").rstrip(), b"[]", b"{}", b"7"]
    bad = [b'["abc', b'{"k": "v}', b'"', bytes([0x5B, 0x22, 0xC3, 0x22, 0x5D]), b'["a\nb"]', b'["abc', b"",
           b'["' + b"x" * 9000 + b'", "unclosed']
    return docs, bad, rng


def test_stage1_batch_in_both_modes(forced, plain):
    from tests.test_gpu_batch import _pack
    docs, bad, rng = _batch_docs()
    buf, offs = _pack(docs)

    def plain_mode(ctx):
        idx, io, st = ctx.stage1_batch(buf, offs)
        pidx, pio, pst = plain.stage1_batch(buf, offs)
        assert st == pst == 0 and np.array_equal(idx, pidx) and np.array_equal(io, pio)
        for k, d in enumerate(docs):
            want, wst = O.stage1(d)
            assert wst == 0 and np.array_equal(idx[int(io[k]):int(io[k + 1])].astype(np.int64) - int(offs[k]), want.astype(np.int64)), k

    forced.run("stage1_batch", plain_mode)
    mixed = list(docs)
    for b in bad:
        mixed.insert(rng.randrange(len(mixed)), b)
    for name, batch in (("isolated-clean", docs), ("isolated-mixed", mixed)):
        buf2, offs2 = _pack(batch)

        def isolated(ctx):
            idx, io, ds, st = ctx.stage1_batch_isolated(buf2, offs2)
            pidx, pio, pds, pst = plain.stage1_batch_isolated(buf2, offs2)
            assert st == pst and np.array_equal(idx, pidx) and np.array_equal(io, pio) and np.array_equal(ds, pds)
            want_or = 0
            for k, d in enumerate(batch):
                want, wst = O.stage1(d + b"\n")
                assert int(ds[k]) == wst, (name, k, d[:40])
                got = idx[int(io[k]):int(io[k + 1])].astype(np.int64) - int(offs2[k])
                assert np.array_equal(got, want.astype(np.int64)) if wst == 0 else got.size == 0, (name, k)
                want_or |= wst
            assert st == want_or and (want_or != 0) == (batch is mixed)

        forced.run(name, isolated)


def test_optimistic_batch_pipeline(forced, plain):
    """sjmi_parse_batch_device_optimistic (and the repair stage behind its SJMI_ST_REJECTED, which makes a stage-1 launch of its
    own) on 300 documents of tools/token_docs.py: as accepted batch, and with documents that fail stage 1 mixed in.  On a Context,
    through sharding.BatchShard: the contexts inside a SimdJsonParser take no debug flag."""
    from tests.test_gpu_batch import _pack
    from tests.test_gpu_pipeline import _run_shard
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from token_docs import document
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(20000)
    try:
        rng = random.Random(4200)
        docs = [document(rng) for _ in range(300)]
    finally:
        sys.setrecursionlimit(limit)
    assert all(O.stage1(d + b"\n")[1] == 0 for d in docs)
    mixed = list(docs)
    for b in (b'["abc', bytes([0x5B, 0x22, 0xC3, 0x22, 0x5D]), b'{"k": "v', b'["a\x01b"]', b'"'):
        mixed[rng.randrange(len(mixed))] = b
    for name, batch, rejected in (("accepted", docs, False), ("repaired", mixed, True)):
        buf, offs = _pack(batch)
        wants = [O.parse(d + b"\n") for d in batch]
        assert sum(1 for w in wants if w.error) >= 30 and sum(1 for w in wants if not w.error) >= 100

        def pipeline(ctx):
            c, tape, to, err, strings, io, idx = _run_shard(ctx, buf, offs, len(batch), want_rejected=rejected)
            pc, ptape, pto, perr, pstrings, pio, pidx = _run_shard(plain, buf, offs, len(batch), want_rejected=rejected)
            assert c == pc and np.array_equal(to, pto) and np.array_equal(err, perr) and strings == pstrings
            assert np.array_equal(io, pio) and np.array_equal(idx, pidx)
            for k, w in enumerate(wants):
                assert int(err[k]) == w.error, (name, k, batch[k][:40], int(err[k]), w.error)
                if not w.error:
                    got = tape[int(to[k]):int(to[k + 1])]
                    assert np.array_equal(got, ptape[int(pto[k]):int(pto[k + 1])]), (name, k)
                    assert_tape_equal(got, strings, w, (name, k))

        forced.run("pipeline-" + name, pipeline)


def test_parse_document_3_mib(forced, plain, twitter):
    doc = b"[" + b",".join([twitter.rstrip()] * 5) + b"]"
    assert 3 << 20 <= len(doc) <= 4 << 20
    want = O.parse(doc)
    assert want.error == 0

    def one(ctx):
        tape, strings, err, st = ctx.parse_document(doc)
        ptape, pstrings, perr, pst = plain.parse_document(doc)
        assert err == perr == 0 and st == pst == 0
        assert np.array_equal(tape, want.tape) and strings == want.strings
        assert np.array_equal(tape, ptape) and strings == pstrings

    forced.run("parse_document", one)


def test_stage1_masks(forced, plain):
    """sjmi_stage1_masks runs kernels of its own (csrc/masks.hip) and queues no k_stage1 launch, so the flag cannot reach it: the
    counters say so, the masks equal the oracle's and the unflagged context's, and their structurals are the indexes of the
    flagged stage-1 launch over the same bytes."""
    picked = [(c, d) for c, d, _i, _s in truth(1) if c.n in (5, 256) and c.kind != "bottom"]
    assert {(c.n, c.open) for c, _ in picked} == {(5, False), (256, True)}
    for c, d in picked:
        text = d[:c.length]
        _idx, _st, want = O.index_blocks(text, want_masks=True)

        def masks(ctx):
            before = ctx.debug_counters()
            got = ctx.stage1_masks(text)
            assert ctx.debug_counters() == before, "the masks call queued a stage-1 launch"
            assert got.shape == want.shape and np.array_equal(got, want), c.name
            assert np.array_equal(got, plain.stage1_masks(text)), c.name
            idx, st = ctx.stage1(text)
            bits = np.unpackbits(got[:, 5].copy().view(np.uint8), bitorder="little")
            assert st == c.want_status and np.array_equal(np.nonzero(bits)[0].astype(np.uint32), idx), c.name

        forced.run("masks-" + c.name, masks)


def test_one_stream_at_two_chunkings(forced, plain):
    """One document of tests/stream_fuzz.py as a stream of chunks, all of 64 bytes and at random sizes: every push is a shard
    launch whose halo / tail / entry-parity flags are OR-ed onto 0x800."""
    from tests.test_gpu_stream_fuzz import _stream_case
    docs = F.corpus()
    di = max((i for i, d in enumerate(docs) if d.name.startswith("valid")), key=lambda i: len(docs[i].data))
    d = docs[di]
    ix, st = O.stage1(d.data)
    want = (ix.astype(np.int64), st)
    chunkings = {}
    for style, last, cuts in F.chunkings(d, di):
        if style in ("b64", "random_a") and last == "rest":
            chunkings.setdefault(style, list(cuts))
    assert set(chunkings) == {"b64", "random_a"} and len(d.data) > 4096
    for style, cuts in chunkings.items():
        def stream(ctx):
            _stream_case(ctx, d, want, cuts, 128, lambda s: s.push)
            _stream_case(plain, d, want, cuts, 128, lambda s: s.push)

        forced.run("stream-" + style, stream)


# ---- two contexts really in flight, from one thread --------------------------------------------------------------------------------
def _twitter_x(twitter, reps):
    """-> (device buffer, length, expected indexes as an int32 tensor, count)"""
    import torch
    n0 = len(twitter)
    idx0, st0 = O.stage1(twitter)
    assert st0 == 0
    buf = torch.zeros(n0 * reps + 128, dtype=torch.uint8, device="cuda")
    buf[:n0 * reps] = torch.frombuffer(bytearray(twitter), dtype=torch.uint8).cuda().repeat(reps)
    want = torch.from_numpy(A.big_expected(idx0, n0, reps).astype(np.int64)).cuda().to(torch.int32)
    return buf, n0 * reps, want, int(want.numel())


class _Launch:
    """one stage1_device launch into an index array and a record of its own"""

    def __init__(self, ctx, buf, length, count, stream):
        import torch
        self.out = torch.full((count + 1 + BEHIND,), PATTERN, dtype=torch.int32, device="cuda")
        self.rec = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.count, self.args = count, (ctx, buf, length, stream)

    def go(self):
        ctx, buf, length, stream = self.args
        ctx.stage1_device(buf.data_ptr(), length, self.out.data_ptr(), self.count + 1, self.rec.data_ptr(), stream.cuda_stream)

    def internal(self):
        return bool((int(self.rec.cpu().numpy()[1]) & 0xFFFFFFFF) & ST_INTERNAL)

    def check(self, want, where):
        import torch
        r = self.rec.cpu().numpy()
        assert int(r[0]) == self.count and (int(r[1]) & 0xFFFFFFFF) == 0, (where, r)
        assert torch.equal(self.out[:self.count], want), where
        assert int(self.out[self.count].item()) == 0, (where, "sentinel")
        assert bool((self.out[self.count + 1:] == PATTERN).all()), (where, "written behind [count]")


def test_a_busy_context_flags_the_others_launch(twitter):
    """The host logic, made certain: context A's launch is queued on a side stream behind torch copies that take tens of
    milliseconds, so its busy_event is pending when context B launches -- B's launch must be flagged; not once A's stream has
    drained; and not once A is destroyed (a destroyed context is not polled)."""
    import torch
    import simdjson_java_amd as S
    buf, length, want, count = _twitter_x(twitter, 2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    src = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    a, b = S.Context(0, 1 << 20), S.Context(0, 1 << 20)
    try:
        la = _Launch(a, buf, length, count, sa)
        lb = [_Launch(b, buf, length, count, sb) for _ in range(3)]
        torch.cuda.synchronize()
        for ctx, stream in ((a, sa), (b, sb)):  # (a first launch allocates: one each, alone on the GPU, before anything is counted)
            _Launch(ctx, buf, length, count, stream).go()
            torch.cuda.synchronize()
        assert a.debug_counters() == [1, 0, 0, 0] and b.debug_counters() == [1, 0, 0, 0]
        with torch.cuda.stream(sa):
            for _ in range(60):
                dst.copy_(src, non_blocking=True)
        la.go()
        lb[0].go()
        if sa.query():
            pytest.fail("premise not met: context A's stream had drained when context B's launch returned")
        assert a.debug_counters()[:2] == [2, 0]
        assert b.debug_counters()[:2] == [2, 1], "B launched while A's launch was pending and was not flagged"
        sa.synchronize()
        sb.synchronize()
        lb[1].go()
        assert b.debug_counters()[:2] == [3, 1], "B was flagged although A's stream had drained"
        sb.synchronize()
        a.close()
        lb[2].go()
        assert b.debug_counters()[:2] == [4, 1], "B was flagged after A was destroyed"
        torch.cuda.synchronize()
        la.check(want, "A")
        for k, l in enumerate(lb):
            l.check(want, "B%d" % k)  # (a record with SJMI_ST_INTERNAL fails here)
        assert b.debug_counters()[2:] == [0, 0]
    finally:
        a.close()
        b.close()
        del src, dst
        torch.cuda.empty_cache()


def test_two_persistent_kernels_side_by_side(twitter):
    """Contexts A and B alternate 20 unsynchronised launches each of twitter.json x 64 on streams of their own: two persistent
    kernels compete for the CUs.  All 40 results against the closed form; from a context's second launch on, a launch is flagged
    whenever the other context's stream was still busy right behind the call (its last launch, queued earlier by this same thread,
    was then pending at the poll as well)."""
    import torch
    import simdjson_java_amd as S
    buf, length, want, count = _twitter_x(twitter, 64)
    rounds = 20
    for attempt in (0, 1):
        ctxs = [S.Context(0, 1 << 20), S.Context(0, 1 << 20)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        try:
            launches = [[_Launch(ctxs[w], buf, length, count, streams[w]) for _ in range(rounds)] for w in (0, 1)]
            torch.cuda.synchronize()
            seen = []
            for k in range(rounds):
                for w in (0, 1):
                    before = ctxs[w].debug_counters()
                    launches[w][k].go()
                    busy = not streams[1 - w].query()
                    after = ctxs[w].debug_counters()
                    assert after[0] == before[0] + 1
                    seen.append((w, k, busy, after[1] - before[1]))
            torch.cuda.synchronize()
            counters = [c.debug_counters() for c in ctxs]
            print("\nside by side: %d of 40 launches flagged, %d with the other stream still busy; counters %s" % (
                sum(f for *_x, f in seen), sum(b for _w, _k, b, _f in seen), counters))
            latched = any(l.internal() for w in (0, 1) for l in launches[w]) or any(c[2] or c[3] for c in counters)
            if not latched:
                for w, k, busy, flagged in seen:
                    assert flagged in (0, 1)
                    assert not (k >= 1 and busy and not flagged), ("launch %d of context %d was not flagged beside a busy stream" % (k, w), seen)
                for w in (0, 1):
                    for k, l in enumerate(launches[w]):
                        l.check(want, (w, k))
                return
            assert attempt == 0, "two persistent kernels side by side tripped the spin bound twice: %s" % counters
            REPEATS.append("side-by-side")
            assert len(REPEATS) <= 1, "more than one case latched SAFE mode: %s" % REPEATS
        finally:
            for c in ctxs:
                c.close()
            del launches
            torch.cuda.empty_cache()
