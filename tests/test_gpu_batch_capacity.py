"""sjmi_parse_batch_device, _optimistic and _rejected (what BatchShard.step runs) at the exact edges of their three capacities: the
batches and cuts of tests/batch_capacity_layouts.py (held to their claims on the CPU by tests/test_batch_capacity_layouts.py), one
array short at a time, through every entry that applies to the batch (batch_capacity_layouts.ENTRIES).

The allocation rule.  Every output array (indexes, string buffer, tape) is allocated ONCE per batch and entry for BatchShard's
default capacities plus 512 canary words, with 128 canary bytes in front and a 128-byte aligned base, and keeps that allocation for
every capacity that is passed: only the capacity argument shrinks.  BatchShard allocates nothing from index_capacity but its own
three arrays (sharding.py: the workspaces are the context's, sized inside the call from the capacities it is given), so the shard is
built with the default ratios, its arrays are replaced by the canaried ones, and shard.index_capacity / sb_capacity / tape_capacity
are assigned before each step -- the way test_gpu_pipeline.py shrinks them; no ratio is passed.  The arrays are filled with the
canary before every call, so a store at or behind a capacity, or in front of a base, shows as a changed word in memory the test owns.

The roomy run (default capacities) is checked against the oracle once per batch and entry by _verify of test_gpu_batch_layouts.py;
every later comparison "with the roomy run" rests on that.  need_idx and need_tape are the oracle's; need_sb is the oracle's where
every document is well-formed (the single document) and else the roomy run's strings.total_bytes, not below the oracle's sum over
the well-formed documents.

What a call must show is written at _at_need and _short.  After every shortfall the roomy call is made again on the same context and
shard and must give the first roomy run's outputs bit for bit -- all of every array, canaries included.

Not here: the record table (strings flags & 2).  It has index_capacity - 1 + 64 entries and every string's opening quote is a
structural, so with an index array that suffices (index_capacity - 1 >= structurals >= strings) it is never short; with one that
does not, stage 1 reports first and no string pass runs."""
import numpy as np
import pytest

from tests import batch_capacity_layouts as CL
from tests.walk_common import assert_tape_equal

pytestmark = pytest.mark.gpu

FRONT = 128  # canary bytes in front of every array (a multiple of the 128-byte alignment the plain pass wants; at least 64)
ST_CAPACITY, ST_REJECTED = 0x100, 0x800
ENTRY_KW = {"optimistic": {}, "exact": {"exact": True}, "rejected": {"rejected": True}}
MESSAGE = {"index": "stage 1 of the shard: capacity", "strings": "string buffer capacity exceeded", "tape": "tape capacity exceeded"}


class Harness:
    """one batch, one entry: the shard with its canaried arrays, the roomy run's outputs"""

    def __init__(self, ctx, name, entry):
        import torch
        from simdjson_java_amd import sharding
        from tests.test_gpu_walk import CANARY
        self.ctx, self.name, self.entry = ctx, name, entry
        self.b, self.e = CL.batch(name), CL.expect(name)
        self.n = len(self.b.docs)
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.current_stream().cuda_stream
        s = self.shard = sharding.BatchShard(ctx, self.b.buf, self.b.offs, self.dev)
        self.roomy = (s.index_capacity, s.sb_capacity, s.tape_capacity)
        self.raw, self.pristine = {}, {}
        for what, cap, dtype, item in (("idx", s.index_capacity, torch.int32, 4), ("sb", s.sb_capacity, torch.uint8, 1),
                                       ("tape", s.tape_capacity, torch.int64, 8)):
            nbytes = (FRONT + (cap + CL.CANARY_WORDS) * item + 7) // 8 * 8
            raw = torch.full((nbytes // 8,), CANARY, dtype=torch.int64, device=self.dev).view(torch.uint8)
            assert raw.data_ptr() % 128 == 0
            self.raw[what], self.pristine[what] = raw, raw.clone()
            setattr(s, what, raw[FRONT:FRONT + (cap + CL.CANARY_WORDS) * item].view(dtype))
        self.small = ("index_offsets", "doc_status", "doc_string_offsets", "tape_offsets", "doc_errors")
        self.counters = ctx.debug_counters()
        self.seen = set()  # (what the runs found where the contract leaves a choice; printed, pytest -s shows it)
        # ---- the roomy run, against the oracle ----
        from tests.test_gpu_batch_layouts import _verify
        first, rec, raised, c = self.call(*self.roomy)
        assert raised is None, (self.tag(), raised)
        self.check_canaries(*self.roomy)
        _verify(self.tag() + ", roomy", self.b.buf, self.b.offs, self.b.docs, self.e.wants, s, c, check_dso=self.e.all_wellformed,
                laid_out=self.b.laid_out)
        assert c["structurals"] == self.e.need_idx - 1 and c["tape_words"] == self.e.need_tape, (self.tag(), c)
        self.need_sb = c["string_bytes"]
        assert self.need_sb >= self.e.sb_wellformed and (self.need_sb == self.e.sb_wellformed or not self.e.all_wellformed)
        self.snap = {w: self.raw[w].clone() for w in self.raw}
        self.snap.update({w: getattr(s, w).clone() for w in self.small})
        self.snap_rec, self.snap_first = rec, first
        self.dso = s.doc_string_offsets.cpu().numpy()[:self.n + 1].astype(np.int64)
        mask = np.zeros(self.e.need_tape, dtype=bool)  # the words of the well-formed documents
        for k in range(self.n):
            if self.e.stage[k] == 0:
                mask[int(self.e.to[k]):int(self.e.to[k + 1])] = True
        self.well_mask = torch.from_numpy(mask).to(self.dev)
        self.well_tape = torch.where(self.well_mask, s.tape[:self.e.need_tape], 0)

    def tag(self):
        return "%s batch, %s entry" % (self.name, self.entry)

    def call(self, ci, cs, ct):
        """canaries everywhere, the per-document outputs set to -1, one step of the entry, check() -> (the entry's own record, the
        record check() judged -- behind its retries through the rejected and the exact call for the optimistic entry, all under the
        same canaries --, check()'s message or None, check()'s counts or None)"""
        import torch
        from simdjson_java_amd.binding import SjmiError
        s = self.shard
        for w in self.raw:
            self.raw[w].copy_(self.pristine[w])
        for w in self.small:
            getattr(s, w).fill_(-1)
        s.result.fill_(-1)
        s.index_capacity, s.sb_capacity, s.tape_capacity = int(ci), int(cs), int(ct)
        s.rejected_steps, s.format_rejected, s.unrepairable = 0, False, False  # (what check() latches: every call is the entry's own)
        torch.cuda.synchronize()  # (stream handle 0 names the engine's own stream, which torch's fills above are not ordered with)
        try:
            s.step(self.stream, **ENTRY_KW[self.entry])  # (returns only if the C call returned 0)
            torch.cuda.synchronize()
        except SjmiError as err:  # (the C call did not return 0)
            raise AssertionError("%s, capacities %d / %d / %d: %s" % (self.tag(), ci, cs, ct, err))
        except Exception as err:  # (a device fault: nothing more is started on this device)
            pytest.exit("%s, capacities %d / %d / %d: %r" % (self.tag(), ci, cs, ct, err), returncode=3)
        first = s.result.cpu().numpy().copy()
        raised = c = None
        try:
            c = s.check()
        except RuntimeError as err:
            raised = str(err)
        torch.cuda.synchronize()
        return first, s.result.cpu().numpy().copy(), raised, c

    def check_canaries(self, ci, cs, ct, what=""):
        """nothing in front of a base, nothing at or behind a capacity"""
        import torch
        for w, cap, item in (("idx", ci, 4), ("sb", cs, 1), ("tape", ct, 8)):
            raw, clean = self.raw[w], self.pristine[w]
            assert torch.equal(raw[:FRONT], clean[:FRONT]), "%s %s: a store in front of %s" % (self.tag(), what, w)
            at = FRONT + int(cap) * item
            if not torch.equal(raw[at:], clean[at:]):
                bad = torch.nonzero(raw[at:] != clean[at:]).flatten()
                raise AssertionError("%s %s: a store at or behind the capacity of %s: %d bytes changed, the first %d bytes behind it, the "
                                     "last %d" % (self.tag(), what, w, bad.numel(), int(bad[0]), int(bad[-1])))

    def same(self, w, upto=None, what=""):
        """array w (or its first `upto` entries) equals the roomy run's"""
        import torch
        if w in self.raw:
            item = {"idx": 4, "sb": 1, "tape": 8}[w]
            end = self.raw[w].numel() if upto is None else FRONT + int(upto) * item
            ok = torch.equal(self.raw[w][:end], self.snap[w][:end])
        else:
            ok = torch.equal(getattr(self.shard, w), self.snap[w])
        assert ok, "%s %s: %s differs from the roomy run's" % (self.tag(), what, w)

    def documents_in_front(self, ct, what):
        """Every well-formed document whose slot ends at or below the tape capacity ct has its tape there.  The roomy run's tapes
        were compared with the oracle's (_verify: assert_tape_equal) and the string buffer is the roomy run's, so equal words are
        the oracle's tape: all words of all these documents are compared on the device; the two nearest to the cut and the first
        one are compared with the oracle here once more, as they stand."""
        import torch
        e, s = self.e, self.shard
        k_end = int(np.searchsorted(e.to, ct, side="right")) - 1  # documents 0 .. k_end - 1 end at or below the capacity
        end = int(e.to[k_end])
        got = torch.where(self.well_mask[:end], s.tape[:end], 0)
        assert torch.equal(got, self.well_tape[:end]), "%s %s: a well-formed document in front of the cut differs" % (self.tag(), what)
        near = [k for k in range(k_end) if e.stage[k] == 0]
        if near:
            strings = bytes(s.sb[:self.need_sb].cpu().numpy())
            for k in sorted(set(near[-2:] + near[:1])):
                assert_tape_equal(s.tape[int(e.to[k]):int(e.to[k + 1])].cpu().numpy().view(np.uint64), strings, e.wants[k][1],
                                  "%s %s: document %d in front of the cut" % (self.tag(), what, k))

    def roomy_again(self, what):
        """the context afterwards: the roomy call on the same context and shard gives the first roomy run's outputs bit for bit, no
        SAFE-mode latch"""
        first, rec, raised, c = self.call(*self.roomy)
        what += ", the roomy call behind it"
        assert raised is None, (self.tag(), what, raised)
        assert np.array_equal(first, self.snap_first) and np.array_equal(rec, self.snap_rec), (self.tag(), what, first, rec, self.snap_rec)
        for w in tuple(self.raw) + self.small:
            self.same(w, what=what)
        now = self.ctx.debug_counters()
        assert now[2] == self.counters[2] == 0 and now[3] == 0, (self.tag(), what, now)


_harness = {}


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    _harness.clear()
    c.close()


def harness(ctx, name, entry):
    """(the roomy run and its oracle check once per batch and entry; nothing changes its snapshot afterwards)"""
    if (name, entry) not in _harness:
        _harness[name, entry] = Harness(ctx, name, entry)
    return _harness[name, entry]


def _at_need(h, ci, cs, ct, what):
    """Capacity equal to the need (or above it): no capacity bit in any record -- check() accepts --, every array equals the roomy
    run's word for word up to the need, the sentinel stands at indexes[count], the canaries are intact"""
    first, rec, raised, c = h.call(ci, cs, ct)
    assert raised is None, (h.tag(), what, raised)
    assert np.array_equal(rec, h.snap_rec), (h.tag(), what, rec, h.snap_rec)
    h.check_canaries(ci, cs, ct, what)
    h.same("idx", h.e.need_idx, what)
    h.same("sb", h.need_sb, what)
    h.same("tape", h.e.need_tape, what)
    for w in h.small:
        h.same(w, what=what)
    assert int(h.shard.idx[h.e.need_idx - 1]) == 0, (h.tag(), what, "the sentinel")


def _short(h, short, ci, cs, ct, what):
    """Any shortfall: the call returns 0, nothing at or behind a capacity or in front of a base has changed in any of the three
    arrays, check() raises the message that names the short array.
    index: stage1.status has SJMI_ST_CAPACITY in the entry's own record (the optimistic entry may add SJMI_ST_REJECTED) and in the one
      check() judged; stage1.count is the complete count need_idx - 1 on the exact entry, and on the others unless the record says
      REJECTED; no document has doc_errors[k] == 0.
    strings: strings.flags & 1; the stage-1 record and the index array up to the sentinel equal the roomy run's.
    tape: walk.flags & 1; walk.tape_words and tape_offsets, the stage-1 and the strings record, the index array, the string buffer
      and doc_string_offsets equal the roomy run's; where the tapes were laid out before the walk every well-formed document whose
      slot ends at or below the capacity has its tape there, against the oracle (packed behind the walk: unspecified,
      k_tape_compact drops whole chunks)."""
    first, rec, raised, c = h.call(ci, cs, ct)
    h.check_canaries(ci, cs, ct, what)
    assert raised is not None and MESSAGE[short] in raised, (h.tag(), what, raised, rec)
    s, e = h.shard, h.e
    if short == "index":
        # (a record that says REJECTED holds nothing valid, the capacity bit included: the optimistic entry declines a batch of ONE
        #  document before any stage runs, and the plain pass over a batch with a document that fails stage 1 counts the structurals
        #  of the batch read as one stream, which may fit.  The exact entry never says REJECTED; check() goes on until no record does)
        assert int(first[1]) & ST_CAPACITY or (h.entry != "exact" and int(first[1]) & ST_REJECTED), (h.tag(), what, first)
        assert int(rec[1]) & ST_CAPACITY, (h.tag(), what, [hex(int(x)) for x in rec])
        assert not int(first[1]) & ST_REJECTED or h.entry != "exact", (h.tag(), what, hex(int(first[1])))
        h.seen.add("index short: the entry's own record says %s" % ("REJECTED" if int(first[1]) & ST_REJECTED else "CAPACITY, the complete count"))
        assert not int(rec[1]) & ST_REJECTED, (h.tag(), what, hex(int(rec[1])))
        for r in (first, rec):
            if not int(r[1]) & ST_REJECTED:
                assert int(r[0]) == e.need_idx - 1, (h.tag(), what, int(r[0]), e.need_idx - 1)
        assert not bool((s.doc_errors[:h.n] == 0).any()), (h.tag(), what, "a document without an error")
    elif short == "strings":
        assert int(rec[4]) & 1, (h.tag(), what, rec)
        assert np.array_equal(rec[:2], h.snap_rec[:2]), (h.tag(), what, rec, h.snap_rec)
        h.same("idx", e.need_idx, what)
    else:
        assert int(rec[8]) & 1, (h.tag(), what, rec)
        assert np.array_equal(rec[:6], h.snap_rec[:6]), (h.tag(), what, rec, h.snap_rec)
        h.same("idx", e.need_idx, what)
        h.same("sb", h.need_sb, what)
        for w in ("tape_offsets", "doc_string_offsets", "index_offsets", "doc_status"):
            h.same(w, what=what)
        if h.b.laid_out:
            h.documents_in_front(ct, what)
    h.roomy_again(what)


def _sweep(h, short, cuts):
    need = {"index": h.e.need_idx, "strings": h.need_sb, "tape": h.e.need_tape}[short]
    assert any(c == need for c, _ in cuts) and any(c == need - 1 for c, _ in cuts)
    failures = []
    for cut, label in cuts:
        caps = list(h.roomy)
        caps[("index", "strings", "tape").index(short)] = cut
        what = "%s capacity %d (%s; the need is %d)" % (short, cut, label, need)
        try:
            if cut >= need:
                _at_need(h, *caps, what)
            else:
                _short(h, short, *caps, what)
        except AssertionError as err:  # (every cut runs: each call starts from canaries and the roomy capacities of the others)
            failures.append("%s: %s" % (what, str(err)[:600]))
    for line in sorted(h.seen):
        print("%s, %s" % (h.tag(), line))
    h.seen.clear()
    assert not failures, "%s: %d of %d cuts fail\n%s" % (h.tag(), len(failures), len(cuts), "\n".join(failures[:12]))


CASES = [(name, entry) for name in CL.BATCHES for entry in CL.ENTRIES[name]]


@pytest.mark.parametrize("name,entry", CASES)
def test_index_capacity_at_its_edges(ctx, name, entry):
    h = harness(ctx, name, entry)
    _sweep(h, "index", CL.index_cuts(name))


@pytest.mark.parametrize("name,entry", CASES)
def test_string_capacity_at_its_edges(ctx, name, entry):
    h = harness(ctx, name, entry)
    _sweep(h, "strings", CL.string_cuts(name, h.need_sb, h.dso))


@pytest.mark.parametrize("name,entry", CASES)
def test_tape_capacity_at_its_edges(ctx, name, entry):
    h = harness(ctx, name, entry)
    _sweep(h, "tape", CL.tape_cuts(name))
