"""sjmi_parse_document (all three stages on the device) over the corpus of tests/single_doc_layouts.py: a document on both sides
of every switch of the single-document walk -- the two byte bounds of coop_walk_launch, 512 structurals, the chunk length's
switch at 262,144, the group sizes, a chunk that leaves its window of relative levels, chunk ends at 64 levels and more, 64
levels reached inside a chunk only -- with containers, keys, empty pairs and grammar errors across the chunk edges.  That
the members are what they claim is asserted on the CPU (tests/test_single_doc_layouts.py).

Every member is parsed into a pageable tape (staged) and into a page-locked one that the walkers write in place, with room
for the oracle's word count and canary words behind it in the same pinned array.  No tolerances: the stage-1 status and the
error code are the oracle's, an accepted document's tape and string buffer too, word for word; SJMI_WALK_NEEDS_HOST comes back
for no member (the reference's default limits admit all of them), and nothing at or behind tape_capacity changes -- for the
documents the chunk path declines as well: their chunk walkers may have written in place before the sweep did."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import single_doc_layouts as L
from tests.test_gpu_walk import CANARY, CANARY_WORDS
from tests.walk_common import NEEDS_HOST

pytestmark = pytest.mark.gpu

MAX_BYTES = 1 << 20
MAX_WORDS = 2 * 524290 + 2  # two words per structural + 2: what a walker can write at most for the largest member
IN_PLACE_MIN = 16           # sjmi_parse_document: a page-locked tape with room for fewer words is staged like a pageable one


class Rig:
    def __init__(self):
        import simdjson_java_amd as S
        import torch
        self.ctx = S.Context(device=0, capacity=MAX_BYTES)
        self.keep = torch.empty(MAX_WORDS + CANARY_WORDS, dtype=torch.int64).pin_memory()
        self.tapes = {"pageable": np.empty(MAX_WORDS + CANARY_WORDS, dtype=np.uint64), "pinned": self.keep.numpy().view(np.uint64)}
        self.sb = np.zeros(MAX_BYTES + 4 * (MAX_BYTES // 2 + 2) + 64, dtype=np.uint8)
        self.in_place_seen = 0

    def parse(self, doc, placement, cap):
        """-> (error, stage-1 status, tape view, string bytes); the tape array is canaries but for what the call wrote"""
        from simdjson_java_amd.binding import lib
        tape = self.tapes[placement]
        tape[:cap + CANARY_WORDS] = np.uint64(CANARY)
        src = np.frombuffer(doc, dtype=np.uint8)
        tl, sl, err, st = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_uint32(0)
        rc = lib().sjmi_parse_document(self.ctx._h, src.ctypes.data if src.size else None, len(doc), 1024, tape.ctypes.data, cap, C.addressof(tl),
                                       self.sb.ctypes.data, self.sb.size, C.addressof(sl), C.addressof(err), C.addressof(st))
        assert rc == 0, (rc, lib().sjmi_last_error(self.ctx._h))
        return err.value, st.value, tape[:tl.value], bytes(self.sb[:sl.value])

    def check(self, what, doc, want, placement):
        """one call against the oracle's parse -> a complaint or None"""
        cap = max(int(want.tape.size), IN_PLACE_MIN)
        err, st, tape, strings = self.parse(doc, placement, cap)
        whole = self.tapes[placement]
        if not (whole[cap:cap + CANARY_WORDS] == np.uint64(CANARY)).all():
            return "%s [%s]: a store at or behind tape_capacity = %d" % (what, placement, cap)
        if st != want.stage1_status:
            return "%s [%s]: stage-1 status %d, the oracle's %d" % (what, placement, st, want.stage1_status)
        if err == NEEDS_HOST:
            return "%s [%s]: handed back (SJMI_WALK_NEEDS_HOST), the oracle's error code %d" % (what, placement, want.error)
        if err != want.error:
            return "%s [%s]: error code %d, the oracle's %d" % (what, placement, err, want.error)
        if err == 0:
            if tape.size != want.tape.size or not np.array_equal(tape, want.tape):
                bad = np.nonzero(tape[:want.tape.size] != want.tape[:tape.size])[0]
                return "%s [%s]: %d tape words, the oracle's %d; first difference at word %s" % (what, placement, tape.size, want.tape.size,
                                                                                                 bad[0] if bad.size else "-")
            if strings != want.strings:
                return "%s [%s]: the string buffer differs" % (what, placement)
        elif placement == "pinned" and want.stage1_status == 0 and (whole[1:cap] != np.uint64(CANARY)).any():
            self.in_place_seen += 1  # (a failed document's words are never downloaded: the walkers wrote them where they are)
        return None

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def run_family(rig, members, want_in_place=True):
    rig.in_place_seen = 0
    problems = []
    for m in members:
        want = O.parse(m.doc)
        assert (want.error == 0) == (m.kind == "valid"), m.name
        for placement in ("pageable", "pinned"):
            p = rig.check(m.name, m.doc, want, placement)
            if p:
                problems.append(p)
    print("%d members, %d complaints" % (len(members), len(problems)))
    for p in problems:
        print("  " + p)
    assert not problems, "%d of %d members: %s" % (len({p.split(" [")[0] for p in problems}), len(members), "; ".join(problems[:12]))
    if want_in_place:
        assert rig.in_place_seen > 0, "no failed document's words were found in the page-locked tape: it was not written in place"


def test_counts(rig):
    """exactly s structurals around 512, the chunk edges, the group sizes' squares and the chunk length's switch; flat and built
    from the unit; closed, unclosed and with trailing content"""
    run_family(rig, L.family("counts"))


def test_phases(rig):
    """every position of the unit as the first structural of a chunk of 128 and of a chunk of 512"""
    run_family(rig, L.family("phases"), want_in_place=False)  # (no member fails)


def test_edge_pairs(rig):
    """structurals e - 1 and e as a valid or an erroneous pair across a chunk edge: what k_coop_walk<true> rebuilds from the two
    bytes in front of a chunk (prev_cls, prev_is_key, prev_empty_open) and root_closed from the scan"""
    run_family(rig, L.family("edge_pairs"))


def test_two_errors(rig):
    """two errors in two chunks, both orders: k_chunk_finish reports the first by position"""
    run_family(rig, L.family("two_errors"))


@pytest.mark.parametrize("length", L.BAND_LENGTHS)
def test_bands(rig, length):
    """Every way through the dispatch at the byte lengths on both sides of its two bounds -- and nothing of an earlier call
    decides a later one: every member is parsed right behind a document of the optimistic band that fails UTF-8 validation and
    right behind one the chunk path declines there (k_chunk_finish ends that call with nothing but the fall-back flag; the host
    reads the stage-1 record beside it before it queues the sweep)."""
    members = [m for m in L.family("bands") if len(m.doc) == length]
    assert len(members) >= 12
    run_family(rig, members)
    poisons = [(d, O.parse(d)) for d in L.poison_documents()]
    assert poisons[0][1].error == 1 and poisons[1][1].error == 0  # SJMI_E_UTF8; accepted by the sweep
    problems = []
    for m in members:
        want = O.parse(m.doc)
        for placement in ("pageable", "pinned"):
            for which, (d, dwant) in zip(("behind a UTF-8 failure", "behind a fall-back"), poisons):
                for p in (rig.check("the document parsed in front", d, dwant, placement), rig.check(m.name + " " + which, m.doc, want, placement)):
                    if p:
                        problems.append(p)
    for p in problems:
        print("  " + p)
    assert not problems, "%d complaints: %s" % (len(problems), "; ".join(problems[:12]))
