"""The claims of tests/batch_capacity_layouts.py, asserted on the CPU from the oracle and the offsets alone: what
tests/test_gpu_batch_capacity.py can notice about the capacity guards depends on them, so a change of the builder that loses one
fails here.  Prints the sizes and the numbers of cuts (pytest -s shows them)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import batch_capacity_layouts as CL
from tests.tok_stream_layouts import predicted_length, tokens

NAMES = list(CL.BATCHES)


def test_the_table_of_entries():
    """optimistic, exact and rejected on the accepted and the repaired batch and on the single document, the exact entry alone on
    the packed batch (the other two only say REJECTED there)"""
    three = ("optimistic", "exact", "rejected")
    assert CL.ENTRIES == {"accepted": three, "repaired": three, "packed": ("exact",), "single": three}
    assert set(CL.ENTRIES) == set(CL.BATCHES) == set(CL.LAID_OUT) == set(CL.TAPE_ROLES)
    for name in NAMES:
        assert CL.batch(name).entries == CL.ENTRIES[name] and CL.batch(name).laid_out == CL.LAID_OUT[name]


@pytest.mark.parametrize("name", NAMES)
def test_documents_cover_the_buffer_and_fail_where_they_should(name):
    b, e = CL.batch(name), CL.expect(name)
    offs = b.offs.astype(np.int64)
    assert offs[0] == 0 and int(offs[-1]) == len(b.buf) < (1 << 17) and (np.diff(offs) >= 0).all()
    for k, d in enumerate(b.docs):
        assert b.buf[int(offs[k]):int(offs[k + 1])] == d
    n = len(b.docs)
    s1 = [k for k in range(n) if e.stage[k] == 1]
    s2 = [k for k in range(n) if e.stage[k] == 2]
    r = b.roles
    if name == "accepted":
        assert 250 <= n <= 400 and all(d.endswith(b"\n") for d in b.docs) and O.stage1(b.buf)[1] == 0
        assert s1 == [] and s2 == sorted([r["fail_space"], r["fail_comma"], r["fail_atom"], r["blank"]])
    elif name == "repaired":
        a = CL.batch("accepted")
        assert all(d.endswith((b"\n", b"\t")) for d in b.docs)
        assert s1 == [0, r["s1_middle"], n - 1] == [r["s1_front"], r["s1_middle"], r["s1_end"]] and 100 < r["s1_middle"] < n - 100
        assert [d for k, d in enumerate(b.docs) if k not in s1] == a.docs  # (the accepted batch with three documents put in)
        assert [O.stage1(b.docs[k])[1] for k in s1] == [6, 1, 6]  # SJMI_ST_UNCLOSED (| UNESCAPED: its separator), SJMI_ST_UTF8
        assert b"\xc3" in b.docs[r["s1_middle"]] and b.docs[0].startswith(b'["abc') and b.docs[n - 1].rstrip(b"\n").endswith(b"\\" * 3)
        assert s2 == sorted(r[x] for x in ("fail_space", "fail_comma", "fail_atom", "blank"))
    elif name == "packed":
        # the rule of sjmi_parse_batch_device_rejected: without separators the repair stage takes a batch only if the last byte of
        # every document is whitespace, an operator or a quote; a document that passes stage 1 and ends in a backslash breaks it
        assert n > CL.PACK_DOCS + 64 and not any(d[-1:] in b"\n\r\t " for d in b.docs if d)
        t = r["trailing_backslash"]
        assert b.docs[t] == b"[1]\\" and e.stage[t] == 2 and O.stage1(b.docs[t])[1] == 0 and b.docs[t + 1] == b'"x"'
        assert s1 == [r["s1_unclosed"]] and set(s2) >= {r["fail_space"], r["fail_comma"]}
        assert r["chunk0_last"] == CL.PACK_DOCS - 1 and r["chunk1_first"] == CL.PACK_DOCS
        for role in ("chunk0_last", "chunk1_first"):  # (cuts on both sides of them and inside them)
            assert e.stage[r[role]] == 0 and e.slots[r[role]] >= 3
        assert all(e.slots[k] == 0 for k in s1 + s2)
    else:
        assert n == 1 and s1 == s2 == [] and e.counts[0] > 64
    for role in ("fail_space", "fail_comma", "fail_atom"):
        if role in r:
            assert b.docs[r[role]].rstrip(b"\n") in CL.STAGE2_FAILURES and e.stage[r[role]] == 2
    print("\n%s: %d documents, %d bytes, need_idx %d, need_tape %d, string bytes of the well-formed documents %d; %d + %d + %d cuts"
          % (name, n, len(b.buf), e.need_idx, e.need_tape, e.sb_wellformed, len(CL.index_cuts(name)), len(CL.tape_cuts(name)),
             len(CL.string_cuts(name, e.sb_wellformed, np.zeros(n + 1, np.int64)))))


@pytest.mark.parametrize("name", ["accepted", "repaired", "packed"])
def test_the_listed_literals_and_the_mix_are_in_the_batch(name):
    from tests.walk_common import AMBIGUOUS, exact_range
    b, e = CL.batch(name), CL.expect(name)
    for role, lit in (("listed", AMBIGUOUS[0]), ("listed2", AMBIGUOUS[2])):
        k = b.roles[role]
        assert lit.encode() in b.docs[k] and not exact_range(lit) and e.stage[k] == 0
    well = [d for k, d in enumerate(b.docs) if e.stage[k] == 0]
    assert any(b"\\u00e9" in d for d in well) and any(b'\\"' in d for d in well) and any(b'"v"' in d for d in well)  # escapes / none
    assert any(b"9223372036854775807" in d for d in well) and any(b".25" in d for d in well)                     # longs, doubles
    assert any(d.startswith(b"[[[[") for d in well)                                                              # nesting
    if name != "packed":
        k = b.roles["two_structurals"]
        assert b.docs[k] == b"[]\n" and e.counts[k] == 2
    k = b.roles["long"]
    d = b.docs[k]
    assert 1990 <= len(d) <= 2100 and len(d) == max(len(x) for x in b.docs)
    assert tokens(d) > 128 and 160 < e.slots[k] == predicted_length(d) < CL.CANARY_WORDS  # (several 64-token steps; a slot that is thinned)
    assert max(e.slots) < CL.CANARY_WORDS


@pytest.mark.parametrize("name", NAMES)
def test_needs_and_offsets_are_the_oracles(name):
    """per document: the index count, the slot (the tape's length, the predicted length, two words or none) and the string bytes"""
    b, e = CL.batch(name), CL.expect(name)
    n_idx = n_tape = n_sb = 0
    for k, d in enumerate(b.docs):
        idx, st = O.stage1(d)
        want = O.parse(d)
        assert int(e.io[k]) == n_idx and int(e.to[k]) == n_tape
        n_idx += 0 if st else idx.size
        if want.error == 0:
            n_tape += want.tape.size
            n_sb += len(want.strings)
            assert want.tape.size == predicted_length(d)  # (with enough room a document's room is its predicted length exactly)
        elif b.laid_out:
            n_tape += 2 if st else predicted_length(d)
    assert e.need_idx == n_idx + 1 and e.need_tape == n_tape and e.sb_wellformed == n_sb
    assert e.all_wellformed == (name == "single")  # (elsewhere need_sb is the roomy run's, not below sb_wellformed)


@pytest.mark.parametrize("name", NAMES)
def test_every_named_cut_point_exists(name):
    b, e = CL.batch(name), CL.expect(name)
    r = b.roles
    n = len(b.docs)
    # ---- index ----
    cuts = dict(CL.index_cuts(name))
    assert cuts[e.need_idx] == "need" and cuts[e.need_idx - 1] == "need - 1" and 1 in cuts and 2 in cuts and min(cuts) == 1
    assert {c % CL.LINE_INDEXES for c in cuts if e.need_idx - 33 <= c <= e.need_idx - 2} == set(range(CL.LINE_INDEXES))
    if n > 1:
        first, middle, last = r["first"], r.get("middle", n // 2), r["last"]
        assert first == (1 if name == "repaired" else 0) and last == n - (2 if name == "repaired" else 1) and n // 3 < middle < 2 * n // 3
        for k in (middle, last):
            assert {int(e.io[k]) - 1, int(e.io[k]), int(e.io[k]) + 1} <= set(cuts) and e.counts[k] >= 3
        assert {int(e.io[first]), int(e.io[first]) + 1} <= set(cuts | {0: ""})
    # ---- strings ----
    dso = np.arange(n + 1, dtype=np.int64) * 1000 + 5000  # (stand-ins for the roomy run's offsets: every cut is there and apart)
    cuts = dict(CL.string_cuts(name, 10 ** 6, dso))
    assert {10 ** 6, 10 ** 6 - 1, 0} <= set(cuts)
    if "strings" in r:
        k = r["strings"]
        assert e.stage[k] == 0 and b.docs[k].rstrip(b"\n") == CL.STRINGS_DOC
        (p0, pc, pl), (q0, qc, ql) = CL.string_record_offsets(name)
        assert (p0, pc, pl, q0, qc) == (0, 4, 8, 9, 13) and ql == 13 + len(CL.STRINGS_RECORDS[1]) - 1
        assert {int(dso[k]) + x for x in (p0, p0 + 2, pc, pl, q0, q0 + 2, qc, ql)} <= set(cuts)
    if n > 1:
        for k in (middle, last):
            assert {int(dso[k]) - 1, int(dso[k]), int(dso[k]) + 1} <= set(cuts) and len(e.wants[k][1].strings) > 0
    # ---- tape ----
    cuts = dict(CL.tape_cuts(name))
    assert {e.need_tape, e.need_tape - 1, 0, 1} <= set(cuts)
    roles = CL.TAPE_ROLES[name]
    for role in roles:
        k = r[role]
        assert {int(e.to[k]) + j for j in CL.slot_words(e.slots[k])} <= set(cuts)
    if name in ("accepted", "repaired", "packed"):
        first, last, long_, listed, failing, two = (r[x] for x in roles[:6])
        assert e.stage[first] == e.stage[last] == e.stage[long_] == e.stage[listed] == 0 and e.stage[failing] == 2
        assert b.docs[long_].lstrip()[:1] == b"[" and tokens(b.docs[long_]) > 64  # (a container root: the token walker's)
        if b.laid_out:
            assert e.slots[failing] == predicted_length(b.docs[failing]) > 2 and e.slots[two] == 2
            assert e.stage[two] == (1 if name == "repaired" else 2)
        else:
            assert e.slots[failing] == e.slots[two] == 0
        assert 0 < int(e.to[long_]) and int(e.to[long_ + 1]) < e.need_tape  # (documents in front of the long one and behind it)
    if name == "packed":
        for role in ("chunk0_last", "chunk1_first"):
            k = r[role]
            for at in (int(e.to[k]), int(e.to[k + 1])):
                assert {at - 1, at, at + 1} <= set(cuts)
        assert int(e.to[CL.PACK_DOCS]) < e.need_tape  # (two compaction workgroups, a cut in each)
    if name == "single":
        count = e.counts[0]
        assert {2 * count + 1, 2 * count + 2, e.slots[0], e.slots[0] - 1, 16} <= set(cuts) and e.slots[0] < 2 * count + 1
    assert len(CL.slot_words(161)) < 161 and CL.slot_words(160) == list(range(160))
