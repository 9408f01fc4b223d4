"""The conditions of the layouts of tests/batch_layouts.py, asserted on the CPU from the oracle and the offsets alone: what
tests/test_gpu_batch_layouts.py can notice about k_doc_prepare depends on them, so a change of the builder that loses one fails
here.  Where a family cannot meet a condition for an offset (17 structurals do not fit in front of offset 5) the condition reads
"every offset that admits it", and the admitted set is written out.  Prints the statistics (pytest -s shows them;
profiles/r13/README.md records them)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import batch_layouts as BL


def _rendered(name):
    return [(L,) + L.render() for L in BL.family(name)]


def _entered(buf):
    return BL.oracle_block_words(buf)[2]


@pytest.mark.parametrize("name", list(BL.FAMILIES))
def test_every_batch_is_one_the_plain_pass_accepts(name):
    """every document passes oracle.stage1 on its own and so does the batch; every document but a batch's last ends in one of the
    three separators, each of which occurs in the family (a batch of a few documents cannot hold all three); sizes"""
    seps = set()
    n_docs = n_bytes = 0
    for L, buf, offs, docs, hz in _rendered(name):
        assert 2 <= len(docs) <= 4000 and len(buf) < (1 << 20), (L.name, len(docs), len(buf))
        assert O.stage1(buf)[1] == 0, L.name
        assert offs[0] == 0 and int(offs[-1]) == len(buf) and (np.diff(offs.astype(np.int64)) >= 0).all()
        for k, d in enumerate(docs):
            assert O.stage1(d)[1] == 0, (L.name, k, d[:40])
            assert buf[int(offs[k]):int(offs[k + 1])] == d
            if k + 1 < len(docs):
                sep = b"\r\n" if d.endswith(b"\r\n") else d[-1:]
                assert sep in BL.SEPS, (L.name, k, d[-8:])
                seps.add(sep)
            if L.wellformed:
                assert O.parse(d).error == 0, (L.name, k, d[:60])
        assert hz and all(0 <= h <= len(docs) for h in hz), L.name
        n_docs += len(docs)
        n_bytes += len(buf)
    assert seps == set(BL.SEPS), (name, seps)
    print("\n%s: %d batches, %d documents, %d bytes" % (name, len(BL.family(name)), n_docs, n_bytes))


def test_offsets_every_boundary_offset_with_every_count_in_front():
    (L, buf, offs, docs, hz), = _rendered("offsets")
    o, c = BL.boundary_profile(buf, offs)
    admitted = {"0": (lambda c: c == 0, range(0, 64)), "1": (lambda c: c == 1, range(2, 64)), "15": (lambda c: c == 15, range(16, 64)),
                "16": (lambda c: c == 16, range(17, 64)), "17": (lambda c: c == 17, range(18, 64)),
                ">=33": (lambda c: c >= 33, range(34, 64))}  # (c structurals and a separator need c + 1 bytes in front of the boundary)
    for name, (pred, want) in admitted.items():
        have = {int(x) for x, y in zip(o, c) if pred(y)}
        assert have >= set(want), (name, sorted(set(want) - have))
        print("offsets: %s structurals in front: %d boundaries, offsets %d..%d" % (name, sum(1 for y in c if pred(y)), min(want), max(want)))
    assert int(c.max()) == 62  # the scalar loop at its longest: offset 63, every byte in front but the separator a structural
    # the structurals in front are of every kind: numbers (two words), strings (the ordinal), ',' (no word)
    in_front = set()
    idx = O.stage1(buf)[0].astype(np.int64)
    for k in range(len(offs)):
        if c[k] >= 15:
            lo = int(offs[k]) - int(o[k])
            in_front |= {buf[int(i)] for i in idx[(idx >= lo) & (idx < int(offs[k]))]}
    assert in_front >= set(b'[],"-1t'), in_front


def test_crowded_blocks_of_many_boundaries_and_lone_separators_around_a_dense_document():
    (L, buf, offs, docs, hz), = _rendered("crowded")
    o, c = BL.boundary_profile(buf, offs)
    per_block = np.bincount(offs.astype(np.int64) >> 6)
    assert per_block.max() >= 8, per_block.max()
    idx = O.stage1(buf)[0].astype(np.int64)
    n_struct = np.diff(np.searchsorted(idx, offs.astype(np.int64)))
    around = [k for k in range(1, len(docs) - 1) if n_struct[k - 1] == 0 and n_struct[k + 1] == 0 and n_struct[k] >= 17 and
              int(offs[k - 1]) >> 6 == int(offs[k + 2]) >> 6]
    assert len(around) >= 10, around
    assert {int(o[k]) - 1 for k in around} >= set(range(0, 31, 2))  # (the lone separator in front of the dense one stands there)
    print("crowded: most boundaries in one block %d, lone-separator / dense / lone-separator in one block %d times" % (per_block.max(), len(around)))


def test_parity_boundary_blocks_entered_inside_a_string_and_whole_blocks_inside_strings():
    (L, buf, offs, docs, hz), = _rendered("parity")
    outside, inside, entered = BL.oracle_block_words(buf)
    o, c = BL.boundary_profile(buf, offs)
    # a boundary block entered inside a string that closes in front of the boundary: root strings admit offsets 2..63 (quote,
    # separator), the arrays with two more strings behind the one that spans the block's start 11..63
    hit, hit_more = set(), set()
    for h in hz:
        b = int(offs[h]) >> 6
        if entered[b] and o[h]:
            hit.add(int(o[h]))
            if buf[b * 64:int(offs[h])].count(b'"') >= 5:
                hit_more.add(int(o[h]))
    assert hit >= set(range(2, 64)), sorted(set(range(2, 64)) - hit)
    assert hit_more >= set(range(11, 64)), sorted(set(range(11, 64)) - hit_more)
    # whole blocks inside a string whose bytes look like structurals: the two bytes of blkw differ on every one of them
    whole = [b for b in range(len(entered) - 1) if entered[b] and entered[b + 1] and b'"' not in buf[b * 64:b * 64 + 64]]
    assert len(whole) >= 40, len(whole)
    assert all(outside[b] != inside[b] and inside[b] == 0 and outside[b] >= 20 for b in whole), [(b, outside[b], inside[b]) for b in whole][:5]
    print("parity: boundary blocks entered inside a string at offsets %d..%d, %d whole blocks inside strings (outside count %d..%d, inside 0)" % (
        min(hit), max(hit), len(whole), min(outside[b] for b in whole), max(outside[b] for b in whole)))


def test_backslash_runs_end_at_the_blocks_edge_in_front_of_a_boundary_block():
    (L, buf, offs, docs, hz), = _rendered("backslash_runs")
    boundary_blocks = {int(x) >> 6 for x in offs if int(x) & 63}
    _, _, masks = O.index_blocks(buf, want_masks=True)  # per block: escaped, quote (unescaped), inString, ...
    found = {}
    pos = 0
    while True:  # every maximal backslash run: (length, where its last byte lies relative to a block's last byte)
        a = buf.find(b"\\", pos)
        if a < 0:
            break
        e = a
        while e < len(buf) and buf[e] == 0x5C:
            e += 1
        n, shift = e - a, ((e - 1) - 63) % 64
        shift = shift - 64 if shift > 32 else shift
        if n in BL.RUNS and shift in (-1, 0, 1) and buf[e] == 0x22:
            quote_block = e >> 6
            # where the quote stands, and the boundary block: the quote's own, or (the quote a block's last byte) the one behind it
            assert e % 64 == (shift + 64) % 64, (n, shift, e)
            assert (quote_block + 1 if shift == -1 else quote_block) in boundary_blocks, (n, shift, e)
            # the quote by the oracle's masks: escaped behind an odd run, an unescaped quote that closes the string behind an even one
            escaped = int(masks[quote_block, 0] >> np.uint64(e & 63)) & 1
            quote = int(masks[quote_block, 1] >> np.uint64(e & 63)) & 1
            in_string = int(masks[quote_block, 2] >> np.uint64(e & 63)) & 1  # (inString holds an opening quote, not a closing one)
            assert (escaped, quote, in_string) == ((1, 0, 1) if n & 1 else (0, 1, 0)), (n, shift, e, escaped, quote, in_string)
            found.setdefault((n, shift), 0)
            found[(n, shift)] += 1
        pos = e
    assert set(found) == {(n, s) for n in BL.RUNS for s in (-1, 0, 1)}, sorted(found)
    # (an odd run escapes the quote, an even one leaves it closing the string: both at every shift, the 5,000s included)
    assert {n & 1 for n in BL.RUNS if n >= 5000} == {0, 1} and {n & 1 for n in BL.RUNS if n < 64} == {0, 1}
    print("backslash_runs: %d (length, shift) pairs, each %d times; lengths %s" % (len(found), min(found.values()), list(BL.RUNS)))


def test_quote_behind_a_primitive_with_well_formed_neighbours_in_its_block():
    (L, buf, offs, docs, hz), = _rendered("quote_behind_primitive")
    seen = {}
    for k in range(len(docs) - 1):
        body = docs[k].rstrip(b"\r\n\t")
        if body in BL.ODD:
            assert O.stage1(docs[k])[1] == 0 and O.parse(docs[k]).error != 0, body
            nxt = docs[k + 1]
            if int(offs[k]) >> 6 == int(offs[k + 2]) >> 6 and O.parse(nxt).error == 0 and b'"' in nxt:
                seen.setdefault(body, set()).add(int(offs[k + 1]) & 63)
    assert set(seen) == set(BL.ODD), set(BL.ODD) - set(seen)
    assert all(len(v) >= 8 for v in seen.values()), {k: len(v) for k, v in seen.items()}
    print("quote_behind_primitive: %s" % {k.decode(): len(v) for k, v in seen.items()})


def test_word_classes_at_the_blocks_edges():
    (L, buf, offs, docs, hz), = _rendered("word_classes")
    idx = set(int(x) for x in O.stage1(buf)[0])
    outside, inside, entered = BL.oracle_block_words(buf)
    last, runs_on = set(), set()
    for s in range(0, len(buf) - 64, 64):
        c = buf[s + 63]
        if s + 63 in idx and c in b"-0123456789tfn":
            last.add(c)
            if buf[s + 64] in b"0123456789.e" and s + 64 not in idx:
                runs_on.add(c)
    assert last == set(b"-0123456789tfn"), bytes(sorted(set(b"-0123456789tfn") - last))
    assert runs_on >= set(b"-0123456789") - set(b"5"), bytes(sorted(runs_on))  # (the 5 stands alone: a one-byte number at the edge)
    blocks = [buf[s:s + 64] for s in range(0, len(buf) - 63, 64)]
    assert any(set(b) <= set(b"[]") for b in blocks), "no block of 64 brackets"
    neg = [i for i, b in enumerate(blocks) if set(b) == set(b"[-1")]
    pos = [i for i, b in enumerate(blocks) if set(b) == set(b"[1")]
    assert neg and pos
    assert min(outside[i] for i in neg) >= 63 and max(outside[i] for i in pos) == 96  # ('[1' x 32: the most words a block makes)
    print("word_classes: starters at a block's last byte %r, running on %r, most words in a block %d" % (
        bytes(sorted(last)), bytes(sorted(runs_on)), outside.max()))


def test_long_documents_of_every_trip_count_at_every_start_block():
    (L, buf, offs, docs, hz), = _rendered("long")
    entered = _entered(buf)
    o64 = offs.astype(np.int64)
    have, seam = set(), set()
    for k in range(len(docs)):
        bs, be = int(o64[k]) >> 6, int(o64[k + 1]) >> 6
        have.add((be - bs, bs % 64))
        # a trip of eight blocks that takes its parity bits from two blkpar words, with blocks entered inside a string on both sides
        # of the seam.  (A document that begins in block 63 enters it outside a string: there the first trip has them behind the
        # seam only, and block 63 entered inside a string is the second trip of a document that begins in block 55.)
        for b0 in range(bs, be, 8):
            if b0 % 64 > 56:
                trip = range(b0, min(b0 + 8, be))
                front = any(entered[b] for b in trip if b % 64 > 56)
                if any(entered[b] for b in trip if b % 64 < 8) and (front or b0 % 64 == 63):
                    seam.add((bs % 64, b0 % 64, front))
    want = {(c, m) for c in BL.BLOCK_COUNTS for m in BL.START_BLOCKS}
    assert have >= want, sorted(want - have)
    assert seam >= {(57, 57, True), (60, 60, True), (63, 63, False), (55, 63, True)}, seam
    print("long: %d (whole blocks, start block) pairs; trips over the seam of two parity words with strings on both sides, as (start block, trip's first block, "
          "strings in front of the seam too): %s; blocks entered inside a string %d of %d" % (len(want), sorted(seam), int(entered.sum()), entered.size))


def test_counts_around_the_workgroup_of_256_documents():
    rendered = _rendered("counts")
    assert [len(docs) for _, _, _, docs, _ in rendered] == list(BL.DOC_COUNTS)
    assert BL.PREP_DOCS == 256
    for L, buf, offs, docs, hz in rendered:
        o, c = BL.boundary_profile(buf, offs)
        for k in (255, 256, 257, 511, 512, 513):
            if k <= len(docs) and len(docs) >= 255:
                assert c[k] >= 17, (L.name, k, int(c[k]))
    print("counts: documents %s, a boundary with >= 17 structurals in front at 255, 256, 257 (511, 512, 513) wherever the batch has it" % (list(BL.DOC_COUNTS),))


def test_tiny_batches_and_the_batchs_end():
    totals = {}
    for L, buf, offs, docs, hz in _rendered("tiny"):
        assert 2 <= len(docs) <= 4
        totals.setdefault(O.stage1(buf)[0].size, []).append(len(docs))
    assert set(totals) == {1, 2, 3, 4, 5} and all(len(set(v)) >= 2 for v in totals.values()), totals
    ends = set()
    for L, buf, offs, docs, hz in _rendered("end"):
        o, c = BL.boundary_profile(buf, offs)
        # the last document's 21 structurals stand in the 64 bytes in front of the batch's end; those of them in the tail block:
        idx = O.stage1(buf)[0].astype(np.int64)
        assert int(((idx >= len(buf) - 64) & (idx < len(buf))).sum()) >= 21, L.name
        tail, sep = len(buf) & 63, docs[-1][-1:] in BL.SEPS
        assert int(c[-1]) == (0 if tail == 0 or (tail == 1 and sep) else 1 if tail == 1 else int(c[-1])) and (tail != 63 or c[-1] >= 21), (L.name, int(c[-1]))
        ends.add((len(buf) & 63, docs[-1][-1:] in BL.SEPS))
    assert ends == {(t, s) for t in (0, 1, 63) for s in (True, False)}, ends
    print("tiny: structurals in all -> documents %s; end: (total_len & 63, last document separated) %s" % (totals, sorted(ends)))


def test_the_repair_inserts_stand_where_they_are_said_to():
    """the three failing documents fail stage 1, are 64 bytes long with their separator (every offset behind them stays), and land a
    block ahead of a hazard / inside a hazard's block / directly behind a hazard, in every family"""
    for name, d, sep in BL.failing_documents():
        assert len(d + sep) == 64 and O.stage1(d + sep)[1] != 0, name
    assert BL.failing_documents()[2][1].endswith(b"\\" * 3) and not BL.failing_documents()[2][1].endswith(b"\\" * 4)
    for fam in BL.FAMILIES:
        places = set()
        for i, L in enumerate(BL.family(fam)):
            ins = BL.repair_inserts(L, rotate=i)
            _, offs0, docs0, hz0 = L.render()
            buf, offs, docs, hz = L.render(inserts=[t[:3] for t in ins])
            assert len(docs) == len(docs0) + len(ins) and len(buf) == len(offs0) * 0 + int(offs0[-1]) + 64 * len(ins)
            assert [int(offs[h]) & 63 for h in hz] == [int(offs0[h]) & 63 for h in hz0]
            for at, d, sep, place, h in ins:
                k = next(j for j in range(len(docs)) if docs[j] == d + sep)
                assert k == 0 or docs[k - 1][-1:] in (b"\n", b"\t"), (L.name, k)  # (the document in front of it is separated from it)
                h1 = hz[L.hazards.index(h)]
                start, hazard = int(offs[k]), int(offs[h1])
                if place == "behind":
                    assert start == hazard
                elif place == "inside":
                    assert start < hazard and (start + 63) >> 6 == hazard >> 6 and start >> 6 < hazard >> 6  # its last bytes share the block
                else:
                    assert start + 64 <= (hazard & ~63)
                places.add(place)
        assert places == {"ahead", "inside", "behind"} or fam == "tiny", (fam, places)  # (a batch of under 64 bytes has no block ahead)
        assert places >= {"inside", "behind"}, (fam, places)


def test_a_surviving_trailing_backslash_stands_in_front_of_a_dense_boundary_block():
    """the batch the repair stage must decline: no separators, `[1]\\` (passes stage 1, fails stage 2) directly in front of `"x"` and a
    dense document in one block; counted on the documents' own structurals (the batch as a whole is no document stream)"""
    L = BL.backslash_in_front_of_dense()
    buf, offs, docs, hz = L.render()
    assert not any(L.seps) and len(buf) == int(offs[-1])
    s1 = [O.stage1(d) for d in docs]
    assert sum(1 for _, st in s1 if st) == 1
    o, c = BL.boundary_profile_per_document(offs, [None if st else ix for ix, st in s1])
    units = [k for k, d in enumerate(docs) if d == b"[1]\\"]
    assert len(units) == 4
    ends = set()
    for k in units:
        assert s1[k][1] == 0 and O.parse(docs[k]).error != 0
        assert docs[k + 1] == b'"x"' and s1[k + 2][0].size == 19 and O.parse(docs[k + 2]).error == 0
        # the boundary behind the dense document: in one block with the neighbour's quote, >= 17 structurals of the block in front
        assert int(offs[k + 1]) >> 6 == int(offs[k + 3]) >> 6 and c[k + 3] >= 17, (k, int(c[k + 3]))
        assert c[k + 4] >= 17  # ... and the one behind its follower
        ends.add(int(offs[k + 1]) & 63)
    assert ends == {0, 4, 13}  # the backslash a block's last byte (twice), and inside the block
    # whole-buffer view: the backslash does escape the neighbour's quote
    _, _, masks = O.index_blocks(buf, want_masks=True)
    for k in units:
        e = int(offs[k + 1])
        assert buf[e] == 0x22 and int(masks[e >> 6, 0] >> np.uint64(e & 63)) & 1
    print("\nbackslash_in_front_of_dense: %d documents, %d bytes, structurals in front of the dense boundaries %s" % (
        len(docs), len(buf), [int(c[k + 3]) for k in units]))
