"""The chunk stream (sjmi_stream_*) and the document split (sjmi_split_*) on the corpus of tests/stream_fuzz.py, at every chunking:
the protocol state that lives in C (csrc/sjmi_api.hip: what is kept of the stream, the halo escalation, from_start, the carried
parity and status; the rescan rule of a split) over k_stage1's shard form.  Expected values come from oracle.stage1 on the WHOLE
document and from stream_fuzz's CPU restatement of `have` and of a filled halo, nothing else.  tests/test_stream_fuzz_corpus.py
holds the corpus to the conditions that make these comparisons mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import stream_fuzz as F
from tests.golden import vectors as V

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sjmi.h")) as _f:
    _H = _f.read()
ST_HALO = int(re.search(r"#define SJMI_ST_HALO (0x[0-9a-fA-F]+)u", _H).group(1), 16)
ERR_ARG = int(re.search(r"#define SJMI_ERR_ARG \((-\d+)\)", _H).group(1))
ERR_CAPACITY = int(re.search(r"#define SJMI_ERR_CAPACITY \((-\d+)\)", _H).group(1))
CANARY = 0x5A5A5A5A
COUNTS = {"pushes": 0, "streams": 0, "scans": 0, "splits": 0}  # what this file did (printed when the context is closed)


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=1 << 20)
    yield c
    c.close()
    # (pytest -s: the volume behind the figures of profiles/r11/README.md)
    print("\nstream_fuzz on the device: %(streams)d streams, %(pushes)d pushes; %(splits)d shards opened, %(scans)d shard scans" % COUNTS)


@pytest.fixture(scope="module")
def truth():
    """oracle.stage1 of every document, once: [(indexes int64, status)]"""
    return [(ix.astype(np.int64), st) for ix, st in (O.stage1(d.data) for d in F.corpus())]


def _rc(excinfo):
    return int(re.search(r"rc=(-?\d+)", str(excinfo.value)).group(1))


def _stream_case(ctx, d, want, cuts, halo, push_of):
    """one document through one stream; push_of(stream) -> push(chunk, is_last) -> (base, indexes, status)"""
    import simdjson_java_amd as S
    want_idx, want_st = want
    model = F.model_stream(d.data, cuts, halo)
    s = ctx.stream(F.max_chunk(cuts), halo)
    COUNTS["streams"] += 1
    where = (d.name, halo, cuts if len(cuts) < 12 else cuts[:6] + ["..."] + cuts[-3:])
    try:
        push = push_of(s)
        got, prev, st = [], 0, 0
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            last = k == len(cuts) - 2
            COUNTS["pushes"] += 1
            if model[k]["error"]:
                # everything that is kept is one backslash run and the stream began in front of it: an error code, on this push
                with pytest.raises(S.SjmiError) as e:
                    push(d.data[a:b], last)
                assert _rc(e) == ERR_CAPACITY, (where, k)
                assert np.array_equal(np.concatenate(got), want_idx[want_idx < a]), (where, k)
                return
            base, idx, st = push(d.data[a:b], last)
            assert base == a, (where, k)
            assert idx.size == 0 or int(idx.max()) < b - a, (where, k, int(idx.max()), b - a)
            assert st & ~want_st == 0 and prev & ~st == 0, (where, k, st, prev, want_st)
            assert last or not st & O.ST_UNCLOSED, (where, k, st)
            prev = st
            got.append(idx.astype(np.int64) + base)
        assert st == want_st, (where, st, want_st)
        got = np.concatenate(got)
        if not np.array_equal(got, want_idx):
            n = min(got.size, want_idx.size)
            bad = int(np.nonzero(got[:n] != want_idx[:n])[0][0]) if not np.array_equal(got[:n], want_idx[:n]) else n
            raise AssertionError("%r: %d indexes for %d, first difference at %d: %s / %s" % (
                where, got.size, want_idx.size, bad, got[bad:bad + 4].tolist(), want_idx[bad:bad + 4].tolist()))
    finally:
        s.close()


@pytest.mark.parametrize("halo", F.STREAM_HALOS)
@pytest.mark.parametrize("part", range(F.N_SLICES))
def test_stream_through_the_c_abi(ctx, truth, part, halo):
    """every (document, chunking) of one slice of the corpus: bases, index bounds, the concatenated indexes, the final verdict and
    how it accumulates, and SJMI_ERR_CAPACITY exactly on the push where a backslash run covers all that is kept"""
    docs, mine = F.corpus(), set(F.slices()[0][part])
    n = 0
    for di, _style, _last, cuts in F.pairs():
        if di in mine:
            _stream_case(ctx, docs[di], truth[di], list(cuts), halo, lambda s: s.push)
            n += len(cuts) - 1
    assert 0 < n <= 3300


@pytest.mark.parametrize("part", range(2))
def test_stream_document_is_the_same_protocol(ctx, truth, part):
    """sharding.stream_document, the Python twin, on a quarter of the corpus with the default halo: the same indexes and verdict"""
    import torch
    from simdjson_java_amd import sharding
    dev = torch.device("cuda", 0)
    docs = F.corpus()
    for di, _style, _last, cuts in F.pairs():
        if di % 4 != 0 or (di // 4) % 2 != part:
            continue
        d, (want_idx, want_st) = docs[di], truth[di]
        chunks = [d.data[a:b] for a, b in zip(cuts, cuts[1:])]
        COUNTS["pushes"] += len(chunks)
        if any(p["error"] for p in F.model_stream(d.data, cuts, 64)):
            with pytest.raises(sharding.HaloTooShort):
                sharding.stream_document(ctx, dev, chunks, halo=64)
            continue
        parts, st = sharding.stream_document(ctx, dev, chunks, halo=64)
        assert [base for base, _ in parts] == list(cuts[:-1]), (d.name, cuts)
        got = np.concatenate([ix.astype(np.int64) + base for base, ix in parts])
        assert st == want_st and np.array_equal(got, want_idx), (d.name, cuts, st, want_st)


def _split_case(ctx, torch, d, want, t, bounds, H):
    """the protocol of a split, all ranks on one device: scan; resolve with the wrong parity, then with the right one; assemble"""
    want_idx, want_st = want
    n_sh = len(bounds)
    halos = [min(H, a) for a, _b in bounds]
    caps = [b - a + 68 for a, b in bounds]
    offs = np.concatenate([[0], np.cumsum([c + 64 for c in caps])]).astype(np.int64)
    ix = torch.full((int(offs[-1]),), CANARY, dtype=torch.int32, device=t.device)
    sp = [ctx.split(t.data_ptr() + a, b - a, h, h == a, r == n_sh - 1, ix.data_ptr() + 4 * int(offs[r]), caps[r])
          for r, ((a, b), h) in enumerate(zip(bounds, halos))]
    COUNTS["splits"] += n_sh
    where = (d.name, H, bounds if n_sh < 8 else bounds[:4] + ["..."] + bounds[-2:])
    try:
        # the kernel cannot see where a backslash run begins that fills the whole halo -- unless the halo begins the document
        reports = [h != a and F.halo_filled(d.data, a, h) for (a, _b), h in zip(bounds, halos)]
        flips = []
        for r, x in enumerate(sp):
            f, st = x.scan()
            COUNTS["scans"] += 1
            flips.append(f)
            assert bool(st & ST_HALO) == reports[r], (where, r, st)
        counts, status, after = [], 0, 0
        for r, x in enumerate(sp):
            entry = sum(flips[:r]) & 1
            _c, st_wrong, _a = x.resolve(1 - entry)
            count, st, after = x.resolve(entry)  # (the second answer is the one that counts: under parity 1 the indexes are rewritten)
            COUNTS["scans"] += 2 - entry
            assert bool(st & ST_HALO) == reports[r] and bool(st_wrong & ST_HALO) == reports[r], (where, r, st, st_wrong)
            assert count <= bounds[r][1] - bounds[r][0] + 1, (where, r, count)
            counts.append(count)
            status |= st
        host = ix.cpu().numpy()
        for r in range(n_sh):
            tail = host[int(offs[r]) + caps[r]:int(offs[r + 1])]
            assert tail.size == 64 and (tail == CANARY).all(), (where, r)
        if any(reports):
            return
        if after:
            status |= O.ST_UNCLOSED
        got = np.concatenate([host[int(offs[r]):int(offs[r]) + counts[r]].view(np.uint32).astype(np.int64) + bounds[r][0] for r in range(n_sh)])
        assert status == want_st, (where, status, want_st)
        assert np.array_equal(got, want_idx), (where, got.size, want_idx.size)
    finally:
        for x in sp:
            x.close()


@pytest.mark.parametrize("part", range(F.N_SLICES))
def test_split_through_the_c_abi(ctx, truth, part):
    """shards of one block to half a document, 2 to 64 ranks, halos of 64, 256 and 4096 bytes (all of the document where it is
    shorter): SJMI_ST_HALO exactly where the halo is one backslash run, else the oracle's indexes and verdict; 64 canary words behind
    every index array.  The shards lie in ONE device buffer, so what follows a shard that is not the last is the document, not zeros."""
    import torch
    dev = torch.device("cuda", 0)
    docs = F.corpus()
    for di in F.slices()[0][part]:
        d = docs[di]
        t = torch.zeros(len(d) + 128, dtype=torch.uint8, device=dev)
        t[:len(d)] = torch.frombuffer(bytearray(d.data), dtype=torch.uint8).to(dev)
        seen = set()
        for bounds in F.split_configs(d, di):
            for H in F.SPLIT_HALOS:
                key = (tuple(bounds), tuple(min(H, a) for a, _b in bounds))
                if key not in seen:  # (a short document has the same halos under 256 and 4096)
                    seen.add(key)
                    _split_case(ctx, torch, d, truth[di], t, bounds, H)


def _shard(ctx, dev, data, halo, entry, from_start):
    import torch
    from simdjson_java_amd import sharding
    sh = sharding.DocumentShard(ctx, data, halo, True, dev, halo_from_start=from_start)
    sh.run(entry)
    torch.cuda.synchronize()
    count, st, after = sh.outcome()
    return sh.idx[:count].cpu().numpy().view(np.uint32).astype(np.int64), st, after


def test_shard_edges_neither_wrapper_reaches(ctx):
    """sjmi_stage1_shard_device2 itself: a LAST shard of no bytes is a tail block and a halo -- a UTF-8 sequence the document ends in
    the middle of is validated there or nowhere; and a shard entered inside a string that is nothing but the closing quote"""
    import torch
    dev = torch.device("cuda", 0)
    ends = [(name, seq, True) for name, seq, _ in V.UTF8_INVALID_END] + [(c, c.encode(), False) for c in ("é", "€", "😀", "a")]
    for name, seq, broken in ends:
        for inside in (False, True):
            for size in (64, 192):
                head = (b'["' + b"a" * (size - 2 - len(seq)) if inside else b"[1," + b" " * (size - 3 - len(seq))) + seq
                assert len(head) == size
                want_idx, want_st = O.stage1(head)
                assert bool(want_st & O.ST_UTF8) == broken and bool(want_st & O.ST_UNCLOSED) == inside
                for halo in sorted({64, size}):
                    for from_start in {False, halo == size}:
                        idx, st, after = _shard(ctx, dev, head[size - halo:], halo, int(inside), from_start)
                        assert idx.size == 0 and after == int(inside), (name, inside, size, halo, idx, after)
                        assert st == (want_st & ~O.ST_UNCLOSED), (name, inside, size, halo, from_start, st, want_st)
    for tail in (b'"', b'"]', b'",1]' + b" " * 70):
        doc = b'["' + b"a" * 62 + tail
        want_idx, want_st = O.stage1(doc)
        assert want_st == 0
        for from_start in (False, True):
            idx, st, after = _shard(ctx, dev, doc, 64, 1, from_start)
            assert st == 0 and after == 0 and np.array_equal(idx, want_idx[want_idx >= 64].astype(np.int64) - 64), (tail, idx)
        # entered outside a string the quote opens one: what the oracle says of the document without its first quote
        other = b"[ " + doc[2:]
        want_idx, want_st = O.stage1(other)
        idx, st, after = _shard(ctx, dev, other, 64, 0, True)
        assert want_st == O.ST_UNCLOSED and st == 0 and after == 1, (tail, st, after)
        assert np.array_equal(idx, want_idx[want_idx >= 64].astype(np.int64) - 64), (tail, idx)


def test_argument_rules(ctx):
    """host checks of sjmi_stream_* / sjmi_split_*: SJMI_ERR_ARG, and the stream goes on as if the call had not been made"""
    import simdjson_java_amd as S
    import torch
    doc = b'["' + b"a" * 190 + b'", 1, 2, "' + b"b" * 120 + b'"]'
    want_idx, want_st = O.stage1(doc)
    with pytest.raises(S.SjmiError) as e:
        ctx.stream(1024, 100)  # halo_bytes is a multiple of 64
    assert _rc(e) == ERR_ARG
    s = ctx.stream(128)
    try:
        for bad, last in ((doc[:100], False), (b"", False), (doc[:192], False), (doc[:192], True)):
            with pytest.raises(S.SjmiError) as e:  # not a multiple of 64; empty and not the last; longer than max_chunk_bytes
                s.push(bad, last)
            assert _rc(e) == ERR_ARG, (len(bad), last)
        got = []
        for a in range(0, len(doc), 128):
            for bad in (doc[:65], b""):
                with pytest.raises(S.SjmiError) as e:
                    s.push(bad, False)
                assert _rc(e) == ERR_ARG
            base, idx, st = s.push(doc[a:a + 128], a + 128 >= len(doc))
            assert base == a
            got.append(idx.astype(np.int64) + base)
        assert st == want_st == 0 and np.array_equal(np.concatenate(got), want_idx.astype(np.int64))
        for chunk, last in ((doc[:64], False), (doc[:64], True), (b"", True)):
            with pytest.raises(S.SjmiError) as e:  # behind the last chunk the stream is finished
                s.push(chunk, last)
            assert _rc(e) == ERR_ARG
    finally:
        s.close()
    dev = torch.device("cuda", 0)
    t = torch.zeros(256 + 128, dtype=torch.uint8, device=dev)
    t[:len(doc[:256])] = torch.frombuffer(bytearray(doc[:256]), dtype=torch.uint8).to(dev)
    ix = torch.empty(256 + 68, dtype=torch.int32, device=dev)
    x = ctx.split(t.data_ptr(), 256, 0, True, False, ix.data_ptr(), ix.numel())
    try:
        with pytest.raises(S.SjmiError) as e:
            x.resolve(0)  # nothing has been scanned
        assert _rc(e) == ERR_ARG
        flips, st = x.scan()
        count, st, after = x.resolve(0)
        w = O.stage1(doc[:256])
        assert flips == after == 1 and st == 0 and np.array_equal(ix[:count].cpu().numpy().view(np.uint32), w[0])
    finally:
        x.close()
    for length, halo, last in ((100, 0, False), (0, 0, False), (128, 32, False), (128, 100, True)):
        x = ctx.split(t.data_ptr() + 128, length, halo, False, last, ix.data_ptr(), ix.numel())
        try:
            with pytest.raises(S.SjmiError) as e:  # the shard's own rules (sjmi_stage1_shard_device2) surface at the scan
                x.scan()
            assert _rc(e) == ERR_ARG, (length, halo, last)
        finally:
            x.close()


def test_an_index_array_that_is_too_small_leaves_the_stream_as_it_was(ctx):
    """include/sjmi.h, sjmi_stream_push: SJMI_ERR_CAPACITY for index_capacity < count + 1 took nothing of the chunk -- the stream's
    offset, kept bytes, parity and verdict are those of before, and the same chunk pushed again goes through.  The chunk is one whose
    halo has to be escalated and that is entered inside a string, so what was kept and carried is needed to get it right."""
    from simdjson_java_amd.binding import lib
    doc = b'["' + b"a" * (256 - 2 - 64) + b"\\" * 64 + (b'\\"x", 1, 2, 3, "\x01", [4, 5],').ljust(128) + b'[6, 7], 8, "open, ' + b"c" * 50
    want_idx, want_st = O.stage1(doc)
    assert want_st == (O.ST_UNESCAPED | O.ST_UNCLOSED)
    cuts = [0, 256, 384, len(doc)]
    assert F.model_stream(doc, cuts, 0)[1]["depth"] == 1
    in_chunk = [int(((want_idx >= a) & (want_idx < b)).sum()) for a, b in zip(cuts, cuts[1:])]
    assert min(in_chunk) >= 2
    s = ctx.stream(256)
    try:
        got = []
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            chunk = np.frombuffer(doc[a:b], dtype=np.uint8)
            for cap in (in_chunk[k], 1, 0):  # count + 1 entries are needed
                small = np.full(in_chunk[k] + 8, CANARY, dtype=np.uint32)
                count, base, st = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
                rc = lib().sjmi_stream_push(s._h, chunk.ctypes.data, chunk.size, int(b == len(doc)), small.ctypes.data, cap,
                                            C.byref(count), C.byref(base), C.byref(st))
                assert rc == ERR_CAPACITY, (k, cap, rc)
                assert (small[cap:] == CANARY).all(), (k, cap)
            base, idx, st = s.push(doc[a:b], b == len(doc))
            assert base == a and idx.size == in_chunk[k], (k, base, idx.size)
            got.append(idx.astype(np.int64) + base)
        assert st == want_st and np.array_equal(np.concatenate(got), want_idx.astype(np.int64))
    finally:
        s.close()
