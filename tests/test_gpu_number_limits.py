"""Device number conversion at its limits (csrc/coop_walk.hip: cw_primitive's integer paths, the scanner of sj_number.h, the
boundary literals that k_slow_doubles / cw_single_finish decide with sj_bigdec.h), every value against the oracle AND against
tests/walk_common.exact_number (Fraction, ties to even):
  * the list of boundary literals at its capacity (CW_SLOW_CAP = 65,536 per launch): exactly full, one over, a single document
    over it (handed back; the parser's host walk takes it), and a tape too small for the literals it would list;
  * where the walkers read: documents that abut without separators, the batch's end at every phase of a 16-byte window, and
    padding bytes that are digits;
  * single documents on the chunk-parallel path with boundary literals, long integers and subnormal / overflowing literals in
    every chunk and on both sides of every chunk boundary."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_walk import CANARY, CANARY_WORDS, gpu_walk
from tests.walk_common import NEEDS_HOST, assert_tape_equal, boundary_literal, exact_number, tape_numbers

pytestmark = pytest.mark.gpu

SLOW_CAP = 1 << 16  # CW_SLOW_CAP: boundary literals one launch decides on the device
_exact = {}


def _want_numbers(lits):
    out = []
    for lit in lits:
        if lit not in _exact:
            _exact[lit] = exact_number(lit)
        out.append(_exact[lit])
    return out


def check_doc(what, doc, lits, err, tape, strings, allow_host=False):
    """One document's verdict and tape against the oracle (doc judged alone), its number words against the exact reference."""
    want = O.parse(doc)
    if err == NEEDS_HOST:
        assert allow_host, (what, doc[:60])
        return "host"
    assert err == want.error, (what, doc[:60], err, want.error)
    if err == 0:
        assert_tape_equal(tape, strings, want, (what, doc[:60]))
        assert tape_numbers(tape) == _want_numbers(lits), (what, doc[:60])
    return "ok"


def _pack_tight(docs):
    """the documents back to back: no separator, doc_offsets[k + 1] = the end of document k"""
    buf = b"".join(docs)
    return buf, np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)


def _pack_nl(docs):
    buf = b"".join(d + b"\n" for d in docs)
    return buf, np.cumsum([0] + [len(d) + 1 for d in docs]).astype(np.uint64)


def run_three_calls(ctx, docs, packed, pad=0):
    """-> (per document: (error, tape or None), strings, host documents); gpu_walk checks host_documents against the errors"""
    tapes, strings, errors = gpu_walk(ctx, docs, packed=packed, pad=pad)
    return [(int(errors[k]), tapes[k]) for k in range(len(docs))], strings, int((errors == NEEDS_HOST).sum())


def run_shard(ctx, docs, packed, exact, pad=0, want_rejected=None):
    """sjmi_parse_batch_device (exact) / sjmi_parse_batch_device_optimistic (and the calls behind SJMI_ST_REJECTED) through
    BatchShard, the 128 bytes behind the batch set to `pad`; a canary behind the tape's capacity."""
    import torch
    from simdjson_java_amd import sharding
    buf, offs = packed
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.buf[len(buf):] = pad
    shard.tape = torch.full((shard.tape_capacity + CANARY_WORDS,), CANARY, dtype=torch.int64, device=shard.device)
    shard.step(torch.cuda.current_stream().cuda_stream, exact=exact)
    torch.cuda.synchronize()
    if want_rejected is not None and not exact:
        assert bool(int(shard.result.cpu().numpy()[1]) & 0x800) == want_rejected
    c = shard.check()
    tape = shard.tape.cpu().numpy().view(np.uint64)
    assert (tape[shard.tape_capacity:] == np.uint64(CANARY)).all(), "a store behind the tape's capacity"
    to = shard.tape_offsets.cpu().numpy()
    err = shard.doc_errors.cpu().numpy()[:len(docs)]
    strings = bytes(shard.sb[:c["string_bytes"]].cpu().numpy())
    assert c["host_documents"] == int((err == NEEDS_HOST).sum())
    return [(int(err[k]), tape[int(to[k]):int(to[k + 1])]) for k in range(len(docs))], strings, c["host_documents"]


PATHS = ["three_calls", "optimistic", "exact"]


def run_path(ctx, path, docs, packed, pad=0, want_rejected=None):
    if path == "three_calls":
        return run_three_calls(ctx, docs, packed, pad)
    return run_shard(ctx, docs, packed, path == "exact", pad, want_rejected)


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=24 * 1024 * 1024)
    yield c
    c.close()


def _boundary_docs(rng, n):
    """n documents with ONE boundary literal each (and easy numbers beside it) -> (documents, their literals)"""
    docs, lits = [], []
    for _ in range(n):
        b = boundary_literal(rng)
        form = rng.randrange(5)
        ls = [b] if form < 3 else ["7", b, "2.5"] if form == 3 else [b, "-12345678901234567"]
        text = ["[%s]", '{"k":%s}', "%s", "[%s,%s,%s]", "[%s,%s]"][form] % tuple(ls)
        docs.append(text.encode())
        lits.append(ls)
    return docs, lits


@pytest.mark.parametrize("path", PATHS)
def test_boundary_literal_list_exactly_full(ctx, path):
    """65,536 boundary literals in one launch, one per document (a fifth of them the root value): all decided on the device,
    every tape word the oracle's, every number the exact reference's."""
    rng = random.Random(65536)
    docs, lits = _boundary_docs(rng, SLOW_CAP)
    got, strings, host = run_path(ctx, path, docs, _pack_nl(docs))
    assert host == 0
    for k, d in enumerate(docs):
        check_doc((path, k), d, lits[k], got[k][0], got[k][1], strings)


@pytest.mark.parametrize("path", PATHS)
def test_boundary_literal_list_over_capacity(ctx, path):
    """65,541 boundary literals, one per document: the five documents whose literal finds the list full come back as
    SJMI_WALK_NEEDS_HOST -- exactly five, counted in host_documents -- and every other document is exact."""
    rng = random.Random(65541)
    docs, lits = _boundary_docs(rng, SLOW_CAP + 5)
    got, strings, host = run_path(ctx, path, docs, _pack_nl(docs))
    handed = 0
    for k, d in enumerate(docs):
        handed += check_doc((path, k), d, lits[k], got[k][0], got[k][1], strings, allow_host=True) == "host"
    assert handed == host == 5


def test_single_document_over_the_list_capacity(ctx):
    """One document with 70,000 boundary literals: sjmi_parse_document hands it back (no tape); sjmi_parser_parse with the GPU
    walk forced takes it on the host and returns the oracle's tape, its numbers the exact reference's."""
    import simdjson_java_amd as S
    rng = random.Random(70000)
    lits = [boundary_literal(rng) for _ in range(70000)]
    doc = ("[" + ",".join(lits) + "]").encode()
    tape, strings, err, st = ctx.parse_document(doc)
    assert st == 0 and err == NEEDS_HOST and tape is None
    p = S.SimdJsonParser(capacity=len(doc) + 64, gpu_walk=True)
    try:
        got = p.parse(doc)
        check_doc("parser", doc, lits, 0, got.tape, got.strings)
        # ... and one under the cap through the same two calls: decided on the device
        small = ("[" + ",".join(lits[:SLOW_CAP]) + "]").encode()
        tape, strings, err, st = ctx.parse_document(small)
        assert st == 0
        check_doc("device", small, lits[:SLOW_CAP], err, tape, strings)
        got = p.parse(small)
        check_doc("parser", small, lits[:SLOW_CAP], 0, got.tape, got.strings)
    finally:
        p.close()


def _pinned_u64(n):
    import torch
    t = torch.empty(n, dtype=torch.int64).pin_memory()
    return t, t.numpy().view(np.uint64)


@pytest.mark.parametrize("easy,hard", [(30, 20), (3000, 40)], ids=["one_wave", "chunked"])
def test_tape_capacity_below_the_boundary_literals(ctx, easy, hard):
    """sjmi_parse_document into a page-locked tape (written in place by the walkers) with room for fewer words than the document
    needs, the boundary literals behind the room or straddling its end: the call reports SJMI_ERR_CAPACITY (the tape's length
    decides, not a hand-back), nothing is stored at or behind tape_capacity, and the same tape with room enough is exact."""
    from simdjson_java_amd.binding import lib
    rng = random.Random(easy)
    lits = [str(i) for i in range(easy)] + [boundary_literal(rng) for _ in range(hard)]
    doc = ("[" + ",".join(lits) + "]").encode()
    assert (len(doc) > 1536) == (easy > 1000)  # (the chunk-parallel walk from a bound of 1,536 bytes on)
    want = O.parse(doc)
    words = want.tape.size
    first = 2 + 2 * easy  # the type word of the first boundary literal
    keep, tape = _pinned_u64(words + CANARY_WORDS)
    sb = np.zeros(len(doc) * 3 + 64, dtype=np.uint8)
    tl, sl, err, st = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_uint32(0)

    src = np.frombuffer(doc, dtype=np.uint8)

    def call(cap):
        tape[:] = np.uint64(CANARY)
        return lib().sjmi_parse_document(ctx._h, src.ctypes.data, len(doc), 1024, tape.ctypes.data, cap, C.addressof(tl), sb.ctypes.data,
                                         sb.size, C.addressof(sl), C.addressof(err), C.addressof(st))
    for cap in (first - 1, first, first + 1, first + 2, first + 2 * hard - 1, words - 2, words - 1):
        rc = call(cap)
        assert rc == -3 and st.value == 0, (cap, rc, err.value)  # SJMI_ERR_CAPACITY
        assert (tape[cap:] == np.uint64(CANARY)).all(), ("a store at or behind tape_capacity", cap)
        assert tape[2] == want.tape[2], "the walk did not write in place"  # (the first number's type word)
    rc = call(words)
    assert rc == 0 and err.value == 0 and tl.value == words
    check_doc("room", doc, lits, 0, tape[:words].copy(), bytes(sb[:sl.value]))
    assert (tape[words:] == np.uint64(CANARY)).all()


def _edge_literals(rng):
    """integers of 1 .. 20 digits (both signs), floats Eisel-Lemire decides, boundary literals"""
    out = []
    for nd in range(1, 21):
        for _ in range(3):
            d = str(rng.randrange(1, 10)) + "".join(str(rng.randrange(10)) for _ in range(nd - 1))
            out += [d, "-" + d]
        out += ["9" * nd, "-" + "9" * nd]
    out += ["0", "-0", "9223372036854775807", "-9223372036854775808", "1.5", "-0.25", "1e22", "1.7976931348623157e308",
            "4.9e-324", "2.2250738585072014e-308", "123456789012345.678", "1E+2", "-9.999999999999999e-5", "0.1",
            "1234567890123456789e-10", "1e-400", "-1e400"]
    out += ["%d.%de%d" % (rng.randrange(10 ** 8), rng.randrange(10 ** 9), rng.randrange(-330, 310)) for _ in range(40)]
    out += [boundary_literal(rng) for _ in range(40)]
    return out


def test_abutting_documents_and_digit_padding(ctx):
    """Batches without separators (doc_offsets only): every root number is followed by the next document's first byte -- a digit
    for most of them -- and the last document ends at every phase of a 16-byte window, the 128 bytes behind the batch digits
    ('9') or zeros.  Every document equals the oracle (judged alone) and the exact reference, through the three calls, the
    optimistic entry (which rejects such a batch) and the exact one, and no output depends on the padding."""
    rng = random.Random(1616)
    lits = _edge_literals(rng)
    for phase in range(16):
        order = list(lits)
        rng.shuffle(order)
        docs, dl = [], []
        for lit in order:
            form = rng.random()
            if form < 0.6:
                docs.append(lit.encode())
                dl.append([lit])
            else:
                docs.append(("[%s]" % lit).encode() if form < 0.8 else ('{"n":%s}' % lit).encode())
                dl.append([lit])
        last = rng.choice([l for l in lits if len(l) >= 16] if phase % 2 else lits)  # (16+ bytes: the second window crosses the end)
        docs.append(last.encode())
        dl.append([last])
        docs.insert(0, b"[" + b" " * ((phase - sum(len(d) for d in docs) - 3) % 16) + b"0]")  # (moves the end to `phase`)
        dl.insert(0, ["0"])
        packed = _pack_tight(docs)
        assert len(packed[0]) % 16 == phase
        for path in PATHS:
            outs = []
            for pad in (ord("9"), 0):
                got, strings, host = run_path(ctx, path, docs, packed, pad, want_rejected=True)
                assert host == 0
                for k, d in enumerate(docs):
                    check_doc((phase, path, pad, k), d, dl[k], got[k][0], got[k][1], strings)
                outs.append([(e, None if t is None else t.tobytes()) for e, t in got])
            assert outs[0] == outs[1], (phase, path)


def test_single_documents_with_digits_behind_their_end(ctx):
    """sjmi_parse_document of a number (at the root and in an array) after a longer document of digits, so the device buffer
    holds digits behind the document's end -- and a caller's buffer with digits behind `length`."""
    rng = random.Random(1717)
    for lit in _edge_literals(rng):
        for doc in (lit.encode(), ("[%s]" % lit).encode()):
            ctx.parse_document(b"9" * (len(doc) + 200))
            tape, strings, err, st = ctx.parse_document(doc)
            check_doc("alone", doc, [lit], err, tape, strings)
            tape, strings, err, st = ctx.parse_document(doc + b"9876543210" * 8, length=len(doc))
            check_doc("length", doc, [lit], err, tape, strings)


def _chunk_doc(rng, n_lits, chunk):
    """An array of n_lits numbers (structural 1 + 2i = literal i) with a boundary literal on both sides of every chunk boundary,
    a 16 .. 18-digit integer and a subnormal / overflowing literal in every chunk; small numbers elsewhere."""
    half = chunk // 2
    lits = []
    pool = ["%d" % rng.randrange(1000) for _ in range(200)] + ["%d.%d" % (rng.randrange(100), rng.randrange(100)) for _ in range(100)]
    special = ["4.9e-324", "-2.4703282292062328e-324", "1e-310", "-2.2250738585072011e-308", "1.8e308", "-1e400",
               "1.7976931348623158e308", "5e-324"]
    for i in range(n_lits):
        r = i % half
        if r in (half - 1, 0) and i > 0:  # literals at structurals chunk * j - 1 and chunk * j + 1
            lits.append(boundary_literal(rng))
        elif r == half - 2 or r == 1:
            lits.append(("-" if rng.random() < 0.5 else "") + str(rng.randrange(10 ** 15, 10 ** 18)))
        elif r == half // 2:
            lits.append(rng.choice(special))
        elif r == half // 2 + 1:
            lits.append(boundary_literal(rng))
        else:
            lits.append(rng.choice(pool))
    return ("[" + ",".join(lits) + "]").encode(), lits


@pytest.mark.parametrize("mib", [1, 16])
def test_chunk_parallel_documents_with_number_edges_in_every_chunk(ctx, mib):
    """Single documents of ~0.8 MB (128-structural chunks) and ~14 MB (512-structural chunks) through sjmi_parse_document:
    boundary literals on both sides of every chunk boundary and in the middle of every chunk, 16 .. 18-digit integers beside
    the boundaries, subnormal and overflowing literals in every chunk -- the tape word for word, the numbers exact."""
    rng = random.Random(mib)
    chunk = 128 if mib == 1 else 512
    n_lits = 131071 if mib == 1 else (mib << 20) // 6  # (at most 262,144 structurals: 128-structural chunks)
    doc, lits = _chunk_doc(rng, n_lits, chunk)
    assert (2 * n_lits + 1 > 262144) == (chunk == 512)
    assert sum(1 for l in lits if len(l) > 19 and "." in l) < SLOW_CAP  # (no hand-back: all decided in the launch)
    tape, strings, err, st = ctx.parse_document(doc)
    assert st == 0
    check_doc(mib, doc, lits, err, tape, strings)
