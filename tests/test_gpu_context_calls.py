"""What a context remembers between the host entry points of the C ABI (include/sjmi.h; DESIGN.md 5.1, what a call leaves and
what it forgets): the two-call forms sjmi_unescape / sjmi_unescape_batch answer for the LAST indexing call on the context and for
nothing older, whatever ran in between; the speculative download of a document of at most 4 KiB stops at its bound;
sjmi_stage1_batch gives the oracle's indexes, offsets and status in both tile modes; and a tape handed to sjmi_parse_document
takes the zero-copy path exactly while it is registered, also with more registered buffers in play than the view cache holds."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

CAPACITY = 1 << 20
NONE64 = 0xFFFFFFFFFFFFFFFF


def _lib():
    from simdjson_java_amd.binding import lib
    return lib()


class Arrays:
    """the output arrays of a run: pageable numpy arrays, or page-locked ones (the zero-copy path of the entry points that have one)"""

    def __init__(self, pinned):
        self.pinned, self.keep = pinned, []

    def __call__(self, n, dtype, fill=None):
        n = max(int(n), 1)
        if self.pinned:
            import torch
            t = torch.empty(n * np.dtype(dtype).itemsize, dtype=torch.uint8).pin_memory()
            self.keep.append(t)
            a = t.numpy().view(dtype)
        else:
            a = np.empty(n, dtype=dtype)
        if fill is not None:
            a[:] = fill
        return a


def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data if a.size else None


def _fei(v):
    return None if v == NONE64 else v


# ---- the host entry points, each with the caller's arrays from `new` and its result in a form that compares with == -----------
def stage1(ctx, new, doc):
    a, idx = _u8(doc), new(len(doc) + 2, np.uint32)
    cnt, st = C.c_uint64(0), C.c_uint32(0)
    ctx._check(_lib().sjmi_stage1(ctx._h, _ptr(a), a.size, idx.ctypes.data, idx.size, C.byref(cnt), C.byref(st)), "sjmi_stage1")
    assert idx[cnt.value] == 0, "sentinel"
    return idx[:cnt.value].tolist(), st.value


def stage1_unescape(ctx, new, doc):
    n = len(doc)
    a, idx, sb = _u8(doc), new(n + 2, np.uint32), new(n + 4 * (n // 2 + 2) + 64, np.uint8)
    cnt, total, fei, st, fec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    ctx._check(_lib().sjmi_stage1_unescape(ctx._h, _ptr(a), n, idx.ctypes.data, idx.size, C.byref(cnt), C.byref(st), sb.ctypes.data, sb.size,
                                           C.byref(total), C.byref(fei), C.byref(fec)), "sjmi_stage1_unescape")
    assert idx[cnt.value] == 0, "sentinel"
    return idx[:cnt.value].tolist(), st.value, bytes(sb[:total.value]), _fei(fei.value), fec.value


def unescape(ctx, new, capacity):
    sb = new(capacity, np.uint8)
    total, fei, fec = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    ctx._check(_lib().sjmi_unescape(ctx._h, sb.ctypes.data, sb.size, C.byref(total), C.byref(fei), C.byref(fec)), "sjmi_unescape")
    return bytes(sb[:total.value]), _fei(fei.value), fec.value


def unescape_batch(ctx, new, capacity, n_docs):
    sb, dso = new(capacity, np.uint8), new(n_docs + 1, np.uint64, 0)
    total, fei, fec = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    ctx._check(_lib().sjmi_unescape_batch(ctx._h, sb.ctypes.data, sb.size, dso.ctypes.data, C.byref(total), C.byref(fei), C.byref(fec)),
               "sjmi_unescape_batch")
    return bytes(sb[:total.value]), dso[:n_docs + 1].tolist(), _fei(fei.value), fec.value


def stage1_batch(ctx, new, buf, offs, isolated=False):
    a, offs = _u8(buf), np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.size - 1
    idx, io, ds = new(a.size + 2, np.uint32), new(n + 1, np.uint64, 0), new(n, np.uint32, 0)
    cnt, st = C.c_uint64(0), C.c_uint32(0)
    if isolated:
        ctx._check(_lib().sjmi_stage1_batch_isolated(ctx._h, _ptr(a), a.size, offs.ctypes.data, n, idx.ctypes.data, idx.size, io.ctypes.data,
                                                     ds.ctypes.data, C.byref(cnt), C.byref(st)), "sjmi_stage1_batch_isolated")
        assert idx[cnt.value] == 0, "sentinel"
        return idx[:cnt.value].tolist(), io[:n + 1].tolist(), ds[:n].tolist(), st.value
    ctx._check(_lib().sjmi_stage1_batch(ctx._h, _ptr(a), a.size, offs.ctypes.data, n, idx.ctypes.data, idx.size, io.ctypes.data, C.byref(cnt),
                                        C.byref(st)), "sjmi_stage1_batch")
    return idx[:cnt.value].tolist(), io[:n + 1].tolist(), st.value


def parse_document(ctx, doc, tape, sb):
    """sjmi_parse_document into the caller's tape and string buffer -> (tape words, string bytes, error, stage-1 status)"""
    a = _u8(doc)
    tl, sl, err, st = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_uint32(0)
    ctx._check(_lib().sjmi_parse_document(ctx._h, _ptr(a), a.size, 1024, tape.ctypes.data, tape.size, C.byref(tl), sb.ctypes.data, sb.size,
                                          C.byref(sl), C.byref(err), C.byref(st)), "sjmi_parse_document")
    return tape[:tl.value].tolist(), bytes(sb[:sl.value]), err.value, st.value


def _pack(docs):
    buf = b"".join(d + b"\n" for d in docs)
    return buf, np.cumsum([0] + [len(d) + 1 for d in docs]).astype(np.uint64)


def _doc(rng, n_items, pad_to=0):
    items = ['{"k%d":["%s",%d,"\\u00e9\\n%s"]}' % (i, "ab\\t" * rng.randint(0, 6), rng.randint(-99, 99), "x" * rng.randint(0, 40)) for i in range(n_items)]
    d = ("[" + ",".join(items) + "]").encode()
    return d + b" " * max(pad_to - len(d), 0)


def _sb_capacity(n):
    return n + 4 * (n // 2 + 2) + 64


# ---- the oracle's answers -------------------------------------------------------------------------------------------------------
def want_stage1(doc):
    idx, st = O.stage1(doc)
    return idx.tolist(), st


def want_strings(buf, idx):
    sb, _, feo, _ = O.unescape_all(buf + b"\0" * 64, np.asarray(idx, dtype=np.uint32))
    assert feo < 0, "the documents of this file have no string errors"
    return sb


def want_batch(buf, offs):
    idx, st = O.stage1(buf)
    return idx.tolist(), np.searchsorted(idx, offs, side="left").tolist(), st


def want_isolated(docs):
    """per document: its status alone (with its separator); a failing document has no structurals"""
    idx, io, ds, pos = [], [0], [], 0
    for d in docs:
        one, st = O.stage1(d + b"\n")
        ds.append(st)
        if not st:
            idx += (one.astype(np.int64) + pos).tolist()
        io.append(len(idx))
        pos += len(d) + 1
    st_or = 0
    for s in ds:
        st_or |= s
    return idx, io, ds, st_or


def want_doc_string_offsets(docs, ds):
    out = [0]
    for d, st in zip(docs, ds):
        out.append(out[-1] + (0 if st else len(want_strings(d, O.stage1(d + b"\n")[0]))))
    return out


# ---- "the answer depends only on the last indexing call" ------------------------------------------------------------------------
_rng = random.Random(22)
A = _doc(_rng, 40)                                    # ~2 KB, some forty 64-byte blocks, 80 strings
B = _doc(_rng, 7)                                     # a few hundred bytes
T_DOCS = [_doc(_rng, k % 4 + 1) for k in range(9)]
T, T_OFFS = _pack(T_DOCS)
T2_DOCS = [_doc(_rng, k % 3 + 1) for k in range(5)] + [b'"tail \\n string"', b"[]"]
T2, T2_OFFS = _pack(T2_DOCS)
TBAD_DOCS = T_DOCS[:4] + [b'["unclosed \\" string'] + T_DOCS[4:]
TBAD, TBAD_OFFS = _pack(TBAD_DOCS)
A_AS_LONG_AS_TBAD = _doc(random.Random(23), 12, pad_to=len(TBAD))   # the same pointer AND length as the batch in front of it
LINES = b'\n{"a":1}\n\r\n[2]\n \t\n3\n"4"\r\n{}\nnull\n[]\ntail'
CHUNK = b"[" + b"1," * 31 + b"1"
assert len(CHUNK) == 64 and len(A_AS_LONG_AS_TBAD) == len(TBAD) and len(A) > 4 * len(B)


def _push_chunk(ctx, new):
    s = ctx.stream(64)
    try:
        return s.push(CHUNK, False)
    finally:
        s.close()


def _masks(ctx, new):
    return ctx.stage1_masks(B)


def _ndjson(ctx, new):
    return ctx.ndjson_offsets(LINES)


def _parse_b(ctx, new):
    n = len(B)
    return parse_document(ctx, B, new(2 * n + 16, np.uint64), new(_sb_capacity(n), np.uint8))


def S1(doc):
    return lambda ctx, new: stage1(ctx, new, doc)


def S1U(doc):
    return lambda ctx, new: stage1_unescape(ctx, new, doc)


def UN(n):
    return lambda ctx, new: unescape(ctx, new, _sb_capacity(n))


def UNB(n, n_docs):
    return lambda ctx, new: unescape_batch(ctx, new, _sb_capacity(n), n_docs)


def BATCH(buf, offs, isolated=False):
    return lambda ctx, new: stage1_batch(ctx, new, buf, offs, isolated)


def _want_unescape(doc):
    return (want_strings(doc, want_stage1(doc)[0]), None, 0)


def _want_unescape_batch(buf, docs, idx, ds):
    return (want_strings(buf, idx), want_doc_string_offsets(docs, ds), None, 0)


# (name, steps in front, the last step(s), the oracle's answer to each of the last steps -- None: the last of them raises)
SEQUENCES = [
    ("stage1, unescape", [], [S1(A), UN(len(A))], lambda: [want_stage1(A), _want_unescape(A)]),
    ("stage1, masks of another document, unescape", [S1(A), _masks], [UN(len(A))], None),
    ("stage1, ndjson offsets, unescape", [S1(A), _ndjson], [UN(len(A))], None),
    ("stage1, parse_document of another document, unescape", [S1(A), _parse_b], [UN(len(A))], None),
    ("stage1, a stream chunk, unescape", [S1(A), _push_chunk], [UN(len(A))], None),
    ("stage1, unescape_batch", [S1(A)], [UNB(len(A), 1)], None),
    ("batch, unescape_batch, unescape", [], [BATCH(T, T_OFFS), UNB(len(T), len(T_DOCS)), UN(len(T))],
     lambda: [want_batch(T, T_OFFS), _want_unescape_batch(T, T_DOCS, want_batch(T, T_OFFS)[0], [0] * len(T_DOCS)), _want_unescape(T)]),
    ("batch, stage1_unescape, unescape_batch", [BATCH(T, T_OFFS), S1U(A)], [UNB(len(T), len(T_DOCS))], None),
    ("isolated batch with a failing document, stage1 of as many bytes, unescape", [BATCH(TBAD, TBAD_OFFS, True)],
     [S1(A_AS_LONG_AS_TBAD), UN(len(TBAD))], lambda: [want_stage1(A_AS_LONG_AS_TBAD), _want_unescape(A_AS_LONG_AS_TBAD)]),
    ("isolated batch, unescape_batch, batch, unescape_batch", [BATCH(TBAD, TBAD_OFFS, True), UNB(len(TBAD), len(TBAD_DOCS))],
     [BATCH(T2, T2_OFFS), UNB(len(T2), len(T2_DOCS))],
     lambda: [want_batch(T2, T2_OFFS), _want_unescape_batch(T2, T2_DOCS, want_batch(T2, T2_OFFS)[0], [0] * len(T2_DOCS))]),
]


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=CAPACITY)
    yield c
    c.close()


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("case", SEQUENCES, ids=[s[0] for s in SEQUENCES])
def test_the_answer_depends_only_on_the_last_indexing_call(ctx, case, pinned):
    """Every sequence on ONE context that has served the sequences in front of it.  A legal last step gives what the same last
    step(s) give on a fresh context, and what the oracle gives; one that asks for a document the context no longer holds raises."""
    import simdjson_java_amd as S
    name, front, last, want = case
    new = Arrays(pinned)
    for step in front:
        step(ctx, new)
    if want is None:
        for step in last[:-1]:
            step(ctx, new)
        with pytest.raises(S.SjmiError):
            last[-1](ctx, new)
        return
    got = [step(ctx, new) for step in last]
    fresh = S.Context(device=0, capacity=CAPACITY)
    try:
        alone = [step(fresh, new) for step in last]
    finally:
        fresh.close()
    assert got == alone, name
    assert got == want(), name


def test_the_isolated_batch_in_front_is_what_the_oracle_says(ctx):
    """(the batch the sequences above start from: the failing document is reported alone, and the string pass skips it)"""
    new = Arrays(False)
    got = stage1_batch(ctx, new, TBAD, TBAD_OFFS, True)
    want = want_isolated(TBAD_DOCS)
    assert got == want and want[2][4] != 0 and sum(1 for s in want[2] if s) == 1
    assert unescape_batch(ctx, new, _sb_capacity(len(TBAD)), len(TBAD_DOCS)) == _want_unescape_batch(TBAD, TBAD_DOCS, want[0], want[2])


# ---- the 4 KiB edge of the speculative download -----------------------------------------------------------------------------------
CANARY32, CANARY8 = 0xC0FFEE11, 0xA5


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("fused", [False, True], ids=["stage1", "stage1_unescape"])
@pytest.mark.parametrize("n", [4096, 4097])
def test_the_4k_edge_of_the_speculative_download(ctx, n, fused, pinned):
    """A document of at most 4 KiB comes back behind ONE synchronisation, its outputs downloaded by their bounds -- min(len + 2,
    index_capacity) entries, min(len + 4 * (len / 2 + 2), string_capacity) bytes; one byte more and count + 1 entries / total_bytes
    bytes are downloaded behind a second one.  Either way: the oracle's indexes and strings, the sentinel, and nothing written
    behind the bound of a pageable array."""
    doc = _doc(random.Random(n), 48, pad_to=n)
    assert len(doc) == n
    new = Arrays(pinned)
    idx = new(n + 2 + 64, np.uint32, CANARY32)
    sb = new(_sb_capacity(n) + 64, np.uint8, CANARY8)
    a = _u8(doc)
    cnt, total, fei, st, fec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    if fused:
        ctx._check(_lib().sjmi_stage1_unescape(ctx._h, a.ctypes.data, n, idx.ctypes.data, idx.size, C.byref(cnt), C.byref(st), sb.ctypes.data,
                                               sb.size, C.byref(total), C.byref(fei), C.byref(fec)), "sjmi_stage1_unescape")
    else:
        ctx._check(_lib().sjmi_stage1(ctx._h, a.ctypes.data, n, idx.ctypes.data, idx.size, C.byref(cnt), C.byref(st)), "sjmi_stage1")
    want_idx, want_st = want_stage1(doc)
    count = cnt.value
    assert st.value == want_st == 0 and idx[:count].tolist() == want_idx and idx[count] == 0
    small = n <= 4096
    if fused:
        want_sb = want_strings(doc, want_idx)
        assert bytes(sb[:total.value]) == want_sb and fei.value == NONE64 and fec.value == 0
    if not pinned:
        idx_bound = min(n + 2, idx.size) if small else count + 1
        assert count + 1 <= idx_bound and (idx[idx_bound:] == CANARY32).all(), "indexes behind the bound"
        sb_bound = (min(n + 4 * (n // 2 + 2), sb.size) if small else total.value) if fused else 0
        assert (sb[sb_bound:] == CANARY8).all(), "string bytes behind the bound"


# ---- sjmi_stage1_batch --------------------------------------------------------------------------------------------------------------
def _batches():
    rng = random.Random(300)
    many = [_doc(rng, rng.randint(0, 3)) if k % 7 else rng.choice([b"[]", b"7", b'"s"', b"", b'{"a":null}']) for k in range(300)]
    broken = list(many[:3])
    broken[1] = b'{"a":"\xff\xfe"}'
    packed = [("one", many[1:2]), ("three", many[3:6]), ("three, one not UTF-8", broken), ("three empty", [b"", b"", b""]), ("300", many),
              ("no documents", [])]
    # (... and three documents of no bytes at all, not even a separator)
    return [(name, docs) + _pack(docs) for name, docs in packed] + [("three of no bytes", [b""] * 3, b"", np.zeros(4, dtype=np.uint64))]


BATCHES = _batches()


@pytest.mark.parametrize("ticket", [False, True], ids=["default", "ticket"])
@pytest.mark.parametrize("case", BATCHES, ids=[b[0] for b in BATCHES])
def test_stage1_batch_against_the_oracle(case, ticket):
    """Indexes, index offsets and status of sjmi_stage1_batch are those of ONE stage-1 pass over the packed batch and a search of
    every document's offset in its indexes; sjmi_unescape_batch behind it gives the oracle's string buffer and every document's
    place in it (a batch that failed stage 1 has no meaningful strings: there the call only has to answer as it does alone)."""
    import simdjson_java_amd as S
    name, docs, buf, offs = case
    new = Arrays(False)
    c = S.Context(device=0, capacity=CAPACITY)
    try:
        c.set_tile_mode(ticket)
        for _ in range(2):  # (the second call finds every buffer grown and the other half of the workspace)
            got = stage1_batch(c, new, buf, offs)
            assert got == want_batch(buf, offs), name
            strings = unescape_batch(c, new, _sb_capacity(len(buf)), len(docs))
            if got[2] == 0:
                assert strings == _want_unescape_batch(buf, docs, got[0], [0] * len(docs)), name
            else:
                assert got[2] == S.ST_UTF8
    finally:
        c.close()


# ---- the tape's place among the cached views ----------------------------------------------------------------------------------------
def test_a_tape_takes_the_zero_copy_path_exactly_while_it_is_registered(ctx, twitter):
    """sjmi_parse_document with a numpy tape: pageable (staged), registered (written in place), pageable again (a stale view
    would fault), registered again -- two calls per state, the same tape, strings and error each time.  Then seven rounds that
    alternate two registered tapes and two registered index / string-buffer pairs: more pointers than the cache has entries."""
    doc = twitter
    n = len(doc)
    want = O.parse(doc)
    assert want.error == 0
    tapes = [np.zeros(2 * n + 16, dtype=np.uint64) for _ in range(2)]
    sbs = [np.zeros(_sb_capacity(n), dtype=np.uint8) for _ in range(2)]
    idxs = [np.zeros(n + 2, dtype=np.uint32) for _ in range(2)]
    first = parse_document(ctx, doc, tapes[0], sbs[0])
    assert first[2] == 0 and first[3] == 0
    assert O.Parsed(np.array(first[0], dtype=np.uint64), first[1], 0, 0, 0).to_python() == want.to_python()
    fused_want = (want_stage1(doc)[0], 0, want_strings(doc, want_stage1(doc)[0]), None, 0)

    def register(arrays, on):
        for a in arrays:
            rc = _lib().sjmi_host_register(ctx._h, a.ctypes.data, a.nbytes) if on else _lib().sjmi_host_unregister(ctx._h, a.ctypes.data)
            assert rc == 0

    for state in ("pageable", "registered", "pageable", "registered"):
        if state == "registered":
            register(tapes[:1], True)
        try:
            for _ in range(2):
                tapes[0][:] = 0
                assert parse_document(ctx, doc, tapes[0], sbs[0]) == first, state
        finally:
            if state == "registered":
                register(tapes[:1], False)
    register(tapes + sbs + idxs, True)
    try:
        for k in range(7):
            tapes[k % 2][:] = 0
            assert parse_document(ctx, doc, tapes[k % 2], sbs[k % 2]) == first, k
            idxs[k % 2][:] = 0
            cnt, total, fei, st, fec = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
            ctx._check(_lib().sjmi_stage1_unescape(ctx._h, _u8(doc).ctypes.data, n, idxs[k % 2].ctypes.data, idxs[k % 2].size, C.byref(cnt),
                                                   C.byref(st), sbs[k % 2].ctypes.data, sbs[k % 2].size, C.byref(total), C.byref(fei),
                                                   C.byref(fec)), "sjmi_stage1_unescape")
            got = (idxs[k % 2][:cnt.value].tolist(), st.value, bytes(sbs[k % 2][:total.value]), _fei(fei.value), fec.value)
            assert got == fused_want, k
    finally:
        register(tapes + sbs + idxs, False)
    assert parse_document(ctx, doc, tapes[1], sbs[1]) == first
