"""The streaming string pass (k_strings, simdjson-java_amd/csrc/strings.hip) on the granule-edge layouts of tests/string_layouts.py,
through every entry point that runs it, against the oracle of the same document:

  * sjmi_stage1 + sjmi_unescape (k_strings<false>) and the fused sjmi_stage1_unescape: the whole string buffer, the first failing
    string's index and its code;
  * sjmi_unescape_device into a sentinel-filled buffer: total bytes, the number of strings (every opening quote, structural or
    not), every record at the offset the block algebra gives it (tests/host_sim, checked against the oracle by
    tests/test_string_layouts.py), the error's byte position, and the capacity clamps;
  * SimdJsonParser.parse in its three stage-2 homes (the k_strings<true> record table the GPU walkers read);
  * batches of the layouts with document starts at every block phase and at granule starts: sjmi_unescape_batch and the fused
    batch pipeline (both entries), over the batch itself and over the sanitized copy.

Family 7 (strings opened by quotes that are no structurals) does not go through the two host forms: they report the failing
string by its position in indexes[], and its quote is not there (the oracle's unescape_all walks the '"' structurals only).  The
device form, the parser and the batches take it."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import string_layouts as L
from tests.test_gpu_parse import _same
from tests.test_gpu_pipeline import _run_shard
from tests.test_gpu_unescape import _check
from tests.test_host_strings import expected_records, sim_runners
from tests.walk_common import assert_tape_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@functools.lru_cache(None)
def layouts(family, big=True):
    return L.FAMILIES[family](big) if family == 8 else L.FAMILIES[family]()


@functools.lru_cache(None)
def _sim():
    return sim_runners()[0]


def expected(doc):
    """-> (records [(position, record | None, code)], record offsets, total bytes) of the string pass over doc: the records are the
    oracle's, the offsets the block algebra's (where a failing string's record ends is the pass's own business)"""
    recs = expected_records(doc)
    sb, soff, _, _ = _sim()(doc)
    assert len(soff) == len(recs)
    return recs, [int(x) for x in soff], len(sb)


def check_records(got, base, recs, soff, what):
    for k, (pos, rec, code) in enumerate(recs):
        off = base + soff[k]
        if rec is None:
            assert got[off:off + 4] == bytes([0xFF, 0xFF, 0xFF, code]), (what, k, pos, got[off:off + 4].hex(), code)
        else:
            assert got[off:off + len(rec)] == rec, (what, k, pos, off)


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=64 * 1024 * 1024)
    yield c
    c.close()


HOST_FAMILIES = [f for f in sorted(L.FAMILIES) if f != 7]


def _check_fused(ctx, doc):
    idx, st, sb, fei, fec = ctx.stage1_unescape(doc)
    assert st == 0
    want_sb, _, want_feo, want_fec = O.unescape_all(doc + b"\0" * 64, idx)
    sb = bytes(sb)
    if want_feo < 0:
        assert fei is None and fec == 0
        assert sb == want_sb
    else:
        quote_positions = [i for i in range(idx.size) if doc[idx[i]] == 0x22]
        assert fei == quote_positions[want_feo]
        assert fec == want_fec
        assert sb[:len(want_sb)] == want_sb


@pytest.mark.parametrize("family", HOST_FAMILIES)
def test_unescape_host_forms(ctx, family):
    for lay in layouts(family):
        try:
            _check(ctx, lay.doc)
            _check_fused(ctx, lay.doc)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (lay.label, e)) from e


def _device(ctx, doc, cap, slack=256, d_buf=None):
    """sjmi_unescape_device into a buffer of cap + slack sentinel bytes -> (buffer bytes, total, first_error_inv, flags, n_strings)"""
    import torch
    if d_buf is None:
        d_buf = torch.zeros(len(doc) + 128, dtype=torch.uint8, device="cuda")
    d_buf[:len(doc)] = torch.frombuffer(bytearray(doc), dtype=torch.uint8).cuda()
    d_idx = torch.zeros(16, dtype=torch.int32, device="cuda")  # (not read by the pass)
    d_sb = torch.full((cap + slack,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx.unescape_device(d_buf.data_ptr(), len(doc), d_idx.data_ptr(), 0, d_sb.data_ptr(), cap, d_res.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = d_res.cpu().numpy().view(np.uint64)
    return bytes(d_sb.cpu().numpy()), int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF, int(r[2]) >> 32


def check_device(ctx, doc, what):
    recs, soff, total = expected(doc)
    got, tot, inv, flags, ns = _device(ctx, doc, total + 64)
    assert (tot, ns, flags) == (total, len(recs), 0), (what, tot, total, ns, len(recs), flags)
    assert set(got[total:]) <= {SENTINEL}, (what, "bytes behind the records changed")
    failing = [k for k, r in enumerate(recs) if r[1] is None]
    if not failing:
        assert inv == 0 and got[:total] == b"".join(r[1] for r in recs), what
    else:
        k = failing[0]
        assert inv != 0, what
        p, code = (~inv & (2**64 - 1)) >> 8, ~inv & 0xFF
        hi = recs[k + 1][0] if k + 1 < len(recs) else len(doc)
        assert code == recs[k][2] and recs[k][0] < p <= hi, (what, p, code, recs[k][0], recs[k][2], hi)
    check_records(got, 0, recs, soff, what)
    return recs, soff, total


@pytest.mark.parametrize("family", sorted(L.FAMILIES))
def test_unescape_device(ctx, family):
    for lay in layouts(family):
        check_device(ctx, lay.doc, lay.label)


def test_unescape_device_new_bytes_under_the_same_pointer(ctx):
    """sjmi_unescape_device derives the block parities itself when no stage-1 launch of the context went over (d_buf, len), and
    those serve that call only: the same buffer refilled with other bytes of the same length (a caching allocator hands blocks out
    again) must not be unescaped with the parities of the bytes it held before (it was: 2050 strings instead of 2049 here)."""
    import torch
    first = b" " * L.G + b'"' * L.G + b" "
    second = b'"' + b"x" * (L.G - 1) + b'"' * L.G + b'"'
    d_buf = torch.zeros(len(first) + 128, dtype=torch.uint8, device="cuda")
    for doc in (first, second, first):
        recs, soff, total = expected(doc)
        got, tot, inv, flags, ns = _device(ctx, doc, total + 64, d_buf=d_buf)
        assert (tot, ns, flags, inv) == (total, len(recs), 0, 0)
        assert got[:total] == b"".join(r[1] for r in recs)


def test_unescape_device_capacity(ctx):
    """Exactly the bytes needed, one byte less, and a cut inside the header of a string that crosses granules (written by the
    granule that closes it): the short ones set flag bit 0, and no byte at or past string_capacity changes."""
    cases = [layouts(1)[3], layouts(2)[0], layouts(2)[-1], layouts(5)[3], layouts(6)[0]]
    for lay in cases:
        recs, soff, total = check_device(ctx, lay.doc, lay.label)
        got, tot, inv, flags, _ = _device(ctx, lay.doc, total)
        assert tot == total and flags & 1 == 0, (lay.label, flags)
        check_records(got, 0, recs, soff, lay.label)
        assert set(got[total:]) <= {SENTINEL}
        cuts = [total - 1]
        for k, (pos, rec, code) in enumerate(recs):  # a record whose string opens in one granule and closes in a later one
            end = recs[k + 1][0] if k + 1 < len(recs) else len(lay.doc)
            if end // L.G > pos // L.G + 1:
                cuts.append(soff[k] + 2)
                break
        assert len(cuts) == 2 or lay.family == 6, lay.label
        for cap in cuts:
            got, tot, inv, flags, _ = _device(ctx, lay.doc, cap)
            assert tot == total and flags & 1, (lay.label, cap, flags)
            assert set(got[cap:]) <= {SENTINEL}, (lay.label, cap, "a byte at or past string_capacity changed")


@pytest.fixture(scope="module", params=["host_walk", "gpu_walk", "by_size"])
def parser(request):
    """as tests/test_gpu_parse.py's fixture, with room for the 8.6 MiB layouts"""
    import simdjson_java_amd as S
    p = S.SimdJsonParser(capacity=16 * 1024 * 1024, gpu_walk={"host_walk": False, "gpu_walk": True, "by_size": None}[request.param])
    yield p
    p.close()


@pytest.mark.parametrize("family", sorted(L.FAMILIES))
def test_parse(parser, family):
    """tape and string buffer (or the error) of the parser against the oracle's, in all three stage-2 homes; family 7's
    documents fail with the primitive's error, not with the string error behind it"""
    n_valid = 0
    for lay in layouts(family):
        try:
            n_valid += _same(parser, lay.doc) is not None
        except AssertionError as e:
            raise AssertionError("%s: %s" % (lay.label, e)) from e
    if family in (1, 3, 4, 5, 6, 8):
        assert n_valid > 0
    if family == 7:
        assert n_valid == 0


def _batch(docs):
    """documents packed with newline separators; in front of document i a filler document that puts its start at byte i % 65
    of a block (64: a granule start) -> (buffer, offsets, documents with the fillers)"""
    out, offs, all_docs = bytearray(), [0], []
    for i, d in enumerate(docs):
        mod, want = (L.G, 0) if i % 65 == 64 else (L.BLK, i % 65)
        gap = (want - len(out) - 3) % mod + 3
        if len(out) % mod != want:
            f = b"[" + b" " * (gap - 3) + b"]"
            all_docs.append(f)
            out += f + b"\n"
            offs.append(len(out))
        assert len(out) % mod == want
        all_docs.append(d)
        out += d + b"\n"
        offs.append(len(out))
    return bytes(out), np.array(offs, dtype=np.uint64), all_docs


def _batch_docs(with_stage1_failure):
    docs = [lay.doc for f in sorted(L.FAMILIES) for lay in layouts(f, False) if len(lay.doc) < (70000 if f == 8 else 1 << 20)]
    if with_stage1_failure:
        docs.insert(len(docs) // 2, b'["unclosed \\n')
        docs.insert(7, bytes([0x5B, 0x22, 0xC3, 0x22, 0x5D]))
    return _batch(docs)


@pytest.mark.parametrize("bad", [False, True], ids=["all_pass_stage1", "with_stage1_failures"])
def test_unescape_batch(bad):
    """sjmi_unescape_batch: per document, its records where its doc_string_offsets entry says (stage-1-failing documents
    contribute none), and the batch's first error"""
    import simdjson_java_amd as S
    buf, offs, docs = _batch_docs(bad)
    ctx = S.Context(0, len(buf) + 64)
    try:
        idx, io, ds, st = ctx.stage1_batch_isolated(buf, offs)
        assert bool(ds.any()) == bad
        sb, dso, fei, fec = ctx.unescape_batch(len(buf) + 4 * idx.size + 64, len(docs))
        cursor, first_code = 0, None
        for k, d in enumerate(docs):
            assert int(dso[k]) == cursor, k
            if ds[k]:
                continue
            recs, soff, total = expected(d + b"\n")
            check_records(sb, cursor, recs, soff, (k, d[:60]))
            if first_code is None:
                first_code = next((r[2] for r in recs if r[1] is None), None)
            cursor += total
        assert int(dso[-1]) == cursor == len(sb)
        assert first_code is not None and fei is not None and fec == first_code
    finally:
        ctx.close()


@pytest.mark.parametrize("exact", [False, True], ids=["optimistic_entry", "exact_entry"])
@pytest.mark.parametrize("bad", [False, True], ids=["all_pass_stage1", "with_stage1_failures"])
def test_batch_pipeline(exact, bad):
    """the fused batch pipeline: every document's error, and the tape of every valid one against the oracle's; a batch with a
    stage-1 failure is rejected by the optimistic entry and runs over the sanitized copy"""
    import simdjson_java_amd as S
    buf, offs, docs = _batch_docs(bad)
    ctx = S.Context(0, 1 << 20)
    try:
        c, tape, to, err, strings, io, idx = _run_shard(ctx, buf, offs, len(docs), exact=exact, want_rejected=bad)
        n_valid = 0
        for k, d in enumerate(docs):
            want = O.parse(d + b"\n")
            assert int(err[k]) == want.error, (k, d[:60], int(err[k]), want.error)
            if not want.error:
                n_valid += 1
                assert_tape_equal(tape[int(to[k]):int(to[k + 1])], strings, want, (k, d[:60]))
        assert n_valid > len(docs) // 2
    finally:
        ctx.close()
