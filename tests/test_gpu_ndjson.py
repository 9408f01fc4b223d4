"""The NDJSON splitter on the GPU (sjmi_ndjson_offsets_device / sjmi_ndjson_offsets; csrc/ndjson.hip) against the reference of
tests/ndjson_common.py: every edge case at buffer offsets 0, 1, 7 and 15 from an aligned base with '\\n' and 'a' bytes around the
buffer, the capacity rule with canaries, the seeded fuzz, scratch reuse and growth; then end to end -- device-made offsets into
sjmi_parse_batch_device_optimistic, every document against the oracle -- and the upper layers (parse_ndjson,
BatchShard.from_ndjson + select) against parse_batch / a shard with host-made offsets."""
import os
import random
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import ndjson_common as NC
from tests.conftest import ROOT
from tests.walk_common import assert_tape_equal

sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

SHIFTS = (0, 1, 7, 15)
FRONT = 64  # bytes in front of the aligned base that are filled too


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module")
def T():
    import simdjson_java_amd as S
    t = int(S.lib().sjmi_ndjson_tile_bytes())
    assert t >= 64 and t % 64 == 0
    return t


def place(buf, shift):
    """-> (a device tensor with buf at FRONT + shift bytes behind its (512-byte aligned) start and PAD_FILL bytes everywhere
    else, 64 and more of them behind the buffer; the device address of the buffer)"""
    import torch
    n = len(buf)
    host = np.frombuffer((NC.PAD_FILL * ((FRONT + shift + n + 192) // 2 + 1))[:FRONT + shift + n + 192], dtype=np.uint8).copy()
    host[FRONT + shift:FRONT + shift + n] = np.frombuffer(buf, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 64 == 0
    return dev, dev.data_ptr() + FRONT + shift


def split(ctx, buf, shift, capacity, null_offsets=False):
    """one call -> (the capacity entries + 4 canaries behind them, the result record as 3 x uint64)"""
    import torch
    dev, ptr = place(buf, shift)
    offs = torch.from_numpy(np.full(capacity + 4, NC.CANARY, dtype=np.uint64).view(np.int64)).cuda()
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.ndjson_offsets_device(ptr, len(buf), 0 if null_offsets else offs.data_ptr(), capacity, res.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return offs.cpu().numpy().view(np.uint64), res.cpu().numpy().view(np.uint64)


def check(ctx, what, buf, shifts=SHIFTS):
    """at every shift with room for everything -> the number of documents"""
    ref = NC.ndjson_reference(buf)
    n_docs = len(ref[0]) - 1
    for shift in shifts:
        offs, res = split(ctx, buf, shift, n_docs + 2)
        NC.check("%s, offset %d" % (what, shift), buf, n_docs + 2, offs, res, ref=ref)
    return n_docs


def test_edge_cases(ctx, T):
    docs = 0
    for name, buf in NC.edge_cases(T):
        docs += check(ctx, name, buf)
    assert docs > 2 * T


def test_an_edge_that_moves_with_the_pointer(ctx, T):
    """the tiles are cut from the 16-byte boundary below the buffer: the same edge cases, placed for a buffer 7 bytes behind one"""
    for name, buf in NC.edge_cases(T):
        if len(buf) > 7 and ("tile" in name or "densest" in name):
            check(ctx, name + " (7 bytes cut)", buf[7:], shifts=(7,))


@pytest.mark.parametrize("n_tiles", (1023, 1024, 1025))
def test_tile_counts_around_one_slice_of_the_scan(ctx, T, n_tiles):
    """(the launcher's grids are the tile count itself -- no kernel strides -- so these are also more tiles than any fixed grid)"""
    buf = NC.sparse_input(n_tiles, T)
    assert (len(buf) + T - 1) // T == n_tiles
    assert check(ctx, "%d tiles" % n_tiles, buf, shifts=(0, 15)) > n_tiles // 4


def test_capacity(ctx, T):
    line = b'{"k": [1, 2, 3]}\n'
    for what, buf in (("a tile and a half of lines", b"\n" + line * (3 * T // 2 // len(line)) + b"tail"),
                      ("the densest output", (b"1\n" * (T + 2))[:2 * T + 3]),
                      ("no document", b" \n\n"), ("one document", b"7\n")):
        n_docs = len(NC.ndjson_reference(buf)[0]) - 1
        for capacity in sorted({0, 1, n_docs, n_docs + 1}):
            for shift in (0, 7):
                offs, res = split(ctx, buf, shift, capacity)
                NC.check("%s, capacity %d, offset %d" % (what, capacity, shift), buf, capacity, offs, res)
                assert bool(int(res[2]) & NC.OVERFLOW) == (capacity < n_docs + 1)
        offs, res = split(ctx, buf, 0, 0, null_offsets=True)  # how a caller sizes its array
        NC.check("%s, NULL offsets" % what, buf, 0, offs, res)


def test_fuzz(ctx, T):
    docs = blank_tails = 0
    for k, buf in enumerate(NC.fuzz_inputs(200, T, seed=77077)):
        docs += check(ctx, "fuzz input %d (%d bytes)" % (k, len(buf)), buf, shifts=(SHIFTS[k % 4],))
        blank_tails += not buf[buf.rfind(b"\n") + 1:].strip(b" \t\r")
    assert docs > 1000 and 0 < blank_tails < 200


def test_scratch_reuse_and_growth(T):
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 16)
    try:
        rng = np.random.default_rng(5)
        for n in (5 * T + 3, 100, 40 * T + 1, T, 41 * T):
            check(c, "%d bytes on one context" % n, NC.fuzz_input(rng, T, n), shifts=(1,))
    finally:
        c.close()


def test_host_form(ctx, T):
    for name, buf in NC.edge_cases(T)[:12] + [("three tiles", NC.fuzz_input(np.random.default_rng(9), T, 3 * T + 65))]:
        want, consumed, tail_blank = NC.ndjson_reference(buf)
        offs, got_consumed, flags = ctx.ndjson_offsets(buf)
        assert offs.tolist() == want and got_consumed == consumed and flags == (NC.TAIL_BLANK if tail_blank else 0), name


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _ndjson_file(break_line=None):
    """a few hundred documents joined with '\\n', blank and CR LF lines sprinkled in, an unterminated tail -> (bytes, documents)"""
    import synth
    docs = synth.small_docs(seed=31, n=300, lo=200, hi=700)
    assert not any(b"\n" in d for d in docs)
    if break_line is not None:
        docs[break_line] = b'["unclosed, ' + docs[break_line][1:40].replace(b'"', b"'").replace(b"\\", b"/")
    rng = random.Random(8)
    out = bytearray(b"\n \r\n")
    for d in docs:
        out += d + rng.choice([b"\n", b"\r\n", b" \n", b"\n\n", b"\n\r\n \t\n", b"\n"])
    return bytes(out) + b'{"unterminated": tr', docs


def _shard_from_device_offsets(ctx, data):
    """sjmi_ndjson_offsets_device over the uploaded bytes, then a BatchShard over [0, consumed) with the offsets left on the device"""
    import torch
    from simdjson_java_amd import sharding
    raw = torch.frombuffer(bytearray(data) + bytearray(64), dtype=torch.uint8).cuda()
    offs = torch.empty(len(data) // 2 + 1, dtype=torch.int64, device="cuda")
    res = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.ndjson_offsets_device(raw.data_ptr(), len(data), offs.data_ptr(), offs.numel(), res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    n_docs, consumed, flags = (int(x) for x in res.cpu().numpy())
    want, want_consumed, _ = NC.ndjson_reference(data)
    assert (n_docs, consumed, flags) == (len(want) - 1, want_consumed, 0)
    assert offs[:n_docs + 1].cpu().numpy().tolist() == want
    return sharding.BatchShard(ctx, raw[:consumed], None, torch.device("cuda", 0), device_offsets=offs[:n_docs + 1]), want


def _outputs(shard, c):
    return (shard.tape.cpu().numpy().view(np.uint64), shard.tape_offsets.cpu().numpy(), shard.doc_errors.cpu().numpy(),
            bytes(shard.sb[:c["string_bytes"]].cpu().numpy()))


def test_device_made_offsets_feed_the_optimistic_pipeline(ctx):
    import torch
    data, docs = _ndjson_file()
    shard, offs = _shard_from_device_offsets(ctx, data)
    assert shard.n_docs == len(docs)
    shard.step(torch.cuda.current_stream().cuda_stream)  # sjmi_parse_batch_device_optimistic
    torch.cuda.synchronize()
    assert not (int(shard.result.cpu().numpy()[1]) & 0x800), "SJMI_ST_REJECTED for offsets the device made"
    c = shard.check()
    assert getattr(shard, "rejected_steps", 0) == 0 and c["failed_documents"] == 0 and c["documents"] == len(docs)
    tape, to, err, strings = _outputs(shard, c)
    for k in range(len(docs)):
        line = data[offs[k]:offs[k + 1]].strip(b" \t\r\n")
        assert line == docs[k]
        want = O.parse(line + b"\n")
        got = tape[int(to[k]):int(to[k + 1])]
        assert int(err[k]) == 0 and want.error == 0
        assert_tape_equal(got, strings, want, k)
        assert O.Parsed(got, strings, 0, 0, 0).to_python() == want.to_python(), k


def test_one_broken_line_stays_one_failing_document(ctx):
    import torch
    bad = 137
    data, docs = _ndjson_file(break_line=bad)
    shard, offs = _shard_from_device_offsets(ctx, data)
    shard.step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(shard.result.cpu().numpy()[1]) & 0x800  # an unclosed string: not a batch for the optimistic pipeline
    c = shard.check()  # sjmi_parse_batch_device_rejected
    assert shard.rejected_steps == 1 and c["failed_documents"] == 1
    tape, to, err, strings = _outputs(shard, c)
    assert np.flatnonzero(err[:len(docs)]).tolist() == [bad]
    assert int(err[bad]) == O.parse(docs[bad] + b"\n").error != 0
    for k in (0, bad - 1, bad + 1, len(docs) - 1):
        want = O.parse(docs[k] + b"\n")
        assert O.Parsed(tape[int(to[k]):int(to[k + 1])], strings, 0, 0, 0).to_python() == want.to_python(), k


def test_parse_ndjson_and_from_ndjson_equal_host_made_offsets(ctx):
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    from tests.test_gpu_batch import _pack
    docs = [b'{"id":%d,"name":"n%d","v":[%d,{"w":null}]}' % (i, i, i * 3) for i in range(40)]
    packed, host_offs = _pack(docs)
    ndjson = b"\r\n" + b"".join(d + (b"\r\n\n" if i % 5 == 0 else b"\n") for i, d in enumerate(docs))
    p = S.SimdJsonParser(capacity=1 << 20)
    try:
        want_tapes, want_strings, want_err = p.parse_batch(packed, host_offs)
        want = [O.Parsed(t, want_strings, 0, 0, 0).to_python() for t in want_tapes]
        for text in (ndjson, ndjson[:-1]):  # (without the last '\n': parse_ndjson appends it)
            tapes, strings, errors = p.parse_ndjson(text)
            assert len(tapes) == len(docs) and not errors.any() and not want_err.any()
            assert [O.Parsed(t, strings, 0, 0, 0).to_python() for t in tapes] == want
    finally:
        p.close()
    plan = S.SelectPlan(["/id", "/name", "/v/1/w", "/nope"])
    dev = torch.device("cuda", 0)
    a = sharding.BatchShard.from_ndjson(ctx, ndjson + b'{"tail', dev)
    assert a.n_docs == len(docs) and a.ndjson_consumed == len(ndjson) and a.ndjson_flags == 0
    b = sharding.BatchShard(ctx, packed, host_offs, dev)
    cols = []
    for shard in (a, b):
        shard.step(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert not (int(shard.result.cpu().numpy()[1]) & 0x800)
        assert shard.check()["failed_documents"] == 0
        types, values = shard.select(plan, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        types, values = types.cpu().numpy(), values.cpu().numpy().view(np.uint64)
        sb = shard.sb.cpu().numpy()
        names = [bytes(sb[int(v) & 0xFFFFFFFF:(int(v) & 0xFFFFFFFF) + (int(v) >> 32)]) for v in values[1]]
        cols.append((types.tolist(), values[0].tolist(), names))
    assert cols[0] == cols[1]
    assert cols[0][1] == list(range(40)) and cols[0][2] == [b"n%d" % i for i in range(40)]
    assert cols[0][0][2] == [ord("n")] * 40 and cols[0][0][3] == [0] * 40
    plan.close()
