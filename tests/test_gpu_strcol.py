"""The string-column gather on the GPU (sjmi_string_column_device through Context.string_column_device and
BatchShard.string_column): every offset, validity word, byte below the capacity and the result record against the numpy
reference of tests/strcol_common.py, and canaries behind everything the call owns.  Synthetic columns carry wild value words in
their NULL rows; the end-to-end tests take their expected bytes from tests/select_common.py over the oracle's parse."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import explode_common as EC
from tests import select_common as SEL
from tests import strcol_common as SC
from tests.test_gpu_batch import _pack

pytestmark = pytest.mark.gpu

SB_SIZE = 1 << 16
STAGE2_FAILS = b'{"user":{"screen_name":"x"},"arr":[1,2,}'


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module", autouse=True)
def side_stream():
    """torch's work and the engine's kernels on ONE stream of their own: handle 0 names the context's stream in the C ABI, so
    torch's default stream cannot carry both"""
    import torch
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    with torch.cuda.stream(side):
        yield side.cuda_stream
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def sb():
    """(the string buffer on the host, the same on the device, placed 5 bytes into its allocation)"""
    import torch
    host = SC.string_buffer(np.random.default_rng(77), SB_SIZE)
    store = torch.zeros(SB_SIZE + 16, dtype=torch.uint8, device="cuda:0")
    store[5:5 + SB_SIZE] = torch.from_numpy(host).to("cuda:0")
    return host, store[5:5 + SB_SIZE]


def run(ctx, stream, types, values, d_sb, capacity, validity=True, type_shift=0, bytes_shift=0, sizing_null=True):
    """one call into out_buffers() on the device; the type column and the bytes are slices of larger tensors"""
    import torch
    dev = d_sb.device
    n = len(types)
    tstore = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    d_types = tstore[type_shift:type_shift + n]
    d_types.copy_(torch.from_numpy(np.ascontiguousarray(types, dtype=np.uint8)))
    d_values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).to(dev)
    offsets, words, data, res = SC.out_buffers(n, capacity, validity)
    d_offsets = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_words = torch.from_numpy(words.view(np.int64)).to(dev) if validity else None
    dstore = torch.full((data.size + 16,), SC.CANARY, dtype=torch.uint8, device=dev)
    d_data = dstore[bytes_shift:bytes_shift + data.size]
    d_res = torch.from_numpy(res.view(np.int64)).to(dev)
    ctx.string_column_device(d_types.data_ptr() if n else 0, d_values.data_ptr() if n else 0, n, d_sb.data_ptr(), d_offsets.data_ptr(),
                             d_words.data_ptr() if validity else 0, d_data.data_ptr() if capacity or not sizing_null else 0, capacity,
                             d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    assert bool((dstore[:bytes_shift] == SC.CANARY).all()) and bool((dstore[bytes_shift + data.size:] == SC.CANARY).all()), "written in front of d_bytes"
    return (d_offsets.cpu().numpy(), d_words.cpu().numpy() if validity else None, d_data.cpu().numpy(), d_res.cpu().numpy())


def check_all(ctx, stream, what, types, values, sb, caps=None, **kw):
    host, d_sb = sb
    ref = SC.reference(types, values, host)
    total = len(ref[2])
    for capacity in SC.capacities(total) if caps is None else [total if c is None else c for c in caps]:
        got = run(ctx, stream, types, values, d_sb, capacity, **kw)
        SC.check("%s, capacity %d of %d" % (what, capacity, total), *got, ref, capacity)
    return total


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_row_counts(ctx, side_stream, sb, n):
    t, v = SC.random_column(np.random.default_rng(1000 + n), n, 9, SB_SIZE)
    check_all(ctx, side_stream, "%d rows" % n, t, v, sb)


def test_the_chunk_scan_takes_a_second_slice(ctx, side_stream, sb):
    """1024 * 1024 + 1 rows: chunk 1024 is the first of the one-workgroup scan's second slice; strings of 0 to 3 bytes"""
    n = 1024 * 1024 + 1
    t, v = SC.big_column(np.random.default_rng(31), n, 3, SB_SIZE)
    t[-1] = SC.STRING
    v[-1] = (3 << 32) | (SB_SIZE - 3)  # (the one row of the last chunk ends the buffer)
    total = check_all(ctx, side_stream, "%d rows" % n, t, v, sb, caps=(0, None))
    assert total > n // 2


@pytest.mark.parametrize("length", SC.EDGE_LENGTHS + (SC.LONG,))
def test_lengths_in_every_position(ctx, side_stream, length):
    import torch
    rng = np.random.default_rng(2000 + length)
    host = SC.string_buffer(rng, SC.LONG + 100)
    big = (host, torch.from_numpy(host).to("cuda:0"))
    cases = [c for c in SC.length_cases(rng, host.size) if c[0].startswith("length %d " % length)]
    assert len(cases) == 5
    for name, t, v in cases:
        assert check_all(ctx, side_stream, name, t, v, big) >= length


def test_every_alignment_of_types_bytes_and_sources(ctx, side_stream, sb):
    rng = np.random.default_rng(3000)
    for src_align in range(16):
        t, v = SC.random_column(rng, 150, 40, SB_SIZE, src_align=src_align)
        total = len(SC.reference(t, v, sb[0])[2])
        for bytes_shift in range(16):
            check_all(ctx, side_stream, "sources at %d, bytes at %d" % (src_align, bytes_shift), t, v, sb, caps=(total, total // 2),
                      type_shift=(bytes_shift + 3 * src_align) % 16, bytes_shift=bytes_shift)
    for type_shift in range(16):
        t, v = SC.random_column(rng, 130, 5, SB_SIZE)
        check_all(ctx, side_stream, "types at %d" % type_shift, t, v, sb, caps=(None, 0), type_shift=type_shift, bytes_shift=(5 * type_shift) % 16)


def test_column_shapes(ctx, side_stream, sb):
    for name, t, v in SC.shape_cases(np.random.default_rng(4000), SB_SIZE):
        check_all(ctx, side_stream, name, t, v, sb)


def test_capacities_and_overflow(ctx, side_stream, sb):
    """check() asserts OVERFLOW exactly when total > capacity and the complete offsets at every capacity"""
    t, v = SC.random_column(np.random.default_rng(5000), 700, 30, SB_SIZE)
    total = len(SC.reference(t, v, sb[0])[2])
    mid = int(SC.reference(t, v, sb[0])[0][350]) + 1  # (inside a string, if row 350 has more than one byte; a capacity either way)
    assert check_all(ctx, side_stream, "capacities", t, v, sb, caps=SC.capacities(total) + [mid]) == total


def test_without_validity_and_the_sizing_call(ctx, side_stream, sb):
    t, v = SC.random_column(np.random.default_rng(6000), 321, 12, SB_SIZE)
    check_all(ctx, side_stream, "no validity", t, v, sb, validity=False)
    # capacity 0 with a d_bytes that is not NULL: still nothing is written there
    check_all(ctx, side_stream, "capacity 0, d_bytes given", t, v, sb, caps=(0,), sizing_null=False)


def test_argument_errors(ctx, side_stream, sb):
    import torch
    import simdjson_java_amd as S
    d = torch.ones(64, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    good = dict(d_types=p, d_values=p, n_rows=3, d_sb=sb[1].data_ptr(), d_offsets=p, d_validity=p, d_bytes=p, byte_capacity=8, d_result=p)
    for bad in (dict(d_types=0), dict(d_values=0), dict(d_offsets=0), dict(d_result=0), dict(d_bytes=0), dict(d_values=p + 4), dict(d_offsets=p + 1)):
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.string_column_device(stream=side_stream, **dict(good, **bad))
    ctx.string_column_device(stream=side_stream, **dict(good, d_types=0, d_values=0, n_rows=0, d_bytes=0, byte_capacity=0, d_validity=0))
    torch.cuda.synchronize()
    assert d.cpu().numpy()[:4].tolist() == [0, 0, 0, 0]  # the zero record over offsets[0] = 0 (the same address here)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: BatchShard.step / select / explode / check / string_column on the committed fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _shard(ctx, docs, stream):
    import torch
    from simdjson_java_amd import sharding
    buf, offs = _pack(docs)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.step(stream)
    return shard


def _check_column(shard, t, v, cells, what, stream):
    ref = SC.reference_from_cells(cells)
    offsets, validity, data, result = shard.string_column(t, v, stream=stream)  # sizes itself: one read-back
    import torch
    torch.cuda.synchronize()
    assert data.numel() == len(ref[2]) and offsets.numel() == len(cells) + 1 and validity.numel() == (len(cells) + 63) // 64
    SC.check(what, offsets.cpu().numpy(), validity.cpu().numpy(), data.cpu().numpy(), result.cpu().numpy(), ref, len(ref[2]), canaries=False)
    half = len(ref[2]) // 2
    got = shard.string_column(t, v, byte_capacity=half, stream=stream)
    torch.cuda.synchronize()
    assert got[2].numel() == half
    SC.check(what + ", half", got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), got[3].cpu().numpy(), ref, half, canaries=False)
    return ref[3]


@pytest.mark.parametrize("fixture,pointers,pick", [("twitter.json", SEL.TWITTER_POINTERS, "statuses"), ("github_events.json", SEL.GITHUB_POINTERS, None)],
                         ids=["twitter", "github"])
def test_select_columns_of_the_fixtures(ctx, side_stream, fixture, pointers, pick):
    import torch
    import simdjson_java_amd as S
    docs = SEL.reserialised(fixture, (lambda d: d[pick]) if pick else (lambda d: d))
    docs = docs[:7] + [STAGE2_FAILS] + docs[7:]  # one document that fails stage 2: NULL on every path
    parsed = [O.parse(d) for d in docs]
    assert parsed[7].error and not parsed[6].error
    want = SEL.expected_columns(parsed, pointers)
    shard = _shard(ctx, docs, side_stream)
    plan = S.SelectPlan(pointers)
    types, values = shard.select(plan, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 1
    valid = 0
    for p, ptr in enumerate(pointers):
        valid += _check_column(shard, types[p], values[p], want[p], "%s %r" % (fixture, ptr), side_stream)
    assert valid > 3 * len(docs)
    plan.close()


def test_exploded_user_mentions(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    docs = SEL.reserialised("twitter.json", lambda d: d["statuses"])
    docs = docs[:3] + [STAGE2_FAILS] + docs[3:]
    parsed = [O.parse(d) for d in docs]
    ptrs = ["/screen_name", "/id", "/nope"]
    want_offs, want = EC.expected_explode(parsed, "/entities/user_mentions", ptrs)
    total = want_offs[-1]
    assert total > 64
    shard = _shard(ctx, docs, side_stream)
    plan = S.ExplodePlan("/entities/user_mentions", ptrs)
    for capacity in (total + 9, total - 5):  # the columns cut to the rows present
        _, et, ev = shard.explode(plan, capacity, side_stream)
        torch.cuda.synchronize()
        assert shard.check()["failed_documents"] == 1
        n = min(total, capacity)
        for p in range(len(ptrs)):
            valid = _check_column(shard, et[p][:n], ev[p][:n], want[p][:n], "user_mentions %r, capacity %d" % (ptrs[p], capacity), side_stream)
            assert valid == (n if p == 0 else 0)
    plan.close()
