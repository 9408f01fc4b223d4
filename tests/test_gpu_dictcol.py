"""The dictionary encoder on the GPU (sjmi_dictionary_column_device through Context.dictionary_column_device and
BatchShard.dictionary_column): every index, validity word, dictionary row, offset and byte and the result record against the
Python-dict reference of tests/dictcol_common.py, with canaries in front of and behind everything the call owns -- the indices at
or above the live rows and the dictionary's arrays behind n_distinct among them.  Synthetic columns carry wild value words in
their NULL rows; colliding strings are built on the CPU with the Python restatement of the hash; the end-to-end tests take their
expected values from tests/select_common.py / tests/explode_common.py over the oracle's parse."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import dictcol_common as DC
from tests import explode_common as EC
from tests import filter_common as FC
from tests import select_common as SEL
from tests.test_gpu_batch import _pack

pytestmark = pytest.mark.gpu


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


class Device:
    """one column on the device: the type column and the string buffer are slices of larger tensors (3 and 5 bytes in)"""

    def __init__(self, types, values, sb, type_shift=3, sb_shift=5):
        import torch
        dev = torch.device("cuda", 0)
        self.n = len(types)
        tstore = torch.zeros(self.n + 16, dtype=torch.uint8, device=dev)
        self.types = tstore[type_shift:type_shift + self.n]
        self.types.copy_(torch.from_numpy(np.ascontiguousarray(types, dtype=np.uint8)))
        self.values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint64).view(np.int64)).to(dev)
        sstore = torch.zeros(sb.size + 16, dtype=torch.uint8, device=dev)
        self.sb = sstore[sb_shift:sb_shift + sb.size]
        self.sb.copy_(torch.from_numpy(sb))


def run(ctx, stream, col, dict_capacity, byte_capacity, row_count=None, validity=True, dict_rows=True, bytes_shift=3):
    """one call into a DC.Out on the device -> the Out, read back.  Every store of the Out is ONE device allocation, and
    d_dict_bytes lies `bytes_shift` bytes into its own (the bytes in front of it are the store's front canary)"""
    import torch
    dev = col.values.device
    out = DC.Out(col.n, dict_capacity, byte_capacity, bytes_front=bytes_shift)
    d = {}
    for name in DC.Out.STORES:
        store = getattr(out, name + "_store")
        d[name] = torch.from_numpy(store.view({"indices": np.int32, "dict_bytes": np.uint8}.get(name, np.int64))).to(dev)
    ptr = lambda name: d[name].data_ptr() + out.guard(name) * d[name].element_size()
    # (an allocation begins at a multiple of 256: the copy's destination is misaligned exactly as bytes_shift says)
    assert d["dict_bytes"].data_ptr() % 256 == 0 and ptr("dict_bytes") % 16 == bytes_shift % 16 and (bytes_shift % 8 == 0 or ptr("dict_bytes") % 8 != 0)
    d_rc = None
    if row_count is not None:
        d_rc = row_count if hasattr(row_count, "data_ptr") else torch.tensor([row_count], dtype=torch.int64, device=dev)
    ctx.dictionary_column_device(col.types.data_ptr() if col.n else 0, col.values.data_ptr() if col.n else 0, col.n, d_rc.data_ptr() if d_rc is not None else 0,
                                 col.sb.data_ptr(), ptr("indices"), ptr("validity") if validity else 0, dict_capacity, ptr("dict_rows") if dict_rows else 0,
                                 ptr("dict_offsets"), ptr("dict_bytes") if byte_capacity else 0, byte_capacity, ptr("result"), stream)
    torch.cuda.synchronize()
    for name in DC.Out.STORES:
        store = getattr(out, name + "_store")
        store[:] = d[name].cpu().numpy().view(store.dtype)
    return out


def check_all(ctx, stream, what, types, values, sb, dict_capacity, caps=(None, 0), row_count=None, bytes_shift=3):
    col = Device(types, values, sb)
    ref = DC.reference(types, values, sb, row_count)
    total = len(ref.dict_bytes)
    for k, cap in enumerate(caps):
        cap = total if cap is None else cap
        out = run(ctx, stream, col, dict_capacity, cap, row_count, validity=k % 3 != 2, dict_rows=k % 4 != 3, bytes_shift=bytes_shift)
        DC.check("%s, capacity %d of %d" % (what, cap, total), out, ref, dict_capacity, cap, validity=k % 3 != 2, dict_rows=k % 4 != 3)
    return ref


@pytest.mark.parametrize("n", DC.ROW_COUNTS)
def test_row_counts(ctx, side_stream, n):
    rng = np.random.default_rng(1000 + n)
    t, v, sb = DC.column_of(rng, DC.mixed_cells(rng, n, DC.NINE))
    ref = check_all(ctx, side_stream, "%d rows" % n, t, v, sb, 16)
    assert n < 200 or ref.n_distinct == 9


def test_late_first_occurrences(ctx, side_stream):
    t, v, sb = DC.column_of(np.random.default_rng(2), DC.late_first_cells())
    assert check_all(ctx, side_stream, "late first rows", t, v, sb, 8).dict_rows.tolist() == [1024, 1087, 2048]


@pytest.mark.parametrize("case", range(4), ids=["all_null", "one_value", "empty_string", "all_distinct"])
def test_uniform_columns(ctx, side_stream, case):
    name, cells, capacity = DC.uniform_cases()[case]
    t, v, sb = DC.column_of(np.random.default_rng(3), cells)
    check_all(ctx, side_stream, name, t, v, sb, capacity)


def test_forced_collisions(ctx, side_stream):
    """dict_capacity 32, so 64 slots: chains, a chain that wraps, tag twins (any implementation that lets the tag decide fails
    these), and load 0.5 exactly"""
    rng = np.random.default_rng(4)
    for name, cells, place in DC.collision_cases():
        t, v, sb = DC.column_of(rng, cells, place=place)
        ref = check_all(ctx, side_stream, name, t, v, sb, 32)
        assert ref.n_distinct == len({c for c in cells if c is not None}) <= 32
    a, b = DC.tag_twins(64, 6, True)
    for shift in range(8):  # the twins' second occurrences at every address modulo 8
        t, v, sb = DC.column_of(rng, [a, b, b, a, b], place={2: shift, 3: (shift + 3) % 8})
        col = Device(t, v, sb, sb_shift=0)
        ref = DC.reference(t, v, sb)
        DC.check("twins at %d" % shift, run(ctx, side_stream, col, 32, 12), ref, 32, 12)
        assert ref.indices.tolist() == [0, 1, 1, 0, 1]


def test_overflow(ctx, side_stream):
    rng = np.random.default_rng(5)
    cells = DC.mixed_cells(rng, 300, [b"v%d" % k for k in range(33)], p_null=0.2)
    t, v, sb = DC.column_of(rng, cells)
    assert check_all(ctx, side_stream, "capacity + 1 values", t, v, sb, 32, caps=(None, 0, 50)).n_distinct == 33
    check_all(ctx, side_stream, "exactly the capacity", t, v, sb, 33)
    cells = DC.mixed_cells(rng, 1500, [b"value %d" % k for k in range(40)], p_null=0.1)
    t, v, sb = DC.column_of(rng, cells)
    check_all(ctx, side_stream, "40 values, capacity 2: the table fills", t, v, sb, 2, caps=(None, 9))
    check_all(ctx, side_stream, "capacity 0 with a VALID row", t, v, sb, 0, caps=(0, 9))
    t, v, sb = DC.column_of(rng, [None] * 130)
    assert check_all(ctx, side_stream, "capacity 0 without one", t, v, sb, 0, caps=(0, 9)).n_distinct == 0


def test_byte_capacities_and_the_empty_string(ctx, side_stream):
    rng = np.random.default_rng(6)
    t, v, sb = DC.column_of(rng, DC.mixed_cells(rng, 400, DC.NINE))
    total = len(DC.reference(t, v, sb).dict_bytes)
    # d_dict_bytes 3 bytes into its allocation, as every call of this file has it, and at other odd and even places
    for shift in (3, 1, 5, 7, 8, 11, 14):
        check_all(ctx, side_stream, "byte capacities, d_dict_bytes %d bytes in" % shift, t, v, sb, 9, caps=(0, total - 1, total, total + 7), bytes_shift=shift)
    t, v, sb = DC.column_of(rng, [None, b"", None, b"", b""])
    ref = check_all(ctx, side_stream, "the empty string alone", t, v, sb, 4, caps=(0, 5))
    assert ref.n_distinct == 1 and ref.dict_offsets.tolist() == [0, 0]


def test_live_rows_from_the_device(ctx, side_stream):
    """d_row_count at a filter's n_kept, at 0 and at a value above n_rows; the rows at or above `live` hold strings that would
    add entries"""
    import torch
    import types as pytypes
    import simdjson_java_amd as S
    rng = np.random.default_rng(7)
    cells = DC.mixed_cells(rng, 1100, DC.NINE[:5]) + [b"behind the live rows %d" % k for k in range(300)]
    t, v, sb = DC.column_of(rng, cells)
    for live in (0, 5000, 1100, 1025):
        ref = check_all(ctx, side_stream, "%d live rows" % live, t, v, sb, 512, row_count=live)
        assert ref.live == min(live, 1400) and (live > 1100 or ref.n_distinct <= 5)
    # the filter's own record as the row count: the first 1100 rows where they are strings, compacted into columns of 1400
    # entries whose rows at or above n_kept hold strings of their own
    col = Device(t, v, sb)
    n, dev = col.n, col.values.device
    kept = [r for r in range(1100) if cells[r] is not None]
    plan = S.FilterPlan([(0, "type_eq", DC.STRING)])
    out_types = col.types.clone()
    out_values = col.values.clone()
    rows = torch.zeros(n, dtype=torch.int64, device=dev)
    result = torch.zeros(2, dtype=torch.int64, device=dev)
    ctx.filter_columns_device(plan, col.types.data_ptr(), col.values.data_ptr(), 1, n, 1100, col.sb.data_ptr(), 0, rows.data_ptr(), n,
                              out_types.data_ptr(), out_values.data_ptr(), result.data_ptr(), side_stream)
    compacted = pytypes.SimpleNamespace(n=n, types=out_types, values=out_values, sb=col.sb)
    out = run(ctx, side_stream, compacted, 512, 8192, row_count=result[0:1])  # (queued behind the filter: the first synchronisation is run()'s)
    assert int(result[0]) == len(kept) and len(kept) < 1100
    t2, v2 = out_types.cpu().numpy(), out_values.cpu().numpy().view(np.uint64)
    assert (t2[len(kept):] == DC.STRING).sum() >= 300  # (what lies behind the kept rows would add entries)
    DC.check("behind a filter", out, DC.reference(t2, v2, sb, len(kept)), 512, 8192)
    assert DC.reference(t2, v2, sb, len(kept)).values == DC.reference_from_cells([(DC.STRING, cells[r]) for r in kept]).values
    plan.close()


def test_contention_and_the_second_slice_of_the_scan(ctx, side_stream):
    """1024 * 1024 + 1 rows over 3 values (a million rows on three slots), the last row a fourth, new value, in chunk 1024 -- the
    first of the one-workgroup scan's second slice.  The same call twice: both equal the reference, and so each other."""
    t, v, sb, ref = DC.contention_column(np.random.default_rng(8), 1024 * 1024 + 1)
    col = Device(t, v, sb)
    outs = [run(ctx, side_stream, col, 8, len(ref.dict_bytes)) for _ in range(2)]
    for k, out in enumerate(outs):
        DC.check("a million rows, run %d" % k, out, ref, 8, len(ref.dict_bytes))
    assert all(np.array_equal(getattr(outs[0], s + "_store"), getattr(outs[1], s + "_store")) for s in DC.Out.STORES)


def test_argument_errors(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    d = torch.full((64,), 0x45, dtype=torch.int64, device="cuda:0")
    before = d.cpu().numpy().copy()
    p = d.data_ptr()
    good = dict(d_types=p, d_values=p, n_rows=3, d_row_count=p, d_sb=p, d_indices=p, d_validity=p, dict_capacity=4, d_dict_rows=p, d_dict_offsets=p,
                d_dict_bytes=p, dict_byte_capacity=8, d_result=p)
    for bad in (dict(dict_capacity=DC.MAX_ENTRIES + 1), dict(d_indices=0), dict(d_dict_offsets=0), dict(d_result=0), dict(d_types=0), dict(d_values=0),
                dict(d_sb=0), dict(d_dict_bytes=0), dict(d_values=p + 4), dict(d_row_count=p + 4), dict(d_validity=p + 4), dict(d_dict_rows=p + 4),
                dict(d_dict_offsets=p + 4), dict(d_result=p + 4), dict(d_indices=p + 2), dict(n_rows=1 << 40)):
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.dictionary_column_device(stream=side_stream, **dict(good, **bad))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), before), "an argument error wrote something"
    # the empty column: NULL inputs, the zero record and dict_offsets[0] = 0
    res = torch.full((8,), 0x45, dtype=torch.int64, device="cuda:0")
    ctx.dictionary_column_device(stream=side_stream, **dict(good, d_types=0, d_values=0, d_sb=0, n_rows=0, d_row_count=0, d_validity=0, d_dict_rows=0,
                                                            d_dict_bytes=0, dict_byte_capacity=0, d_dict_offsets=res.data_ptr() + 48, d_result=res.data_ptr()))
    ctx.dictionary_column_device(stream=side_stream, **dict(good, dict_capacity=DC.MAX_ENTRIES, d_types=p + 3, d_dict_rows=0, d_dict_bytes=0,
                                                            dict_byte_capacity=0, d_row_count=res.data_ptr() + 48, d_dict_offsets=d.data_ptr() + 256,
                                                            d_result=d.data_ptr() + 128))  # (live = 0 from the device, the largest table)
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 0x45]
    assert d.cpu().numpy()[16:22].tolist() == [0] * 6 and int(d[32]) == 0 and np.array_equal(d.cpu().numpy()[:16], before[:16])


# ---------------------------------------------------------------------------------------------------------------------
# end to end: BatchShard.step / select / explode / filter / check / dictionary_column on the committed fixtures
# ---------------------------------------------------------------------------------------------------------------------
def _shard(ctx, docs, stream):
    import torch
    from simdjson_java_amd import sharding
    buf, offs = _pack(docs)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.step(stream)
    return shard


def _check_tensors(what, got, ref, n_rows, dict_capacity):
    """what BatchShard.dictionary_column returned (it sized the bytes itself), cut to what the call owns"""
    indices, validity, dict_rows, dict_offsets, dict_bytes, result = [g.cpu().numpy() for g in got]
    assert indices.shape == (n_rows,) and indices.dtype == np.int32 and validity.shape == ((n_rows + 63) // 64,)
    assert dict_rows.shape == (dict_capacity,) and dict_offsets.shape == (dict_capacity + 1,) and dict_bytes.size == len(ref.dict_bytes)
    assert result.tolist() == [ref.live, ref.n_valid, ref.n_other, ref.n_distinct, len(ref.dict_bytes), 0], (what, result.tolist())
    nd = ref.n_distinct
    assert np.array_equal(indices[:ref.live], ref.indices), what
    assert np.array_equal(validity.view(np.uint64)[:(ref.live + 63) // 64], ref.validity), what
    assert np.array_equal(dict_rows[:nd], ref.dict_rows) and np.array_equal(dict_offsets[:nd + 1], ref.dict_offsets), what
    assert bytes(dict_bytes) == ref.dict_bytes, what
    return [bytes(dict_bytes[int(dict_offsets[j]):int(dict_offsets[j + 1])]) for j in range(nd)]


def test_github_events_end_to_end(ctx, side_stream):
    """parse -> select -> dictionary_column for /type and /actor/login, and /type once more behind a filter with its n_kept as
    the row count, queued back to back"""
    import torch
    import simdjson_java_amd as S
    pointers = ["/type", "/actor/login", "/public"]
    docs = SEL.reserialised("github_events.json", lambda d: d)
    docs = docs[:7] + [b'{"type":"PushEvent","arr":[1,2,}'] + docs[7:]  # one document that fails stage 2: NULL on every path
    parsed = [O.parse(d) for d in docs]
    assert parsed[7].error and not parsed[6].error
    want = SEL.expected_columns(parsed, pointers)
    shard = _shard(ctx, docs, side_stream)
    plan = S.SelectPlan(pointers)
    types, values = shard.select(plan, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 1
    for p in (0, 1):
        ref = DC.reference_from_cells(want[p])
        got = shard.dictionary_column(types[p], values[p], 64, stream=side_stream)  # sizes itself: one read-back
        torch.cuda.synchronize()
        entries = _check_tensors(pointers[p], got, ref, len(docs), 64)
        assert entries == ref.values and ref.n_valid == len(docs) - 1
    assert DC.reference_from_cells(want[0]).n_distinct == 7 and DC.reference_from_cells(want[0]).values[0] == b"PushEvent"
    # ... behind a filter: the events whose actor is not the first event's
    terms = [(1, "string_ne", want[1][0][1])]
    keep = FC.reference_from_cells(terms, want, len(docs))
    kept = np.flatnonzero(keep)
    assert 8 < kept.size < len(docs) - 1
    fplan = S.FilterPlan(terms)
    _, ot, ov, _, result = shard.filter(fplan, types, values, stream=side_stream)
    got = shard.dictionary_column(ot[0], ov[0], 16, byte_capacity=4096, row_count=result[0:1], stream=side_stream)
    torch.cuda.synchronize()
    ref = DC.reference_from_cells([want[0][r] for r in kept])
    assert int(result[0]) == kept.size
    got = got[:4] + (got[4][:len(ref.dict_bytes)],) + got[5:]
    _check_tensors("/type of the kept events", got, ref, len(docs), 16)
    fplan.close()
    plan.close()


def test_twitter_statuses_exploded_end_to_end(ctx, side_stream):
    """parse -> explode /statuses -> dictionary_column for /user/lang and /source, cut to the rows present"""
    import torch
    import simdjson_java_amd as S
    from tests.conftest import load_fixture
    docs = [load_fixture("twitter.json")]
    parsed = [O.parse(d) for d in docs]
    ptrs = ["/user/lang", "/source"]
    want_offs, want = EC.expected_explode(parsed, "/statuses", ptrs)
    total = want_offs[-1]
    assert total == 100
    shard = _shard(ctx, docs, side_stream)
    plan = S.ExplodePlan("/statuses", ptrs)
    offs, et, ev = shard.explode(plan, total + 9, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 0
    for p in range(2):
        ref = DC.reference_from_cells(want[p])
        got = shard.dictionary_column(et[p][:total], ev[p][:total], 128, stream=side_stream)
        torch.cuda.synchronize()
        assert _check_tensors(ptrs[p], got, ref, total, 128) == ref.values and 1 < ref.n_distinct < total and ref.n_valid == total
        # ... and uncut, the last row offset read on the device
        got = shard.dictionary_column(et[p], ev[p], 128, byte_capacity=len(ref.dict_bytes), row_count=offs[1:2], stream=side_stream)
        torch.cuda.synchronize()
        _check_tensors(ptrs[p] + ", row count on the device", got, ref, total + 9, 128)
    plan.close()
