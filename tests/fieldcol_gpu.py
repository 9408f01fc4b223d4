"""The GPU harness that tests/test_gpu_arrowcol.py and tests/test_gpu_timecol.py share: the context and the stream of a module,
one call into canaried buffers on the device, the four call forms, a parsed batch for the chained tests and the comparison of
what BatchShard returned.  `common` is the operator's tests/<op>_common.py; a case with a string buffer (case.sb) goes through
Context.time_columns_device, one without through Context.arrow_columns_device.  A test module imports the fixtures by name."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import explode_common as EC
from tests import select_common as SEL
from tests.test_gpu_batch import _pack


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 4 << 20)
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


def run(common, ctx, stream, case, data=True, validity=True, type_shift=0):
    """one call into out_buffers() on the device: the type columns are a slice of a larger tensor, the string buffer (where the
    case has one) is a tensor of exactly its bytes, the output blocks lie FRONT words behind the beginning of theirs; -> the
    whole arrays, canaries included"""
    import torch
    dev = torch.device("cuda", 0)
    n_cols, stride = case.types.shape
    cells = n_cols * stride
    tstore = torch.zeros(cells + 16, dtype=torch.uint8, device=dev)
    d_types = tstore[type_shift:type_shift + cells]
    d_types.copy_(torch.from_numpy(case.types.reshape(-1)))
    d_values = torch.from_numpy(case.values.view(np.int64).reshape(-1)).to(dev)
    d_sb = torch.from_numpy(case.sb).to(dev) if hasattr(case, "sb") else None
    d, b, res = common.out_buffers(case, data, validity)
    d_data = torch.from_numpy(d.view(np.int64)).to(dev) if data else None
    d_valid = torch.from_numpy(b.view(np.int64)).to(dev) if validity else None
    d_res = torch.from_numpy(res.view(np.int64)).to(dev)
    d_rc = torch.tensor([case.row_count], dtype=torch.int64, device=dev) if case.row_count is not None else None
    call, strings = (ctx.arrow_columns_device, ()) if d_sb is None else (ctx.time_columns_device, (d_sb.data_ptr(),))
    call(case.fields, d_types.data_ptr() if cells else 0, d_values.data_ptr() if cells else 0, n_cols, stride, case.n_rows,
         d_rc.data_ptr() if d_rc is not None else 0, *strings, d_data.data_ptr() + 8 * common.FRONT if data else 0, case.data_stride if data else 0,
         d_valid.data_ptr() + 8 * common.FRONT if validity else 0, case.validity_stride, d_res.data_ptr(), stream)
    torch.cuda.synchronize()
    return d_data.cpu().numpy() if data else None, d_valid.cpu().numpy() if validity else None, d_res.cpu().numpy()


FORMS = ((True, True), (True, False), (False, True), (False, False))  # both blocks, no validity, the counting call, records only


def check_all(common, ctx, stream, case, forms=FORMS, shift=1, ref=None):
    ref = common.reference(case) if ref is None else ref
    for k, (data, validity) in enumerate(forms):
        got = run(common, ctx, stream, case, data, validity, type_shift=(5 * k + shift) % 16)
        common.check("%s, data %s, validity %s" % (case.name, data, validity), *got, case, ref)
    return ref


@pytest.fixture(scope="module")
def parsed_batch(request, ctx, side_stream):
    """300 documents of the test module's _document(), one of which (its FAILS) fails, stepped, selected by its POINTERS, exploded
    by its ELEMENT_POINTERS and accepted by check(); the expected cells of both"""
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    m = request.module
    docs = [m._document(i) for i in range(300)]
    docs = docs[:17] + [m.FAILS] + docs[17:]
    parsed = [O.parse(d) for d in docs]
    assert parsed[17].error and sum(bool(p.error) for p in parsed) == 1
    want = SEL.expected_columns(parsed, m.POINTERS)
    want_offs, want_rows = EC.expected_explode(parsed, "/arr", m.ELEMENT_POINTERS)
    buf, offs = _pack(docs)
    shard = sharding.BatchShard(ctx, buf, offs, torch.device("cuda", 0))
    shard.step(side_stream)
    sel, exp = S.SelectPlan(m.POINTERS), S.ExplodePlan("/arr", m.ELEMENT_POINTERS)
    capacity = want_offs[-1] + 9
    shard.select(sel, side_stream)
    shard.explode(exp, capacity, side_stream)
    torch.cuda.synchronize()
    assert shard.check()["failed_documents"] == 1
    yield shard, sel, exp, capacity, len(docs), want, want_offs, want_rows
    sel.close()
    exp.close()


def _check_tensors(what, fields, data, validity, results, ref, n_rows):
    """what BatchShard.arrow_columns / timestamp_columns returned, cut to what the call owns, against the reference"""
    data, validity, results = data.cpu().numpy().view(np.uint64), validity.cpu().numpy().view(np.uint64), results.cpu().numpy().view(np.uint64)
    assert data.shape == (len(fields), n_rows) and validity.shape == (len(fields), (n_rows + 63) // 64) and results.shape == (len(fields), len(ref.records[0]))
    assert [tuple(r) for r in results.tolist()] == ref.records, (what, results.tolist(), ref.records)
    for f in range(len(fields)):
        assert data[f, :len(ref.data[f])].tolist() == ref.data[f], "%s: the data of field %d differ" % (what, f)
        assert validity[f, :len(ref.validity[f])].tolist() == ref.validity[f], "%s: the validity of field %d differs" % (what, f)
