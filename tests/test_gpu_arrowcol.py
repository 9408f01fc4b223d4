"""The Arrow column export on the GPU (sjmi_arrow_columns_device through Context.arrow_columns_device and BatchShard.arrow_columns):
every data word, validity word and record against the Python reference of tests/arrowcol_common.py, and canaries in front of,
between and behind everything the call owns.  Synthetic column sets carry wild value words in every cell whose value must not
matter; the chained and end-to-end tests take their expected cells from tests/select_common.py and tests/explode_common.py over
the oracle's parse."""
import functools

import numpy as np
import pytest

from tests import arrowcol_common as AC
from tests import fieldcol_gpu as G
from tests import filter_common as FC
from tests import select_common as SEL
from tests.fieldcol_gpu import FORMS, _check_tensors, ctx, parsed_batch, side_stream  # (the fixtures: by name)

pytestmark = pytest.mark.gpu


run, check_all = functools.partial(G.run, AC), functools.partial(G.check_all, AC)


@pytest.mark.parametrize("n", AC.ROW_COUNTS)
def test_row_counts_and_live_counts(ctx, side_stream, n):
    valid = 0
    for case in AC.row_count_cases(n):
        valid += sum(r[1] for r in check_all(ctx, side_stream, case, shift=n % 16).records)
    assert n < 63 or valid > n


def test_the_types_at_every_shift(ctx, side_stream):
    case = AC.type_shift_case()
    ref = AC.reference(case)
    for shift in range(16):
        AC.check("shift %d" % shift, *run(ctx, side_stream, case, type_shift=shift), case, ref)


def test_every_kind_on_a_cell_of_every_type(ctx, side_stream):
    case = AC.kind_table_case()
    ref = check_all(ctx, side_stream, case)
    assert [r[1] for r in ref.records] == [4, 7, 9, 6]


def test_numeric_edges(ctx, side_stream):
    case = AC.numeric_edge_case()
    ref = check_all(ctx, side_stream, case)
    assert ref.records[2][3] == 5 and ref.records[4][1] == 7


def test_schemas(ctx, side_stream):
    for case in AC.schema_cases():
        ref = check_all(ctx, side_stream, case)
        assert any(0 < r[1] < r[0] for r in ref.records), case.name


def test_fuzz(ctx, side_stream):
    for seed in list(AC.FUZZ_SEEDS)[:40]:
        case = AC.fuzz_case(seed)
        check_all(ctx, side_stream, case, forms=FORMS[:1] if seed % 4 else FORMS, shift=seed % 16)


def test_past_one_grid_trip(ctx, side_stream):
    """3 fields x 70,001 rows, without and with a row count that ends inside the last but one chunk"""
    case = AC.past_one_grid_trip_case()
    ref = check_all(ctx, side_stream, case, forms=FORMS[:1])
    assert all(0 < r[1] < r[0] for r in ref.records) and ref.records[1][3] > 0
    cut = case._replace(name=case.name + ", cut", row_count=68 * 1024 - 30)
    check_all(ctx, side_stream, cut, forms=(FORMS[0], FORMS[3]))


def test_argument_errors(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import binding
    d = torch.ones(64, dtype=torch.int64, device="cuda:0")
    d_res = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    raw = lambda **kw: np.array([tuple(dict(dict(column=0, kind=1, flags=0, reserved=0), **kw).values())], dtype=binding.ARROW_FIELD)
    good = dict(fields=[(1, "int64"), (0, "bool")], d_types=p, d_values=p, n_cols=2, col_stride=4, n_rows=3, d_row_count=p, d_data=p, data_stride=3,
                d_validity=p, validity_stride=1, d_results=d_res.data_ptr())
    for bad in (dict(fields=[]), dict(fields=[(0, "bool")] * 65), dict(fields=[(2, "int64")]), dict(fields=raw(kind=0)), dict(fields=raw(kind=4)),
                dict(fields=raw(kind=2, flags=1)), dict(fields=raw(kind=3, flags=1)), dict(fields=raw(flags=2)), dict(fields=raw(reserved=1)),
                dict(col_stride=2), dict(data_stride=2), dict(d_data=0), dict(d_data=0, data_stride=0, validity_stride=0), dict(d_results=0),
                dict(d_types=0), dict(d_values=0), dict(d_values=p + 4), dict(d_row_count=p + 4), dict(d_data=p + 4), dict(d_validity=p + 2),
                dict(d_results=p + 4), dict(n_rows=1 << 40, col_stride=1 << 40, data_stride=1 << 40, validity_stride=1 << 34)):
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.arrow_columns_device(stream=side_stream, **dict(good, **bad))
    with pytest.raises(ValueError):
        binding.arrow_fields([(0, "int32")])
    with pytest.raises(ValueError):
        binding.arrow_fields([(0, "bool", "lossy")])
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [-1] * 8 and d.cpu().tolist() == [1] * 64  # nothing was launched
    # legal: no rows with NULL columns; odd type pointers; the counting call without validity; a row count of 0
    ctx.arrow_columns_device(stream=side_stream, **dict(good, d_types=0, d_values=0, n_rows=0, col_stride=0, d_row_count=0, d_data=0, data_stride=0,
                                                         d_validity=0, validity_stride=0))
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [0] * 8
    zero = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_res.fill_(-1)
    ctx.arrow_columns_device(stream=side_stream, **dict(good, d_types=p + 3, d_row_count=zero.data_ptr()))
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [0] * 8 and d.cpu().tolist() == [1] * 64


# ---------------------------------------------------------------------------------------------------------------------
# chained on the device and end to end: BatchShard.step / select / explode / check / filter / arrow_columns
# ---------------------------------------------------------------------------------------------------------------------
POINTERS = ["/id", "/x", "/ok", "/s"]
ELEMENT_POINTERS = ["/v", "/b"]
FAILS = b'{"id":1,"x":2,"arr":[1,2,}'
SELECT_FIELDS = [(0, "int64"), (0, "float64"), (1, "int64", "integral_doubles"), (1, "float64"), (1, "int64"), (2, "bool"), (3, "bool")]
ELEMENT_FIELDS = [(0, "float64"), (0, "int64", "integral_doubles"), (1, "bool")]


def _document(i):
    """ints above 2^53, 1.0-style doubles, booleans, nulls, missing keys and strings where numbers are expected"""
    members = []
    if i % 7 != 3:
        members.append(b'"id":%d' % ((1 << 53) + i if i % 3 == 0 else -i * 1009 if i % 3 == 1 else i))
    x = (b"%d.0" % i, b"%d.5" % i, b"%d" % (i * 7), b'"%d"' % i, b"null", b"-0.0", b"9223372036854775808.0", b"1e3")[i % 8]
    if i % 11 != 5:
        members.append(b'"x":' + x)
    members.append(b'"ok":' + (b"true", b"false", b"null", b"1", b'"true"')[i % 5])
    members.append(b'"s":"t%d"' % i)
    elems = [b'{"v":%s,"b":%s}' % ((b"%d" % ((1 << 60) + j), b"%d.0" % j, b"2.25", b"null", b'"v"')[(i + j) % 5], (b"true", b"false", b"null", b"0")[(i + 2 * j) % 4])
             for j in range(i % 4)]
    if i % 6:
        members.append(b'"arr":[%s]' % b",".join(elems + ([b"{}"] if i % 5 == 0 else [])))
    return b"{%s}" % b",".join(members)


def test_selected_documents_end_to_end(ctx, side_stream, parsed_batch):
    import torch
    shard, sel, _, _, n_docs, want, _, _ = parsed_batch
    SEL.check_columns(shard.sel_types.cpu().numpy(), shard.sel_values.cpu().numpy(), shard.sb.cpu().numpy(), want, "selected")
    ref = AC.reference_from_cells(SELECT_FIELDS, want, n_docs)
    # the documents are made so that every count of the records is exercised, by the reference
    assert ref.records[0][1] < n_docs and ref.records[1][3] > 20 and ref.records[2][1] > ref.records[4][1] > 0 and ref.records[2][2] > 0
    assert 0 < ref.records[5][1] < n_docs and ref.records[5][2] > 0 and ref.records[6] == (n_docs, 0, n_docs - 1, 0)
    got = shard.arrow_columns(SELECT_FIELDS, shard.sel_types, shard.sel_values, stream=side_stream)
    torch.cuda.synchronize()
    _check_tensors("selected", SELECT_FIELDS, *got, ref, n_docs)
    ids = got[0][1].view(torch.float64).cpu().numpy()  # a float64 field's row is read as doubles
    assert ids[0] == float(1 << 53) and ids[1] == -1009.0


def test_filter_result_chains_the_row_count_on_the_device(ctx, side_stream, parsed_batch):
    """select -> filter -> arrow_columns(row_count = the filter's n_kept) queued back to back: ONE synchronisation, at the end"""
    import torch
    import simdjson_java_amd as S
    shard, sel, _, _, n_docs, want, _, _ = parsed_batch
    terms = [(0, "type_eq", AC.LONG), (2, "type_ne", AC.NULL)]
    keep = FC.reference_from_cells(terms, want, n_docs)
    kept = np.flatnonzero(keep)
    assert 64 < kept.size < n_docs - 64 and not keep[17]
    plan = S.FilterPlan(terms)
    types, values = shard.select(sel, side_stream)
    _, ot, ov, _, result = shard.filter(plan, types, values, stream=side_stream)
    got = shard.arrow_columns(SELECT_FIELDS, ot, ov, row_count=result[0:1], stream=side_stream)
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [kept.size, 0]
    ref = AC.reference_from_cells(SELECT_FIELDS, [[col[r] for r in kept] for col in want], kept.size)
    _check_tensors("filtered", SELECT_FIELDS, *got, ref, n_docs)
    plan.close()


def test_explode_offsets_chain_the_row_count_on_the_device(ctx, side_stream, parsed_batch):
    """explode -> arrow_columns(row_count = the last row offset) queued back to back: ONE synchronisation, at the end"""
    import torch
    shard, _, exp, capacity, n_docs, _, want_offs, want_rows = parsed_batch
    total = want_offs[-1]
    assert total > 128
    offs, et, ev = shard.explode(exp, capacity, side_stream)
    got = shard.arrow_columns(ELEMENT_FIELDS, et, ev, row_count=offs[n_docs:n_docs + 1], stream=side_stream)
    torch.cuda.synchronize()
    assert int(offs[n_docs]) == total
    ref = AC.reference_from_cells(ELEMENT_FIELDS, want_rows, total)
    assert ref.records[0][3] > 0 and ref.records[0][2] > 0 and ref.records[1][1] < ref.records[0][1] and 0 < ref.records[2][1] < total
    _check_tensors("exploded", ELEMENT_FIELDS, *got, ref, capacity)
