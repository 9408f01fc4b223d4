"""The timestamp column export on the GPU (sjmi_time_columns_device through Context.time_columns_device and
BatchShard.timestamp_columns): every data word, validity word and record against the Python reference of tests/timecol_common.py,
and canaries in front of, between and behind everything the call owns.  Synthetic column sets carry wild value words in every
cell whose value must not matter, string cells of impossible lengths that point at and past the end of the string buffer, and
strings that end with the buffer's last byte; the chained and end-to-end tests take their expected cells from
tests/select_common.py and tests/explode_common.py over the oracle's parse."""
import functools

import numpy as np
import pytest

from tests import fieldcol_gpu as G
from tests import filter_common as FC
from tests import select_common as SEL
from tests import timecol_common as TC
from tests.fieldcol_gpu import FORMS, _check_tensors, ctx, parsed_batch, side_stream  # (the fixtures: by name)

pytestmark = pytest.mark.gpu


run, check_all = functools.partial(G.run, TC), functools.partial(G.check_all, TC)


def test_named_strings(ctx, side_stream):
    case = TC.named_case()
    ref = check_all(ctx, side_stream, case)
    rec = dict(zip(case.fields, ref.records))
    assert rec[(0, "ns")][4] == 8 and rec[(0, "us")][4] == 0 and rec[(0, "s", "naive_utc")][1] > rec[(0, "s")][1] > 40
    assert rec[(0, "s")][5] > rec[(0, "ms")][5] > rec[(0, "us")][5] > rec[(0, "ns")][5] == 0
    # the edges, read from the device's own words: INT64_MAX, NULL, INT64_MIN, NULL at NANO; the floor below the epoch at SECOND
    got = run(ctx, side_stream, case)[0].view(np.uint64)[TC.FRONT:].reshape(-1)
    ns, s = case.fields.index((0, "ns")) * case.data_stride, case.fields.index((0, "s")) * case.data_stride
    assert got[ns:ns + 4].tolist() == [TC.INT64_MAX, 0, TC.INT64_MIN & TC.MASK, 0]
    assert int(got[s + TC.NAMED.index(b"1969-12-31T23:59:59.5Z")]) == TC.MASK  # -1


def test_every_position_replaced(ctx, side_stream):
    ref = check_all(ctx, side_stream, TC.replaced_case(), forms=FORMS[:2])
    assert ref.records[0] == (105, 3, 0, 102, 0, 0) and ref.records[1] == (105, 3, 0, 102, 0, 3)


def test_every_type_under_the_field(ctx, side_stream):
    case = TC.type_table_case()
    ref = check_all(ctx, side_stream, case)
    assert ref.records[0] == (case.n_rows, 2, case.n_rows - 5, 1, 0, 1)


def test_the_last_bytes_of_the_string_buffer(ctx, side_stream):
    for case in TC.last_bytes_case():
        ref = check_all(ctx, side_stream, case, forms=FORMS[:1])
        assert ref.records[1][1] >= 3 and ref.records[1][3] >= 7


@pytest.mark.parametrize("n", TC.ROW_COUNTS)
def test_row_counts_and_live_counts(ctx, side_stream, n):
    valid = 0
    for case in TC.row_count_cases(n):
        valid += sum(r[1] for r in check_all(ctx, side_stream, case, forms=FORMS if n <= 256 else (FORMS[0], FORMS[3]), shift=n % 16).records)
    assert n < 63 or valid > n


def test_the_types_at_every_shift(ctx, side_stream):
    case = TC.type_shift_case()
    ref = TC.reference(case)
    for shift in range(16):
        TC.check("shift %d" % shift, *run(ctx, side_stream, case, type_shift=shift), case, ref)


def test_schemas(ctx, side_stream):
    for case in TC.schema_cases():
        ref = check_all(ctx, side_stream, case, forms=(FORMS[0], FORMS[2]))
        assert any(0 < r[1] < r[0] for r in ref.records), case.name


def test_fuzz(ctx, side_stream):
    for seed in list(TC.FUZZ_SEEDS)[:40]:
        case = TC.fuzz_case(seed)
        check_all(ctx, side_stream, case, forms=FORMS[:1] if seed % 4 else FORMS, shift=seed % 16)


def test_past_one_grid_trip(ctx, side_stream):
    """2 fields x 70,001 rows, without and with a row count that ends inside a chunk near the end"""
    case = TC.past_one_grid_trip_case()
    ref = check_all(ctx, side_stream, case, forms=FORMS[:1])
    assert all(0 < r[1] < r[0] and r[2] > 0 and r[3] > 0 for r in ref.records) and ref.records[1][4] > 0 and ref.records[0][5] > 0
    cut = case._replace(name=case.name + ", cut", row_count=68 * 1024 - 30)
    check_all(ctx, side_stream, cut, forms=(FORMS[0], FORMS[3]))


def test_argument_errors(ctx, side_stream):
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import binding
    d = torch.ones(64, dtype=torch.int64, device="cuda:0")
    d_res = torch.full((12,), -1, dtype=torch.int64, device="cuda:0")
    p = d.data_ptr()
    raw = lambda **kw: np.array([tuple(dict(dict(column=0, unit=2, flags=0, reserved=0), **kw).values())], dtype=binding.TIME_FIELD)
    good = dict(fields=[(1, "us"), (0, "ns", "naive_utc")], d_types=p, d_values=p, n_cols=2, col_stride=4, n_rows=3, d_row_count=p, d_sb=p, d_data=p,
                data_stride=3, d_validity=p, validity_stride=1, d_results=d_res.data_ptr())
    for bad in (dict(fields=[]), dict(fields=[(0, "s")] * 65), dict(fields=[(2, "us")]), dict(fields=raw(unit=4)), dict(fields=raw(unit=1 << 31)),
                dict(fields=raw(flags=2)), dict(fields=raw(flags=3)), dict(fields=raw(reserved=1)), dict(col_stride=2), dict(data_stride=2),
                dict(d_data=0), dict(d_data=0, data_stride=0, validity_stride=0), dict(d_results=0), dict(d_types=0), dict(d_values=0), dict(d_sb=0),
                dict(d_values=p + 4), dict(d_row_count=p + 4), dict(d_data=p + 4), dict(d_validity=p + 2), dict(d_results=p + 4),
                dict(n_rows=1 << 40, col_stride=1 << 40, data_stride=1 << 40, validity_stride=1 << 34)):
        with pytest.raises(S.SjmiError, match=r"rc=-2"):
            ctx.time_columns_device(stream=side_stream, **dict(good, **bad))
    with pytest.raises(ValueError):
        binding.time_fields([(0, "minutes")])
    with pytest.raises(ValueError):
        binding.time_fields([(0, "us", "local")])
    assert binding.time_fields([(0, "us"), (2, "ns", "naive_utc")]).tolist() == [(0, 2, 0, 0), (2, 3, 1, 0)]
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [-1] * 12 and d.cpu().tolist() == [1] * 64  # nothing was launched
    # legal: no rows with NULL columns and no string buffer; odd type pointers; the counting call without validity; a row count of 0
    ctx.time_columns_device(stream=side_stream, **dict(good, d_types=0, d_values=0, d_sb=0, n_rows=0, col_stride=0, d_row_count=0, d_data=0, data_stride=0,
                                                        d_validity=0, validity_stride=0))
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [0] * 12
    zero = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    d_res.fill_(-1)
    ctx.time_columns_device(stream=side_stream, **dict(good, d_types=p + 3, d_row_count=zero.data_ptr()))
    torch.cuda.synchronize()
    assert d_res.cpu().tolist() == [0] * 12 and d.cpu().tolist() == [1] * 64


# ---------------------------------------------------------------------------------------------------------------------
# chained on the device and end to end: BatchShard.step / select / explode / check / filter / timestamp_columns
# ---------------------------------------------------------------------------------------------------------------------
POINTERS = ["/created_at", "/updated", "/id"]
ELEMENT_POINTERS = ["/at", "/n"]
FAILS = b'{"created_at":"2015-01-01T15:00:00Z","arr":[1,2,}'
SELECT_FIELDS = [(0, "us"), (0, "s"), (1, "ns", "naive_utc"), (1, "ms"), (2, "us")]
ELEMENT_FIELDS = [(0, "s", "naive_utc"), (0, "ns"), (1, "ms")]


def _document(i):
    """ISO strings of every shape -- escaped ones among them: the parser sees unescaped bytes --, malformed ones, numbers and
    nulls where a time is expected, missing keys"""
    stamp = b"20%02d-%02d-%02dT%02d:%02d:%02d" % (i % 100, i % 12 + 1, i % 28 + 1, i % 24, i % 60, (7 * i) % 60)
    created = (b'"%sZ"' % stamp, b'"%s\\u005a"' % stamp, b'"%s.%03d+05:30"' % (stamp, i % 1000), b'"%s"' % stamp.replace(b"T", b" "), b"null",
               b'"%s\\u002d08:00"' % stamp, b"%d" % (1420124400 + i), b'"2015-02-30T00:00:00Z"', b'"%s.%09dZ"' % (stamp, i * 1000003 % 1000000000),
               b'"1969-12-31T23:59:59.%dZ"' % (i % 10), b'"\\u0032015-01-01t00:00:00z"')[i % 11]
    members = []
    if i % 13 != 7:
        members.append(b'"created_at":' + created)
    members.append(b'"updated":' + (b'"%s.%06d"' % (stamp, i), b'"%s-00:00"' % stamp, b'"2262-04-11T23:47:16.854775808Z"', b"true", b'"%sZ"' % stamp[:16])[i % 5])
    members.append(b'"id":%d' % i)
    elems = [b'{"at":%s,"n":%d}' % ((b'"%s.%d"' % (stamp, j), b'"%sz"' % stamp, b"null", b'"%s+24:00"' % stamp, b"1.5")[(i + j) % 5], j) for j in range(i % 4)]
    if i % 6:
        members.append(b'"arr":[%s]' % b",".join(elems + ([b"{}"] if i % 5 == 0 else [])))
    return b"{%s}" % b",".join(members)


def test_selected_documents_end_to_end(ctx, side_stream, parsed_batch):
    """parse -> select -> timestamp_columns against the reference over the oracle's parse"""
    import torch
    shard, sel, _, _, n_docs, want, _, _ = parsed_batch
    SEL.check_columns(shard.sel_types.cpu().numpy(), shard.sel_values.cpu().numpy(), shard.sb.cpu().numpy(), want, "selected")
    ref = TC.reference_from_cells(SELECT_FIELDS, want, n_docs)
    # the documents are made so that every count of the records is exercised, by the reference
    us, s, ns_naive, ms, ids = ref.records
    assert 150 < us[1] < n_docs and us[2] > 20 and us[3] > 20 and us[5] > 0 and s[5] > us[5] and ns_naive[4] > 0 and ms[3] > ns_naive[3] > 0 and ms[1] > 0
    assert ids == (n_docs, 0, n_docs - 1, 0, 0, 0)
    escaped = [r for r in range(n_docs) if want[0][r][0] == TC.STRING and want[0][r][1].startswith(b"2015-01-01t00")]
    assert escaped and all(ref.validity[0][r >> 6] >> (r & 63) & 1 for r in escaped)  # (the 2 came out as '2')
    got = shard.timestamp_columns(SELECT_FIELDS, shard.sel_types, shard.sel_values, stream=side_stream)
    torch.cuda.synchronize()
    _check_tensors("selected", SELECT_FIELDS, *got, ref, n_docs)
    assert int(got[0][1, 0]) == TC.string_value(b"2000-01-01T00:00:00Z", "s", False)[0]  # document 0, at SECOND


def test_filter_result_chains_the_row_count_on_the_device(ctx, side_stream, parsed_batch):
    """select -> filter -> timestamp_columns(row_count = the filter's n_kept) queued back to back: ONE synchronisation, at the end"""
    import torch
    import simdjson_java_amd as S
    shard, sel, _, _, n_docs, want, _, _ = parsed_batch
    terms = [(0, "type_eq", TC.STRING), (1, "type_ne", TC.TRUE)]
    keep = FC.reference_from_cells(terms, want, n_docs)
    kept = np.flatnonzero(keep)
    assert 64 < kept.size < n_docs - 64 and not keep[17]
    plan = S.FilterPlan(terms)
    types, values = shard.select(sel, side_stream)
    _, ot, ov, _, result = shard.filter(plan, types, values, stream=side_stream)
    got = shard.timestamp_columns(SELECT_FIELDS, ot, ov, row_count=result[0:1], stream=side_stream)
    torch.cuda.synchronize()
    assert result.cpu().tolist() == [kept.size, 0]
    ref = TC.reference_from_cells(SELECT_FIELDS, [[col[r] for r in kept] for col in want], kept.size)
    assert ref.records[0][2] == 0 and 0 < ref.records[0][3] < kept.size
    _check_tensors("filtered", SELECT_FIELDS, *got, ref, n_docs)
    plan.close()


def test_explode_offsets_chain_the_row_count_on_the_device(ctx, side_stream, parsed_batch):
    """explode -> timestamp_columns(row_count = the last row offset) queued back to back: ONE synchronisation, at the end"""
    import torch
    shard, _, exp, capacity, n_docs, _, want_offs, want_rows = parsed_batch
    total = want_offs[-1]
    assert total > 128
    offs, et, ev = shard.explode(exp, capacity, side_stream)
    got = shard.timestamp_columns(ELEMENT_FIELDS, et, ev, row_count=offs[n_docs:n_docs + 1], stream=side_stream)
    torch.cuda.synchronize()
    assert int(offs[n_docs]) == total
    ref = TC.reference_from_cells(ELEMENT_FIELDS, want_rows, total)
    naive, ns, n = ref.records
    assert naive[1] > ns[1] > 0 and naive[2] > 0 and naive[3] > 0 and naive[5] > 0 and n[1] == 0 and n[2] > 0
    _check_tensors("exploded", ELEMENT_FIELDS, *got, ref, capacity)
