"""What BatchShard's operator methods hand the engine (sharding.py): for every entry point the scalars, and for every pointer whether
it is NULL or which of the method's tensors it addresses -- in particular NULL for every tensor that has no entries, whatever its
own pointer is.  CPU test with a recording stub in place of binding.Context; the expected calls are literals."""
import ctypes as C

import numpy as np
import pytest
import torch

CPU = torch.device("cpu")


class _Plan:
    n_paths = 2


class _Engine:
    """Records every call as it arrives.  Where the method reads a record back, writes the words it needs: `sizes` = the byte
    counts the sizing calls report, in call order; `ndjson` = (n_docs, consumed, flags, offsets)."""

    def __init__(self, sizes=(), ndjson=None):
        self.calls, self.sizes, self.ndjson = [], list(sizes), ndjson

    def _entry(name, size_word=None, d_result=None):
        def f(self, *args):
            self.calls.append((name,) + args)
            if size_word is not None and not args[d_result - 1] and self.sizes:  # (a sizing call: capacity 0 in front of the record)
                (C.c_int64 * (size_word + 1)).from_address(args[d_result])[size_word] = self.sizes.pop(0)
        return f

    select_batch_device = _entry("select_batch_device")
    explode_batch_device = _entry("explode_batch_device")
    string_column_device = _entry("string_column_device", 0, 8)
    filter_columns_device = _entry("filter_columns_device")
    arrow_columns_device = _entry("arrow_columns_device")
    time_columns_device = _entry("time_columns_device")
    dictionary_column_device = _entry("dictionary_column_device", 4, 12)

    def ndjson_offsets_device(self, d_buf, length, d_doc_offsets, offset_capacity, d_result, stream=0):
        self.calls.append(("ndjson_offsets_device", d_buf, length, d_doc_offsets, offset_capacity, d_result, stream))
        n_docs, consumed, flags, offsets = self.ndjson
        (C.c_int64 * 3).from_address(d_result)[:] = [n_docs, consumed, flags]
        (C.c_int64 * len(offsets)).from_address(d_doc_offsets)[:] = offsets


def _shard(engine, n_docs):
    from simdjson_java_amd import sharding
    docs = [b'{"a":%d}\n' % k for k in range(n_docs)]
    offs = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    data = b"".join(docs)  # (a shard without bytes is made from a tensor, as from_ndjson makes it)
    return sharding.BatchShard(engine, data if data else torch.zeros(0, dtype=torch.uint8), offs, CPU)


def _named(engine, shard, **tensors):
    """The recorded calls with every pointer replaced by the name of the tensor it addresses (the shard's own, or one of
    `tensors`), objects by their names in `tensors`; a pointer to anything else is "other", NULL stays 0."""
    for name in ("tape", "tape_offsets", "doc_errors", "sb", "offs"):
        tensors[name] = getattr(shard, name)
    names, objects = {}, {}
    for name, t in tensors.items():
        if not torch.is_tensor(t):
            objects[id(t)] = name
        elif t.data_ptr():
            assert t.data_ptr() not in names, "two of the method's tensors share an address"
            names[t.data_ptr()] = name
    out = []
    for call in engine.calls:
        row = []
        for a in call:
            if isinstance(a, int) and not isinstance(a, bool):
                row.append(names.get(a, "other" if a >= 1 << 32 else a))
            else:
                row.append(objects.get(id(a), a))
        out.append(tuple(row))
    return out


def _pair_1d(n_rows):
    return torch.zeros(n_rows, dtype=torch.uint8), torch.zeros(n_rows, dtype=torch.int64)


def _pair_2d(stride=8):
    return torch.zeros((2, stride), dtype=torch.uint8), torch.zeros((2, stride), dtype=torch.int64)


@pytest.mark.parametrize("n_docs,expected", [
    (0, [("select_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 0, 0, 0, 7)]),
    (5, [("select_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 5, "sel_types", "sel_values", 7)]),
])
def test_select(n_docs, expected):
    eng, plan = _Engine(), _Plan()
    sh = _shard(eng, n_docs)
    types, values = sh.select(plan, stream=7)
    assert types is sh.sel_types and values is sh.sel_values
    assert types.shape == values.shape == (2, n_docs) and types.dtype == torch.uint8 and values.dtype == torch.int64
    assert _named(eng, sh, plan=plan, sel_types=types, sel_values=values) == expected
    assert sh.select(plan)[0] is types and sh.select(_Plan())[0] is not types  # (allocated once per plan)


@pytest.mark.parametrize("n_docs,row_capacity,expected", [
    (0, 0, [("explode_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 0, "exp_row_offsets", 0, 0, 0, 7)]),
    (0, 6, [("explode_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 0, "exp_row_offsets", 6, "exp_types", "exp_values", 7)]),
    (5, 0, [("explode_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 5, "exp_row_offsets", 0, 0, 0, 7)]),
    (5, 6, [("explode_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 5, "exp_row_offsets", 6, "exp_types", "exp_values", 7)]),
])
def test_explode(n_docs, row_capacity, expected):
    eng, plan = _Engine(), _Plan()
    sh = _shard(eng, n_docs)
    row_offsets, types, values = sh.explode(plan, row_capacity, stream=7)
    assert row_offsets.shape == (n_docs + 1,) and types.shape == values.shape == (2, row_capacity)
    assert _named(eng, sh, plan=plan, exp_row_offsets=row_offsets, exp_types=types, exp_values=values) == expected
    assert sh.explode(plan, row_capacity)[1] is types and sh.explode(plan, row_capacity + 1)[1] is not types


@pytest.mark.parametrize("n_rows,byte_capacity,sizes,expected", [
    # byte_capacity=None: the sizing call, then the second one with what the record said -- or none for an empty column
    (0, None, [0], [("string_column_device", 0, 0, 0, "sb", "offsets", 0, 0, 0, "result", 7)]),
    (5, None, [0], [("string_column_device", "types", "values", 5, "sb", "offsets", "validity", 0, 0, "result", 7)]),
    (5, None, [9], [("string_column_device", "types", "values", 5, "sb", "offsets", "validity", 0, 0, "result", 7),
                    ("string_column_device", "types", "values", 5, "sb", "offsets", "validity", "data", 9, "result", 7)]),
    (0, None, [9], [("string_column_device", 0, 0, 0, "sb", "offsets", 0, 0, 0, "result", 7),
                    ("string_column_device", 0, 0, 0, "sb", "offsets", 0, "data", 9, "result", 7)]),
    (0, 0, [], [("string_column_device", 0, 0, 0, "sb", "offsets", 0, 0, 0, "result", 7)]),
    (5, 0, [], [("string_column_device", "types", "values", 5, "sb", "offsets", "validity", 0, 0, "result", 7)]),
    (0, 16, [], [("string_column_device", 0, 0, 0, "sb", "offsets", 0, "data", 16, "result", 7)]),
    (5, 16, [], [("string_column_device", "types", "values", 5, "sb", "offsets", "validity", "data", 16, "result", 7)]),
])
def test_string_column(n_rows, byte_capacity, sizes, expected):
    eng = _Engine(sizes)
    sh = _shard(eng, 3)
    types, values = _pair_1d(n_rows)
    offsets, validity, data, result = sh.string_column(types, values, byte_capacity, stream=7)
    assert offsets.shape == (n_rows + 1,) and validity.shape == ((n_rows + 63) // 64,) and result.shape == (4,)
    assert data.dtype == torch.uint8 and data.numel() == (byte_capacity if byte_capacity is not None else sizes[0] if sizes else 0)
    assert _named(eng, sh, types=types, values=values, offsets=offsets, validity=validity, data=data, result=result) == expected


@pytest.mark.parametrize("n_rows,out_capacity,expected", [
    (None, None, [("filter_columns_device", "plan", "types", "values", 2, 8, 8, "sb", "keep", "rows", 8, "out_types", "out_values", "result", 7)]),
    (5, None, [("filter_columns_device", "plan", "types", "values", 2, 8, 5, "sb", "keep", "rows", 5, "out_types", "out_values", "result", 7)]),
    (5, 3, [("filter_columns_device", "plan", "types", "values", 2, 8, 5, "sb", "keep", "rows", 3, "out_types", "out_values", "result", 7)]),
    (5, 0, [("filter_columns_device", "plan", "types", "values", 2, 8, 5, "sb", "keep", 0, 0, 0, 0, "result", 7)]),
    (0, None, [("filter_columns_device", "plan", 0, 0, 2, 8, 0, "sb", 0, 0, 0, 0, 0, "result", 7)]),
    (0, 3, [("filter_columns_device", "plan", 0, 0, 2, 8, 0, "sb", 0, "rows", 3, "out_types", "out_values", "result", 7)]),
])
def test_filter(n_rows, out_capacity, expected):
    eng, plan = _Engine(), _Plan()
    sh = _shard(eng, 3)
    types, values = _pair_2d()
    rows, out_types, out_values, keep, result = sh.filter(plan, types, values, n_rows, out_capacity, stream=7)
    live = 8 if n_rows is None else n_rows
    capacity = live if out_capacity is None else out_capacity
    assert rows.shape == (capacity,) and out_types.shape == out_values.shape == (2, capacity)
    assert keep.shape == ((live + 63) // 64,) and result.shape == (2,)
    assert _named(eng, sh, plan=plan, types=types, values=values, rows=rows, out_types=out_types, out_values=out_values, keep=keep,
                  result=result) == expected


_FIELD_CASES = [
    (None, False, ("fields", "types", "values", 2, 8, 8, 0), ("data", 8, "validity", 1, "results", 7)),
    (5, False, ("fields", "types", "values", 2, 8, 5, 0), ("data", 5, "validity", 1, "results", 7)),
    (5, True, ("fields", "types", "values", 2, 8, 5, "row_count"), ("data", 5, "validity", 1, "results", 7)),
    (0, False, ("fields", 0, 0, 2, 8, 0, 0), (0, 0, 0, 0, "results", 7)),
    (0, True, ("fields", 0, 0, 2, 8, 0, "row_count"), (0, 0, 0, 0, "results", 7)),
]


@pytest.mark.parametrize("n_rows,with_count,head,tail", _FIELD_CASES)
@pytest.mark.parametrize("method,entry,record_words,strings", [("arrow_columns", "arrow_columns_device", 4, ()),
                                                                ("timestamp_columns", "time_columns_device", 6, ("sb",))])
def test_field_columns(method, entry, record_words, strings, n_rows, with_count, head, tail):
    eng = _Engine()
    sh = _shard(eng, 3)
    types, values = _pair_2d()
    fields = [(0, "int64"), (1, "int64"), (1, "int64")]  # (the stub does not encode them)
    row_count = torch.tensor([4], dtype=torch.int64) if with_count else None
    data, validity, results = getattr(sh, method)(fields, types, values, n_rows, row_count, stream=7)
    live = 8 if n_rows is None else n_rows
    assert data.shape == (3, live) and validity.shape == (3, (live + 63) // 64) and results.shape == (3, record_words)
    tensors = dict(fields=fields, types=types, values=values, data=data, validity=validity, results=results)
    if with_count:
        tensors["row_count"] = row_count
    assert _named(eng, sh, **tensors) == [(entry,) + head + strings + tail]


@pytest.mark.parametrize("n_rows,dict_capacity,byte_capacity,with_count,sizes,expected", [
    # d_indices is never NULL: a column without rows gets a throwaway word ("other")
    (0, 0, None, False, [0], [("dictionary_column_device", 0, 0, 0, 0, "sb", "other", 0, 0, 0, "dict_offsets", 0, 0, "result", 7)]),
    (0, 4, 16, True, [], [("dictionary_column_device", 0, 0, 0, "row_count", "sb", "other", 0, 4, "dict_rows", "dict_offsets", "data", 16,
                           "result", 7)]),
    (5, 0, 0, False, [], [("dictionary_column_device", "types", "values", 5, 0, "sb", "indices", "validity", 0, 0, "dict_offsets", 0, 0,
                            "result", 7)]),
    (5, 4, None, False, [0], [("dictionary_column_device", "types", "values", 5, 0, "sb", "indices", "validity", 4, "dict_rows", "dict_offsets",
                               0, 0, "result", 7)]),
    (5, 4, None, True, [9], [("dictionary_column_device", "types", "values", 5, "row_count", "sb", "indices", "validity", 4, "dict_rows",
                              "dict_offsets", 0, 0, "result", 7),
                             ("dictionary_column_device", "types", "values", 5, "row_count", "sb", "indices", "validity", 4, "dict_rows",
                              "dict_offsets", "data", 9, "result", 7)]),
    (5, 4, 16, True, [], [("dictionary_column_device", "types", "values", 5, "row_count", "sb", "indices", "validity", 4, "dict_rows",
                           "dict_offsets", "data", 16, "result", 7)]),
])
def test_dictionary_column(n_rows, dict_capacity, byte_capacity, with_count, sizes, expected):
    eng = _Engine(sizes)
    sh = _shard(eng, 3)
    types, values = _pair_1d(n_rows)
    row_count = torch.tensor([4], dtype=torch.int64) if with_count else None
    indices, validity, dict_rows, dict_offsets, data, result = sh.dictionary_column(types, values, dict_capacity, byte_capacity, row_count,
                                                                                    stream=7)
    assert indices.shape == (n_rows,) and indices.dtype == torch.int32 and validity.shape == ((n_rows + 63) // 64,)
    assert dict_rows.shape == (dict_capacity,) and dict_offsets.shape == (dict_capacity + 1,) and result.shape == (6,)
    assert data.dtype == torch.uint8 and data.numel() == (byte_capacity if byte_capacity is not None else sizes[0])
    tensors = dict(types=types, values=values, indices=indices, validity=validity, dict_rows=dict_rows, dict_offsets=dict_offsets,
                   data=data, result=result)
    if with_count:
        tensors["row_count"] = row_count
    assert _named(eng, sh, **tensors) == expected


@pytest.mark.parametrize("as_tensor", [False, True])
def test_from_ndjson(as_tensor):
    from simdjson_java_amd import sharding
    text = b'{"a":1}\n\n[2]\n{"tail"'
    eng = _Engine(ndjson=(2, 13, 0, [0, 9, 13]))
    data = torch.frombuffer(bytearray(text), dtype=torch.uint8) if as_tensor else text
    sh = sharding.BatchShard.from_ndjson(eng, data, CPU, index_ratio=2)
    # (the padded upload and the result record are the method's own: "other")
    assert _named(eng, sh) == [("ndjson_offsets_device", "other", len(text), "offs", len(text) // 2 + 1, "other", 0)]
    assert (sh.n, sh.n_docs, sh.ndjson_consumed, sh.ndjson_flags) == (13, 2, 13, 0) and sh.offs.tolist() == [0, 9, 13]
    assert sh.buf.numel() == 13 + 128 and bytes(sh.buf.numpy()) == text[:13] + bytes(128)
    assert sh.index_capacity == 13 // 2 + 2 + 16


def test_from_ndjson_without_a_document_is_an_empty_shard():
    from simdjson_java_amd import sharding
    eng = _Engine(ndjson=(0, 3, 1, [0]))
    sh = sharding.BatchShard.from_ndjson(eng, b"\n\n\n", CPU)
    assert (sh.n, sh.n_docs, sh.ndjson_consumed, sh.ndjson_flags) == (0, 0, 3, 1) and bytes(sh.buf.numpy()) == bytes(128)


@pytest.mark.parametrize("as_tensor", [False, True])
def test_uploads_are_zero_padded(as_tensor):
    """BatchShard and DocumentShard: the bytes (or the uint8 tensor) followed by 128 zero bytes, on the device"""
    from simdjson_java_amd import sharding
    text = b"[1, 2, 3]" + b" " * 55
    data = torch.frombuffer(bytearray(text), dtype=torch.uint8) if as_tensor else text
    sh = sharding.BatchShard(_Engine(), data, [0, len(text)], CPU)
    assert sh.buf.dtype == torch.uint8 and bytes(sh.buf.numpy()) == text + bytes(128)
    ds = sharding.DocumentShard(_Engine(), data, 0, True, CPU)
    assert ds.buf.dtype == torch.uint8 and bytes(ds.buf.numpy()) == text + bytes(128) and ds.length == len(text)
