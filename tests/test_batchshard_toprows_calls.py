"""What BatchShard.top_rows hands the engine (sharding.py): the scalars, and for every pointer whether it is NULL or which tensor it
addresses.  CPU test with the recording stub of tests/test_batchshard_calls.py in place of binding.Context; the expected calls
are literals."""
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _shard


class _TopEngine(_Engine):
    top_rows_device = _Engine._entry("top_rows_device")


# (n_rows, k, kind, largest, with types / validity / carried columns / row count) -> the call
@pytest.mark.parametrize("n_rows,k,kind,largest,with_types,with_validity,n_cols,with_count,expected", [
    (5, 3, "long", True, True, True, 2, True,
     [("top_rows_device", "key_types", "key_validity", "key_values", 5, "row_count", 1, 0, 3, "types", "values", 2, 8, "rows", "out_types",
       "out_values", "result", 7)]),
    (5, 3, "double", False, True, False, 0, False,
     [("top_rows_device", "key_types", 0, "key_values", 5, 0, 2, 1, 3, 0, 0, 0, 0, "rows", 0, 0, "result", 7)]),
    (5, 2048, "long", False, False, True, 1, False,
     [("top_rows_device", 0, "key_validity", "key_values", 5, 0, 1, 1, 2048, "types", "values", 1, 8, "rows", "out_types", "out_values", "result", 7)]),
    (5, 0, "double", True, False, False, 1, True,
     [("top_rows_device", 0, 0, "key_values", 5, "row_count", 2, 0, 0, "types", "values", 1, 8, 0, 0, 0, "result", 7)]),
    (0, 4, "long", True, True, True, 0, True,
     [("top_rows_device", 0, 0, 0, 0, "row_count", 1, 0, 4, 0, 0, 0, 0, "rows", 0, 0, "result", 7)]),
])
def test_top_rows(n_rows, k, kind, largest, with_types, with_validity, n_cols, with_count, expected):
    eng = _TopEngine()
    sh = _shard(eng, 3)
    key_values = torch.zeros(n_rows, dtype=torch.int64)
    tensors = dict(key_values=key_values)
    if with_types:
        tensors["key_types"] = torch.zeros(n_rows, dtype=torch.uint8)
    if with_validity:
        tensors["key_validity"] = torch.zeros((n_rows + 63) // 64, dtype=torch.int64)
    if n_cols:
        tensors["types"], tensors["values"] = torch.zeros((n_cols, 8), dtype=torch.uint8), torch.zeros((n_cols, 8), dtype=torch.int64)
    if with_count:
        tensors["row_count"] = torch.tensor([4], dtype=torch.int64)
    rows, out_types, out_values, result = sh.top_rows(tensors.get("key_types"), key_values, k, kind=kind, largest=largest,
                                                      key_validity=tensors.get("key_validity"), types=tensors.get("types"),
                                                      values=tensors.get("values"), row_count=tensors.get("row_count"), stream=7)
    assert rows.shape == (k,) and rows.dtype == torch.int64 and result.shape == (9,) and result.dtype == torch.int64
    assert out_types.shape == (n_cols, k) and out_types.dtype == torch.uint8 and out_values.shape == (n_cols, k) and out_values.dtype == torch.int64
    assert _named(eng, sh, rows=rows, out_types=out_types, out_values=out_values, result=result, **tensors) == expected


def test_n_rows_below_the_column():
    eng = _TopEngine()
    sh = _shard(eng, 3)
    key_types, key_values = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.int64)
    rows, _, _, result = sh.top_rows(key_types, key_values, 2, n_rows=6)
    assert _named(eng, sh, key_types=key_types, key_values=key_values, rows=rows, result=result) == [
        ("top_rows_device", "key_types", 0, "key_values", 6, 0, 1, 0, 2, 0, 0, 0, 0, "rows", 0, 0, "result", 0)]


def test_top_rows_returns_new_tensors_and_checks_its_columns():
    eng = _TopEngine()
    sh = _shard(eng, 3)
    key_types, key_values = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    a, b = sh.top_rows(key_types, key_values, 2), sh.top_rows(key_types, key_values, 2)
    assert a[0].data_ptr() != b[0].data_ptr() and a[3].data_ptr() != b[3].data_ptr()
    types, values = torch.zeros((1, 4), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int64)
    for bad in (dict(key_types=key_types.to(torch.int64)), dict(key_types=key_types[:3]), dict(key_values=key_values.to(torch.float64)),
                dict(key_validity=torch.zeros(0, dtype=torch.int64)), dict(row_count=torch.zeros(2, dtype=torch.int64)), dict(k=2049), dict(k=-1),
                dict(kind="string"), dict(n_rows=5), dict(types=types[:, :3].contiguous(), values=values[:, :3].contiguous()),
                dict(types=types, values=values.to(torch.int32))):
        args = dict(key_types=key_types, key_values=key_values, k=2)
        args.update(bad)
        with pytest.raises(AssertionError):
            sh.top_rows(**args)
