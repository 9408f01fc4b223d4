"""What BatchShard.parent_columns and BatchShard.explode_with_parents hand the engine (sharding.py): the scalars, and for every
pointer whether it is NULL or which tensor -- and which cell of it -- it addresses.  CPU test with the recording stub of
tests/test_batchshard_calls.py in place of binding.Context; the expected calls are literals."""
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _Plan, _shard


class _ParentEngine(_Engine):
    parent_columns_device = _Engine._entry("parent_columns_device")


# (sparse, n_rows, n_cols, with a row count, with parents) -> the call
@pytest.mark.parametrize("sparse,n_rows,n_cols,with_count,with_parents,expected", [
    (False, 6, 2, True, True,
     [("parent_columns_device", "row_offsets", 3, 0, 6, "row_count", "types", "values", 2, 5, "parent_types", "parents", "out_types", "out_values",
       6, "result", 7)]),
    (True, 4, 1, False, True,
     [("parent_columns_device", "row_offsets", 3, "rows", 4, 0, "types", "values", 1, 5, "parent_types", "parents", "out_types", "out_values", 4,
       "result", 7)]),
    (False, 6, 0, False, True,
     [("parent_columns_device", "row_offsets", 3, 0, 6, 0, 0, 0, 0, 0, "parent_types", "parents", 0, 0, 6, "result", 7)]),
    (True, 4, 2, True, False,
     [("parent_columns_device", "row_offsets", 3, "rows", 4, "row_count", "types", "values", 2, 5, 0, 0, "out_types", "out_values", 4, "result", 7)]),
    (False, 0, 2, False, True,
     [("parent_columns_device", "row_offsets", 3, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, "result", 7)]),
])
def test_parent_columns(sparse, n_rows, n_cols, with_count, with_parents, expected):
    eng = _ParentEngine()
    sh = _shard(eng, 3)
    tensors = dict(row_offsets=torch.zeros(4, dtype=torch.int64))
    if sparse:
        tensors["rows"] = torch.zeros(n_rows, dtype=torch.int64)
    if n_cols:
        tensors["types"], tensors["values"] = torch.zeros((n_cols, 5), dtype=torch.uint8), torch.zeros((n_cols, 5), dtype=torch.int64)
    if with_count:
        tensors["row_count"] = torch.tensor([4], dtype=torch.int64)
    parent_types, parents, out_types, out_values, result = sh.parent_columns(
        tensors["row_offsets"], tensors.get("types"), tensors.get("values"), rows=tensors.get("rows"), n_rows=None if sparse else n_rows,
        row_count=tensors.get("row_count"), with_parents=with_parents, stream=7)
    if with_parents:
        assert parent_types.shape == parents.shape == (n_rows,) and parent_types.dtype == torch.uint8 and parents.dtype == torch.int64
        tensors.update(parent_types=parent_types, parents=parents)
    else:
        assert parent_types is None and parents is None
    assert out_types.shape == out_values.shape == (n_cols, n_rows) and out_types.dtype == torch.uint8 and out_values.dtype == torch.int64
    assert result.shape == (3,) and result.dtype == torch.int64
    assert _named(eng, sh, out_types=out_types, out_values=out_values, result=result, **tensors) == expected


def test_parent_columns_returns_new_tensors_and_checks_its_arguments():
    eng = _ParentEngine()
    sh = _shard(eng, 3)
    row_offsets = torch.zeros(4, dtype=torch.int64)
    types, values = torch.zeros((1, 3), dtype=torch.uint8), torch.zeros((1, 3), dtype=torch.int64)
    a, b = sh.parent_columns(row_offsets, types, values, n_rows=5), sh.parent_columns(row_offsets, types, values, n_rows=5)
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a, b))
    rows = torch.zeros(6, dtype=torch.int64)
    sh.parent_columns(row_offsets, None, None, rows=rows, n_rows=4)
    assert eng.calls[-1][3:5] == (rows.data_ptr(), 4)
    for bad in (dict(n_rows=None), dict(row_offsets=row_offsets.to(torch.int32)), dict(row_offsets=torch.zeros(0, dtype=torch.int64)),
                dict(rows=rows.to(torch.int32)), dict(rows=rows, n_rows=7), dict(row_count=torch.zeros(2, dtype=torch.int64)),
                dict(types=types[:, :2].contiguous(), values=values[:, :2].contiguous()), dict(values=values.to(torch.int32)), dict(n_rows=-1)):
        args = dict(row_offsets=row_offsets, types=types, values=values, n_rows=5)
        args.update(bad)
        with pytest.raises(AssertionError):
            sh.parent_columns(**args)


@pytest.mark.parametrize("row_capacity", [6, 0])
def test_explode_with_parents_is_one_allocation_and_one_stream(row_capacity):
    eng, plan = _ParentEngine(), _Plan()
    sh = _shard(eng, 3)
    n_columns = getattr(plan, "n_columns", plan.n_paths)
    before = dict(vars(sh))
    doc_types, doc_values = torch.zeros((3, 4), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.int64)
    row_offsets, types, values, result = sh.explode_with_parents(plan, row_capacity, doc_types, doc_values, stream=7)
    assert row_offsets.shape == (4,) and row_offsets.dtype == torch.int64 and result.shape == (3,)
    assert types.shape == values.shape == (n_columns + 3 + 1, row_capacity) and types.dtype == torch.uint8 and values.dtype == torch.int64
    assert types.is_contiguous() and values.is_contiguous()
    # exp_* and what check() queues again are left alone
    assert vars(sh).keys() == before.keys() and all(vars(sh)[name] is value for name, value in before.items())
    assert sh._exp_pending is None and sh._exp_plan is None and not hasattr(sh, "exp_types")
    T, V, O = types.data_ptr(), values.data_ptr(), row_offsets.data_ptr()
    cells = lambda base, n, size: base + n * row_capacity * size if row_capacity else 0
    assert eng.calls == [
        ("explode_batch_device", plan, sh.tape.data_ptr(), sh.tape_offsets.data_ptr(), sh.doc_errors.data_ptr(), sh.sb.data_ptr(), 3, O,
         row_capacity, cells(T, 0, 1), cells(V, 0, 8), 7),
        # dense; the row count is the last row offset; the document columns behind the explode's, the parent ids last
        ("parent_columns_device", O, 3, 0, row_capacity, O + 8 * 3, doc_types.data_ptr() if row_capacity else 0,
         doc_values.data_ptr() if row_capacity else 0, 3 if row_capacity else 0, 4, cells(T, n_columns + 3, 1), cells(V, n_columns + 3, 8),
         cells(T, n_columns, 1), cells(V, n_columns, 8), row_capacity, result.data_ptr(), 7)]
    again = sh.explode_with_parents(plan, row_capacity, doc_types, doc_values)
    assert again[0].data_ptr() != O and again[3].data_ptr() != result.data_ptr() and eng.calls[-1][-1] == eng.calls[-2][-1] == 0
