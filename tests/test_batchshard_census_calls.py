"""What BatchShard.key_census and BatchShard.explode (with a members plan) hand the engine (sharding.py): the scalars, and for
every pointer whether it is NULL or which tensor it addresses.  CPU test with the recording stub of tests/test_batchshard_calls.py
in place of binding.Context; the expected calls are literals."""
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _shard


class _CensusEngine(_Engine):
    key_census_device = _Engine._entry("key_census_device")


class _MembersPlan:
    n_paths, n_columns, members = 2, 3, True


@pytest.mark.parametrize("n_rows,n_keys,with_validity,with_count,expected", [
    (5, 3, True, True, [("key_census_device", "indices", "validity", "types", 5, "row_count", 3, "counts", "result", 7)]),
    (5, 3, False, False, [("key_census_device", "indices", 0, "types", 5, 0, 3, "counts", "result", 7)]),
    (5, 0, True, False, [("key_census_device", "indices", "validity", "types", 5, 0, 0, 0, "result", 7)]),
    (0, 3, True, True, [("key_census_device", 0, 0, 0, 0, "row_count", 3, "counts", "result", 7)]),
    (0, 0, False, False, [("key_census_device", 0, 0, 0, 0, 0, 0, 0, "result", 7)]),
])
def test_key_census(n_rows, n_keys, with_validity, with_count, expected):
    eng = _CensusEngine()
    sh = _shard(eng, 3)
    indices, types = torch.zeros(n_rows, dtype=torch.int32), torch.zeros(n_rows, dtype=torch.uint8)
    validity = torch.zeros((n_rows + 63) // 64, dtype=torch.int64) if with_validity else None
    row_count = torch.tensor([4], dtype=torch.int64) if with_count else None
    counts, result = sh.key_census(indices, validity, types, n_keys, row_count, stream=7)
    assert counts.shape == (n_keys, 8) and counts.dtype == torch.int64 and result.shape == (4,)
    tensors = dict(indices=indices, types=types, counts=counts, result=result)
    if with_validity:
        tensors["validity"] = validity
    if with_count:
        tensors["row_count"] = row_count
    assert _named(eng, sh, **tensors) == expected


@pytest.mark.parametrize("row_capacity", [0, 6])
def test_explode_with_a_members_plan_has_a_key_column(row_capacity):
    eng, plan = _CensusEngine(), _MembersPlan()
    sh = _shard(eng, 5)
    row_offsets, types, values = sh.explode(plan, row_capacity, stream=7)
    assert types.shape == values.shape == (3, row_capacity)
    cols = ("exp_types", "exp_values") if row_capacity else (0, 0)
    assert _named(eng, sh, plan=plan, exp_row_offsets=row_offsets, exp_types=types, exp_values=values) == [
        ("explode_batch_device", "plan", "tape", "tape_offsets", "doc_errors", "sb", 5, "exp_row_offsets", row_capacity) + cols + (7,)]
