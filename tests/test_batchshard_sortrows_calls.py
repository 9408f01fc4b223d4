"""What BatchShard.sort_rows hands the engine (sharding.py): one sort_rows_device call per key, from the last key to the first, the
row buffers they exchange, the carried columns on the last call only, and no read-back of anything.  CPU test with the recording
stub of tests/test_batchshard_calls.py in place of binding.Context; the expected calls are literals."""
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _shard


class _SortEngine(_Engine):
    sort_rows_device = _Engine._entry("sort_rows_device")


@pytest.fixture
def no_read_back(monkeypatch):
    """anything that waits for the device, or brings a value to the host, fails the test"""
    def forbidden(*a, **kw):
        raise AssertionError("sort_rows() synchronised or read a tensor back")
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, forbidden)
    monkeypatch.setattr(torch.cuda, "synchronize", forbidden)


def _key(n, kind, descending, with_types=True, with_validity=False):
    key = (torch.zeros(n, dtype=torch.uint8) if with_types else None, torch.zeros(n, dtype=torch.int64), kind, descending)
    return key + ((torch.zeros((n + 63) // 64, dtype=torch.int64),) if with_validity else ())


def test_one_key_with_everything(no_read_back):
    eng = _SortEngine()
    sh = _shard(eng, 3)
    key = _key(6, "double", True, with_validity=True)
    types, values = torch.zeros((2, 8), dtype=torch.uint8), torch.zeros((2, 8), dtype=torch.int64)
    rows_in, row_count = torch.zeros(5, dtype=torch.int64), torch.tensor([4], dtype=torch.int64)
    rows, out_types, out_values, records = sh.sort_rows([key], types=types, values=values, rows=rows_in, row_count=row_count, stream=7)
    assert rows.shape == (5,) and rows.dtype == torch.int64 and records.shape == (1, 9) and records.dtype == torch.int64
    assert out_types.shape == (2, 5) and out_types.dtype == torch.uint8 and out_values.shape == (2, 5) and out_values.dtype == torch.int64
    assert _named(eng, sh, key_types=key[0], key_values=key[1], key_validity=key[4], types=types, values=values, rows_in=rows_in,
                  row_count=row_count, rows=rows, out_types=out_types, out_values=out_values, records=records) == [
        ("sort_rows_device", "key_types", "key_validity", "key_values", 6, "rows_in", 5, "row_count", 2, 1, "types", "values", 2, 8, "rows",
         "out_types", "out_values", 5, "records", 7)]


def test_one_key_with_nothing(no_read_back):
    eng = _SortEngine()
    sh = _shard(eng, 3)
    key = _key(6, "long", False, with_types=False)
    rows, out_types, out_values, records = sh.sort_rows([key])
    assert rows.shape == (6,) and out_types.shape == (0, 6) and out_values.shape == (0, 6)
    assert _named(eng, sh, key_values=key[1], rows=rows, records=records) == [
        ("sort_rows_device", 0, 0, "key_values", 6, 0, 6, 0, 1, 0, 0, 0, 0, 0, "rows", 0, 0, 0, "records", 0)]
    # n_rows below the source rows; no position at all
    eng.calls.clear()
    rows, _, _, records = sh.sort_rows([key], n_rows=4)
    assert _named(eng, sh, key_values=key[1], rows=rows, records=records)[0][4:8] == (6, 0, 4, 0)
    eng.calls.clear()
    rows, _, _, records = sh.sort_rows([key], rows=torch.zeros(0, dtype=torch.int64))
    assert _named(eng, sh, key_values=key[1], records=records) == [
        ("sort_rows_device", 0, 0, "key_values", 6, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, "records", 0)]


@pytest.mark.parametrize("n_keys", [2, 3, 4])
def test_the_chain_goes_from_the_last_key_to_the_first_through_two_buffers(no_read_back, n_keys):
    eng = _SortEngine()
    sh = _shard(eng, 3)
    keys = [_key(6, "long" if i % 2 else "double", i % 2 == 0, with_validity=i == 1) for i in range(n_keys)]
    types, values = torch.zeros((1, 6), dtype=torch.uint8), torch.zeros((1, 6), dtype=torch.int64)
    rows_in = torch.zeros(6, dtype=torch.int64)
    rows, out_types, out_values, records = sh.sort_rows(keys, types=types, values=values, rows=rows_in, stream=3)
    assert records.shape == (n_keys, 9) and len(eng.calls) == n_keys
    for call, at in enumerate(range(n_keys - 1, -1, -1)):  # (the last key first)
        got = eng.calls[call]
        last = at == 0
        assert got[0] == "sort_rows_device" and got[3] == keys[at][1].data_ptr() and got[1] == keys[at][0].data_ptr()
        assert got[2] == (keys[at][4].data_ptr() if len(keys[at]) == 5 else 0)
        assert got[4:9] == (6, rows_in.data_ptr() if call == 0 else eng.calls[call - 1][14], 6, 0, 1 if at % 2 else 2) and got[9] == (at % 2 == 0)
        # the carried columns and their outputs: the last call only
        assert got[10:14] == ((types.data_ptr(), values.data_ptr(), 1, 6) if last else (0, 0, 0, 0))
        assert got[15:18] == ((out_types.data_ptr(), out_values.data_ptr(), 6) if last else (0, 0, 0))
        assert got[18] == records[at].data_ptr() and got[19] == 3
    outs = [c[14] for c in eng.calls]
    assert outs[-1] == rows.data_ptr() and len(set(outs)) == 2 and rows_in.data_ptr() not in outs
    assert all(outs[i] != outs[i + 1] and outs[i] == outs[i % 2] for i in range(n_keys - 1))  # (two buffers, alternating: none is read and written)


def test_sort_rows_returns_new_tensors_and_checks_its_columns():
    eng = _SortEngine()
    sh = _shard(eng, 3)
    key = _key(4, "long", False)
    a, b = sh.sort_rows([key]), sh.sort_rows([key])
    assert a[0].data_ptr() != b[0].data_ptr() and a[3].data_ptr() != b[3].data_ptr()
    types, values = torch.zeros((1, 4), dtype=torch.uint8), torch.zeros((1, 4), dtype=torch.int64)
    good = dict(keys=[key])
    for bad in (dict(keys=[]), dict(keys=[key[:3]]), dict(keys=[(key[0], key[1], "string", False)]), dict(keys=[(key[0][:3], key[1], "long", False)]),
                dict(keys=[(key[0], key[1].to(torch.float64), "long", False)]), dict(keys=[key, _key(5, "long", False)]),
                dict(keys=[key + (torch.zeros(0, dtype=torch.int64),)]), dict(row_count=torch.zeros(2, dtype=torch.int64)), dict(n_rows=5),
                dict(rows=torch.zeros(3, dtype=torch.int32)), dict(rows=torch.zeros(3, dtype=torch.int64), n_rows=4),
                dict(types=types[:, :3].contiguous(), values=values[:, :3].contiguous()), dict(types=types, values=values.to(torch.int32))):
        with pytest.raises(AssertionError):
            sh.sort_rows(**dict(good, **bad))
