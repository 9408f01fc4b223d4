"""What BatchShard.group_stats hands the engine (sharding.py): the scalars, and for every pointer whether it is NULL or which tensor
it addresses.  CPU test with the recording stub of tests/test_batchshard_calls.py in place of binding.Context; the expected calls
are literals.  And sharding.decode_group_stats on hand-made words."""
import math
import struct

import numpy as np
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _shard


class _GroupEngine(_Engine):
    group_stats_device = _Engine._entry("group_stats_device")


@pytest.mark.parametrize("n_rows,n_keys,with_validity,with_count,expected", [
    (5, 3, True, True, [("group_stats_device", "indices", "validity", "types", "values", 5, "row_count", 3, "stats", "result", 7)]),
    (5, 3, False, False, [("group_stats_device", "indices", 0, "types", "values", 5, 0, 3, "stats", "result", 7)]),
    (5, 0, True, False, [("group_stats_device", "indices", "validity", "types", "values", 5, 0, 0, 0, "result", 7)]),
    (0, 3, True, True, [("group_stats_device", 0, 0, 0, 0, 0, "row_count", 3, "stats", "result", 7)]),
    (0, 0, False, False, [("group_stats_device", 0, 0, 0, 0, 0, 0, 0, 0, "result", 7)]),
])
def test_group_stats(n_rows, n_keys, with_validity, with_count, expected):
    eng = _GroupEngine()
    sh = _shard(eng, 3)
    indices, types = torch.zeros(n_rows, dtype=torch.int32), torch.zeros(n_rows, dtype=torch.uint8)
    values = torch.zeros(n_rows, dtype=torch.int64)
    validity = torch.zeros((n_rows + 63) // 64, dtype=torch.int64) if with_validity else None
    row_count = torch.tensor([4], dtype=torch.int64) if with_count else None
    stats, result = sh.group_stats(indices, validity, types, values, n_keys, row_count, stream=7)
    assert stats.shape == (n_keys, 10) and stats.dtype == torch.int64 and result.shape == (5,) and result.dtype == torch.int64
    tensors = dict(indices=indices, types=types, values=values, stats=stats, result=result)
    if with_validity:
        tensors["validity"] = validity
    if with_count:
        tensors["row_count"] = row_count
    assert _named(eng, sh, **tensors) == expected


def test_group_stats_returns_new_tensors_and_checks_its_columns():
    eng = _GroupEngine()
    sh = _shard(eng, 3)
    indices, types, values = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64)
    a, b = sh.group_stats(indices, None, types, values, 2), sh.group_stats(indices, None, types, values, 2)
    assert a[0].data_ptr() != b[0].data_ptr() and a[1].data_ptr() != b[1].data_ptr()
    for bad in (dict(indices=indices.to(torch.int64)), dict(types=types[:3]), dict(values=values.to(torch.float64)), dict(values=values[:3]),
                dict(validity=torch.zeros(0, dtype=torch.int64)), dict(row_count=torch.zeros(2, dtype=torch.int64))):
        args = dict(indices=indices, validity=None, types=types, values=values, n_keys=2, row_count=None)
        args.update(bad)
        with pytest.raises(AssertionError):
            sh.group_stats(**args)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_decode_group_stats():
    from simdjson_java_amd.sharding import decode_group_stats
    M = (1 << 64) - 1
    inf = math.inf
    words = np.array([
        # a negative 128-bit sum: -(2^64 + 5) = hi -2, lo 2^64 - 5
        [3, 0, 1, (1 << 64) - 5, M - 1, 0, (-(1 << 63)) & M, 7, _bits(inf), _bits(-inf)],
        # a sum above 2^64: 3 * (2^63 - 1) = hi 1, lo 2^63 - 3; doubles with -0.0 as their minimum
        [3, 2, 0, (1 << 63) - 3, 1, _bits(2.5), (1 << 63) - 1, (1 << 63) - 1, _bits(-0.0), _bits(2.5)],
        # empty classes: the contract's constants
        [0, 0, 4, 0, 0, 0, (1 << 63) - 1, 1 << 63, _bits(inf), _bits(-inf)],
        # only doubles; a sum of -1 in 128 bits would be hi = lo = all ones
        [1, 1, 0, M, M, _bits(-inf), M, M, _bits(-inf), _bits(-inf)],
    ], dtype=np.uint64)
    for stats in (words, words.view(np.int64)):
        got = decode_group_stats(stats)
        assert got[0] == dict(n_long=3, n_double=0, n_other=1, sum_long=-(1 << 64) - 5, sum_double=0.0, min_long=-(1 << 63), max_long=7,
                              min_double=None, max_double=None)
        assert got[1]["sum_long"] == 3 * ((1 << 63) - 1) > 1 << 64 and (got[1]["min_long"], got[1]["max_long"]) == ((1 << 63) - 1, (1 << 63) - 1)
        assert got[1]["min_double"] == 0.0 and math.copysign(1, got[1]["min_double"]) == -1 and got[1]["max_double"] == got[1]["sum_double"] == 2.5
        assert got[2] == dict(n_long=0, n_double=0, n_other=4, sum_long=0, sum_double=0.0, min_long=None, max_long=None, min_double=None,
                              max_double=None)
        assert got[3]["sum_long"] == -1 and (got[3]["min_long"], got[3]["max_long"]) == (-1, -1)
        assert got[3]["sum_double"] == got[3]["min_double"] == got[3]["max_double"] == -inf
        assert all(type(v) in (int, float, type(None)) for d in got for v in d.values())
    assert decode_group_stats(np.zeros((0, 10), dtype=np.int64)) == []
