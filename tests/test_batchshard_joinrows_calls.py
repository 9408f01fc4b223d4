"""What BatchShard.join_rows hands the engine (sharding.py): one sort_rows_device call on the right key (LONG, ascending, no
carried columns), then one join_rows_device call with both sides, the sort's rows and record, the outputs of its own making --
or the join alone where right_sorted is given --, and no read-back of anything.  CPU test with the recording stub of
tests/test_batchshard_calls.py in place of binding.Context; the expected calls are literals."""
import pytest
import torch

from tests.test_batchshard_calls import _Engine, _named, _shard


class _JoinEngine(_Engine):
    sort_rows_device = _Engine._entry("sort_rows_device")

    def join_rows_device(self, left, d_left_rows_in, n_left, d_left_count, right, *rest):
        """(the two sides arrive as tuples: recorded flat, a marker in front of each)"""
        self.calls.append(("join_rows_device", "L") + tuple(left) + (d_left_rows_in, n_left, d_left_count, "R") + tuple(right) + rest)


@pytest.fixture
def no_read_back(monkeypatch):
    """anything that waits for the device, or brings a value to the host, fails the test"""
    def forbidden(*a, **kw):
        raise AssertionError("join_rows() synchronised or read a tensor back")
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, forbidden)
    monkeypatch.setattr(torch.cuda, "synchronize", forbidden)


def _key(n, with_types=True, with_validity=False):
    key = (torch.zeros(n, dtype=torch.uint8) if with_types else None, torch.zeros(n, dtype=torch.int64))
    return key + ((torch.zeros((n + 63) // 64, dtype=torch.int64),) if with_validity else ())


def _cols(n_cols, stride):
    return torch.zeros((n_cols, stride), dtype=torch.uint8), torch.zeros((n_cols, stride), dtype=torch.int64)


def test_the_sort_then_the_join_with_everything(no_read_back):
    eng = _JoinEngine()
    sh = _shard(eng, 3)
    lkey, rkey = _key(6, with_validity=True), _key(9)
    left, right = _cols(2, 8), _cols(3, 9)
    lrows, lcount = torch.zeros(5, dtype=torch.int64), torch.tensor([4], dtype=torch.int64)
    rrows, rcount = torch.zeros(7, dtype=torch.int64), torch.tensor([6], dtype=torch.int64)
    out = sh.join_rows(lkey, rkey, how="left", left=left, right=right, left_rows=lrows, left_count=lcount, right_rows=rrows, right_count=rcount,
                       pair_capacity=40, with_offsets=True, stream=7)
    left_rows, right_rows, lt, lv, rt, rv, offsets, record, (order, sort_record) = out
    assert left_rows.shape == right_rows.shape == (40,) and left_rows.dtype == right_rows.dtype == torch.int64
    assert lt.shape == lv.shape == (2, 40) and rt.shape == rv.shape == (3, 40) and lt.dtype == rt.dtype == torch.uint8
    assert offsets.shape == (6,) and record.shape == (9,) and order.shape == (7,) and sort_record.shape == (9,)
    assert _named(eng, sh, lk_types=lkey[0], lk_values=lkey[1], lk_validity=lkey[2], rk_types=rkey[0], rk_values=rkey[1], l_types=left[0], l_values=left[1],
                  r_types=right[0], r_values=right[1], lrows=lrows, lcount=lcount, rrows=rrows, rcount=rcount, left_rows=left_rows, right_rows=right_rows,
                  lt=lt, lv=lv, rt=rt, rv=rv, offsets=offsets, record=record, order=order, sort_record=sort_record) == [
        ("sort_rows_device", "rk_types", 0, "rk_values", 9, "rrows", 7, "rcount", 1, 0, 0, 0, 0, 0, "order", 0, 0, 0, "sort_record", 7),
        ("join_rows_device", "L", "lk_types", "lk_validity", "lk_values", 6, "l_types", "l_values", 2, 8, "lrows", 5, "lcount",
         "R", "rk_types", 0, "rk_values", 9, "r_types", "r_values", 3, 9, "order", 7, "sort_record", 1, 40, "left_rows", "right_rows", "lt", "lv", "rt",
         "rv", 40, "offsets", "record", 7)]


@pytest.mark.parametrize("how,code", [("inner", 0), ("semi", 2), ("anti", 3)])
def test_the_join_with_nothing(no_read_back, how, code):
    eng = _JoinEngine()
    sh = _shard(eng, 3)
    lkey, rkey = _key(6, with_types=False), _key(4, with_types=False)
    left_rows, right_rows, lt, lv, rt, rv, offsets, record, (order, sort_record) = sh.join_rows(lkey, rkey, how=how, pair_capacity=10)
    assert offsets is None and lt.shape == rt.shape == (0, 10) and (right_rows is None) == (code >= 2)
    assert _named(eng, sh, lk_values=lkey[1], rk_values=rkey[1], left_rows=left_rows, right_rows=right_rows, record=record, order=order,
                  sort_record=sort_record) == [
        ("sort_rows_device", 0, 0, "rk_values", 4, 0, 4, 0, 1, 0, 0, 0, 0, 0, "order", 0, 0, 0, "sort_record", 0),
        ("join_rows_device", "L", 0, 0, "lk_values", 6, 0, 0, 0, 0, 0, 6, 0, "R", 0, 0, "rk_values", 4, 0, 0, 0, 0, "order", 4, "sort_record", code, 10,
         "left_rows", "right_rows" if code < 2 else 0, 0, 0, 0, 0, 0, 0, "record", 0)]


def test_right_sorted_suppresses_the_sort(no_read_back):
    """build once, probe many: the second call queues the join alone, on the rows and the record of the first call's sort"""
    eng = _JoinEngine()
    sh = _shard(eng, 3)
    lkey, other, rkey = _key(6), _key(11), _key(4)
    first = sh.join_rows(lkey, rkey, pair_capacity=10, n_right=3)
    assert [c[0] for c in eng.calls] == ["sort_rows_device", "join_rows_device"] and eng.calls[0][6] == 3
    eng.calls.clear()
    second = sh.join_rows(other, rkey, how="anti", right_sorted=first[8], pair_capacity=0, stream=5)
    order, sort_record = first[8]
    assert second[8] is first[8] and second[7].data_ptr() != first[7].data_ptr()
    assert _named(eng, sh, lk_types=other[0], lk_values=other[1], rk_types=rkey[0], rk_values=rkey[1], record=second[7], order=order,
                  sort_record=sort_record) == [
        ("join_rows_device", "L", "lk_types", 0, "lk_values", 11, 0, 0, 0, 0, 0, 11, 0, "R", "rk_types", 0, "rk_values", 4, 0, 0, 0, 0, "order", 3,
         "sort_record", 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, "record", 5)]
    # no position on the right: a sort and a join with NULL for the empty tensors
    eng.calls.clear()
    sh.join_rows(lkey, rkey, pair_capacity=1, right_rows=torch.zeros(0, dtype=torch.int64))
    assert eng.calls[0][5:7] == (0, 0) and eng.calls[0][14] == 0 and eng.calls[1][22:25] == (0, 0, 0)


def test_join_rows_checks_its_arguments():
    eng = _JoinEngine()
    sh = _shard(eng, 3)
    lkey, rkey = _key(6), _key(4)
    good = dict(left_key=lkey, right_key=rkey, pair_capacity=8)
    sh.join_rows(**good)
    for bad in (dict(how="outer"), dict(pair_capacity=None), dict(pair_capacity=-1), dict(left_key=lkey[:1]), dict(left_key=(lkey[0][:3], lkey[1])),
                dict(right_key=(rkey[0], rkey[1].to(torch.float64))), dict(left_key=lkey + (torch.zeros(0, dtype=torch.int64),)), dict(n_left=7),
                dict(left_rows=torch.zeros(3, dtype=torch.int32)), dict(left_rows=torch.zeros(3, dtype=torch.int64), n_left=4), dict(n_right=5),
                dict(left_count=torch.zeros(2, dtype=torch.int64)), dict(left=_cols(1, 5)), dict(right=_cols(1, 3)), dict(how="semi", right=_cols(1, 4)),
                dict(right_sorted=(torch.zeros(4, dtype=torch.int32), torch.zeros(9, dtype=torch.int64))),
                dict(right_sorted=(torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int64)))):
        with pytest.raises(AssertionError):
            sh.join_rows(**dict(good, **bad))
