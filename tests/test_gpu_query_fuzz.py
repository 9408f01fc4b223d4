"""The queries of tests/query_fuzz.py on the device: per case one BatchShard (the constructor, or from_ndjson for the NDJSON case),
one step that check() accepts, then every query of the case back to back on ONE context and one stream that is not the default
one -- a query queued whole, row counts read on the device, one synchronisation before its outputs are read (but for the
wrappers that read a size back themselves: group_by_string, discover_keys, a sizing string_column).  Back to back on purpose: the
torch.empty outputs of a call then hold an earlier query's cells behind their live rows, and the context's scratch is reused and
grown across calls of different sizes.  The answers are query_fuzz.expected()'s, from json.loads alone; nothing behind the live
rows of an output is looked at."""
import time

import numpy as np
import pytest

from tests import query_fuzz as QF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(0, 1 << 21)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side():
    """the one stream of the module that is not the default one: torch's work and the engine's kernels of every case go on it"""
    import torch
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert stream.cuda_stream != 0
    yield stream
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (what the cases' shards held goes back to the device, not to the tests behind this module)


class DeviceBackend:
    """the backend of query_fuzz.run_query over BatchShard: a handle is a tensor on the device"""

    def __init__(self, ctx, side, name):
        import torch
        from simdjson_java_amd import sharding
        c = QF.case(name)
        self.torch, self.device = torch, torch.device("cuda", 0)
        self.torch_stream, self.stream = side, side.cuda_stream
        packed = b"".join(d + b"\n" for d in c.docs)
        offsets = np.cumsum([0] + [len(d) + 1 for d in c.docs]).astype(np.uint64)
        with torch.cuda.stream(self.torch_stream):
            if c.ndjson:
                self.shard = sharding.BatchShard.from_ndjson(ctx, packed, self.device)
                assert self.shard.ndjson_consumed == len(packed)
            else:
                self.shard = sharding.BatchShard(ctx, packed, offsets, self.device)
            torch.cuda.synchronize()
            assert self.shard.n_docs == c.n_docs and self.shard.offs.cpu().numpy().view(np.uint64).tolist() == offsets.tolist()
            self.shard.step(self.stream)
            torch.cuda.synchronize()
            report = self.shard.check()
            torch.cuda.synchronize()
            assert np.flatnonzero(self.shard.doc_errors.cpu().numpy()[:c.n_docs]).tolist() == c.failing and report["failed_documents"] == len(c.failing)
            self.sb = bytes(self.shard.sb[:report["string_bytes"]].cpu().numpy())
        self.plans = {}

    def close(self):
        for plan in self.plans.values():
            plan.close()

    def plan(self, kind, *key):
        import simdjson_java_amd as S
        if (kind, key) not in self.plans:
            make = {"select": lambda p: S.SelectPlan(list(p)), "filter": lambda t: S.FilterPlan(list(t)),
                    "explode": lambda base, p, members: S.ExplodePlan(base, list(p), members=members)}[kind]
            self.plans[(kind, key)] = make(*key)
        return self.plans[(kind, key)]

    def host(self, handle):
        a = handle.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a

    def sync(self):
        self.torch.cuda.synchronize()

    def string_buffer(self):
        return self.sb

    def select(self, pointers):
        return self.shard.select(self.plan("select", tuple(pointers)), self.stream)

    def explode(self, base, pointers, capacity, members):
        return self.shard.explode(self.plan("explode", base, tuple(pointers), members), capacity, self.stream)

    def filter(self, terms, types, values, n_rows, out_capacity):
        return self.shard.filter(self.plan("filter", tuple(terms)), types, values, n_rows, out_capacity, self.stream)

    def top_rows(self, key_types, key_values, k, kind, largest, key_validity, types, values, n_rows, row_count):
        return self.shard.top_rows(key_types, key_values, k, kind, largest, key_validity, types, values, n_rows, row_count, self.stream)

    def string_column(self, types, values):
        return self.shard.string_column(types, values, None, self.stream)

    def dictionary_column(self, types, values, dict_capacity, byte_capacity, row_count):
        return self.shard.dictionary_column(types, values, dict_capacity, byte_capacity, row_count, self.stream)

    def group_stats(self, indices, validity, types, values, n_keys, row_count):
        return self.shard.group_stats(indices, validity, types, values, n_keys, row_count, self.stream)

    def key_census(self, indices, validity, types, n_keys, row_count):
        return self.shard.key_census(indices, validity, types, n_keys, row_count, self.stream)

    def arrow_columns(self, fields, types, values, n_rows, row_count):
        return self.shard.arrow_columns(list(fields), types, values, n_rows, row_count, self.stream)

    def timestamp_columns(self, fields, types, values, n_rows, row_count):
        return self.shard.timestamp_columns(list(fields), types, values, n_rows, row_count, self.stream)

    def group_by_string(self, key_types, key_values, val_types, val_values, dict_capacity, row_count):
        return self.shard.group_by_string(key_types, key_values, val_types, val_values, dict_capacity, row_count, self.stream)

    def discover_keys(self, base, dict_capacity):
        return self.shard.discover_keys(base, dict_capacity, self.stream)


RAN = set()


def run_case(ctx, side, name):
    import torch
    started = time.perf_counter()
    B = DeviceBackend(ctx, side, name)
    try:
        with torch.cuda.stream(B.torch_stream):
            for q in QF.queries(name):
                first = QF.run_query(B, name, q)
                if name in QF.LARGEST_CASES and q["shape"] in ("order_by", "group_by") and q.get("capacity") is None:
                    assert QF.same_runs(first, QF.run_query(B, name, q))  # (every word but sum_double the same in a second run)
                RAN.add((name, q["name"]))
            torch.cuda.synchronize()
    finally:
        B.close()
    print("%s: %d queries in %.2f s" % (name, len(QF.queries(name)), time.perf_counter() - started))


@pytest.mark.parametrize("name", QF.CASE_IDS)
def test_the_queries_on_the_device(ctx, side, name):
    run_case(ctx, side, name)


def test_no_query_was_skipped(ctx, side):
    """every (case, query) pair ran -- the ones a selection of tests left out run here -- and there are as many as the corpus says"""
    for name in QF.CASE_IDS:
        if any((name, q["name"]) not in RAN for q in QF.queries(name)):
            run_case(ctx, side, name)
    assert len(RAN) == QF.N_PAIRS == len(QF.pairs())
