"""The queries of tests/query_fuzz.py through the host simulations of the column operators, chained as the device chains them: the
documents parsed by oracle.parse, every operator's numpy outputs the next one's inputs -- cut and strided as BatchShard's wrappers
cut and stride them, row counts handed on as the one word the operator in front wrote.  What lies behind the live rows of an
output here are the canaries of the runners, which are no cells of the query either.  The answers are query_fuzz.expected()'s,
from json.loads alone.  A query that fails here fails in a pass header; one that fails only on the GPU, in a device form or a
launcher."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import arrowcol_common as AC
from tests import explode_common as EC
from tests import fieldcol_common as F
from tests import filter_common as FC
from tests import query_fuzz as QF
from tests import test_host_arrowcol as HA
from tests import test_host_census as HC
from tests import test_host_dictcol as HD
from tests import test_host_explode as HE
from tests import test_host_filter as HF
from tests import test_host_groupstats as HG
from tests import test_host_members as HM
from tests import test_host_select as HS
from tests import test_host_strcol as HSC
from tests import test_host_timecol as HTC
from tests import test_host_toprows as HT
from tests import timecol_common as TC

SCHEDULES = ((64, 0), (0, 1))  # (rows per chunk -- 0: the kernels' own --, order of the chunks where the simulation takes one)
TOP_KINDS = {"long": 1, "double": 2}


@pytest.fixture(scope="module")
def libs():
    return {m.__name__.rsplit("_", 1)[-1]: m.load_sim() for m in (HA, HC, HD, HE, HF, HG, HM, HS, HSC, HTC, HT)}


_PARSED = {}


def parsed_case(name):
    if name not in _PARSED:
        parsed = [O.parse(d) for d in QF.case(name).docs]
        _PARSED[name] = (parsed, EC.pack(parsed))
    return _PARSED[name]


def _row_count(rc):
    return None if rc is None else int(np.asarray(rc).reshape(-1)[0])


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _u64(a):
    a = np.asarray(a)
    return np.ascontiguousarray(a.view(np.uint64) if a.dtype == np.int64 else a, dtype=np.uint64)


class HostBackend:
    """the backend of query_fuzz.run_query over the host simulations: a handle is a numpy array"""

    def __init__(self, libs, name, chunk, order):
        self.libs, self.chunk, self.order = libs, chunk, order
        self.parsed, self.packed = parsed_case(name)
        self.sb = self.packed[3]

    def rows_per_chunk(self, sim):
        """the chunk of the schedule, or the kernels' own for a simulation that does not take 0 for it"""
        return self.chunk or getattr(self.libs[sim], "sim_%s_chunk_rows" % sim)()

    def host(self, handle):
        return np.asarray(handle)

    def sync(self):
        pass

    def string_buffer(self):
        return self.sb.tobytes()

    def select(self, pointers):
        types, values, sb = HS.run_sim(self.libs["select"], self.parsed, pointers)
        assert sb == self.sb.tobytes()
        return types, values

    def explode(self, base, pointers, capacity, members):
        run, lib = (HM.run_sim, self.libs["members"]) if members else (HE.run_sim, self.libs["explode"])
        offs, types, values, sb = run(lib, self.parsed, base, pointers, capacity)
        assert sb == self.sb.tobytes()
        return offs, types, values

    def filter(self, terms, types, values, n_rows, out_capacity):
        n_cols, stride = types.shape
        n_rows = stride if n_rows is None else n_rows
        capacity = n_rows if out_capacity is None else out_capacity
        case = FC.Case("query", list(terms), _u8(types), _u64(values), n_rows, self.sb)
        words, rows, ot, ov, res = HF.run_sim(self.libs["filter"], case, self.rows_per_chunk("filter"), capacity)
        return rows, ot[:n_cols * capacity].reshape(n_cols, capacity), ov[:n_cols * capacity].reshape(n_cols, capacity), words, res

    def top_rows(self, key_types, key_values, k, kind, largest, key_validity, types, values, n_rows, row_count):
        carry = None if types is None else (_u8(types), _u64(values))
        rows, ot, ov, result, _ = HT.run(self.libs["toprows"], None if key_types is None else _u8(key_types), None if key_validity is None else _u64(key_validity),
                                         _u64(key_values), TOP_KINDS[kind], largest, k, carry, _row_count(row_count), n_rows, self.chunk, self.order)
        return rows, ot, ov, result

    def string_column(self, types, values):
        sizing = HSC.run_sim(self.libs["strcol"], _u8(types), _u64(values), self.sb, self.rows_per_chunk("strcol"), 0)
        return HSC.run_sim(self.libs["strcol"], _u8(types), _u64(values), self.sb, self.rows_per_chunk("strcol"), int(sizing[3][0]))

    def dictionary_column(self, types, values, dict_capacity, byte_capacity, row_count):
        lib = self.libs["dictcol"]
        out = HD.run_sim(lib, _u8(types), _u64(values), self.sb, self.rows_per_chunk("dictcol"), dict_capacity, byte_capacity, self.order, 0,
                         _row_count(row_count))
        return tuple(out.view(s) for s in out.STORES)

    def group_stats(self, indices, validity, types, values, n_keys, row_count):
        return HG.run(self.libs["groupstats"], np.ascontiguousarray(indices, dtype=np.int32), _u64(validity), _u8(types), _u64(values), n_keys,
                      _row_count(row_count), self.chunk, self.order)

    def key_census(self, indices, validity, types, n_keys, row_count):
        return HC.run(self.libs["census"], np.ascontiguousarray(indices, dtype=np.int32), _u64(validity), _u8(types), n_keys, _row_count(row_count),
                      self.chunk, self.order)

    def _fields(self, run, sim, case, n_fields):
        d, b, res = run(self.libs[sim], case, self.rows_per_chunk(sim))
        return (d[F.FRONT:F.FRONT + n_fields * case.data_stride].reshape(n_fields, case.data_stride),
                b[F.FRONT:F.FRONT + n_fields * case.validity_stride].reshape(n_fields, case.validity_stride), res)

    def arrow_columns(self, fields, types, values, n_rows, row_count):
        case = AC.Case("query", list(fields), _u8(types), _u64(values), n_rows, _row_count(row_count), *F.strides(n_rows, 0))
        return self._fields(HA.run_sim, "arrowcol", case, len(fields))

    def timestamp_columns(self, fields, types, values, n_rows, row_count):
        case = TC.Case("query", list(fields), _u8(types), _u64(values), self.sb, n_rows, _row_count(row_count), *F.strides(n_rows, 0))
        return self._fields(HTC.run_sim, "timecol", case, len(fields))

    def group_by_string(self, key_types, key_values, val_types, val_values, dict_capacity, row_count):
        """as BatchShard.group_by_string: the dictionary sized by a first call, then the statistics of its n_distinct entries"""
        from simdjson_java_amd.sharding import decode_group_stats
        sizing = self.dictionary_column(key_types, key_values, dict_capacity, 0, row_count)
        indices, validity, _, dict_offsets, dict_bytes, dres = self.dictionary_column(key_types, key_values, dict_capacity, int(sizing[5][4]), row_count)
        n_keys = int(dres[3])
        stats, gres = self.group_stats(indices, validity, val_types, val_values, n_keys, row_count)
        ends, raw = dict_offsets[:n_keys + 1], dict_bytes.tobytes()
        decoded = decode_group_stats(stats)
        return [(raw[int(ends[j]):int(ends[j + 1])], decoded[j]) for j in range(n_keys)], dres, gres

    def discover_keys(self, base, dict_capacity):
        """as BatchShard.discover_keys: a sizing explode, the full one, the dictionary of the keys and the census of the types"""
        total = int(self.explode(base, [""], 0, True)[0][-1])
        offs, types, values = self.explode(base, [""], max(total, 1), True)
        rc = offs[-1:]
        sizing = self.dictionary_column(types[1], values[1], dict_capacity, 0, rc)
        indices, validity, _, dict_offsets, dict_bytes, dres = self.dictionary_column(types[1], values[1], dict_capacity, int(sizing[5][4]), rc)
        n_keys = int(dres[3])
        counts, cres = self.key_census(indices, validity, types[0], n_keys, rc)
        ends, raw = dict_offsets[:n_keys + 1], dict_bytes.tobytes()
        return [(raw[int(ends[j]):int(ends[j + 1])], [int(x) for x in counts[j]]) for j in range(n_keys)], offs, dres, cres


RAN = set()


def run_case(libs, name, schedules):
    c = QF.case(name)
    parsed, _ = parsed_case(name)
    assert [k for k, p in enumerate(parsed) if p.error] == c.failing
    for chunk, order in schedules:
        B = HostBackend(libs, name, chunk, order)
        for q in QF.queries(name):
            QF.run_query(B, name, q)
            RAN.add((name, q["name"]))


@pytest.mark.parametrize("name", QF.CASE_IDS)
def test_the_queries_through_the_host_simulations(libs, name):
    """every query of the case at chunks of 64 rows and at the kernels' own with the chunks in another order; the three largest
    cases at the kernels' own only"""
    run_case(libs, name, SCHEDULES[1:] if name in QF.LARGEST_CASES else SCHEDULES)


def test_no_query_was_skipped(libs):
    """every (case, query) pair ran -- the ones a selection of tests left out run here -- and there are as many as the corpus says"""
    for name in QF.CASE_IDS:
        if any((name, q["name"]) not in RAN for q in QF.queries(name)):
            run_case(libs, name, SCHEDULES[1:])
    assert len(RAN) == QF.N_PAIRS == len(QF.pairs())
