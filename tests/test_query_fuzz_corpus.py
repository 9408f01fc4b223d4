"""The conditions of the corpus of tests/query_fuzz.py, asserted on the CPU without a line of the product: what
tests/test_host_query_fuzz.py and tests/test_gpu_query_fuzz.py can notice depends on them, so a change of a seed or a size that
loses one fails here.  Prints the statistics (pytest -s shows them)."""
import json

import pytest

from oracle import oracle as O
from tests import members_common as MC
from tests import query_fuzz as QF


def _python(v):
    """an oracle to_python() tree as json.loads(object_pairs_hook=list of pairs) gives the document, a double as its bits"""
    t = v[0]
    if t == "o":
        return {"pairs": [(bytes(k).decode("utf-8"), _python(e)) for k, e in v[2]]}
    if t == "a":
        return [_python(e) for e in v[2]]
    return {"s": lambda: bytes(v[1]).decode("utf-8"), "l": lambda: v[1], "d": lambda: ("double", v[1]), "t": lambda: True, "f": lambda: False, "n": lambda: None}[t]()


def _loaded(text):
    return json.loads(text, object_pairs_hook=lambda pairs: {"pairs": pairs}, parse_float=lambda s: ("double", QF.bits_of(float(s))))


def _no_duplicate_keys(v):
    if isinstance(v, dict):
        keys = [k for k, _ in v["pairs"]]
        return len(set(keys)) == len(keys) and all(_no_duplicate_keys(e) for _, e in v["pairs"])
    return all(_no_duplicate_keys(e) for e in v) if isinstance(v, list) else True


@pytest.mark.parametrize("name", QF.CASE_IDS)
def test_the_documents_are_what_json_loads_says(name):
    """every document that is not on the failing list: the oracle accepts it and reads what json.loads reads, the type of every
    number and the sign of every zero included, and no object has a key twice; every failing document fails"""
    c = QF.case(name)
    assert c.n_docs == len(c.docs) == len(c.rows) and sum(len(d) + 1 for d in c.docs) < 1 << 20
    for k, d in enumerate(c.docs):
        p = O.parse(d)
        if k in c.failing:
            assert p.error != 0 and c.rows[k] is QF.FAILED and d in QF.FAILING, (name, k)
            continue
        assert p.error == 0 and c.rows[k] is not QF.FAILED, (name, k, d)
        want = _loaded(d)
        assert _python(p.to_python()) == want and _no_duplicate_keys(want), (name, k, d)
        assert not c.ndjson or b"\n" not in d
    assert bool(c.failing) == (name not in ("d1_longs_v1", "d65_mixed_v40_clean", "d1023_mixed_v40_ndjson"))


def test_the_cases_are_the_ones_of_the_issue():
    cases = [QF.case(name) for name in QF.CASE_IDS]
    assert 12 <= len(cases) <= 16
    assert {c.n_docs for c in cases} == {1, 63, 64, 65, 1023, 1024, 1025, 2500} and {c.V for c in cases} == {1, 3, 40, 600}
    assert {c.profile for c in cases} == {"longs", "doubles", "mixed", "ties"}
    assert all(c.n_docs == 2500 for c in cases if c.V == 600)
    assert sum(not c.failing for c in cases) >= 2 and sum(c.ndjson and not c.failing for c in cases) == 1
    assert QF.LDS_KEYS == MC.header_constant("SJMI_GROUP_LDS_KEYS") and QF.TOP_MAX_K == MC.header_constant("SJMI_TOP_MAX_K")
    seen = set()
    for c in cases:
        assert c.V < 40 or set(QF.SPECIAL_KEYS) <= set(c.vocabulary)
        seen |= {r.get("grp") for r in c.rows if isinstance(r, dict) and isinstance(r.get("grp"), str)}
    assert set(QF.SPECIAL_KEYS) <= seen  # "", 1, 7, 8, 9 and 300 bytes, the twins, 2-, 3- and 4-byte characters, a quote and a backslash
    assert sorted(len(k.encode("utf-8")) for k in QF.SPECIAL_KEYS[:6]) == [0, 1, 7, 8, 9, 300]


def test_the_corpus_covers_what_it_claims():
    st = QF.statistics()
    print()
    for key in sorted(st):
        print("%-28s %s" % (key, sorted(st[key]) if isinstance(st[key], set) else st[key]))
    # the number of (case, query) pairs is the constant the host and the GPU tests hold their runs against
    assert st["pairs"] == QF.N_PAIRS == len(QF.pairs())
    # every filter of every query keeps a row and drops a row
    assert st["filters"] > 100 and not st["filters_that_do_not_split"], st["filters_that_do_not_split"]
    assert st["overflows"] >= 20
    # every numeric comparison and every string op; a long cell against a double constant and a double cell against a long one
    assert set(QF.NUM_OPS) | {"string_eq", "string_ne", "string_prefix", "type_eq", "type_ne"} <= st["ops"], sorted(st["ops"])
    assert st["long_cell_double_constant"] > 0 and st["double_cell_long_constant"] > 0
    assert st["rounds_onto_the_constant"] > 0  # (2^53 + 1 against 2^53 as a double: equal only to a comparison that rounds the long)
    # top_rows: ties at the cut in a third of the order-by queries that cut, a long that ties with a double, every counter
    assert st["order_by_cuts"] > 100 and 3 * st["order_by_ties_at_the_cut"] >= st["order_by_cuts"], (st["order_by_ties_at_the_cut"], st["order_by_cuts"])
    assert st["a_long_and_a_double_tie"] > 0 and st["n_inexact"] > 0 and st["n_null"] > 0 and st["n_other"] > 0 and st["fewer_than_k"] > 0
    # groups: every mix of classes, doubles that are all -0.0, a key of one row, a wave of one key, empty groups behind n_distinct
    for what in ("only_longs", "only_doubles", "both", "neither", "all_negative_zero", "once", "aligned_runs", "empty_groups"):
        assert st[what] > 0, what
    assert st["keys_with_two_source_texts"] >= 5
    assert st["distinct_of_the_600"] > QF.LDS_KEYS
    # row counts on either side of a 1024-row boundary, given by the host and read on the device
    for what in ("n_rows", "row_counts"):
        assert any(0 < x < 1024 for x in st[what]) and any(x > 1024 for x in st[what]), (what, sorted(st[what]))
    assert {1023, 1024, 1025} <= st["n_rows"]
