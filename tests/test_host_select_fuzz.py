"""CPU check of the selector's walk (simdjson-java_amd/csrc/sj_select.h through tests/host_sim/sel_sim.cpp) on the seeded corpus
of tests/select_fuzz.py: random documents and plans, plans at the limits of include/sjmi.h, every (path, document) pair against
tests/select_common.py.  The generator's own conditions are asserted first; the guarded pass (every tape and every document's
last string record against a page that cannot be read) runs in a child process, so that a stray load is a failed test."""
import os
import subprocess
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import select_common as SC
from tests import select_fuzz as F
from tests.conftest import ROOT
from tests.test_host_select import load_sim, run_sim


@pytest.fixture(scope="module")
def lib():
    return load_sim()


def test_the_corpus_covers_what_it_claims():
    """conditions, not measurements: counted from the documents and select_common alone"""
    S = SC.slice_words()
    st = F.statistics()
    print("corpus: %d documents, %d pairs, %.1f%% present; plans of %s paths; nesting up to %d; matched key lengths %d..%d; duplicates %r; "
          "%d matches behind a descent" % (st["documents"], st["pairs"], 100.0 * st["present"] / st["pairs"], sorted(st["plan_sizes"]),
                                           st["max_nesting"], min(st["matched_key_lengths"]), max(st["matched_key_lengths"]),
                                           st["duplicates"], st["behind_a_descent"]))
    assert 4 * st["present"] >= st["pairs"] and 4 * (st["pairs"] - st["present"]) >= st["pairs"]
    assert set(range(41)) <= st["matched_key_lengths"] and {100, 1000, 4096} <= st["matched_key_lengths"]
    assert {0, 15, 16, 17, 31, 32} <= st["matched_positions"]
    assert st["behind_a_descent"] > 0
    assert all(n > 0 for n in st["duplicates"].values()), st["duplicates"]
    assert {S - 1, S, S + 1} <= st["tape_words"] and max(st["tape_words"]) > 4 * S
    assert st["max_nesting"] > 16
    assert set(F.OBJECT_SIZES) <= st["object_sizes"] and any(n >= 200 for n in st["object_sizes"])
    assert {0, 1, 15, 16, 17, 33} <= st["array_sizes"]
    assert st["types"] == {SC.MISSING} | set(b'"ldtfn[{')
    assert {1, 64} <= st["plan_sizes"]
    assert st["last_record_key_shapes"] == {"0", "1-3", "4-7", "whole words", "tail"} and st["last_record_value"] > 0


def test_every_plan_of_the_corpus_compiles_to_what_plan_fits_says():
    for name, docs, ptrs in F.corpus():
        assert F.plan_fits(ptrs) and 1 <= len(ptrs) <= F.MAX_PATHS, name


@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(lib, n):
    name, docs, ptrs, parsed, want = F.parsed_corpus()[n]
    types, values, sb = run_sim(lib, parsed, ptrs)
    SC.check_columns(types, values, sb, want, name)
    if n % 8 == 0 or name.startswith("limit"):  # one path per plan: sharing trie nodes changes nothing
        for p, ptr in enumerate(ptrs):
            t1, v1, _ = run_sim(lib, parsed, [ptr])
            assert (t1[0] == types[p]).all() and (v1[0] == values[p]).all(), (name, ptr)


def guarded_pass():
    """the whole corpus through sim_select_guarded; -> the number of pairs compared"""
    lib = load_sim()
    pairs = 0
    for name, docs, ptrs, parsed, want in F.parsed_corpus():
        types, values, sb = run_sim(lib, parsed, ptrs, guarded=True)
        SC.check_columns(types, values, sb, want, name + " (guarded)")
        pairs += len(ptrs) * len(docs)
    return pairs


def test_no_load_leaves_a_tape_or_a_string_record(lib):
    """in a child process: a load past a tape's last word or past a document's last string record ends it with SIGSEGV"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, "the guarded pass ended with status %d:\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().startswith("guarded pass: ")


if __name__ == "__main__":
    from oracle import oracle
    oracle.build()
    print("guarded pass: %d pairs" % guarded_pass())
