"""CPU check of explode's walk (simdjson-java_amd/csrc/sj_select.h: sel_explode_count / sel_explode_rows, which csrc/explode.hip
compiles verbatim) against the oracle: tests/host_sim/explode_sim.cpp runs it with sequential group primitives over tapes and
string buffers made by oracle.parse; tests/explode_common.py says what the row offsets and every cell must be.  The guarded
pass (every tape and every document's last string record against a page that cannot be read) runs in a child process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import oracle as O
from tests import host_sim_lib
from tests import explode_common as EC
from tests import select_common as SC
from tests import select_fuzz as F
from tests.conftest import ROOT


def load_sim():
    """tests/host_sim/explode_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("explode", ("sj_select.h",))
    lib.sim_explode.restype = C.c_int
    lib.sim_explode.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.sim_explode_guarded.restype = C.c_int
    lib.sim_explode_guarded.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.sim_explode_slice_words.restype = C.c_uint32
    return lib


def run_sim(lib, parsed, base, pointers, capacity, guarded=False):
    """-> (row offsets [n + 1], types [n_paths, capacity] or None, values, the batch's string buffer); the columns are filled
    with the sentinels first"""
    base = base.encode("utf-8") if isinstance(base, str) else bytes(base)
    ptrs = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    bblob = np.frombuffer(base + b"\0", dtype=np.uint8)
    blob = np.frombuffer(b"".join(ptrs) + b"\0", dtype=np.uint8)
    poffs = np.zeros(len(ptrs) + 1, dtype=np.uint64)
    poffs[1:] = np.cumsum([len(p) for p in ptrs], dtype=np.uint64)
    tape, toffs, errs, sb, lo, hi = EC.pack(parsed)
    n = len(parsed)
    offs = np.full(n + 1, EC.SENTINEL_V, dtype=np.uint64)
    types = values = None
    if capacity:
        types = np.full((len(ptrs), capacity), EC.SENTINEL_T, dtype=np.uint8)
        values = np.full((len(ptrs), capacity), EC.SENTINEL_V, dtype=np.uint64)
    tp, vp = (types.ctypes.data, values.ctypes.data) if capacity and ptrs else (None, None)
    if guarded:
        rc = lib.sim_explode_guarded(bblob.ctypes.data, len(base), blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data,
                                     errs.ctypes.data, sb.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, offs.ctypes.data, capacity, tp, vp)
    else:
        rc = lib.sim_explode(bblob.ctypes.data, len(base), blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data,
                             errs.ctypes.data, sb.ctypes.data, n, offs.ctypes.data, capacity, tp, vp)
    assert rc == 0, rc
    return offs, types, values, sb.tobytes()


@pytest.fixture(scope="module")
def lib():
    return load_sim()


def check(lib, parsed, base, pointers, what="", guarded=False, expected=None):
    """the explode at a capacity of the total + 3, at the total, one less, half, and 0 -> (rows, cells that are not MISSING)"""
    want_offs, want = expected or EC.expected_explode(parsed, base, pointers)
    total = want_offs[-1]
    present = 0
    for capacity in sorted({total + 3, total, max(total - 1, 0), total // 2, 0}, reverse=True):
        offs, types, values, sb = run_sim(lib, parsed, base, pointers, capacity, guarded)
        got = EC.check_explode(offs, types, values, sb, want_offs, want, capacity, "%s, capacity %d of %d" % (what, capacity, total))
        present = max(present, got)
    return total, present


def test_slice_constant_is_the_headers(lib):
    assert lib.sim_explode_slice_words() == SC.slice_words()


def test_twitter_statuses_of_one_document(lib):
    name, docs, base, ptrs = EC.twitter_case()
    parsed = [O.parse(d) for d in docs]
    assert len(parsed[0].tape) > 4 * SC.slice_words()
    rows, present = check(lib, parsed, base, ptrs, name)
    assert rows == 100 and present > 12 * rows


@pytest.mark.parametrize("case", EC.github_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_github_events(lib, case):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    rows, present = check(lib, parsed, base, ptrs, name)
    assert rows >= 10 and present > 4 * rows
    if base:
        offs = EC.expected_explode(parsed, base, ptrs)[0]
        assert 0 in np.diff(offs) and max(np.diff(offs)) > 1  # events without commits, and events with several


@pytest.mark.parametrize("case", EC.base_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_base_cases(lib, case):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    rows, present = check(lib, parsed, base, ptrs, name)
    if name in ("base missing", "base an object", "base a string", "base a scalar"):
        # the other documents of these cases do hold an array there
        offs = EC.expected_explode(parsed, base, ptrs)[0]
        assert offs[1] == 0 and rows == 1
    if name == "failed documents between good ones":
        assert [p.error != 0 for p in parsed] == [False, True, False, True, True, False, True, True, False] and rows == 7
    if name == "around the slice":
        S = SC.slice_words()
        assert [len(p.tape) for p in parsed[:4]] == [S - 1, S, S + 1, 2 * S + 1]


def test_the_row_count_follows_the_chain_not_the_scope_count(lib):
    parsed = EC.saturated_count_documents()
    ptrs = ["", "/a", "/0"]
    for base, docs in (("", [parsed[0], parsed[2], parsed[3]]), ("/x", [parsed[1]])):
        want_offs, want = EC.expected_explode(docs, base, ptrs)
        assert list(np.diff(want_offs)) == [5] * len(docs)  # (the oracle's own walk goes by the chain too)
        rows, present = check(lib, docs, base, ptrs, "hand-built scope counts")
        assert rows == 5 * len(docs) and present == 7 * len(docs)


# ---- the seeded corpus -----------------------------------------------------------------------------------------------------
def test_the_corpus_covers_what_it_claims():
    """conditions on the inputs, from the oracle alone, before anything of the product runs"""
    st = EC.fuzz_statistics()
    print("explode corpus: %d cases, %d with rows, %d rows, %d cells, %.1f%% present, array sizes %s" %
          (st["cases"], st["cases_with_rows"], st["rows"], st["cells"], 100.0 * st["present"] / max(1, st["cells"]), sorted(st["array_sizes"])[:40]))
    assert st["cases"] == len(F.CASE_IDS) and 2 * st["cases_with_rows"] >= st["cases"]
    assert {0, 1, 15, 16, 17} <= st["array_sizes"] and max(st["array_sizes"]) > 256
    assert st["types"] == {SC.MISSING} | set(b'"ldtfn[{')


@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(lib, n):
    name, docs, parsed, base, eptrs, expected = EC.fuzz_cases()[n]
    check(lib, parsed, base, eptrs, name, expected=expected)


def guarded_pass():
    """the fixed cases and the whole corpus through sim_explode_guarded; -> the number of rows"""
    lib = load_sim()
    rows = 0
    fixed = [EC.twitter_case()] + EC.github_cases() + EC.base_cases()
    for name, docs, base, ptrs in fixed:
        rows += check(lib, [O.parse(d) for d in docs], base, ptrs, name + " (guarded)", guarded=True)[0]
    rows += check(lib, EC.saturated_count_documents()[:1], "", ["", "/a"], "scope counts (guarded)", guarded=True)[0]
    for name, docs, parsed, base, eptrs, expected in EC.fuzz_cases():
        rows += check(lib, parsed, base, eptrs, name + " (guarded)", guarded=True, expected=expected)[0]
    return rows


def test_no_load_leaves_a_tape_or_a_string_record(lib):
    """in a child process: a load past a tape's last word or past a document's last string record ends it with SIGSEGV"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, "the guarded pass ended with status %d:\n%s" % (r.returncode, r.stderr.decode(errors="replace")[-2000:])
    assert r.stdout.decode().startswith("guarded pass: ")


if __name__ == "__main__":
    O.build()
    print("guarded pass: %d rows" % guarded_pass())
