"""CPU check of a members explode's walk (simdjson-java_amd/csrc/sj_select.h: sel_explode_count<true> / sel_explode_rows<true>,
which csrc/explode.hip compiles verbatim) against the oracle: tests/host_sim/members_sim.cpp runs it with sequential group
primitives over tapes and string buffers made by oracle.parse; tests/members_common.py says what the row offsets and every cell
must be.  The guarded pass (every tape and every document's last string record against a page that cannot be read) runs in a
child process."""
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
from tests import members_common as MC
from tests import select_common as SC
from tests import select_fuzz as F
from tests.conftest import ROOT

_SIG = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
        C.c_uint64, C.c_void_p, C.c_void_p]


def load_sim():
    """tests/host_sim/members_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("members", ("sj_select.h",))
    for name in ("sim_members", "sim_array"):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = _SIG
    lib.sim_members_guarded.restype = C.c_int
    lib.sim_members_guarded.argtypes = _SIG[:9] + [C.c_void_p, C.c_void_p] + _SIG[9:]
    lib.sim_members_slice_words.restype = C.c_uint32
    lib.sim_members_group.restype = C.c_uint32
    return lib


def run_sim(lib, parsed, base, pointers, capacity, guarded=False, entry="sim_members", packed=None):
    """-> (row offsets [n + 1], types [n_cols, capacity] or None, values, the batch's string buffer); the columns are filled
    with the sentinels first"""
    base = base.encode("utf-8") if isinstance(base, str) else bytes(base)
    ptrs = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    n_cols = len(ptrs) + (entry != "sim_array")
    bblob = np.frombuffer(base + b"\0", dtype=np.uint8)
    blob = np.frombuffer(b"".join(ptrs) + b"\0", dtype=np.uint8)
    poffs = np.zeros(len(ptrs) + 1, dtype=np.uint64)
    poffs[1:] = np.cumsum([len(p) for p in ptrs], dtype=np.uint64)
    tape, toffs, errs, sb, lo, hi = packed or EC.pack(parsed)
    n = len(parsed)
    offs = np.full(n + 1, EC.SENTINEL_V, dtype=np.uint64)
    types = values = None
    if capacity:
        types = np.full((n_cols, capacity), EC.SENTINEL_T, dtype=np.uint8)
        values = np.full((n_cols, capacity), EC.SENTINEL_V, dtype=np.uint64)
    tp, vp = (types.ctypes.data, values.ctypes.data) if capacity and n_cols else (None, None)
    if guarded:
        rc = lib.sim_members_guarded(bblob.ctypes.data, len(base), blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data,
                                     errs.ctypes.data, sb.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, offs.ctypes.data, capacity, tp, vp)
    else:
        rc = getattr(lib, entry)(bblob.ctypes.data, len(base), blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data,
                                 errs.ctypes.data, sb.ctypes.data, n, offs.ctypes.data, capacity, tp, vp)
    assert rc == 0, rc
    return offs, types, values, sb.tobytes()


@pytest.fixture(scope="module")
def lib():
    return load_sim()


def check(lib, parsed, base, pointers, what="", guarded=False, expected=None, capacities=None):
    """the explode at the capacities of members_common.capacity_cuts (or the given ones) -> (rows, cells that are not MISSING)"""
    want_offs, want = expected or MC.expected_members(parsed, base, pointers)
    total = want_offs[-1]
    present = 0
    packed = EC.pack(parsed)
    for capacity in sorted(capacities if capacities is not None else {total + 3, total, max(total - 1, 0), total // 2, 0}, reverse=True):
        offs, types, values, sb = run_sim(lib, parsed, base, pointers, capacity, guarded, packed=packed)
        got = EC.check_explode(offs, types, values, sb, want_offs, want, capacity, "%s, capacity %d of %d" % (what, capacity, total))
        present = max(present, got)
    return total, present


def test_constants_are_the_headers(lib):
    assert lib.sim_members_slice_words() == SC.slice_words() and lib.sim_members_group() == 16
    assert MC.header_constant("SJMI_EXPLODE_MEMBERS_MAX_PATHS") == MC.header_constant("SJMI_SELECT_MAX_PATHS") - 1 == 63


@pytest.mark.parametrize("case", MC.size_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_object_sizes_and_column_counts(lib, case):
    """0 .. 33 members (the selector's round of 16 that stages the base, every edge of the row buffer) at 1, 2, 12, 13 and 64 columns"""
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    want_offs, want = MC.expected_members(parsed, base, ptrs)
    assert list(np.diff(want_offs)) == MC.MEMBER_COUNTS and len(want) == len(ptrs) + 1
    rows, present = check(lib, parsed, base, ptrs, name, expected=(want_offs, want), capacities=MC.capacity_cuts(want_offs))
    assert rows == sum(MC.MEMBER_COUNTS) and present >= rows  # (the key column at least)


@pytest.mark.parametrize("case", MC.base_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", ""))
def test_base_cases(lib, case):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    want_offs, want = MC.expected_members(parsed, base, ptrs)
    rows, present = check(lib, parsed, base, ptrs, name, expected=(want_offs, want), capacities=MC.capacity_cuts(want_offs))
    counts = list(np.diff(want_offs))
    if name in ("base missing", "base an array", "base a scalar"):
        assert counts[0] == 0 and rows >= 1 and counts.count(0) == len(counts) - 1  # (one other document does hold an object there)
    if name == "base at the root":
        assert counts == [3, 0, 1, 0, 0, 0]
    if name == "base behind duplicate keys":
        assert counts == [1, 0, 2]  # (get()'s first match decides the base)
    if name == "duplicate keys inside the base":
        assert counts == [5, 3] and [k for _, k in want[-1][:5]] == [b"a", b"a", b"b", b"a", b"b"]
    if name == "the empty key":
        assert [k for _, k in want[-1]] == [b"", b"a", b"", b"", b""]
    if name == "escaped keys":
        assert [k for _, k in want[-1]] == [b"A", b"A", b'q"r', "é".encode(), b"a\\b", b"\n", b"a"]
    if name == "inner members are not rows":
        assert counts == [3, 1]
    if name == "failed documents between good ones":
        assert [p.error != 0 for p in parsed] == [False, True, False, True, True, False, True, True, False] and rows == 7
    if name.startswith("around the slice"):
        S = SC.slice_words()
        assert [len(p.tape) for p in parsed[:4]] == [S - 1, S, S + 1, 2 * S + 1] and counts[:4] == ([3] * 4 if not base else [2] * 4)


@pytest.mark.parametrize("case", MC.github_cases(), ids=lambda c: c[0].replace(" ", "_").replace(",", "").replace("'", ""))
def test_github_events(lib, case):
    name, docs, base, ptrs = case
    parsed = [O.parse(d) for d in docs]
    rows, present = check(lib, parsed, base, ptrs, name)
    assert rows >= 4 * len(docs) if not base else rows >= len(docs)


def test_the_row_count_follows_the_chain_not_the_scope_count(lib):
    ptrs = ["", "/a", "/0"]
    for parsed, base in MC.hand_built_scope_counts():
        want_offs, want = MC.expected_members([parsed], base, ptrs)
        assert list(np.diff(want_offs)) == [5]  # (the oracle's own walk goes by the chain too)
        rows, present = check(lib, [parsed], base, ptrs, "hand-built scope counts", expected=(want_offs, want))
        assert rows == 5 and present == 5 + 5 + 1 + 1


def test_an_array_plan_is_as_it_was(lib):
    """the array instantiation of the same header on the members' documents and on explode's own: the oracle's arrays, and no rows
    for a base that is an object"""
    for name, docs, base, ptrs in EC.base_cases()[:9] + [(n, d, b, p) for n, d, b, p in MC.base_cases()[:7]]:
        parsed = [O.parse(d) for d in docs]
        want_offs, want = EC.expected_explode(parsed, base, ptrs)
        total = want_offs[-1]
        for capacity in (total + 3, max(total - 1, 0), 0):
            offs, types, values, sb = run_sim(lib, parsed, base, ptrs, capacity, entry="sim_array")
            EC.check_explode(offs, types, values, sb, want_offs, want, capacity, name + " (array plan)")


# ---- the seeded corpus -----------------------------------------------------------------------------------------------------
def test_the_corpus_covers_what_it_claims():
    """conditions on the inputs, from the oracle alone, before anything of the product runs"""
    st = MC.fuzz_statistics()
    print("members corpus: %d cases, %d with rows, %d rows, %d cells, %.1f%% present, object sizes %s" %
          (st["cases"], st["cases_with_rows"], st["rows"], st["cells"], 100.0 * st["present"] / max(1, st["cells"]), sorted(st["sizes"])[:40]))
    assert st["cases"] == len(F.CASE_IDS) and 2 * st["cases_with_rows"] >= st["cases"]
    assert st["types"] == {SC.MISSING} | set(b'"ldtfn[{')
    assert {0, 1, 15, 16, 17} <= st["sizes"]


@pytest.mark.parametrize("n", range(len(F.CASE_IDS)), ids=F.CASE_IDS)
def test_fuzz(lib, n):
    name, docs, parsed, base, eptrs, expected = MC.fuzz_cases()[n]
    check(lib, parsed, base, eptrs, name, expected=expected)


def guarded_pass():
    """the fixed cases and the whole corpus through sim_members_guarded; -> the number of rows"""
    lib = load_sim()
    rows = 0
    for name, docs, base, ptrs in MC.size_cases() + MC.base_cases() + MC.github_cases():
        rows += check(lib, [O.parse(d) for d in docs], base, ptrs, name + " (guarded)", guarded=True)[0]
    parsed, base = MC.hand_built_scope_counts()[0]
    rows += check(lib, [parsed], base, ["", "/a"], "scope counts (guarded)", guarded=True)[0]
    for name, docs, parsed, base, eptrs, expected in MC.fuzz_cases():
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
