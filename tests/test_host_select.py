"""CPU check of the device-resident selector's walk (simdjson-java_amd/csrc/sj_select.h, the header csrc/select.hip
compiles verbatim) against the oracle: tests/host_sim/sel_sim.cpp runs it with sequential group primitives over tapes and
string buffers made by oracle.parse; tests/select_common.py says what every (path, document) pair must be."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import host_sim_lib
from tests import select_common as SC
from tests.conftest import ROOT, load_fixture
from tests.golden.vectors import TWITTER_DEFAULT_PROFILE_USERS


def load_sim():
    """tests/host_sim/sel_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("sel", ("sj_select.h",))
    lib.sim_select.restype = C.c_int
    lib.sim_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                               C.c_void_p, C.c_void_p]
    lib.sim_select_guarded.restype = C.c_int
    lib.sim_select_guarded.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_uint64, C.c_void_p, C.c_void_p]
    lib.sim_select_slice_words.restype = C.c_uint32
    return lib


def run_sim(lib, parsed, pointers, guarded=False):
    """parsed: oracle.Parsed per document -> (types [n_paths, n_docs], values, the batch's string buffer).  guarded: through
    sim_select_guarded -- every tape and every document's last string record end at a page that cannot be read."""
    ptrs = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    blob = np.frombuffer(b"".join(ptrs) + b"\0", dtype=np.uint8)
    poffs = np.zeros(len(ptrs) + 1, dtype=np.uint64)
    poffs[1:] = np.cumsum([len(p) for p in ptrs], dtype=np.uint64)
    tapes, sbs, toffs, errs, base, sb_lo, sb_hi = [], [], [0], [], 0, [], []
    for p in parsed:
        errs.append(p.error)
        t = p.tape.copy() if p.error == 0 else np.full(3, 0x7B00000000000099, dtype=np.uint64)  # (a failed document's slot: garbage)
        end = base
        if p.error == 0:
            # STRING payloads are offsets into the batch's shared buffer: only words at chain positions may be moved
            i, n = 1, len(t) - 1
            while i < n:
                ty = int(t[i]) >> 56
                if ty == ord('"'):
                    off = int(t[i]) & 0x00FFFFFFFFFFFFFF
                    end = max(end, base + off + 4 + int.from_bytes(p.strings[off:off + 4], "big"))  # where the document's last record ends
                    t[i] = np.uint64(int(t[i]) + base)
                i += 2 if ty in (ord("l"), ord("d")) else 1
            sbs.append(p.strings)
            sb_lo.append(base)
            base += len(p.strings)
        else:
            sb_lo.append(base)
        sb_hi.append(end)
        tapes.append(t)
        toffs.append(toffs[-1] + len(t))
    tape = np.concatenate(tapes) if tapes else np.zeros(1, dtype=np.uint64)
    sb = np.frombuffer(b"".join(sbs) + b"\0" * 8, dtype=np.uint8)
    n = len(parsed)
    types = np.full((len(ptrs), n), 0xEE, dtype=np.uint8)
    values = np.full((len(ptrs), n), 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    toffs, errs = np.array(toffs, dtype=np.uint64), np.array(errs + [0], dtype=np.int32)
    if guarded:
        lo, hi = np.array(sb_lo + [0], dtype=np.uint64), np.array(sb_hi + [0], dtype=np.uint64)
        rc = lib.sim_select_guarded(blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data, errs.ctypes.data,
                                    sb.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, types.ctypes.data, values.ctypes.data)
    else:
        rc = lib.sim_select(blob.ctypes.data, poffs.ctypes.data, len(ptrs), tape.ctypes.data, toffs.ctypes.data, errs.ctypes.data,
                            sb.ctypes.data, n, types.ctypes.data, values.ctypes.data)
    assert rc == 0, rc
    return types, values, sb.tobytes()


@pytest.fixture(scope="module")
def sim():
    lib = load_sim()

    def run(parsed, pointers, guarded=False):
        return run_sim(lib, parsed, pointers, guarded)
    run.slice_words = lib.sim_select_slice_words()
    return run


def check(sim, docs, pointers, what=""):
    parsed = [O.parse(d) for d in docs]
    types, values, sb = sim(parsed, pointers)
    return SC.check_columns(types, values, sb, SC.expected_columns(parsed, pointers), what), types, values, sb


def test_slice_constant_is_the_headers(sim):
    assert sim.slice_words == SC.slice_words()


def test_twitter_statuses(sim):
    docs = SC.reserialised("twitter.json", lambda d: d["statuses"])
    assert len(docs) == 100
    present, types, values, sb = check(sim, docs, SC.TWITTER_POINTERS, "twitter")
    assert present > 12 * len(docs)
    # BenchmarkCorrectnessTest.java:23-55: the unique screen names of the users with a default profile
    names = set()
    for k in range(len(docs)):
        if types[0][k] == ord("t"):
            ln, off = int(values[1][k]) >> 32, int(values[1][k]) & 0xFFFFFFFF
            names.add(sb[off:off + ln])
    assert len(names) == TWITTER_DEFAULT_PROFILE_USERS


def test_github_events(sim):
    docs = SC.reserialised("github_events.json", lambda d: d)
    assert len(docs) == 30
    present, *_ = check(sim, docs, SC.GITHUB_POINTERS, "github")
    assert present > 8 * len(docs)


def test_wide_object_every_member_and_every_near_miss(sim):
    """wide_bench.json as ONE document: far larger than the slice, so this is the walk over global memory"""
    doc = load_fixture("wide_bench.json")
    parsed = O.parse(doc)
    assert parsed.error == 0 and len(parsed.tape) > 4 * sim.slice_words
    root = parsed.to_python()
    keys = [k for k, _ in root[2]]
    assert root[0] == "o" and len(keys) == 982
    keyset = set(keys)
    assert any(b"/" in k for k in keys) and any(b"~" in k for k in keys) and any(b'"' in k for k in keys) and any(b"\\" in k for k in keys)
    for lo in range(0, len(keys), 48):
        part = keys[lo:lo + 48]
        ptrs = [b"/" + SC.escape_token(k) for k in part]
        types, values, sb = sim([parsed], ptrs)
        assert SC.check_columns(types, values, sb, SC.expected_columns([parsed], ptrs), "wide") == len(part)
        near = []
        for k in part:
            if not k:
                continue  # (the empty key has no byte to change)
            m = bytearray(k)
            m[len(m) // 2] ^= 1
            if bytes(m) not in keyset:
                near.append(b"/" + SC.escape_token(bytes(m)))
        assert len(near) > len(part) // 2
        types, values, sb = sim([parsed], near)
        assert not types.any() and not values.any()
        assert SC.check_columns(types, values, sb, SC.expected_columns([parsed], near), "wide, one byte changed") == 0


def test_rfc6901_examples(sim):
    ex = json.load(open(os.path.join(ROOT, "tests", "golden", "rfc6901_example.json")))
    assert len(ex["pointers"]) == 12
    doc = ex["document"].encode()
    present, types, values, sb = check(sim, [doc], ex["pointers"], "rfc6901")
    assert present == 12
    plain = json.loads(ex["document"])
    for p, want in enumerate(ex["values"]):
        t, v = int(types[p][0]), int(values[p][0])
        if p == 0:
            assert t == ord("{") and v == (len(plain) << 32) | 1
        elif isinstance(want, list):
            assert t == ord("[") and v >> 32 == len(want)
        elif isinstance(want, str):
            assert t == ord('"') and sb[(v & 0xFFFFFFFF):(v & 0xFFFFFFFF) + (v >> 32)] == want.encode()
        else:
            assert t == ord("l") and v == want


@pytest.mark.parametrize("case", SC.adversarial_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_adversarial(sim, case):
    name, docs, pointers = case
    present, types, values, sb = check(sim, docs, pointers, name)
    assert present > 0
    # the same paths compiled one per plan: sharing trie nodes changes nothing
    for p, ptr in enumerate(pointers):
        t1, v1, _ = sim([O.parse(d) for d in docs], [ptr])
        assert (t1[0] == types[p]).all() and (v1[0] == values[p]).all(), (name, ptr)


def test_slice_edges_are_what_they_claim(sim):
    S = sim.slice_words
    for target in (S - 1, S, S + 1):
        assert len(O.parse(SC.sized_document(target)).tape) == target


def test_failed_documents_are_missing_and_never_read(sim):
    docs = [b'{"a":1}', b'{"a":}', b'{"a":2}', b'[1,', b'{"a":"\\q"}', b'{"a":3}']
    parsed = [O.parse(d) for d in docs]
    assert [p.error != 0 for p in parsed] == [False, True, False, True, True, False]
    types, values, sb = sim(parsed, ["/a", "", "/a/b"])
    SC.check_columns(types, values, sb, SC.expected_columns(parsed, ["/a", "", "/a/b"]), "failed documents")
    assert list(types[0]) == [ord("l"), 0, ord("l"), 0, 0, ord("l")] and list(values[0]) == [1, 0, 2, 0, 0, 3]
