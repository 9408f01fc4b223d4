"""What an explode must give, from the oracle alone: the base pointer resolved on oracle.Parsed.to_python() with the steps of
tests/select_common.py, the base array's elements taken from the oracle's iterator-chain walk, and select_common.expected_one
on each element, container results moved to the element's tape index inside its document.  Shares no code with the product.
Used by the host simulation's tests, the GPU tests and tools/bench_explode.py; every cell is compared."""
import functools
import random

import numpy as np

from tests import select_common as SC
from tests import select_fuzz as F

SENTINEL_T, SENTINEL_V = 0xEE, 0xEEEEEEEEEEEEEEEE


def base_elements(root, base):
    """-> [(element, its tape index)] of the array the base pointer reaches in a to_python() tree; [] when there is none"""
    cur = (root, 1)  # the root value is tape word 1
    for token in SC.pointer_tokens(base):
        cur = SC._step(cur[0], cur[1], token)
        if cur is None:
            return []
    v, idx = cur
    if v[0] != "a":
        return []
    out, p = [], idx + 1
    for e in v[2]:
        out.append((e, p))
        p += SC._words(e)
    return out


def expected_cell(elem, idx, pointer):
    """expected_one with the element as the root; a container's tape index counts from the document's first word"""
    t, payload = SC.expected_one(elem, pointer)
    if t in (ord("["), ord("{")):
        payload += idx - 1  # (expected_one numbered the element's own word 1)
    return (t, payload)


def expected_explode(parsed_docs, base, pointers):
    """parsed_docs: oracle.Parsed or None (a failed document) per document -> (row_offsets [n + 1], [path][row] of expected_cell)"""
    offs, cols = [0], [[] for _ in pointers]
    for p in parsed_docs:
        elems = [] if p is None or p.error else base_elements(p.to_python(), base)
        for e, idx in elems:
            for q, ptr in enumerate(pointers):
                cols[q].append(expected_cell(e, idx, ptr))
        offs.append(offs[-1] + len(elems))
    return offs, cols


def check_explode(row_offsets, types, values, sb, want_offsets, want, capacity, what=""):
    """row_offsets [n + 1]; types / values [n_paths, capacity] (None with capacity 0), filled with the sentinels before the run.
    Compares the offsets, EVERY cell below the capacity, and that every cell at or behind the total keeps its sentinel.
    -> the number of cells that are not MISSING"""
    assert [int(x) for x in row_offsets] == list(want_offsets), (what, "row offsets")
    total = want_offsets[-1]
    if not capacity or not want:
        return 0
    n = min(total, capacity)
    assert types.shape == (len(want), capacity) and values.shape == types.shape
    present = SC.check_columns(types[:, :n], values[:, :n], sb, [col[:n] for col in want], what)
    assert (types[:, n:] == SENTINEL_T).all() and (values[:, n:] == SENTINEL_V).all(), (what, "a cell past the rows was written")
    return present


def pack(parsed):
    """oracle.Parsed per document -> the batch as the device pipeline lays it out: (tape, tape_offsets [n + 1], doc_errors,
    string buffer, per document the first byte of its records and where its last record ends).  A failed document's slot
    holds garbage."""
    tapes, sbs, toffs, errs, base, sb_lo, sb_hi = [], [], [0], [], 0, [], []
    for p in parsed:
        errs.append(p.error)
        t = p.tape.copy() if p.error == 0 else np.full(3, 0x5B00000000000099, dtype=np.uint64)
        end = base
        if p.error == 0:
            # STRING payloads are offsets into the batch's shared buffer: only words at chain positions may be moved
            i, n = 1, len(t) - 1
            while i < n:
                ty = int(t[i]) >> 56
                if ty == ord('"'):
                    off = int(t[i]) & 0x00FFFFFFFFFFFFFF
                    end = max(end, base + off + 4 + int.from_bytes(p.strings[off:off + 4], "big"))
                    t[i] = np.uint64(int(t[i]) + base)
                i += 2 if ty in (ord("l"), ord("d")) else 1
            sbs.append(bytes(p.strings))
            sb_lo.append(base)
            base += len(p.strings)
        else:
            sb_lo.append(base)
        sb_hi.append(end)
        tapes.append(t)
        toffs.append(toffs[-1] + len(t))
    tape = np.concatenate(tapes) if tapes else np.zeros(1, dtype=np.uint64)
    sb = np.frombuffer(b"".join(sbs) + b"\0" * 8, dtype=np.uint8)
    return (tape, np.array(toffs, dtype=np.uint64), np.array(errs + [0], dtype=np.int32), sb,
            np.array(sb_lo + [0], dtype=np.uint64), np.array(sb_hi + [0], dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by the host-simulation tests and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
ELEMENT_POINTERS = ["", "/a", "/a/0", "/0", "/1", "/b/c", "/nope", "/0/0"]


def base_cases():
    """-> [(name, [document bytes], base pointer, [element pointer])]"""
    S = SC.slice_words()
    ints = [str(v) for v in SC.HEADER_LOOKING]
    dbls = [SC._double_text(v) for v in SC.HEADER_LOOKING[:6]]
    mixed = b'[1,"s",null,true,false,2.5,{"a":[7,8],"b":{"c":"deep"}},[[9],{"a":1}],{"a":{"0":"key"}},[]]'
    return [
        ("base missing", [b'{"x":[1,2]}', b'{"arr":[1]}', b'{}', b'[]', b'7', b'{"arr":{"arr":[1,2]}}'], "/arr", ELEMENT_POINTERS),
        ("base an object", [b'{"arr":{"0":1,"1":2}}', b'{"arr":[{"a":1}]}', b'{"arr":{}}'], "/arr", ELEMENT_POINTERS),
        ("base a string", [b'{"arr":"[1,2]"}', b'{"arr":[["x"]]}', b'{"arr":""}'], "/arr", ELEMENT_POINTERS),
        ("base a scalar", [b'{"arr":5}', b'{"arr":null}', b'{"arr":true}', b'{"arr":1.5}', b'{"arr":[5]}', b'{"arr":false}'], "/arr", ELEMENT_POINTERS),
        ("base an empty array", [b'{"arr":[]}', b'{"arr":[[]]}', b'{"arr":[]}', b'{"arr":[{}]}', b'[]'], "/arr", ELEMENT_POINTERS),
        ("array of arrays", [b'{"arr":[[1,2],[],[[3]],[4,[5,6]]]}', b'{"arr":[[["x","y"]]]}'], "/arr", ELEMENT_POINTERS),
        ("array at the root", [mixed, b'[]', b'[[]]', b'{"0":[1]}', b'"[1]"', b'[{"a":[1,2,3]},{"a":[]},{"b":{"c":null}}]'], "", ELEMENT_POINTERS),
        ("base by index and deep", [b'{"a":[0,{"b":[[1],[{"a":[5,6]},{"a":{"0":"k"}}]]}]}', b'{"a":[0,{"b":[[1]]}]}', b'{"a":[0]}'], "/a/1/b/1", ELEMENT_POINTERS),
        ("duplicate keys in front of the base", [b'{"arr":[1,2],"arr":[3,4,5]}', b'{"arr":5,"arr":[1]}', b'{"x":{"arr":[9]},"arr":[{"a":1,"a":2}],"arr":[]}',
                                                  b'{"arr":[],"arr":[1,2,3]}'], "/arr", ELEMENT_POINTERS),
        ("header-looking integers", [("[" + ",".join(ints) + "]").encode(), ('{"arr":[%s,{"a":%s},[%s]]}' % (",".join(ints), ints[0], ints[1])).encode()] +
         [('[{"a":%s,"b":{"c":%s}},%s,[%s,%s]]' % (ints[i], ints[(i + 1) % 10], ints[(i + 2) % 10], ints[(i + 3) % 10], ints[(i + 4) % 10])).encode() for i in range(10)],
         "", ELEMENT_POINTERS),
        ("header-looking doubles", [("[" + ",".join(dbls) + "]").encode()] +
         [('[{"a":%s,"b":{"c":%s}},%s,[%s,%s]]' % (dbls[i], dbls[(i + 1) % 6], dbls[(i + 2) % 6], dbls[(i + 3) % 6], dbls[(i + 4) % 6])).encode() for i in range(6)],
         "", ELEMENT_POINTERS),
        ("around the slice", [SC.sized_document(S - 1), SC.sized_document(S), SC.sized_document(S + 1), SC.sized_document(2 * S + 1), b'{"pad":[[1],2]}'],
         "/pad", ["", "/0"]),
        ("around the slice, base at the end", [SC.sized_document(S - 1), SC.sized_document(S), SC.sized_document(S + 1), SC.sized_document(2 * S + 1)],
         "/last/x", ["", "/0"]),
        ("failed documents between good ones", [b'{"arr":[1,2]}', b'{"arr":[1,}', b'{"arr":[3]}', b'[1,', b'{"arr":["\\q"]}', b'{"arr":[4,5,6]}', b'{"arr":}', b'{"arr":["abc', b'{"arr":[7]}'],
         "/arr", ["", "/a"]),
        ("no element pointers", [b'{"arr":[1,2]}', b'{"arr":[]}', b'{"arr":[3]}'], "/arr", []),
        ("duplicate element pointers", [b'{"arr":[{"a":1},{"a":"s"},{}]}', b'{"arr":[{"a":[2]}]}'], "/arr", ["/a", "", "/a", "/a", ""]),
    ]


def twitter_case():
    from tests.conftest import load_fixture
    return ("twitter", [load_fixture("twitter.json")], "/statuses", SC.TWITTER_POINTERS)


GITHUB_ROOT_POINTERS = SC.GITHUB_POINTERS
COMMIT_POINTERS = ["/sha", "/author/name", "/author/email", "/message", "/distinct", "/url", "", "/author", "/nope", "/author/name/0"]


def github_cases():
    from tests.conftest import load_fixture
    whole = load_fixture("github_events.json")
    events = SC.reserialised("github_events.json", lambda d: d)
    return [("github, one document", [whole], "", GITHUB_ROOT_POINTERS), ("github, one document per event", events, "/payload/commits", COMMIT_POINTERS)]


def saturated_count_documents():
    """hand-built tapes: an array header whose 24-bit scope count disagrees with its chain (five elements under a saturated
    0xFFFFFF, and under 2, and under 0) -> [oracle.Parsed]"""
    from oracle import oracle as O
    out = []
    for doc, field in ((b'[1,"two",[3],{"a":4},null]', 0xFFFFFF), (b'{"x":[1,"two",[3],{"a":4},null]}', 0xFFFFFF), (b'[1,"two",[3],{"a":4},null]', 2),
                       (b'[1,"two",[3],{"a":4},null]', 0)):
        p = O.parse(doc)
        at = 1 if doc[:1] == b"[" else 3
        w = int(p.tape[at])
        assert w >> 56 == ord("[") and (w >> 32) & 0xFFFFFF == 5
        tape = p.tape.copy()
        tape[at] = np.uint64((w & ~(0xFFFFFF << 32)) | (field << 32))
        out.append(O.Parsed(tape, p.strings, 0, 0, 0))
    return out


# ---- the seeded corpus: the documents of tests/select_fuzz.py, a base per case that the documents really contain --------------
def _array_pointers(v, tokens, out, depth=0):
    """every array of a to_python() tree that a pointer of at most 16 steps reaches (first matching key): pointer -> size"""
    if v[0] == "a":
        out.setdefault(F.pointer(tokens), len(v[2]))
        if depth < F.MAX_STEPS:
            for k, e in enumerate(v[2][:3]):
                _array_pointers(e, tokens + [b"%d" % k], out, depth + 1)
    elif v[0] == "o" and depth < F.MAX_STEPS:
        seen = set()
        for key, e in v[2]:
            if key not in seen and len(key) <= 64:
                seen.add(key)
                _array_pointers(e, tokens + [bytes(key)], out, depth + 1)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    """-> [(name, documents, [oracle.Parsed], base, element pointers, (row offsets, expected cells))], one per case of
    select_fuzz.corpus().  The base is chosen by the case's number from the arrays its documents hold: the one that is an
    array in most documents, the one that holds the largest array, a random one, and (every eighth case) a pointer that
    reaches an object or nothing.  The element pointers are drawn by select_fuzz.draw_plan from the elements themselves."""
    out = []
    for n, (name, docs, ptrs, parsed, _) in enumerate(F.parsed_corpus()):
        rng = random.Random(F.SEED * 77 + n)
        roots = [p.to_python() for p in parsed]
        sizes = {}  # pointer -> [size per document that has an array there]
        for r in roots:
            found = {}
            _array_pointers(r, [], found)
            for ptr, size in found.items():
                sizes.setdefault(ptr, []).append(size)
        cands = sorted(sizes)
        if n % 8 == 7 or not cands:
            base = rng.choice([b"/nope", b"/0/nope"] + [c + b"/x" for c in cands[:2]])
        elif n % 4 == 0:
            base = max(cands, key=lambda c: (max(sizes[c]), c))
        elif n % 4 == 1:
            base = max(cands, key=lambda c: (len(sizes[c]), sum(sizes[c]), c))
        else:
            base = rng.choice(cands)
        elems = [e for r in roots for e, _ in base_elements(r, base)]
        n_paths = F.PLAN_SIZES[(n + 3) % len(F.PLAN_SIZES)]
        eptrs = F.draw_plan(rng, elems[:: max(1, len(elems) // 40)], n_paths) if elems else [b"", b"/a"]
        if b"" not in eptrs:
            eptrs[-1] = b""  # the element itself: every type an element has is a result type
        out.append((name, docs, parsed, base, eptrs, expected_explode(parsed, base, eptrs)))
    return out


def fuzz_statistics():
    """what the corpus test asserts before anything else: counted from the oracle's trees alone"""
    st = {"cases": 0, "cases_with_rows": 0, "array_sizes": set(), "types": set(), "rows": 0, "cells": 0, "present": 0}
    for name, docs, parsed, base, eptrs, (offs, want) in fuzz_cases():
        st["cases"] += 1
        st["cases_with_rows"] += offs[-1] > 0
        st["rows"] += offs[-1]
        for p in parsed:
            root = p.to_python()
            cur = (root, 1)
            for token in SC.pointer_tokens(base):
                cur = SC._step(cur[0], cur[1], token) if cur is not None else None
            if cur is not None and cur[0][0] == "a":
                st["array_sizes"].add(len(cur[0][2]))
        for col in want:
            for t, _ in col:
                st["types"].add(t)
                st["cells"] += 1
                st["present"] += t != SC.MISSING
    return st
