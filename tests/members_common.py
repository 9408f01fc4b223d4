"""What a members explode and a key census must give, from the oracle alone: the base pointer resolved on
oracle.Parsed.to_python() with the steps of tests/select_common.py, the base OBJECT's members taken from the oracle's own walk
(key at p, value at p + 1, p += 1 + the value's words), explode_common.expected_cell on each member's value, and the key as a
string cell behind them; the census is a Python Counter over (index, class).  Shares no code with the product.  Used by the
host simulations' tests, the GPU tests and tools/bench_members.py; every cell is compared."""
import collections
import functools
import random

import numpy as np

from tests import explode_common as EC
from tests import select_common as SC
from tests import select_fuzz as F

QUOTE = ord('"')
CLASSES = 8
CLASS_OF = {ord("l"): 0, ord("d"): 1, QUOTE: 2, ord("t"): 3, ord("f"): 3, ord("n"): 4, ord("["): 5, ord("{"): 6}


def header_constant(name):
    """an unsigned #define of include/sjmi.h, evaluated (SJMI_EXPLODE_MEMBERS_MAX_PATHS is written by SJMI_SELECT_MAX_PATHS)"""
    import os
    import re
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "include", "sjmi.h")).read()
    body = re.search(r"#define\s+%s\s+(.+?)\s*(?:/\*.*)?$" % name, text, re.M).group(1)
    body = re.sub(r"SJMI_[A-Z_]+", lambda m: str(header_constant(m.group(0))), body)
    return int(eval(re.sub(r"(\d+)u\b", r"\1", body), {"__builtins__": {}}))


def base_members(root, base):
    """-> [(key bytes, value, the value's tape index)] of the object the base pointer reaches in a to_python() tree, duplicates
    included, in tape order; [] when there is none"""
    cur = (root, 1)  # the root value is tape word 1
    for token in SC.pointer_tokens(base):
        cur = SC._step(cur[0], cur[1], token)
        if cur is None:
            return []
    v, idx = cur
    if v[0] != "o":
        return []
    out, p = [], idx + 1
    for key, val in v[2]:
        out.append((bytes(key), val, p + 1))
        p += 1 + SC._words(val)
    return out


def expected_members(parsed_docs, base, pointers):
    """parsed_docs: oracle.Parsed or None (a failed document) per document -> (row_offsets [n + 1], [column][row]): a column of
    expected_cell per element pointer, then the key column"""
    offs, cols = [0], [[] for _ in range(len(pointers) + 1)]
    for p in parsed_docs:
        members = [] if p is None or p.error else base_members(p.to_python(), base)
        for key, val, idx in members:
            for q, ptr in enumerate(pointers):
                cols[q].append(EC.expected_cell(val, idx, ptr))
            cols[-1].append((QUOTE, key))
        offs.append(offs[-1] + len(members))
    return offs, cols


def buffer_rows(n_cols):
    """the rows k_explode_rows buffers for n_cols columns (csrc/explode.hip: EXP_ROWS, EXP_CELLS) -- where its edges lie"""
    return min(8, 96 // n_cols)


def _obj(n, value=lambda k: "%d" % k):
    return ("{" + ",".join('"k%d":%s' % (k, value(k)) for k in range(n)) + "}").encode()


ELEMENT_POINTERS = EC.ELEMENT_POINTERS
MEMBER_COUNTS = [0, 1, 7, 8, 9, 15, 16, 17, 33]


def pointers_for(n_cols):
    """n_cols - 1 element pointers: the fixed ones, then padding that misses"""
    base = ["", "/a", "/0", "/b/c"]
    return (base + ["/pad%d" % k for k in range(64)])[:n_cols - 1]


def size_cases():
    """objects of every MEMBER_COUNTS size at the root and under /o, for every column count that moves a buffer edge
    -> [(name, documents, base, element pointers)]"""
    out = []
    values = lambda k: ['%d' % k, '"s%d"' % k, '{"a":%d,"b":{"c":null}}' % k, '[%d,[1]]' % k, "true", "null", "1.5"][k % 7]
    for n_cols in (1, 2, 12, 13, 64):
        docs = [_obj(n, values) for n in MEMBER_COUNTS]
        out.append(("sizes at the root, %d columns" % n_cols, docs, "", pointers_for(n_cols)))
        out.append(("sizes under a key, %d columns" % n_cols, [b'{"x":1,"o":' + d + b',"y":[2]}' for d in docs], "/o", pointers_for(n_cols)))
    return out


def base_cases():
    """-> [(name, [document bytes], base pointer, [element pointer])]"""
    S = SC.slice_words()
    ints = [str(v) for v in SC.HEADER_LOOKING]
    dbls = [SC._double_text(v) for v in SC.HEADER_LOOKING[:6]]
    P = ELEMENT_POINTERS
    return [
        ("base at the root", [b'{"a":1,"b":"s","c":null}', b'{}', b'{"":0}', b'[{"a":1}]', b'7', b'"{}"'], "", P),
        ("deep base", [b'{"a":{"b":{"c":{"k":1,"l":[2],"m":{"a":3}}}}}', b'{"a":{"b":{"c":{}}}}', b'{"a":{"b":5}}'], "/a/b/c", P),
        ("base through an array index", [b'{"a":[0,{"b":[[1],{"x":{"a":[5,6]},"y":{"a":{"0":"k"}}}]}]}', b'{"a":[0,{"b":[[1]]}]}', b'{"a":[0]}'], "/a/1/b/1", P),
        ("base behind duplicate keys", [b'{"o":{"first":1},"o":{"second":2,"third":3}}', b'{"o":5,"o":{"k":1}}', b'{"x":{"o":{"n":9}},"o":{"a":{"a":1},"a":2},"o":{}}'], "/o", P),
        ("base missing", [b'{"x":{"a":1}}', b'{"o":{"k":1}}', b'{}', b'[]', b'7', b'{"x":{"o":{"k":1}}}'], "/o", P),
        ("base an array", [b'{"o":[{"a":1},{"b":2}]}', b'{"o":{"k":[1,2]}}', b'{"o":[]}', b'[1,2]'], "/o", P),
        ("base a scalar", [b'{"o":5}', b'{"o":null}', b'{"o":true}', b'{"o":1.5}', b'{"o":{"k":5}}', b'{"o":false}', b'{"o":"{\\"k\\":1}"}'], "/o", P),
        ("duplicate keys inside the base", [b'{"a":1,"a":"two","b":3,"a":[4],"b":{"a":5}}', b'{"k":1,"k":2,"k":3}'], "", P),
        ("the empty key", [b'{"":1,"a":2,"":{"":3}}', b'{"":{"":{"":1}}}', b'{"":""}'], "", P + ["/"]),
        ("escaped keys", [b'{"\\u0041":1,"A":2,"q\\"r":3,"\\u00e9":4,"a\\\\b":{"a":5},"\\n":"nl"}', b'{"\\u0061":{"\\u0061":1}}'], "", P),
        ("inner members are not rows", [b'{"a":{"b":{"c":"deep","d":1},"e":2},"f":[{"g":1,"h":2},[3]],"i":{"j":{"k":{"l":1}}}}',
                                         b'{"o":{"p":{"q":1,"r":2,"s":3}}}'], "", P),
        ("header-looking integers", [("{" + ",".join('"k%d":%s' % (i, v) for i, v in enumerate(ints)) + "}").encode()] +
         [('{"a":%s,"b":{"c":%s},"c":%s,"d":[%s,%s]}' % (ints[i], ints[(i + 1) % 10], ints[(i + 2) % 10], ints[(i + 3) % 10], ints[(i + 4) % 10])).encode()
          for i in range(10)], "", P),
        ("header-looking doubles", [("{" + ",".join('"k%d":%s' % (i, v) for i, v in enumerate(dbls)) + "}").encode()] +
         [('{"a":%s,"b":{"c":%s},"c":%s,"d":[%s,%s]}' % (dbls[i], dbls[(i + 1) % 6], dbls[(i + 2) % 6], dbls[(i + 3) % 6], dbls[(i + 4) % 6])).encode()
          for i in range(6)], "", P),
        ("around the slice, base at the front", [SC.sized_document(S - 1), SC.sized_document(S), SC.sized_document(S + 1), SC.sized_document(2 * S + 1),
                                                   b'{"pad":[[1],2]}'], "", ["", "/0", "/x/1"]),
        ("around the slice, base at the end", [SC.sized_document(S - 1), SC.sized_document(S), SC.sized_document(S + 1), SC.sized_document(2 * S + 1)],
         "/last", ["", "/0"]),
        ("failed documents between good ones", [b'{"a":1,"b":2}', b'{"a":1,}', b'{"c":3}', b'{"a"', b'{"a":"\\q"}', b'{"d":4,"e":5,"f":6}', b'{"a":}', b'{"a":"abc',
                                                 b'{"g":7}'], "", ["", "/a"]),
        ("no element pointers", [b'{"a":1,"b":2}', b'{}', b'{"c":3}'], "", []),
        ("duplicate element pointers", [b'{"x":{"a":1},"y":{"a":"s"},"z":{}}', b'{"w":{"a":[2]}}'], "", ["/a", "", "/a", "/a", ""]),
    ]


def github_cases():
    events = SC.reserialised("github_events.json", lambda d: d)
    return [("github, the events' root", events, "", ["", "/login", "/commits/0/sha", "/id"]),
            ("github, the events' payload", events, "/payload", ["", "/0/sha", "/login", "/labels/0/name"])]


def hand_built_scope_counts():
    """hand-built tapes: an object header whose 24-bit scope count disagrees with its chain (five members under a saturated
    0xFFFFFF, under 2 and under 0) -> [(oracle.Parsed, base)]"""
    from oracle import oracle as O
    out = []
    for doc, at, base, field in ((b'{"a":1,"b":"two","c":[3],"d":{"a":4},"e":null}', 1, "", 0xFFFFFF),
                                 (b'{"x":{"a":1,"b":"two","c":[3],"d":{"a":4},"e":null}}', 3, "/x", 0xFFFFFF),
                                 (b'{"a":1,"b":"two","c":[3],"d":{"a":4},"e":null}', 1, "", 2),
                                 (b'{"a":1,"b":"two","c":[3],"d":{"a":4},"e":null}', 1, "", 0)):
        p = O.parse(doc)
        w = int(p.tape[at])
        assert w >> 56 == ord("{") and (w >> 32) & 0xFFFFFF == 5
        tape = p.tape.copy()
        tape[at] = np.uint64((w & ~(0xFFFFFF << 32)) | (field << 32))
        out.append((O.Parsed(tape, p.strings, 0, 0, 0), base))
    return out


def capacity_cuts(offsets):
    """row capacities that cut a document after its first member, before its last, and exactly at its end (and none, and room)"""
    total, cuts = offsets[-1], {0, offsets[-1], offsets[-1] + 3}
    for lo, hi in zip(offsets, offsets[1:]):
        if hi - lo >= 3:
            cuts |= {lo + 1, hi - 1, hi}
    return sorted(c for c in cuts if c <= total + 3)


# ---- the seeded corpus: the documents of tests/select_fuzz.py, an object base per case --------------------------------------
def _object_pointers(v, tokens, out, depth=0):
    """every object of a to_python() tree that a pointer of at most 16 steps reaches (first matching key): pointer -> size"""
    if v[0] == "o":
        out.setdefault(F.pointer(tokens), len(v[2]))
        if depth < F.MAX_STEPS:
            seen = set()
            for key, e in v[2]:
                if key not in seen and len(key) <= 64:
                    seen.add(key)
                    _object_pointers(e, tokens + [bytes(key)], out, depth + 1)
    elif v[0] == "a" and depth < F.MAX_STEPS:
        for k, e in enumerate(v[2][:3]):
            _object_pointers(e, tokens + [b"%d" % k], out, depth + 1)


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    """-> [(name, documents, [oracle.Parsed], base, element pointers, (row offsets, expected columns))], one per case of
    select_fuzz.corpus().  The base is chosen by the case's number from the objects its documents hold, as
    explode_common.fuzz_cases chooses arrays: the one that holds the largest object, the one that is an object in most
    documents, a random one, and (every eighth case) a pointer that reaches an array, a scalar or nothing.  The element
    pointers are drawn by select_fuzz.draw_plan from the members' values; a members plan has at most 63."""
    limit = header_constant("SJMI_EXPLODE_MEMBERS_MAX_PATHS")
    out = []
    for n, (name, docs, ptrs, parsed, _) in enumerate(F.parsed_corpus()):
        rng = random.Random(F.SEED * 79 + n)
        roots = [p.to_python() for p in parsed]
        sizes = {}
        for r in roots:
            found = {}
            _object_pointers(r, [], found)
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
        values = [val for r in roots for _, val, _ in base_members(r, base)]
        n_paths = min(F.PLAN_SIZES[(n + 3) % len(F.PLAN_SIZES)], limit)
        eptrs = F.draw_plan(rng, values[:: max(1, len(values) // 40)], n_paths) if values else [b"", b"/a"]
        if b"" not in eptrs:
            eptrs[-1] = b""  # the value itself: every type a member's value has is a result type
        out.append((name, docs, parsed, base, eptrs, expected_members(parsed, base, eptrs)))
    return out


def fuzz_statistics():
    """what the corpus test asserts before anything else: counted from the oracle's trees alone"""
    st = {"cases": 0, "cases_with_rows": 0, "types": set(), "rows": 0, "cells": 0, "present": 0, "sizes": set()}
    for name, docs, parsed, base, eptrs, (offs, want) in fuzz_cases():
        st["cases"] += 1
        st["cases_with_rows"] += offs[-1] > 0
        st["rows"] += offs[-1]
        st["sizes"] |= set(int(x) for x in np.diff(offs))
        for col in want[:-1]:
            for t, _ in col:
                st["types"].add(t)
                st["cells"] += 1
                st["present"] += t != SC.MISSING
    return st


# ---- the census -----------------------------------------------------------------------------------------------------------
def census_class(t):
    return CLASS_OF.get(int(t), 7)


def pack_bits(bits):
    """a bool per row -> the LSB-first validity words (uint64)"""
    padded = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded, bitorder="little").view(np.uint64).copy()


def expected_census(indices, validity_bits, types, n_keys, live):
    """indices (ints), validity_bits (None: all valid, else a bool per row), types (bytes / ints), the first `live` rows
    -> (counts [n_keys][8], n_counted, n_out_of_range)"""
    c, outside = collections.Counter(), 0
    for r in range(live):
        if validity_bits is not None and not validity_bits[r]:
            continue
        ix = int(indices[r])
        if 0 <= ix < n_keys:
            c[(ix, census_class(types[r]))] += 1
        else:
            outside += 1
    counts = [[c[(k, cl)] for cl in range(CLASSES)] for k in range(n_keys)]
    return counts, sum(c.values()), outside


def expected_census_large(indices, validity_bits, types, n_keys, live):
    """expected_census for columns of a million rows: the same count, the Counter being numpy's bincount over index * 8 + class
    (tests/test_host_census.py holds the two against each other)"""
    ix = np.asarray(indices[:live], dtype=np.int64)
    valid = np.ones(live, dtype=bool) if validity_bits is None else np.asarray(validity_bits[:live], dtype=bool)
    inside = valid & (ix >= 0) & (ix < n_keys)
    table = np.full(256, 7, dtype=np.int64)
    for t, cl in CLASS_OF.items():
        table[t] = cl
    bins = ix[inside] * CLASSES + table[np.asarray(types[:live], dtype=np.uint8)[inside]]
    counts = np.bincount(bins, minlength=n_keys * CLASSES).reshape(n_keys, CLASSES)
    return counts.tolist(), int(inside.sum()), int((valid & ~inside).sum())


def python_key_census(pairs_per_document):
    """[[(key str, value)] per document] (json.loads(..., object_pairs_hook=list) of the base objects, None where there is none)
    -> [(key bytes, [8 counts])] in first-occurrence order, from Python's own types"""
    order, counts = [], {}
    for pairs in pairs_per_document:
        for key, val in pairs or []:
            k = key.encode("utf-8")
            if k not in counts:
                counts[k] = [0] * CLASSES
                order.append(k)
            if isinstance(val, bool):
                cl = 3
            elif isinstance(val, int):
                cl = 0
            elif isinstance(val, float):
                cl = 1
            elif isinstance(val, str):
                cl = 2
            elif val is None:
                cl = 4
            elif isinstance(val, Pairs):  # (a list too: asked first)
                cl = 6
            else:
                assert isinstance(val, list)
                cl = 5
            counts[k][cl] += 1
    return [(k, counts[k]) for k in order]


class Pairs(list):
    """what object_pairs_hook makes of an object, told apart from an array"""


def loads_pairs(text):
    import json
    return json.loads(text, object_pairs_hook=Pairs)


def resolve_pairs(doc, base):
    """the base object's pairs of a loads_pairs() document, by first matching key / index; None when the base is no object"""
    cur = doc
    for token in SC.pointer_tokens(base):
        tok = token.decode("utf-8")
        if isinstance(cur, Pairs):
            hit = [v for k, v in cur if k == tok]
            if not hit:
                return None
            cur = hit[0]
        elif isinstance(cur, list):
            if not SC._INDEX.fullmatch(token) or int(tok) >= len(cur):
                return None
            cur = cur[int(tok)]
        else:
            return None
    return cur if isinstance(cur, Pairs) else None
