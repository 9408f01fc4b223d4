"""Exhaustive short token sequences for the walkers' verdicts: which error a document gets when it holds more than one fault.

The cooperative walkers (csrc/coop_walk.hip) decide stage 2 with local predicates and scans; their contract is that a document's
error is the failing predicate at the LOWEST position, exactly where JsonIterator.java would have stopped -- also when a literal
that the walk defers (`-`, `nul`) and a grammar fault share one document, and when a stage-1 verdict meets either.  The families
below enumerate every such meeting up to a few tokens and put single faults at every lane of a token step in long documents; the
truth is the oracle's restatement (oracle/sj_oracle.c) alone.  tests/test_grammar_sweep_corpus.py pins the counts and the oracle's
code histograms, tests/test_gpu_grammar_sweep.py sends every family through every entry of the device parse.

A document is its tokens joined by one blank.  Plain module: no import of the product, not a conftest."""
import itertools

import numpy as np

T9 = [b"[", b"{", b"]", b"}", b'"s"', b"1", b"true", b",", b":"]
T13 = T9 + [b"-", b"nul", b"1.5", b"null"]
# an unclosed string, a control character in a string, a truncated UTF-8 sequence: the three stage-1 verdicts
T12S = T9 + [b'"u', b'"\x01"', b'"\xc3"']

DEFERRED = {b"-": b"1", b"nul": b"null"}  # the bad literals of T13 and what mends them

EDIT_UNITS = (1, 2, 3, 5)


def sequences(tokens, longest):
    """every sequence of 1..longest tokens, shortest first, each length in product order"""
    return [b" ".join(seq) for n in range(1, longest + 1) for seq in itertools.product(tokens, repeat=n)]


def n_sequences(n_tokens, longest):
    return sum(n_tokens ** n for n in range(1, longest + 1))


def short9(longest=6):
    return sequences(T9, longest)


def short13():
    return sequences(T13, 5)


def short12s():
    return sequences(T12S, 4)


def unit_tokens():
    """the object of tests/single_doc_layouts.py (UNIT_TOKENS without its trailing comma) with a -2.5 at the end of its inner array,
    `"n":[1,{"x":null},-2.5]`: 29 tokens, 7 of them (six strings and the float) outside T13"""
    from tests.single_doc_layouts import UNIT_TOKENS
    unit = [t.encode() for t in UNIT_TOKENS[:-1]]
    at = len(unit) - 2  # in front of the inner array's closing bracket
    assert unit[at:] == [b"]", b"}"]
    unit[at:at] = [b",", b"-2.5"]
    assert len(unit) == 29 and sum(t not in T13 for t in unit) == 7
    return unit


def edit_base(units):
    """`[ UNIT , UNIT , ... ]`: 30 * units + 1 tokens"""
    unit, out = unit_tokens(), [b"["]
    for u in range(units):
        out += ([b","] if u else []) + unit
    return out + [b"]"]


def edits_of(base):
    """single-token edits: in front of every position (and behind the last token) each T13 token inserted; at every position the
    token deleted, and replaced by each other T13 token"""
    out = []
    for p in range(len(base) + 1):
        out += [base[:p] + [t] + base[p:] for t in T13]
        if p < len(base):
            out.append(base[:p] + base[p + 1:])
            out += [base[:p] + [t] + base[p + 1:] for t in T13 if t != base[p]]
    return [b" ".join(d) for d in out]


def edits(units=EDIT_UNITS):
    return [d for u in units for d in edits_of(edit_base(u))]


FAMILIES = {"short9": short9, "short13": short13, "short12s": short12s, "edits": edits}
COUNTS = {"short9": 597870, "short13": 402233, "short12s": 22620, "edits": 826 + 1613 + 2400 + 3974}
SHORT9_UP_TO_5 = n_sequences(9, 5)  # short9 lists the shorter sequences first: its first 66,429 documents

_docs, _answers = {}, {}


def family(name):
    """the documents of one family (built once: a later caller gets the same list and must leave it unchanged)"""
    if name not in _docs:
        _docs[name] = FAMILIES[name]()
        assert len(_docs[name]) == COUNTS[name], (name, len(_docs[name]))
    return _docs[name]


def pack(docs):
    """each document followed by one '\\n' -> (buffer, offsets uint64[n + 1]); what tests/test_gpu_batch.py's _pack gives"""
    lengths = np.fromiter(map(len, docs), dtype=np.int64, count=len(docs))
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum(lengths + 1, out=offs[1:])
    return (b"\n".join(docs) + b"\n") if docs else b"", offs


def oracle_errors(docs, max_depth=1024):
    """the oracle's error code of every document + '\\n' (sjo_digest_many: stage 1 and stage 2 of the restatement, in C)"""
    import os
    from oracle import oracle as O
    buf, offs = pack(docs)
    return O.digest_many(buf, offs, max_depth=max_depth, threads=min(16, os.cpu_count() or 1))[1]


def answers(name, max_depth=1024):
    """-> (errors int32[n], {k: oracle.Parsed} for the documents with error 0) of family `name`, from the oracle; made once per
    process and shared: leave both unchanged"""
    from oracle import oracle as O
    if (name, max_depth) not in _answers:
        docs = family(name)
        errors = oracle_errors(docs, max_depth)
        parsed = {int(k): O.parse(docs[k] + b"\n", max_depth=max_depth) for k in np.nonzero(errors == 0)[0]}
        assert all(p.error == 0 for p in parsed.values())
        errors.setflags(write=False)
        _answers[(name, max_depth)] = errors, parsed
    return _answers[(name, max_depth)]


def histogram(errors):
    codes, counts = np.unique(errors, return_counts=True)
    return {int(c): int(n) for c, n in zip(codes, counts)}


def two_faults(docs, errors):
    """-> bool[n]: the document holds a bad literal of T13 AND is still rejected with every such token mended (`-` -> `1`,
    `nul` -> `null`): a deferred literal and another fault in one document.  `docs` must hold the mended documents too."""
    where = {d: k for k, d in enumerate(docs)}
    out = np.zeros(len(docs), dtype=bool)
    for k, d in enumerate(docs):
        tokens = d.split(b" ")
        if any(t in DEFERRED for t in tokens):
            out[k] = errors[where[b" ".join(DEFERRED.get(t, t) for t in tokens)]] != 0
    return out


def shuffled(docs, seed):
    """-> (permutation int64[n], the documents in that order): every seam of a run gets unrelated neighbours"""
    perm = np.random.RandomState(seed).permutation(len(docs))
    return perm, [docs[i] for i in perm]


def predicted_lengths(docs, errors=None):
    """tests/tok_stream_layouts.py's predicted_length for a whole list: the tape slot laid out for a document before the walk,
    2 + 1 per token + 1 more per number; -1 where the document fails stage 1.  errors: the oracle's codes, if at hand.

    The documents that pass stage 1 are indexed as ONE buffer, a '\\n' behind each: a document that passes on its own ends outside
    a string, and the blank in front of the next one makes that one's first scalar a structural as its own start does."""
    from oracle import oracle as O
    if errors is None:
        errors = oracle_errors(docs)
    errors = np.asarray(errors)
    ok = ~((errors >= 1) & (errors <= 3))
    out = np.full(len(docs), -1, dtype=np.int64)
    buf, offs = pack([d for d, o in zip(docs, ok) if o])
    idx, st = O.stage1(buf)
    assert st == 0
    first = np.frombuffer(buf, dtype=np.uint8)[idx.astype(np.int64)]
    token = (first != 0x2C) & (first != 0x3A)
    number = (first == 0x2D) | ((first >= 0x30) & (first <= 0x39))
    doc_of = np.searchsorted(offs.astype(np.int64), idx.astype(np.int64), side="right") - 1
    out[ok] = 2 + np.bincount(doc_of, weights=token.astype(np.int64) + number, minlength=int(ok.sum())).astype(np.int64)
    return out
