"""Seam layouts for the stream walker (k_tok_stream, coop_walk.hip; its model tools/tok_stream_model.py): batches in which broken
documents of every kind stand directly beside well-formed ones, at every lane of a token step and at every position of a run.

A wave walks a RUN of consecutive documents as one token stream, so a 64-token step can hold the end of one document, a whole small
one and the start of a third.  The layout is `filler, broken, valid, broken, broken, valid, ...` in groups of GROUP documents: the
filler `[1,1,...]` of p tokens (p swept over 0..127, the ring's size) shifts every seam behind it through every lane of a step
(steps are 64 tokens, or 63 in front of an opening bracket whose successor is not at hand yet, so sweeping covers every phase
either way), and GROUP is prime and above every run size under test, so each seam also lands first, in the middle, last and across a
run boundary.

Each document carries the mechanism by which the stream walker is expected to notice it (KINDS).  Plain module, not a conftest."""
import random

# kind -> documents.  The mechanism, in the kernel's terms:
#   s1       fails stage 1: the run goes to the exact walker whole
#   empty    no structural at all: sent alone, the run goes on
#   sep      separators only: failed by the ingest
#   bad      a BAD token in its own step (grammar, LOW = a token at depth < 1 after the root's end, a bad string, DEEP)
#   nc       its root not closed when the next document starts (NC), or the run's last one (A_d != c_dbase)
#   lit      fails only in the deferred literal parser, after the stream walker wrote its words
#   scalar   a valid scalar root: the exact walker's
#   deep     valid, deeper than the walker's 63 levels: the exact walker's
BROKEN = {
    "s1": [b'["abc', b'[1,"a\x01"]', bytes([0x5B, 0x22, 0xC3, 0x22, 0x5D]), b'{"k":"\xff"}'],
    "empty": [b"", b"   ", b"\t"],
    "sep": [b",", b":", b",,"],
    "bad": [b"[1 2]", b'{"a"}', b"[,]", b"[1]]", b"[] []", b"[1],2", b"[1] [2,[3]]", b'{} {"a":[1]}', b"]]]][[[[", b'["\\q"]',
            b'{"a":1,}', b"[1,]", b'{"k":2"v"}', b"}", b"[}"],
    "nc": [b"[", b"[1,2", b'{"a":[1', b"[[[[1", b'[{"a":[{"b":[1', b'{"a":[1,2,3', b'{"x":{"y":{', b"[[],[", b'[{"a":{}},'],
    "lit": [b"[tru]", b"[01]", b"[-]", b"[1e]", b'{"a":nul}', b"[1,2,fals]"],
    "scalar": [b"7", b'"s"', b"true", b"-1.5e3", b"null"],
    "deep": [b"[" * 64 + b"]" * 64, b"[" * 70 + b"1" + b"]" * 70],
}


def _nested(depth, rng):
    """a well-formed document `depth` levels deep, containers of both kinds"""
    out, close = [], []
    for i in range(depth):
        if rng.random() < 0.5:
            out.append(b"[1,")
            close.append(b"]")
        else:
            out.append(b'{"k%d":' % i)
            close.append(b"}")
    return b"".join(out) + b"2" + b"".join(reversed(close))


def _unclosed(depth, rng):
    """open `depth` levels, close none of them (an NC document of that depth)"""
    return b"".join(rng.choice([b"[", b"[1,", b'{"a":', b'{"a":1,"b":']) for _ in range(depth)) + b"1"


def _valid(rng):
    r = rng.random()
    if r < 0.15:
        return rng.choice([b"[]", b"{}"])
    if r < 0.3:
        return rng.choice([b'[{"b":1}]', b'{"a":[1,2,3]}', b'[[1,2],{"c":[]}]', b'{"a":{"b":{"c":[true,null]}}}', b'["x","y\\n"]'])
    if r < 0.45:  # across one or more step boundaries
        n = rng.choice([40, 63, 64, 65, 100, 140, 200])
        return b"[" + b",".join(rng.choice([b"1", b'"s"', b"[]", b"{}", b"true", b"-2.5"]) for _ in range(n)) + b"]"
    if r < 0.55:  # levels 62-63: a negative-depth neighbour's wrapped levels are real here
        return _nested(rng.choice([61, 62, 63]), rng)
    if r < 0.75:
        return _nested(rng.randint(1, 12), rng)
    n = rng.randint(1, 30)
    return b"{" + b",".join(b'"k%d":%s' % (i, rng.choice([b"1", b"[1,2]", b'{"z":null}', b'"v"', b"[]"])) for i in range(n)) + b"}"


GROUP = 23  # documents per group: prime, above every run size under test (1, 2, 3, 5, 8, 16)
PATTERN = "BVBBV"  # broken, valid, broken, broken, valid, ... behind the filler


def filler(p):
    """a well-formed document of exactly p tokens (p = 0: none)"""
    if p == 0:
        return None
    if p == 1:
        return b'"f"'
    return b"[" + b",".join([b"1"] * (p - 2)) + b"]"


def broken_pool(rng, kinds=None):
    """every broken document, each NC depth 1..62 among them"""
    pool = []
    for kind, docs in BROKEN.items():
        if kinds is None or kind in kinds:
            pool += [(kind, d) for d in docs]
    if kinds is None or "nc" in kinds:
        pool += [("nc", _unclosed(k, rng)) for k in range(1, 63)]
    return pool


def groups(seed=0, n_groups=128, kinds=None, group=GROUP):
    """-> list of groups, each a list of (kind, document); kind "valid" / "filler" for the well-formed ones.  Group g has a filler of
    g % 128 tokens; the broken documents cycle through the pool so that each kind meets every filler length in turn."""
    rng = random.Random(seed)
    pool = broken_pool(rng, kinds)
    rng.shuffle(pool)
    out, b = [], 0
    for g in range(n_groups):
        f = filler(g % 128)
        docs = [("filler", f)] if f is not None else []
        i = 0
        while len(docs) < group:
            if PATTERN[i % len(PATTERN)] == "B":
                docs.append(pool[b % len(pool)])
                b += 1
            else:
                docs.append(("valid", _valid(rng)))
            i += 1
        out.append(docs)
    return out


def batch(seed=0, n_docs=18000, kinds=None):
    """-> (documents, kinds): groups laid end to end up to about n_docs documents (every filler length 0..127 many times over)"""
    gs = groups(seed, (n_docs + GROUP - 1) // GROUP, kinds)
    docs = [d for g in gs for _, d in g]
    return docs, [k for g in gs for k, _ in g]


def tokens(doc):
    """the document's tokens: structurals other than ',' and ':' (None if it fails stage 1)"""
    from oracle import oracle as O
    idx, st = O.stage1(doc)
    if st:
        return None
    return sum(1 for x in idx if doc[int(x)] not in b",:")


def predicted_length(doc):
    """the tape slot laid out for a document before the walk: 2 + 1 per token + 1 more per number (None if it fails stage 1)"""
    from oracle import oracle as O
    idx, st = O.stage1(doc)
    if st:
        return None
    words = 2
    for x in idx:
        c = doc[int(x)]
        if c in b",:":
            continue
        words += 2 if (c == 0x2D or 0x30 <= c <= 0x39) else 1
    return words
