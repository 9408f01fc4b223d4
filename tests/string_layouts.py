"""Granule-edge layouts for the streaming string pass (k_strings, simdjson-java_amd/csrc/strings.hip): documents that put string
openings, closings, escapes, errors, backslash runs and \\uXXXX sequences at the places where the pass hands state from one
64-byte block (one lane) to the next and from one 4 KiB granule (one wave's unit of work) to the next.

What crosses those edges in the kernel:
  * a string still open at a granule's end gets its header from the granule that closes it, which walks back over the OPEN
    RECORDS of the granules in between; that string's first error travels along the same walk;
  * a backslash run longer than the 8 bytes in front of a block resolves through sj_carry_slow, one longer than the 16-byte
    halo through sj_backslash_run_parity; lane 0 of a granule looks for a \\u sequence reaching into it in its halo;
  * a granule with at most STR_UQ_ITEMS = 128 \\uXXXX items (a surrogate pair is one) decodes them from an LDS queue, one with
    more in a lane-local loop;
  * "a""b" (a closing quote directly in front of an opening one) takes the g.bad fix-up; a granule of nothing but quotes fills
    the tile to its bound.

Every layout passes stage 1 (tests/test_string_layouts.py checks it) and carries MARKS: (absolute offset, bytes expected there)
for each named feature, so that a test can assert that the feature sits where its label says.  Offsets are relative to the
document's first byte.  Plain module, not a conftest."""
import collections
import itertools
import random

G = 4096  # bytes of a granule
BLK = 64  # bytes of a block

Layout = collections.namedtuple("Layout", "family label doc marks")

# every error kind of StringParser.parseString (tests/golden/vectors.py STRING_ERRORS without the trailing-content and
# unclosed-string vectors, which stage 1 / stage 2 decide), plus the reserved low surrogate; each as it sits inside a longer
# string, followed by a byte that is no hex digit, no backslash and no quote
ERRORS = [
    ("low_no_u", b"\\uD8001"), ("low_no_u", b"\\uD800\\1"), ("low_no_u", b"\\uD800u"), ("low_no_u", b"\\uD800\\e"),
    ("low_no_u", b"\\uD800\\DC00"), ("low_no_u", b"\\uD800"), ("low_no_u", b"\\uD83Dx"),
    ("low_range", b"\\uD800\\u"), ("low_range", b"\\uD83D\\u0041"), ("low_range", b"\\uD83D\\uD83D"),
    ("low_reserved", b"\\uDE00"),
    ("bad_unicode", b"\\u"), ("bad_unicode", b"\\u1"), ("bad_unicode", b"\\u12"), ("bad_unicode", b"\\u123"), ("bad_unicode", b"\\u12G4"),
    ("escape", b"\\g"), ("escape", b"\\q"), ("escape", "\\ą".encode()),
]
# filler of failing strings: no hex digit, no 'u', no backslash, no quote (nothing can extend an error sequence)
_PLAIN = b"ghijklmnopqrstvwxyz"


def plain(n, phase=0):
    return bytes(_PLAIN[(phase + i) % len(_PLAIN)] for i in range(n))


_TOKENS = [b"abcdefgh", b"\\n", b"\\u00e9", b"\\\\", b"xyz ", b"\\uD83D\\uDE00", b"\\t", b"\\u20AC", b"\\/", b"\xc3\xa9", b"IJKLMNOPQRSTUVWXYZ"]


def body(n, seed=0):
    """n bytes of valid string content with escapes and UTF-8 sprinkled in; no quote, no escaped quote (a middle granule of a
    long string holds no quote byte at all), never ending inside an escape"""
    rng = random.Random(seed)
    out = bytearray()
    while True:
        t = rng.choice(_TOKENS)
        if len(out) + len(t) > n:
            break
        out += t
    return bytes(out) + b"a" * (n - len(out))


def edges(step, phase, exclude_granules=False):
    """absolute positions k * step + phase, k >= 1 (without the granule edges if asked: block edges that are only block edges)"""
    for k in itertools.count(1):
        if exclude_granules and (k * step) % G == 0:
            continue
        yield k * step + phase


def pack(items, close=b"]"):
    """items: (literal, anchor, step, phase, exclude_granules, marks) -> an array document in which each literal's byte `anchor`
    sits at the next position k * step + phase that leaves room behind the previous literal; marks: (offset in the literal, bytes).
    -> (document, absolute marks)."""
    out = bytearray(b"[")
    amarks = []
    for lit, anchor, step, phase, excl, marks in items:
        sep = b"," if len(out) > 1 else b""
        for e in edges(step, phase, excl):
            start = e - anchor
            if start >= len(out) + len(sep):
                break
        out += sep + b" " * (start - len(out) - len(sep))
        assert len(out) == start
        out += lit
        amarks += [(start + r, m) for r, m in marks]
    out += close
    return bytes(out), amarks


def single(prefix_valid, lit, marks, anchor, at, after):
    """one document: valid strings, then `lit` with byte `anchor` at absolute offset `at`, then the strings `after`"""
    out = bytearray(b"[" + b",".join(prefix_valid))
    start = at - anchor
    sep = b"," if len(out) > 1 else b""
    assert start >= len(out) + len(sep), (start, len(out))
    out += sep + b" " * (start - len(out) - len(sep)) + lit
    out += b"".join(b"," + a for a in after) + b"]"
    return bytes(out), [(start + r, m) for r, m in marks]


VALID_AFTER = [b'"after\\n"', b'"\\u00e9\\uD83D\\uDE00"', b'"' + body(5000, 7) + b'"', b'""', b'"z"']


# ---- 1. strings that cross 1, 2, 3 and 5 granule edges ------------------------------------------------------------------
OPEN_AT = (4093, 4094, 4095, 4096, 4097)
CLOSE_AT = (0, 1, 2, 4093, 4094, 4095)
SPANS = (1, 2, 3, 5)


def spanning(span, o, c, seed=0, content=None):
    """a string whose opening quote sits at granule-relative offset o (4096, 4097: bytes 0, 1 of the next granule) of a granule
    and whose closing quote sits at offset c of the granule `span` granules behind the opening quote's granule
    -> (literal, the opening quote's offset in its granule, body length)"""
    o_rel = o % G
    n = span * G + c - o_rel - 1
    b = content(n) if content else body(n, seed)
    return b'"' + b + b'"', o_rel, n


def family_spans():
    out = []
    for span in SPANS:
        items = []
        for o in OPEN_AT:
            for c in CLOSE_AT:
                lit, ph, n = spanning(span, o, c, seed=span * 100 + o + c)
                items.append((lit, 0, G, ph, False, [(0, b'"'), (n + 1, b'"')]))
        doc, marks = pack(items)
        out.append(Layout(1, "30 strings, each crossing %d granule edge(s): opening quote at granule offsets %s, closing at %s"
                          % (span, OPEN_AT, CLOSE_AT), doc, marks))
    return out


# ---- 2. errors inside those strings -------------------------------------------------------------------------------------
def failing_spanning(span, o, c, errs):
    """the string of spanning(), plain content with the errors `errs` = [(where, bytes)] placed: 'open' = right behind the
    opening quote, 'middle' = offset 2000 of the first granule behind the opening one, 'close' = ending at the closing quote"""
    o_rel = o % G
    n = span * G + c - o_rel - 1
    content = bytearray(plain(n))
    marks = []
    for where, e in errs:
        if where == "open":
            at = 0
        elif where == "middle":
            at = G - o_rel - 1 + 2000
        else:
            at = n - len(e)
        content[at:at + len(e)] = e
        marks.append((1 + at, e))
    return b'"' + bytes(content) + b'"', o_rel, n, marks


def family_errors():
    out = []
    shapes = [(2, 4093, 2), (2, 4097, 4095), (5, 4094, 0), (3, 4096, 4094), (1, 4095, 4095)]
    i = 0
    for kind, e in ERRORS:
        for where in ("open", "middle", "close"):
            span, o, c = shapes[i % len(shapes)]
            i += 1
            if where == "middle" and span < 2:
                span = 2
            lit, ph, n, m = failing_spanning(span, o, c, [(where, e)])
            doc, marks = single([b'"before\\t"'], lit, [(0, b'"'), (n + 1, b'"')] + m, 0, 3 * G + ph, VALID_AFTER)
            out.append(Layout(2, "%s %r in the %s granule of a string crossing %d granule edge(s) (open at %d, close at %d)"
                              % (kind, e, where, span, o, c), doc, marks))
    # two errors of one string in different granules: the first by position wins, with its own code
    pairs = [(b"\\g", b"\\uDE00"), (b"\\uDE00", b"\\u12G4"), (b"\\u12G4", b"\\uD800x"), (b"\\uD83D\\u0041", b"\\q")]
    for (e1, e2), (w1, w2) in itertools.product(pairs, [("open", "middle"), ("middle", "close"), ("open", "close")]):
        lit, ph, n, m = failing_spanning(3, 4094, 1, [(w1, e1), (w2, e2)])
        doc, marks = single([b'"x"'], lit, [(0, b'"')] + m, 0, 2 * G + ph, VALID_AFTER)
        out.append(Layout(2, "two errors, %r in the %s granule before %r in the %s granule" % (e1, w1, e2, w2), doc, marks))
    # failing strings beside each other and beside valid ones, each crossing granule edges
    items = []
    for k, (kind, e) in enumerate(ERRORS):
        where = ("open", "middle", "close")[k % 3]
        lit, ph, n, m = failing_spanning(2 + k % 2 if where == "middle" else 1 + k % 3, OPEN_AT[k % 5], CLOSE_AT[k % 6], [(where, e)])
        items.append((lit, 0, G, ph, False, [(0, b'"')] + m))
        v, vph, vn = spanning(1, OPEN_AT[(k + 2) % 5], CLOSE_AT[(k + 3) % 6], seed=k)
        items.append((v, 0, G, vph, False, [(0, b'"')]))
    doc, marks = pack(items)
    out.append(Layout(2, "every error kind in a string crossing granule edges, each followed by a valid one", doc, marks))
    return out


# ---- 3. escapes straddling block and granule edges -----------------------------------------------------------------------
ESCAPES = [b"\\n", b"\\\\", b'\\"', b"\\u00e9", b"\\u20AC", b"\\uD83D\\uDE00"]
BAD_ESCAPES = [b"\\uD83Dx", b"\\uD83D\\u0041", b"\\uDE00", b"\\u12G4", b"\\q"]
BACKS = range(1, 13)


def _edge_kinds():
    return (("block", BLK, True), ("granule", G, False))


def family_escapes():
    out = []
    for name, step, excl in _edge_kinds():
        items = []
        for e in ESCAPES:
            for back in BACKS:
                lit = b'"' + b"pre" + e + b"post" + b'"'
                items.append((lit, 4, step, -back, excl, [(4, e)]))
        doc, marks = pack(items)
        out.append(Layout(3, "every escape with its backslash 1..12 bytes in front of a %s edge" % name, doc, marks))
        for e in BAD_ESCAPES:
            items = []
            for back in BACKS:
                lit = b'"' + b"pre" + e + plain(6) + b'"'
                items.append((lit, 4, step, -back, excl, [(4, e)]))
                items.append((b'"ok\\n' + plain(back) + b'"', 0, 1, 0, False, []))
            doc, marks = pack(items)
            out.append(Layout(3, "%r with its backslash 1..12 bytes in front of a %s edge, 12 times" % (e, name), doc, marks))
            for back in (1, 2, 5, 6, 11, 12):  # alone: the first error is this one
                lit = b'"' + b"pre" + e + plain(6) + b'"'
                doc, marks = single([b'"a\\t"'], lit, [(4, e)], 4, (3 if step == G else 7) * step - back, VALID_AFTER[:2])
                out.append(Layout(3, "%r with its backslash %d bytes in front of a %s edge" % (e, back, name), doc, marks))
    return out


# ---- 4. backslash runs ending around block and granule starts --------------------------------------------------------------
RUNS = list(range(1, 41)) + list(range(63, 71))
FOLLOW = [b'"', b"u0041", b"n"]


def run_literal(n, f):
    """'"', some content, n backslashes, then f; closed however the run resolves (an even run in front of '"' closes it)"""
    lit = b'"ab' + b"\\" * n + f
    if not (f == b'"' and n % 2 == 0):
        lit += b'z"'
    return lit


def family_runs():
    out = []
    for name, step, excl in _edge_kinds():
        for d in (-1, 0, 1):
            items = []
            for n in RUNS:
                for f in FOLLOW:
                    # the run's last backslash at edge + d
                    items.append((run_literal(n, f), 3 + n - 1, step, d, excl, [(3, b"\\" * n), (3 + n, f)]))
            doc, marks = pack(items)
            out.append(Layout(4, "backslash runs of %d..%d bytes ending at offset %+d of a %s start, followed by '\"', 'u0041', 'n'"
                              % (RUNS[0], RUNS[-1], d, name), doc, marks))
    return out


# ---- 5. the \uXXXX density threshold -----------------------------------------------------------------------------------------
U_ITEMS = [b"\\u0041", b"\\u00e9", b"\\u20AC", b"\\uD83D\\uDE00", b"\\u07FF", b"\\uFFFF", b"\\u0000"]
U_MAX = (G - 10) // 6  # 6-byte items that fit a granule behind 10 plain bytes: 681


def u_granule(n, seed=0, bad_at=None, only_short=False):
    """content of one granule's worth holding exactly n \\uXXXX items (a pair counts once), padded with plain bytes"""
    rng = random.Random(seed)
    out = bytearray(b"a" * 10)
    for i in range(n):
        left = n - i - 1
        cands = [u for u in U_ITEMS if len(out) + len(u) + 6 * left <= G and (not only_short or len(u) == 6)]
        u = b"\\uDE00" if i == bad_at else rng.choice(cands)
        out += u
    assert len(out) <= G, (n, len(out))
    return bytes(out) + b"b" * (G - len(out))


def family_density():
    """single long strings whose content begins exactly at a granule start: granule by granule the item counts given"""
    out = []
    plans = [[127], [128], [129], [U_MAX], [128, 129], [129, 128], [U_MAX, 127], [127, U_MAX, 128], [0, 129, 0]]
    for counts in plans:
        content = b"".join(u_granule(n, seed=i * 7 + n, only_short=(n == U_MAX)) for i, n in enumerate(counts))
        lit = b'"' + content + b'"'
        doc, marks = pack([(lit, 1, G, 0, False, [(1, b"a" * 10)])])
        out.append(Layout(5, "a string whose granules hold %s \\u items" % counts, doc, marks))
    for n, bad in ((129, 128), (128, 127), (U_MAX, 500), (130, 0)):
        content = u_granule(n, seed=n, bad_at=bad, only_short=(n == U_MAX))
        lit = b'"' + content + b'"'
        doc, marks = pack([(lit, 1, G, 0, False, [(1, b"a" * 10)]), (VALID_AFTER[1], 0, 1, 0, False, [])])
        out.append(Layout(5, "a granule of %d \\u items, item %d an error" % (n, bad + 1), doc, marks))
    # items straddling granule edges: one continuous run of them across three granules, every phase of a 6-byte item at the edge
    for shift in range(6):
        rng = random.Random(shift)
        content = b"a" * shift + b"".join(rng.choice(U_ITEMS) for _ in range(3 * G // 6))
        lit = b'"' + content + b'"'
        doc, marks = pack([(lit, 0, G, G - 30, False, [(0, b'"')])])
        out.append(Layout(5, "a run of \\u items across three granules, shifted by %d" % shift, doc, marks))
    return out


# ---- 6. tile-filling granules and adjacent strings ----------------------------------------------------------------------------
def family_tile():
    out = []
    q = b'"' * G
    out.append(Layout(6, "a granule of 4096 quotes: 2048 empty strings", q, [(0, q)]))
    out.append(Layout(6, "two granules of quotes", q + q, [(0, q + q)]))
    out.append(Layout(6, "a granule of spaces, then a granule of quotes", b" " * G + q + b" ", [(G, q)]))
    out.append(Layout(6, "a string open at the granule start, then the granule full of quotes",
                      b'"' + b"x" * (G - 1) + q + b'"', [(G, q)]))
    out.append(Layout(6, "4094 quotes from offset 1", b" " + b'"' * (G - 2) + b" " * (G + 1), [(1, b'"' * (G - 2))]))
    e = b"[" + b",".join([b'""'] * 3000) + b"]"
    out.append(Layout(6, '["","",...]: 3000 empty strings', e, [(1, b'"",""')]))
    for name, step, excl in _edge_kinds():
        for shapes in ([b'"a","b"', b'"","b"', b'"ab","cd","e"', b'"a",""'], [b'"a""b"', b'""""', b'"ab""cd""e"', b'"a""""b"']):
            items = []
            for p in range(64) if step == BLK else range(G - 8, G):
                for s in shapes:
                    items.append((s, 0, step, p % step, excl, [(0, s)]))
            doc, marks = pack(items)
            valid = b"," in shapes[0]
            out.append(Layout(6, "%s at every lane phase of a %s (%s)" % (shapes[0].decode(), name,
                                                                          "valid array" if valid else "adjacent strings: stage 2 fails"),
                              doc, marks))
    # (alone at every phase, as a whole document: stage 2 fails on the second string)
    for p in (0, 1, 2, 3, 31, 61, 62, 63):
        out.append(Layout(6, '"a""b" alone at offset %d' % p, b" " * p + b'"a""b"', [(p, b'"a""b"')]))
    bs = b"\\\\" * 4095
    out.append(Layout(6, "a string of 4095 escaped backslashes", b'"' + bs + b'"', [(1, bs)]))
    out.append(Layout(6, "4096 escaped backslashes from a granule start", b'["' + b" " * (G - 2) + b"\\\\" * G + b'"]',
                      [(G, b"\\\\" * G)]))
    return out


# ---- 7. quotes that open strings without being structurals ----------------------------------------------------------------
def family_nonstructural():
    """A quote directly behind a primitive opens a string for the string pass but is no structural (the scalar start rule of
    stage 1): the document fails stage 2 with the primitive's error, and a string error behind it must not win."""
    out = []
    prims = [b'1"a"', b'true"\\q"', b'1"\\uD800"', b'null"\\uDE00\\n"', b'-0"' + plain(5000) + b'"']
    later_bad = b'"\\uDE00"'
    for prim in prims:
        for at in (100, G - 3, G - 1, G, G + 1, 2 * G - 2):
            anchor = prim.index(b'"')
            doc, marks = single([b'"v\\n"'], prim, [(anchor, b'"')], anchor, at, [b'"b"', later_bad] + VALID_AFTER[:2])
            out.append(Layout(7, "%r with its quote at %d, a failing string later" % (prim[:20], at), doc, marks))
    # the non-structural string itself crossing granule edges, in front of valid strings
    lit = b'true"\\q' + plain(2 * G) + b'"'
    doc, marks = single([b'"v"'], lit, [(4, b'"\\q')], 4, G - 2, VALID_AFTER)
    out.append(Layout(7, "true\"\\q...\" crossing two granule edges", doc, marks))
    doc, marks = single([], b'[1"\\uD800", "b"]', [(2, b'"\\uD800')], 2, G - 1, [])
    out.append(Layout(7, '[1"\\uD800", "b"] nested, quote at a granule end', doc, marks))
    return out


# ---- 8. sizes ----------------------------------------------------------------------------------------------------------------
TAILS = (0, 1, 63, 64, 65, 4095)


def sized(length, seed):
    """an array of strings (escapes, UTF-8, strings crossing blocks and granules) of exactly `length` bytes (>= 2)"""
    rng = random.Random(seed)
    parts, size = [], 1
    while True:
        s = b'"' + body(rng.choice([0, 3, 30, 70, 200, 1000, 5000]), rng.randrange(1 << 30)) + b'"'
        if size + len(s) + 2 > length:
            break
        parts.append(s)
        size += len(s) + 1
    doc = b"[" + b",".join(parts)
    return doc + b" " * (length - len(doc) - 1) + b"]"


def size_list(big=True):
    """(granules, tail) pairs: a document of granules * 4096 + tail bytes"""
    out = [(0, t) for t in TAILS if t >= 2] + [(g, t) for g in (1, 2, 127, 128, 129) for t in TAILS]
    if big:
        out += [(256, 0), (257, 65), (1023, 4095), (2100, 0), (2100, 63)]
    return out


def family_sizes(big=True):
    out = []
    for g, t in size_list(big):
        n = g * G + t
        out.append(Layout(8, "%d bytes: %d granules and a tail of %d" % (n, g, t), sized(n, g * 7 + t), []))
    return out


FAMILIES = {1: family_spans, 2: family_errors, 3: family_escapes, 4: family_runs, 5: family_density, 6: family_tile,
            7: family_nonstructural, 8: family_sizes}


def all_layouts(big=True):
    out = []
    for k, f in FAMILIES.items():
        out += f(big) if k == 8 else f()
    return out
