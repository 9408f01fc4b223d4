"""Layouts for the accepted batch's layout pass (k_doc_prepare, batch.hip; k_batch_layout / k_tape_offsets, walk.hip): small seeded
batches that put a document boundary at every place of a 64-byte block where the pass can go wrong.

k_doc_prepare reads, per boundary, the boundary's block (SWAR masks of quotes, backslashes, ',' ':' '-' digits), sixteen index entries
behind the block's first one (blkidx) with a scalar loop for the rest, the block's entry parity (blkpar), the backslash run that ends
at the block's start, and per document the word counts of its whole blocks (blkw, eight per trip, parities from one or two blkpar
words).  FAMILIES names the hazards; tests/test_batch_layouts.py holds every family to its conditions with the oracle alone, and
tests/test_gpu_batch_layouts.py sends them through BatchShard.step.

A family is a list of Layout objects (one batch each).  Every document passes oracle.stage1 on its own and every document but a
batch's last ends in '\\n', '\\r\\n' or '\\t', so the plain pass accepts every batch.  Layout.hazards lists the boundaries (indexes
into doc_offsets) a layout was built for.  Plain module, not a conftest."""
import random

import numpy as np

SEPS = (b"\n", b"\r\n", b"\t")
PATTERN = b"[1,-2,true]{}:"  # bytes that look like structurals: inside a string they make a block's two word counts differ
PREP_DOCS = 256  # documents per workgroup of k_doc_prepare (stage1.h)

ELEMENTS = {"num": [b"1", b"-2", b"7"], "str": [b'""', b'"a"'], "atom": [b"true", b"null", b"false"],
            "mix": [b"1", b'"a"', b"-3", b"true", b'""']}
KINDS = ("brk", "num", "str", "atom", "mix")
FOLLOWERS = [b'["s","t"]', b'{"k":"v","n":[1,"s"]}', b'"root"', b'[-1,"a\\"b",2.5]', b'{"a":{"b":"c"}}']


def dense(c, kind):
    """a well-formed document of exactly c structurals in as few bytes as the kind allows"""
    if kind == "brk":
        return b"[" * (c // 2) + (b"1" if c & 1 else b"") + b"]" * (c // 2)
    el = ELEMENTS[kind]
    if c == 1:
        return el[0]
    if c == 2:
        return b"[]"
    if c & 1:
        return b"[" + b",".join(el[i % len(el)] for i in range((c - 1) // 2)) + b"]"
    return b"[[]" + b"".join(b"," + el[i % len(el)] for i in range((c - 4) // 2)) + b"]"


def pattern_bytes(n, phase=0):
    return bytes(PATTERN[(phase + i) % len(PATTERN)] for i in range(n))


class Layout:
    def __init__(self, name, wellformed=True):
        self.name = name
        self.wellformed = wellformed  # every document is well-formed: doc_string_offsets is checked against the oracle directly
        self.bodies, self.seps, self.hazards = [], [], []
        self.pos = 0
        self._sep = 0

    def sep1(self):
        """the one-byte separators in turn"""
        self._sep += 1
        return (b"\n", b"\t")[self._sep & 1]

    def add(self, body, sep=None, hazard=False):
        """append a document; hazard: the boundary BEHIND it is one"""
        sep = self.sep1() if sep is None else sep
        self.bodies.append(bytes(body))
        self.seps.append(sep)
        self.pos += len(body) + len(sep)
        if hazard:
            self.hazards.append(len(self.bodies))

    def mark(self):
        """the boundary at the current position is a hazard"""
        self.hazards.append(len(self.bodies))

    def align(self, mod, modulus=64):
        """a padding document (brackets around blanks, or a root string) after which the position is mod (modulo modulus)"""
        need = (mod - self.pos) % modulus
        if need == 0:
            return
        if need < 3:
            need += modulus
        if len(self.bodies) % 3 == 2 and need >= 4:
            self.add(b'"' + pattern_bytes(need - 3, self.pos) + b'"', b"\n")
        elif need >= 8 and len(self.bodies) % 3 == 1:
            self.add(b"[" + b" " * (need - 4) + b"]", b"\r\n")
        else:
            self.add(b"[" + b" " * (need - 3) + b"]", b"\t")

    # -- what a test runs ---------------------------------------------------------------------------------------------------
    def render(self, blank_separators=False, inserts=()):
        """-> (buffer, doc_offsets np.uint64, documents as the oracle sees them, hazards).  blank_separators: every separator
        byte a space.  inserts: [(boundary, document, separator)], each put in at that boundary of the ORIGINAL numbering."""
        items = [(b, (b" " * len(s)) if blank_separators else s) for b, s in zip(self.bodies, self.seps)]
        shift = [0] * (len(items) + 2)
        for at, body, sep in sorted(inserts, key=lambda t: -t[0]):
            items.insert(at, (bytes(body), sep))
            for h in range(at + 1, len(shift)):  # (the boundary it is put in at stays the end of the document in front)
                shift[h] += 1
        buf, offs = bytearray(), [0]
        for b, s in items:
            buf += b + s
            offs.append(len(buf))
        hazards = [h + shift[h] for h in self.hazards]
        return bytes(buf), np.array(offs, dtype=np.uint64), [b + s for b, s in items], hazards


# ---- the oracle's view of a batch ------------------------------------------------------------------------------------------
def oracle_block_words(data):
    """The reference of SjBlockMasks::words, from the oracle alone: -> (outside, inside, entered), one entry per 64-byte block
    (len // 64 + 1 of them).  outside[b] = tape words of block b's structurals when the block is entered outside a string, inside[b]
    = when it is entered inside one: 1 for every structural whose byte is not ',' or ':', 1 more if it is '-' or a digit.  The
    polarity in which `data` itself enters a block (entered[b], from the oracle's inString mask of the block in front) is
    counted on oracle.stage1(data); the other one on oracle.stage1 of a block of one quote and 63 blanks + data, which flips the
    string parity of every block and leaves the escape and scalar carries as they are (a blank in front of byte 0 is what the
    start of a buffer is to them)."""
    from oracle import oracle as O
    data = bytes(data)
    nb = len(data) // 64 + 1
    _, _, masks = O.index_blocks(data, want_masks=True)
    entered = np.zeros(nb, dtype=np.uint8)
    entered[1:] = (masks[:nb - 1, 2] >> np.uint64(63)).astype(np.uint8)
    a = np.frombuffer(data, dtype=np.uint8)

    def count(buf, idx, skip):
        idx = idx.astype(np.int64)
        idx = idx[idx >= skip]
        c = buf[idx]
        w = (c != 0x2C) & (c != 0x3A)
        w = w.astype(np.int64) + ((c == 0x2D) | ((c >= 0x30) & (c <= 0x39)))
        return np.bincount((idx - skip) >> 6, weights=w, minlength=nb).astype(np.int64)[:nb]
    own = count(a, O.stage1(data)[0], 0)
    flipped = b'"' + b" " * 63 + data
    other = count(np.frombuffer(flipped, dtype=np.uint8), O.stage1(flipped)[0], 64)
    outside = np.where(entered == 0, own, other)
    inside = np.where(entered == 1, own, other)
    return outside, inside, entered


def boundary_profile(buf, offs):
    """per boundary: (offset inside its block, structurals of its block in front of it), from oracle.stage1 of the whole batch"""
    from oracle import oracle as O
    idx, st = O.stage1(buf)
    assert st == 0, st
    offs = np.asarray(offs, dtype=np.int64)
    idx = idx.astype(np.int64)
    o = offs & 63
    c = np.searchsorted(idx, offs, side="left") - np.searchsorted(idx, offs - o, side="left")
    return o, c


def boundary_profile_per_document(offs, indexes):
    """the same from the documents' own structurals: indexes[k] = document k's oracle.stage1 indexes relative to its start, or None
    where it fails stage 1 (it has none).  What holds when the batch as a whole is not one document stream: failing documents,
    missing separators"""
    offs = np.asarray(offs, dtype=np.int64)
    parts = [np.asarray(ix, dtype=np.int64) + offs[k] for k, ix in enumerate(indexes) if ix is not None]
    idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    o = offs & 63
    c = np.searchsorted(idx, offs, side="left") - np.searchsorted(idx, offs - o, side="left")
    return o, c


# ---- the families -----------------------------------------------------------------------------------------------------------
COUNT_CLASSES = (0, 1, 15, 16, 17, 33, "most")  # structurals of the block in front of the boundary ("most": as many as fit, >= 33)


def family_offsets():
    """every boundary offset 0..63 with 0 / 1 / 15 / 16 / 17 / >= 33 structurals of the block in front of it"""
    L = Layout("offsets")
    unit = 0
    for cls in COUNT_CLASSES:
        for o in range(64):
            unit += 1
            follower = FOLLOWERS[unit % len(FOLLOWERS)]
            if cls == 0:
                if o == 0:
                    L.align(0)
                    L.mark()
                else:
                    sep = SEPS[unit % 3] if o >= 2 else L.sep1()
                    L.align(62)
                    L.add(b"[]" + b" " * (o - len(sep)), sep, hazard=True)
                L.add(follower)
                continue
            c = max(33, o - 1) if cls == "most" else cls
            done = False
            for t in range(len(KINDS)):
                kind = "brk" if cls == "most" else KINDS[(unit + t) % len(KINDS)]
                d = dense(c, kind)
                for sep in (SEPS[unit % 3], b"\n"):
                    if len(d) + len(sep) <= o:
                        L.align(0)
                        d2 = dense(c - 1, kind) if c >= 2 else b""
                        if unit % 4 == 0 and c >= 2 and len(d2) + len(sep) + 2 <= o:
                            # (a boundary inside the block in front of the hazard: a one-structural document, then the rest)
                            L.add(b"7", b"\n")
                            L.add(b" " * (o - len(d2) - len(sep) - 2) + d2, sep, hazard=True)
                        else:
                            L.add(b" " * (o - len(d) - len(sep)) + d, sep, hazard=True)
                        L.add(follower)
                        done = True
                        break
                if done:
                    break
    return [L]


def family_crowded():
    """several boundaries in one block: twelve of them, documents without a structural around a dense one"""
    L = Layout("crowded", wellformed=False)
    smalls = [b"1", b'"a"', b"[]", b"{}", b"-2", b"", b"7", b'""', b"0", b"", b"[1]", b"true"]
    for s in (0, 7, 30):
        L.align(s)
        for i, d in enumerate(smalls):
            L.add(d, hazard=True)
    for i, s in enumerate(range(0, 31, 2)):
        d = dense(17 + i % 3, KINDS[i % len(KINDS)])
        if s + len(d) + 4 > 63:
            d = dense(17 + i % 3, "brk")
        L.align(s)
        L.add(b"", hazard=True)
        L.add(d, hazard=True)
        L.add(b"", hazard=True)
        L.add(FOLLOWERS[i % len(FOLLOWERS)])
    L.align(5)
    for i in range(9):
        L.add(b"", hazard=True)
    L.add(b'["x"]')
    return [L]


def family_parity():
    """boundary blocks entered inside a string that closes in them; whole blocks inside strings that look like structurals"""
    L = Layout("parity")
    for o in range(2, 64):  # a root string: ... x x " SEP | boundary at o
        L.align(59)
        L.add(b'"' + pattern_bytes(o + 2, o) + b'"', L.sep1(), hazard=True)
        L.add(FOLLOWERS[o % len(FOLLOWERS)], hazard=True)
    for o in range(11, 64):  # an array whose first string closes in the block, two more strings behind it
        L.align(59)
        L.add(b'["' + pattern_bytes(o - 11 + 3, o) + b'","y","z"]', L.sep1(), hazard=True)
        L.add(FOLLOWERS[o % len(FOLLOWERS)])
    for i, n in enumerate((130, 200, 333, 500, 1000, 2000)):
        L.align((7 * i) % 64)
        L.add(b'["' + pattern_bytes(n, i) + b'",' + (b'"q",' if i & 1 else b"") + b"-5]", SEPS[i % 3], hazard=True)
        L.add(FOLLOWERS[i % len(FOLLOWERS)])
    return [L]


RUNS = (1, 2, 63, 64, 65, 128, 129, 5000, 5001)


def family_backslash_runs():
    """backslash runs inside a string that end on the last byte of a block (and one byte earlier / later), the quote behind them
    escaped (odd run) or closing (even run), a boundary in the block behind"""
    L = Layout("backslash_runs")
    unit = 0
    for n in RUNS:
        for shift in (0, -1, 1):
            for lead in (0, 20):
                unit += 1
                L.align(lead)
                f = (63 + shift - (L.pos + 1 + n)) % 64
                body = b'["' + b"a" * f + b"\\" * n + b'"' + (b'z"' if n & 1 else b"") + b"]"
                L.add(body, SEPS[unit % 3], hazard=True)
                L.add(FOLLOWERS[unit % len(FOLLOWERS)], hazard=True)
                L.add(b'{"k":"v"}')
    return [L]


ODD = [b'1"a"', b'true"x"', b'null"n""m"', b'-0"z"', b'[1"a","b"]', b'{"k":2"v"}']


def family_quote_behind_primitive():
    """a quote directly behind a primitive (passes stage 1, fails stage 2, opens a string all the same) in front of well-formed
    documents with strings in the same block"""
    L = Layout("quote_behind_primitive", wellformed=False)
    for i, odd in enumerate(ODD):
        for s in range(0, 48, 3):
            L.align(s)
            L.add(odd, hazard=True)
            L.add(b'["p","q"]', hazard=True)
            L.add(b'{"k":"v"}')
    L.align(0)
    for odd in ODD[:4]:  # ... several of them in one block
        L.add(odd, hazard=True)
    L.add(b'["p","q"]', hazard=True)
    L.add(b'"r"')
    return [L]


STARTERS = [b"-1.5", b"0.25", b"1e3", b"234", b"345", b"456", b"567", b"678", b"789", b"890", b"987", b"-7", b"0", b"5",
            b"true", b"false", b"null"]


def family_word_classes():
    """a number / an atom whose first byte is a block's last and that runs on over the next block's start; a block of 64 brackets;
    '[-1' and '[1' repeated (the most words a block can make)"""
    L = Layout("word_classes", wellformed=False)
    for i, tok in enumerate(STARTERS):
        L.align(0)
        L.add(b"[" + b" " * 62 + tok + b',"s"]', SEPS[i % 3], hazard=True)
        L.add(FOLLOWERS[i % len(FOLLOWERS)], hazard=True)
        L.align(40)  # ... as the root of its document, the boundary 23 bytes in front of it
        L.mark()
        L.add(b" " * 23 + tok, L.sep1(), hazard=True)
        L.add(b'["s"]')
    for a in (0, 63, 1):
        L.align(a)
        L.add(b"[" * 32 + b"]" * 32, L.sep1(), hazard=True)
        L.add(b'["s"]')
    for a in (0, 1, 2):
        L.align(a)
        L.add(b"[-1" * 50, L.sep1(), hazard=True)  # (not closed: fails stage 2, its slot is its predicted length)
        L.add(b'["s"]')
        L.align(a)
        L.add(b"[1" * 50, L.sep1(), hazard=True)
        L.add(b'{"k":"v"}')
        L.align(a)
        L.add(b"[-1," * 40 + b"-1" + b"]" * 40, L.sep1(), hazard=True)
        L.add(b'["s"]')
    return [L]


BLOCK_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65)
START_BLOCKS = (0, 55, 56, 57, 60, 63)


def long_document(n, rng):
    """a well-formed document of exactly n bytes (n >= 2): long strings that look like structurals, numbers, atoms"""
    if n < 8:
        return b"[" + b" " * (n - 2) + b"]"
    out = [b"["]
    room = n - 2
    first = True
    while room >= 6:
        r = rng.random()
        if r < 0.6:
            m = min(room - (0 if first else 1) - 2, rng.choice([3, 30, 70, 130, 200, 450]))
            item = b'"' + pattern_bytes(m, rng.randrange(14)) + b'"'
        else:
            item = rng.choice([b"-12", b"true", b"[]", b"3.5", b'{"a":1}'])
        piece = (b"" if first else b",") + item
        if len(piece) > room:
            break
        out.append(piece)
        room -= len(piece)
        first = False
    return b"".join(out) + b" " * room + b"]"


def family_long():
    """documents of 0 .. 65 whole blocks that begin in block 0 / 55 / 56 / 57 / 60 / 63 of a 64-block parity word"""
    L = Layout("long")
    rng = random.Random(1301)
    unit = 0
    for cnt in BLOCK_COUNTS:
        for m in START_BLOCKS:
            unit += 1
            r = (0, 5, 63, 31)[unit % 4] if cnt else (0, 5, 31, 17)[unit % 4]
            sep = SEPS[unit % 3]
            L.align(m * 64 + r, 4096)
            L.mark()
            delta = rng.randrange(0, 64 - r) if cnt else rng.randrange(4, 64 - r)
            L.add(long_document(cnt * 64 + delta - len(sep), rng), sep, hazard=True)
            L.add(FOLLOWERS[unit % len(FOLLOWERS)], hazard=True)
    return [L]


DOC_COUNTS = (2, 3, 255, 256, 257, 511, 512, 513)


def family_counts():
    """2 .. 513 documents (k_doc_prepare's workgroup holds 256), a dense boundary at documents 255, 256, 257 (and 511, 512, 513)"""
    out = []
    rng = random.Random(1302)
    plain = FOLLOWERS + [b"[]", b"{}", b"12", b'{"k":[1,2,{"z":"w"}]}', b'["abc","def",null]']
    for n in DOC_COUNTS:
        L = Layout("counts_%d" % n)
        while len(L.bodies) < n:
            k = len(L.bodies)
            if k in (253, 509) and k + 1 < n:  # the three dense documents behind it begin a block
                need = -L.pos % 64
                L.add(b"[" + b" " * ((need if need >= 3 else need + 64) - 3) + b"]", b"\n")
            elif k in (254, 255, 256, 510, 511, 512) and n > 253:
                L.add(dense(19, "num" if k % 256 == 254 else "brk"), hazard=True)
            else:
                L.add(rng.choice(plain), SEPS[k % 3], hazard=(k < 3 or k == n - 1))
        out.append(L)
    return out


TINY = [[b"7", b""], [b"", b"7"], [b"", b"", b'"a"'], [b"1", b"2"], [b"[]", b""], [b"", b"", b"[]", b""], [b"[]", b"1"],
        [b"1", b'"b"', b"3"], [b"[]", b"[]"], [b"[1]", b"2"], [b"1", b"2", b"3", b"4"], [b"[1]", b"[]"], [b"[1,2]", b""],
        [b'["a"]', b"1", b"2"], [b"", b'{"k":1}']]


def family_tiny():
    """2 .. 4 documents of 1 .. 5 structurals in all: the index array read one entry at a time / one clamped group of four"""
    out = []
    for i, docs in enumerate(TINY):
        L = Layout("tiny_%d" % i, wellformed=all(docs))
        for j, d in enumerate(docs):
            last = j == len(docs) - 1
            L.add(d, b"" if last and i % 3 == 0 and d else SEPS[(i + j) % 3], hazard=True)
        out.append(L)
    return out


def family_end():
    """total_len & 63 in {0, 1, 63}, the last document with and without a separator, structurals in front of the batch's end"""
    out = []
    for tail in (0, 1, 63):
        for sep in (b"\n", b""):
            L = Layout("end_%d_%s" % (tail, "sep" if sep else "nosep"))
            for i in range(5):
                L.add(FOLLOWERS[i], SEPS[i % 3], hazard=True)
            d = dense(21, "mix")
            L.align((tail - len(d) - len(sep)) % 64)
            L.add(d, sep, hazard=True)
            out.append(L)
    return out


def backslash_in_front_of_dense():
    """NOT a batch the plain pass accepts, and not one the repair stage takes: documents without any separator, among them `[1]\\`
    -- it passes stage 1 and survives, and its trailing backslash would escape the first byte of its neighbour `"x"` -- directly in
    front of a dense document, all in one block, so that the boundary behind the dense one has >= 17 structurals of its block in
    front of it; once with the backslash inside the block, once as the last byte of the block in front.  One document that fails
    stage 1 tells by its slot which call laid the tapes out.  -> Layout (every separator empty)"""
    L = Layout("backslash_in_front_of_dense", wellformed=False)

    def pad(mod):
        need = (mod - L.pos) % 64
        need = need if need >= 2 else need + 64
        L.add(b"[" + b" " * (need - 2) + b"]", b"")
    for i in range(40):
        L.add([b'["s","t"]', b'{"k":"v","n":[1,"s"]}', b'{"a":{"b":"c"}}', b"[[1,2],[-3]]"][i % 4], b"")
    L.add(b'{"k":"v', b"")  # (an unclosed string: fails stage 1)
    L.add(b'["p"]', b"")
    for start, kind in ((0, "brk"), (60, "num"), (9, "str"), (60, "brk")):
        pad(start)
        L.add(b"[1]\\", b"", hazard=True)
        L.add(b'"x"', b"", hazard=True)
        L.add(dense(19, kind), b"", hazard=True)
        L.add(b'["s","t"]', b"", hazard=True)
        L.add(b'{"k":"v"}', b"")
    return L


FAMILIES = {
    "offsets": family_offsets,
    "crowded": family_crowded,
    "parity": family_parity,
    "backslash_runs": family_backslash_runs,
    "quote_behind_primitive": family_quote_behind_primitive,
    "word_classes": family_word_classes,
    "long": family_long,
    "counts": family_counts,
    "tiny": family_tiny,
    "end": family_end,
}

_cache = {}


def family(name):
    """the layouts of a family (built once: they are deterministic and nothing may change them)"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


# ---- documents that fail stage 1, for the repair stage: 64 bytes with their separator, so that every offset behind them stays ---
def failing_documents():
    """-> [(name, document, separator)]: an unclosed string, invalid UTF-8, a failing document that ends in an odd backslash run"""
    return [("unclosed", b'["abc' + b"x" * 58, b"\n"),
            ("utf8", b'["' + b"y" * 58 + b"\xc3" + b'"]', b"\t"),
            ("backslash", b'["q' + b"z" * 57 + b"\\" * 3, b"\n")]


def repair_inserts(layout, rotate=0):
    """Where the three failing documents go, as render()'s inserts: one at least a block ahead of a hazard, one inside a hazard's
    block (at a boundary of that block in front of the hazard; its last bytes then share the block with the hazard), one directly
    behind a hazard -- three different hazards where the layout has them.  -> [(boundary, document, separator, place, hazard)]"""
    buf, offs, _, hz = layout.render()
    offs = offs.astype(np.int64)
    fails = failing_documents()
    n = len(offs) - 1
    out, used = [], set()
    hs = sorted(set(hz))
    picks = {"ahead": None, "inside": None, "behind": None}
    third = max(1, len(hs) // 3)
    for place, lo in (("ahead", 0), ("inside", third), ("behind", 2 * third)):
        order = hs[lo:] + hs[:lo]
        for h in order:
            blk = int(offs[h]) & ~63
            if place == "behind":
                at = h
            elif place == "inside":
                cand = [j for j in range(h) if blk < offs[j] < offs[h]]
                at = cand[0] if cand else None
            else:
                cand = [j for j in range(h) if offs[j] <= blk - 64]
                at = cand[-1] if cand else None
            if at is not None and at not in used and (at < n or layout.seps[-1]):  # (never behind a last document without a separator)
                used.add(at)
                picks[place] = (at, h)
                break
    for i, place in enumerate(("ahead", "inside", "behind")):
        if picks[place] is None:
            continue
        name, d, sep = fails[(i + rotate) % 3]
        out.append((picks[place][0], d, sep, place, picks[place][1]))
    return out
