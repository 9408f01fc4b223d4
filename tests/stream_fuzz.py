"""A seeded corpus of documents and chunkings for the chunk stream (sjmi_stream_*) and the document split (sjmi_split_*), shared by
tests/test_stream_fuzz_corpus.py (no GPU: the corpus' own conditions) and tests/test_gpu_stream_fuzz.py.  Imports nothing from the
product.  What must come out of a stream or a split is decided by oracle.stage1 on the WHOLE document; this file decides what goes
in, restates on the CPU what the C state machine keeps of a stream (model_stream: `have`, the halo escalation, from_start) and what
a shard's kernel says about its halo (halo_filled), and counts what the corpus covers (statistics()).

corpus() -> [Doc].  A document is clean filler (tests/test_gpu_stage1._json_like, cut and mended so that it begins and ends outside
a string and is valid UTF-8) with HAZARDS planted at chosen offsets: every hazard is recorded as (class, key, edge), edge a multiple
of 64, the hazard's byte number `key` (its split position) lying exactly on the edge -- so a chunking that cuts at `edge` puts the
hazard across two chunks at that split.  Hazards that make a document invalid get a document of their own: a status bit that a
second hazard would set as well could not show that the first one was missed.

chunkings(doc) -> [(style, last, cuts)]: cuts[0] == 0, cuts[-1] == len(doc), chunk k = [cuts[k], cuts[k + 1]); every cut but the last is a multiple
of 64; a zero-length last chunk shows as cuts[-2] == cuts[-1]."""
import functools
import random

from tests.golden import vectors as V
from tests.test_gpu_stage1 import _json_like

SEED = 20261101
RUNS = list(range(1, 10)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4031, 4032, 4033]
STREAM_HALOS = (0, 128, 4096, 8192)  # halo_bytes of sjmi_stream_open (0 = 64)
KEEP_MIN = 4096                      # sjmi_stream_open: keep = max(halo, 4096)
LAST_LENGTHS = (0, 1, 63, 64, 65)    # ... and "rest": whatever the chunking leaves
RANDOM_CHUNKS = (64, 64, 128, 192, 1024, 4096, 4160, 8192)
N_SLICES = 4                         # the corpus in slices of about equal numbers of pushes (one test function each)
MAX_DOC = 24 * 1024 + 512

BS, QUOTE = 0x5C, 0x22
_UTF8_VALID = {"utf8_2": "é".encode(), "utf8_3": "€".encode(), "utf8_4": "😀".encode()}
_SCALARS = {"number": b"12345678901234567890", "true": b"true", "bare_word": b"abcde"}
_ON_EDGE = {"empty_string": (b",", b'""', b","), "quote_comma": (b'"ab', b'",', b"1,"), "quote_colon": (b'{"k', b'":', b"1},")}


class Doc:
    def __init__(self, name, data, hazards):
        self.name, self.data, self.hazards = name, bytes(data), list(hazards)  # hazards: (class, key, edge)

    def __len__(self):
        return len(self.data)


class _Builder:
    """Appends bytes and follows the two facts a planter needs to know: inside a string? an escape pending?"""

    def __init__(self, rng, name):
        self.rng, self.name, self.buf, self.in_str, self.esc, self.hazards = rng, name, bytearray(), False, False, []

    def raw(self, data):
        for c in data:
            if self.esc:
                self.esc = False
            elif c == BS:
                self.esc = True
            elif c == QUOTE:
                self.in_str = not self.in_str
        self.buf += data

    def settle(self):
        """back outside a string, no escape pending"""
        if self.esc:
            self.raw(b"x")
        if self.in_str:
            self.raw(b'"')

    def fill(self, n):
        """n bytes of clean text that begins and ends outside a string"""
        assert not self.in_str and not self.esc and n >= 0
        if n < 8:
            self.raw(b" " * n)
            return
        t = _json_like(self.rng, n - 2).decode("utf-8", "ignore").encode()  # (the cut may have halved a character)
        probe = _Builder(None, None)
        probe.raw(t)
        if probe.esc:
            t = t[:-1] + b"x"
        if probe.in_str:
            t += b'"'
        self.raw(t + b" " * (n - len(t)))
        assert not self.in_str and not self.esc

    def plant(self, cls, key, seq, split, pre=b"", post=b"", min_offset=0, gap_blocks=None, settle=True):
        """filler, then pre + seq + post with seq[split] on a multiple of 64 (split may exceed len(seq): the edge lies behind it)"""
        self.settle()
        need = max(len(self.buf), min_offset) + len(pre) + split
        extra = self.rng.choice((0, 0, 1, 2, 5)) if gap_blocks is None else gap_blocks
        edge = (need + 63) // 64 * 64 + 64 * extra
        self.fill(edge - split - len(pre) - len(self.buf))
        self.raw(pre)
        assert (len(self.buf) + split) % 64 == 0
        self.raw(seq)
        self.raw(post)
        self.hazards.append((cls, key, edge))
        if settle:
            self.settle()

    def finish(self, mod=None):
        """close what is open and pad so that len % 64 == mod"""
        self.settle()
        if mod is not None:
            self.fill((mod - len(self.buf)) % 64)
        return self.done()

    def done(self):
        assert 256 <= len(self.buf) <= MAX_DOC, (self.name, len(self.buf))
        return Doc(self.name, self.buf, self.hazards)


# ---- the hazard classes: class -> the keys (split positions) each must meet a chunk edge at --------------------------------------
def _valid_items():
    """(class, key, seq, split, pre, post): hazards that leave a document valid; many share a document"""
    items = []
    for split in (0, 1, 2):
        items.append(("esc_quote", split, b'\\"', split, b'"ab', b'cd"'))
    for split in (0, 1, 2, 3, 4):
        items.append(("esc3_quote", split, b'\\\\\\"', split, b'"ab', b'cd"'))
    for L in RUNS:
        items.append(("bsrun_quote", L, b"\\" * L + b'"', L, b'"a', b"z"))
        items.append(("bsrun_letter", L, b"\\" * L + b"x", L, b'"a', b"z"))
    for L in (7, 63, 64, 127, 255, 1023):  # the quote is the last byte in front of the edge, the run fills the halo in front of it
        items.append(("bsrun_then_quote", L, b"\\" * L + b'"', L + 1, b'"a', b"z"))
    for L in (64, 256, 1024):  # the string's opening quote is the byte in front of a run that fills the halo exactly
        items.append(("quote_then_bsrun", L, b"\\" * L + b'"', L, b'"', b"z"))
    for cls, seq in _UTF8_VALID.items():
        for split in range(1, len(seq)):
            items.append((cls, split, seq, split, b'"ab', b'cd"'))
    for cls, seq in _SCALARS.items():
        for split in range(1, len(seq)):
            items.append((cls, split, seq, split, b",", b","))
    for cls, (pre, seq, post) in _ON_EDGE.items():
        for split in (0, 1, 2):
            items.append((cls, split, seq, split, pre, post))
    for c in (0x01, 0x0A):
        for split in (0, 1):
            items.append(("ctrl_outside_%02x" % c, split, bytes([c]), split, b",", b","))
    return items


def _ctrl_in_string(c, blocks, split):
    """a control byte on the edge, the string's opening quote `blocks` blocks in front of it (at byte 17 of its block)"""
    return ("ctrl_in_string_%02x_%d" % (c, blocks), split, bytes([c]), split, b'"' + b"s" * (64 * blocks - 18 - split), b'tail"')


def required_keys():
    """class -> set of keys: condition (a) of the corpus"""
    req = {}
    for cls, key, *_ in _valid_items():
        req.setdefault(cls, set()).add(key)
    for L in RUNS:
        req.setdefault("bsrun_end", set()).add(L)
    for name, seq, _ in V.UTF8_INVALID_MID:
        req["utf8_mid:" + name] = set(range(0, len(seq) + 1))
    for name, _seq, _ in V.UTF8_INVALID_END:
        req["utf8_end:" + name] = {0, 1, 63}  # len(document) % 64
    for c in (0x01, 0x0A):
        for blocks in (1, 2, 40):
            req["ctrl_in_string_%02x_%d" % (c, blocks)] = {0, 1}
    req["lone_quote"] = {0, 1}
    req["leading_run"] = {100, 4095, 4096, 4200}
    req["bsrun_long"] = {4096, 4160, 5000, 8001}
    req["one_string"] = {0}
    return req


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(SEED)
    docs = []
    # ---- valid hazards, many per document; the long runs far enough in that 4 KiB of the stream are kept in front of them
    items = _valid_items()
    rng.shuffle(items)
    limits = [600, 600, 900, 1500, 3000, 6000, 12000]
    b, limit = None, 0
    for it in items:
        cls, key, seq, split, pre, post = it
        if b is not None and len(b.buf) + len(seq) + 600 > limit:
            docs.append(b.finish(rng.choice((0, 1, 63, rng.randrange(64)))))
            b = None
        if b is None:
            b, limit = _Builder(rng, "valid_%d" % len(docs)), max(rng.choice(limits), len(seq) + 6000 if len(seq) > 1000 else 0)
        b.plant(cls, key, seq, split, pre, post, min_offset=4224 if len(seq) >= 1000 and rng.random() < 0.8 else 0)
    docs.append(b.finish(0))
    # ---- a backslash run that ends the document exactly on an edge: inside a string (unclosed) and outside one
    for k, L in enumerate(RUNS):
        b = _Builder(rng, "bsrun_end_%d" % L)
        b.fill(rng.choice((200, 300, 500)))
        b.plant("bsrun_end", L, b"\\" * L, L, b'"a' if k % 2 else b",", b"", min_offset=4224 if L >= 1000 and k % 3 else 0, settle=False)
        docs.append(b.done())
    # ---- a document that begins with a backslash run (the halo reaches the document's first byte while the stream is short)
    for L in (100, 4095, 4096, 4200):
        b = _Builder(rng, "leading_run_%d" % L)
        b.raw(b"\\" * L + b'"x" [1,2,3]')
        b.hazards.append(("leading_run", L, (L + 63) // 64 * 64))
        b.settle()
        b.plant("bsrun_quote", 5, b"\\" * 5 + b'"', 5, b'"a', b"z")
        b.fill(rng.choice((200, 400)))
        docs.append(b.finish(rng.choice((0, 1, 63))))
    # ---- a run longer than the 4 KiB a stream keeps by default, in the middle of a document (8 KiB of halo see its beginning)
    for L in (4096, 4160, 5000, 8001):  # (8001: 8 KiB of halo are assembled from many chunks and walked from end to end)
        b = _Builder(rng, "long_run_%d" % L)
        b.plant("bsrun_long", L, b"\\" * L + b'"', L, b'"a', b"z", min_offset=rng.choice((0, 4224)))
        b.fill(rng.choice((200, 400)))
        docs.append(b.finish(rng.choice((0, 1, 63))))
    # ---- one string from the second byte to the end
    b = _Builder(rng, "one_string")
    b.raw(b'["')
    while len(b.buf) < 6000:
        b.raw(rng.choice((b"abc def", b'\\"', "é€😀".encode(), b"\\\\", b"{[,:]}", b"12", b"\\n")) * rng.randint(1, 9))
    if b.esc:
        b.raw(b"n")
    b.hazards.append(("one_string", 0, 64))
    docs.append(b.done())
    # ---- hazards that make the document invalid: one document each
    n_inv = 0

    def small(name):
        nonlocal n_inv
        n_inv += 1
        bb = _Builder(rng, name)
        bb.fill(rng.choice((0, 70, 200, 450)))
        return bb

    for name, seq, _ in V.UTF8_INVALID_MID:
        for split in range(0, len(seq) + 1):
            b = small("utf8_mid:%s@%d" % (name, split))
            inside = (n_inv % 3) != 0
            b.plant("utf8_mid:" + name, split, seq, split, b'"ab' if inside else b",", b'cd"' if inside else b",")
            b.fill(rng.choice((190, 260, 700)))
            docs.append(b.finish(rng.choice((0, 1, 63, rng.randrange(64)))))
    for name, seq, _ in V.UTF8_INVALID_END:
        for mod in (0, 1, 63):  # the sequence ends the document, len % 64 == mod
            b = small("utf8_end:%s%%%d" % (name, mod))
            b.fill(200)
            b.settle()
            n = (len(b.buf) + len(seq) + 2 + 63) // 64 * 64 + mod  # the document's length
            b.fill(n - len(seq) - 1 - len(b.buf))
            b.raw(b",")
            b.raw(seq)
            assert len(b.buf) == n and n % 64 == mod
            b.hazards.append(("utf8_end:" + name, mod, n // 64 * 64))
            docs.append(b.done())
    for c in (0x01, 0x0A):
        for blocks in (1, 2, 40):
            for split in (0, 1):
                b = small("ctrl_in_string_%02x_%d@%d" % (c, blocks, split))
                b.plant(*_ctrl_in_string(c, blocks, split))
                b.fill(rng.choice((150, 300)))
                docs.append(b.finish(rng.choice((0, 1, 63))))
    for split in (0, 1):  # a lone quote: everything behind it is inside a string, which never closes
        b = small("lone_quote@%d" % split)
        b.plant("lone_quote", split, b'"', split, b",", b"", settle=False)
        b.raw(b"".join(rng.choice((b"abc", b" ", b",", b"12", b"[", b"}")) for _ in range(rng.choice((100, 1500)))))
        b.raw(b" " * ((split - len(b.buf)) % 64))  # (len % 64 is 0 or 1)
        docs.append(b.done())
    # ---- combinations of verdicts; the control character lies several chunks behind its string's opening quote
    for want in (3, 5, 6, 7):
        b = small("combo_%d" % want)
        if want & 1:
            name, seq, _ = V.UTF8_INVALID_MID[want]
            b.plant("utf8_mid:" + name, 1, seq, 1, b",", b",")
        if want & 4:
            b.plant(*_ctrl_in_string(0x0A, 40 if want & 2 else 2, want & 1))
        if want & 2:
            b.plant("lone_quote", 1, b'"', 1, b",", b"", settle=False)
            b.raw(b"never closed " * 30)
            docs.append(b.done())
        else:
            docs.append(b.finish(0))
    names = [d.name for d in docs]
    assert len(set(names)) == len(names)
    return tuple(docs)


# ---- chunkings ------------------------------------------------------------------------------------------------------------------
def _body(style, B, rng):
    """cuts of [0, B) in the given style (without 0), B itself the last one"""
    if style == "b64" or style == "b128":
        step = 64 if style == "b64" else 128
        return list(range(step, B, step)) + [B]
    if style == "one":
        return [B]
    if style == "block_rest":
        return ([64] if B > 64 else []) + [B]
    if style == "rest_block":
        r = (B - 1) // 64 * 64
        return ([r] if r > 0 else []) + [B]
    cuts, at = [], 0
    while at < B:
        at = min(at + rng.choice(RANDOM_CHUNKS), B)
        cuts.append(at)
    return cuts


STYLES = ("b64", "b128", "one", "block_rest", "rest_block", "random_a", "random_b")


def chunkings(doc, index=0):
    """-> [(style, last, cuts)], deterministic in (document, index); every feasible last length of LAST_LENGTHS is used with the
    cheap styles, and with all styles on documents of up to 2 KiB; the all-64 and all-128 chunkings of larger documents take
    one of them in turn, and "rest" """
    n = len(doc)
    rng = random.Random(SEED * 1000 + index)
    lasts = [l for l in LAST_LENGTHS if l <= n - 64 and (n - l) % 64 == 0]
    out, seen = [], set()
    for si, style in enumerate(STYLES):
        if n <= 2048 or style not in ("b64", "b128"):
            options = lasts + ["rest"]
        else:
            options = [lasts[(index + si) % len(lasts)]] if lasts else []
            options.append("rest")
        for last in options:
            if last == "rest":
                cuts = [0] + _body(style, n, rng)
            else:
                cuts = [0] + _body(style, n - last, rng) + [n]
            if tuple(cuts) not in seen:
                seen.add(tuple(cuts))
                out.append((style, last, cuts))
    for _style, _last, cuts in out:
        assert cuts[0] == 0 and cuts[-1] == n and all(c % 64 == 0 for c in cuts[:-1])
        assert all(b > a for a, b in zip(cuts[:-2], cuts[1:-1])) and cuts[-1] >= cuts[-2]
    return out


def max_chunk(cuts):
    return max(1, max(b - a for a, b in zip(cuts, cuts[1:])))


@functools.lru_cache(maxsize=None)
def pairs():
    """every (document index, style, last, cuts) of the corpus"""
    return tuple((di, style, last, tuple(cuts)) for di, d in enumerate(corpus()) for style, last, cuts in chunkings(d, di))


@functools.lru_cache(maxsize=None)
def slices():
    """the documents dealt into N_SLICES bins of about equal numbers of pushes -> [[document index]]"""
    cost = {}
    for di, _s, _l, cuts in pairs():
        cost[di] = cost.get(di, 0) + len(cuts) - 1
    bins, load = [[] for _ in range(N_SLICES)], [0] * N_SLICES
    for di in sorted(cost, key=lambda i: -cost[i]):
        k = load.index(min(load))
        bins[k].append(di)
        load[k] += cost[di]
    return tuple(tuple(sorted(b)) for b in bins), tuple(load)


# ---- the CPU restatement of what is kept of a stream, and of a shard's report about its halo ------------------------------------
def halo_filled(data, a, h):
    """What a shard that begins at `a` with `h` bytes of halo finds out (csrc/stage1.hip, halo_short): everything readable in front
    of it is one backslash run -- the byte in front of the shard may be the quote the run would escape -- so the run may go on
    where nothing is readable.  (With FLAG_HALO_FROM_START nothing is in front of the halo and this is not reported.)"""
    return h > 0 and data[a - 1] in (BS, QUOTE) and data[a - h:a - 1] == b"\\" * (h - 1)


def model_stream(data, cuts, halo):
    """sjmi_stream_push, push by push: have = min(have + len, max(halo, 4096)); a chunk whose halo is filled is repeated with four
    times as much until the halo reaches the stream's first byte (exact) or everything that is kept (SJMI_ERR_CAPACITY).
    -> one dict per push, up to and including a push that fails."""
    halo = halo or 64
    keep, have, out = max(halo, KEEP_MIN), 0, []
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        last = k == len(cuts) - 2
        want, depth = halo, 0
        while True:
            h = min(want, have) // 64 * 64
            from_start = h == a
            filled = halo_filled(data, a, h)
            error = filled and not from_start and h >= have // 64 * 64
            if not filled or from_start or error:
                break
            want *= 4
            depth += 1
        nh = min(have + (b - a), keep)
        out.append({"a": a, "len": b - a, "have": have, "h": h, "depth": depth, "from_start": from_start, "filled": filled, "error": error,
                    "short": not last and b - a < have,    # the chunk is shorter than what is kept in front of it
                    "overlap": not last and b - a < nh})   # the keep copy's source and destination overlap (the bounce branch)
        if error:
            break
        if not last:
            have = nh
    return out


def shard_bounds(n, parts):
    """sharding.split_points without its empty shards (a shard that is not the last one has at least one block)"""
    bounds = [0]
    for r in range(1, parts):
        bounds.append(max((n * r // parts) // 64 * 64, bounds[-1]))
    bounds = sorted(set(bounds))  # (every one of them is below n)
    return [(a, b) for a, b in zip(bounds, bounds[1:] + [n])]


def split_configs(doc, index):
    """-> [[(a, b)]]: the shard bounds a document is split at"""
    n = len(doc)
    rng = random.Random(SEED * 77 + index)
    out = []
    for parts in (2, 3, 7, 16, min(n // 64, 64)):
        bd = shard_bounds(n, parts)
        if bd not in out:
            out.append(bd)
    inner = sorted(rng.sample(range(64, n // 64 * 64 + 1, 64), min(rng.choice((1, 3, 9)), n // 64)))
    bd = [(a, b) for a, b in zip([0] + inner, inner + [n])]
    if bd not in out:
        out.append(bd)
    return out


SPLIT_HALOS = (64, 256, 4096)


# ---- what the corpus covers -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def statistics():
    from oracle import oracle as O
    docs = corpus()
    st = {"documents": len(docs), "bytes": sum(len(d) for d in docs), "min_len": min(len(d) for d in docs), "max_len": max(len(d) for d in docs),
          "pairs": len(pairs()), "pushes": sum(len(c) - 1 for _d, _s, _l, c in pairs())}
    status = [O.stage1(d.data)[1] for d in docs]
    st["status_counts"] = {s: status.count(s) for s in sorted(set(status))}
    st["accepted"] = status.count(0)
    met = {}
    for di, _s, _l, cuts in pairs():
        edges = set(cuts[1:-1])
        for cls, key, edge in docs[di].hazards:
            if edge in edges:
                met.setdefault(cls, set()).add(key)
    st["met"] = met
    st["unmet"] = sorted((cls, key) for cls, keys in required_keys().items() for key in keys if key not in met.get(cls, ()))
    st["last_lengths"] = {}
    for _di, _s, last, _c in pairs():
        st["last_lengths"][last] = st["last_lengths"].get(last, 0) + 1
    for halo in STREAM_HALOS:
        h = {"short_pairs": 0, "overlap_pairs": 0, "depths": {}, "filled_from_start": 0, "filled_reported": 0, "have_eq_keep": 0,
             "have_grows_in_steps": 0, "pushes": 0}
        keep = max(halo or 64, KEEP_MIN)
        for di, _s, _l, cuts in pairs():
            m = model_stream(docs[di].data, cuts, halo)
            h["pushes"] += len(m)
            h["short_pairs"] += any(p["short"] for p in m)
            h["overlap_pairs"] += any(p["overlap"] for p in m)
            h["have_eq_keep"] += any(p["have"] == keep for p in m)
            h["have_grows_in_steps"] += sum(1 for p in m if 0 < p["have"] < keep and p["len"] < p["have"]) >= 3
            for p in m:
                h["depths"][p["depth"]] = h["depths"].get(p["depth"], 0) + 1
                h["filled_from_start"] += p["filled"] and p["from_start"]
                h["filled_reported"] += p["error"]
        st["halo_%d" % (halo or 64)] = h
    scans = shards = reported = 0
    for di, d in enumerate(docs):
        for bd in split_configs(d, di):
            for H in SPLIT_HALOS:
                shards += len(bd)
                reported += sum(1 for a, _b in bd if min(H, a) != a and halo_filled(d.data, a, min(H, a)))
    st["split_shards"], st["split_shards_reporting_halo"] = shards, reported
    st["slice_pushes"] = slices()[1]
    return st


def format_statistics(st):
    lines = ["%d documents, %d bytes (%d..%d each); %d accepted by the oracle (%.0f %%); verdicts %s" % (
        st["documents"], st["bytes"], st["min_len"], st["max_len"], st["accepted"], 100.0 * st["accepted"] / st["documents"], st["status_counts"]),
        "%d (document, chunking) pairs, %d pushes per halo; last chunk lengths %s; pushes per slice %s" % (
            st["pairs"], st["pushes"], st["last_lengths"], list(st["slice_pushes"])),
        "%d hazard classes, %d (class, split) positions, %d of them never on a chunk edge" % (
            len(required_keys()), sum(len(k) for k in required_keys().values()), len(st["unmet"]))]
    for halo in STREAM_HALOS:
        h = st["halo_%d" % (halo or 64)]
        lines.append("halo %4d: %d pushes; pairs with a chunk shorter than what is kept %d (%.0f %%), with the overlap branch %d; have == keep in %d "
                     "pairs, grows in small steps in %d; escalation depths %s; a run fills all that is kept: %d resolved from the start, %d reported" % (
                         halo or 64, h["pushes"], h["short_pairs"], 100.0 * h["short_pairs"] / st["pairs"], h["overlap_pairs"], h["have_eq_keep"],
                         h["have_grows_in_steps"], dict(sorted(h["depths"].items())), h["filled_from_start"], h["filled_reported"]))
    lines.append("split: %d shards over all (document, bounds, halo), %d of them report SJMI_ST_HALO" % (st["split_shards"], st["split_shards_reporting_halo"]))
    return "\n".join(lines)
