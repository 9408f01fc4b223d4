"""Batches and cut points for the three capacities of sjmi_parse_batch_device / _optimistic / _rejected (index_capacity,
string_capacity, tape_capacity): small seeded batches in which every guard that keeps "a shortfall is reported, never overrun"
(include/sjmi.h) has a document to go wrong on, and the capacities at which each guard decides.  Everything here comes from the
oracle and the offsets alone; tests/test_batch_capacity_layouts.py holds the builder to its claims on the CPU and
tests/test_gpu_batch_capacity.py sends every cut through BatchShard.step.

The batches (Batch.roles names the documents the cuts are placed on):
  accepted  about 300 documents, each ending in '\\n', every one passes stage 1: the plain pass accepts, the tapes are laid out before
            the walk.  Strings with and without escapes, longs and doubles, nesting, two boundary literals of walk_common.AMBIGUOUS
            (listed for the exact walker and the boundary-literal kernel), `[1 1]` `{"a":1,}` `nul` (fail stage 2, keep their
            predicted slot), `[]`, a blank document (a two-word slot), one document near 2 KiB of more than 160 tape words
  repaired  the same with an unclosed string in front, invalid UTF-8 in the middle and an odd backslash run in front of the end
            (batch_layouts.failing_documents): two-word slots, no indexes; the repair stage takes it
  packed    no separators and a document that passes stage 1 and ends in a backslash (batch_layouts.backslash_in_front_of_dense):
            neither the plain pass nor the repair stage takes it (sjmi.h at sjmi_parse_batch_device_rejected: the last byte of every
            document must be whitespace, an operator or a quote), the exact entry's per-document passes do; tapes packed by
            k_tape_compact, PACK_DOCS documents per workgroup, a failing document's slot empty.  More than PACK_DOCS documents.
  single    one document of more than 64 structurals

ENTRIES is the table of which entry runs on which batch.  Plain module, not a conftest."""
import random

import numpy as np

from tests import batch_layouts as BL

PACK_DOCS = 1024  # documents per workgroup of k_tape_compact (walk.hip)
LINE_INDEXES = 32  # indexes of a 128-byte line
CANARY_WORDS = 512  # what the GPU test allocates behind every array; no slot of these batches is longer (see tape_cuts)

ENTRIES = {"accepted": ("optimistic", "exact", "rejected"), "repaired": ("optimistic", "exact", "rejected"), "packed": ("exact",),
           "single": ("optimistic", "exact", "rejected")}
LAID_OUT = {"accepted": True, "repaired": True, "packed": False, "single": False}  # tapes laid out before the walk / packed behind it

STAGE2_FAILURES = (b"[1 1]", b'{"a":1,}', b"nul")
STRINGS_DOC = b'["plain","esc\\n\\u00e9\\"q"]'  # record 0 without an escape, record 1 with three
STRINGS_RECORDS = (b"plain", b'esc\n\xc3\xa9"q')


class Batch:
    def __init__(self, name, buf, offs, docs, roles):
        self.name, self.buf, self.offs, self.docs, self.roles = name, buf, offs, docs, roles
        self.entries, self.laid_out = ENTRIES[name], LAID_OUT[name]


def _ambiguous():
    from tests.walk_common import AMBIGUOUS
    return [("[%s]" % AMBIGUOUS[0]).encode(), ('{"x":%s,"s":"t"}' % AMBIGUOUS[2]).encode()]


def long_document():
    """near 2 KiB, more than 64 tokens (several steps of the token walker), more than 160 and fewer than CANARY_WORDS tape words"""
    items, i = [], 0
    while sum(len(x) + 1 for x in items) < 1990:
        items.append([b'"a string of the long document, number %03d"' % i, b"%d" % (i * 7919), b"-%d.5" % i, b'{"k":%d}' % i, b"[]",
                      b'"esc\\t%d"' % i, b"true"][i % 7])
        i += 1
    return b"[" + b",".join(items) + b"]"


def _mix(rng, i):
    r = rng.randrange(7)
    if r == 0:
        return b'{"id":%d,"name":"user %d","tags":["a","b\\n"],"score":%d.5,"ok":true,"nested":{"k":[1,2,{"z":null}]}}' % (i, i, i % 97)
    if r == 1:
        return b'["plain %d","tab\\there","quote\\"q","\\u00e9\\u4e2d","back\\\\slash"]' % i
    if r == 2:
        return b"[%d,-%d,%d.25,1e%d,-0.0,9223372036854775807]" % (i, i * 31, i, i % 20)
    if r == 3:
        return b'[[[[%d]]],{"a":{"b":{"c":[true,false,null]}}}]' % i
    if r == 4:
        return b'{"k%d":"v","n":[1,"s"]}' % i
    if r == 5:
        return b"[" + b",".join(b'"s%d"' % j for j in range(i % 9)) + b"]"
    return BL.FOLLOWERS[i % len(BL.FOLLOWERS)]


def _accepted_documents():
    """-> (documents without their separator, roles)"""
    rng = random.Random(2911)
    docs = [_mix(rng, i) for i in range(300)]
    roles = {}

    def put(at, role, d):
        docs[at] = d
        roles[role] = at
    amb = _ambiguous()
    put(0, "first", b'["first",1,{"a":"b\\n"}]')
    put(17, "listed", amb[0])
    put(40, "two_structurals", b"[]")
    put(61, "fail_space", STAGE2_FAILURES[0])
    put(97, "strings", STRINGS_DOC)
    put(120, "long", long_document())
    put(150, "middle", b'{"middle":[1,"m\\\\",2.5],"t":null}')
    put(171, "fail_comma", STAGE2_FAILURES[1])
    put(200, "blank", b"")
    put(230, "listed2", amb[1])
    put(262, "fail_atom", STAGE2_FAILURES[2])
    put(299, "last", b'{"last":[1.5,"z"],"t":true}')
    return docs, roles


def _pack(name, items, roles):
    buf, offs = bytearray(), [0]
    for d, sep in items:
        buf += d + sep
        offs.append(len(buf))
    return Batch(name, bytes(buf), np.array(offs, dtype=np.uint64), [d + s for d, s in items], roles)


def accepted():
    docs, roles = _accepted_documents()
    return _pack("accepted", [(d, b"\n") for d in docs], roles)


def repaired():
    docs, roles = _accepted_documents()
    items = [(d, b"\n") for d in docs]
    fails = {name: (d, sep) for name, d, sep in BL.failing_documents()}
    # (from the back, so that the positions in front stay: at the end, in the middle, in front)
    items.append(fails["backslash"])
    items.insert(151, fails["utf8"])
    items.insert(0, fails["unclosed"])
    roles = {r: k + 1 + (1 if k >= 151 else 0) for r, k in roles.items()}
    roles.update(s1_front=0, s1_middle=152, s1_end=len(items) - 1)
    return _pack("repaired", items, roles)


def packed():
    L = BL.backslash_in_front_of_dense()
    items = [(b, b"") for b in L.bodies]
    roles = {"first": 0, "s1_unclosed": 40, "trailing_backslash": L.hazards[0] - 1}
    rng = random.Random(2912)
    amb = _ambiguous()

    def put(role, d):
        roles[role] = len(items)
        items.append((d, b""))
    put("long", long_document())
    put("listed", amb[0])
    put("fail_space", STAGE2_FAILURES[0])
    put("strings", STRINGS_DOC)
    put("fail_comma", STAGE2_FAILURES[1])
    put("listed2", amb[1])
    while len(items) < PACK_DOCS + 90:
        k = len(items)
        if k == PACK_DOCS // 2:
            put("middle", b'{"middle":[1,"m\\\\",2.5],"t":null}')
        elif k == PACK_DOCS - 1:
            put("chunk0_last", b'{"end of":"the first chunk","n":[1,2]}')
        elif k == PACK_DOCS:
            put("chunk1_first", b'["the second chunk begins",-3,{}]')
        else:
            d = _mix(rng, k)
            items.append((d if d[-1:] in b"]}" else b"[" + d + b"]", b""))
    put("last", b'{"last":[1.5,"z"],"t":true}')
    return _pack("packed", items, roles)


def single():
    d = b"[" + b",".join([b"%d" % i, b'"s%d\\n"' % i, b"{}"][i % 3] for i in range(90)) + b"]"
    return _pack("single", [(d, b"\n")], {"first": 0, "last": 0})


BATCHES = {"accepted": accepted, "repaired": repaired, "packed": packed, "single": single}
_cache = {}


def batch(name):
    """(built once: deterministic, and nothing may change it)"""
    if name not in _cache:
        _cache[name] = BATCHES[name]()
    return _cache[name]


# ---- the oracle's view: needs and offsets ----------------------------------------------------------------------------------------
class Expect:
    """wants[k] = (oracle.stage1(doc), oracle.parse(doc)), as _verify of test_gpu_batch_layouts.py takes them; counts[k] = the
    document's indexes (0 where it fails stage 1); slots[k] = its tape slot as _verify defines it (well-formed: the tape's length;
    laid out and failing stage 2: the predicted length, failing stage 1: two words; packed and failing: none); io / to = their
    running sums (index_offsets / tape_offsets); need_idx = io[n] + 1 (the sentinel), need_tape = to[n]; sb_wellformed = the string
    bytes of the well-formed documents, which is need_sb where every document is well-formed (all_wellformed)"""

    def __init__(self, b):
        from oracle import oracle as O
        from tests.tok_stream_layouts import predicted_length
        self.wants = [(O.stage1(d), O.parse(d)) for d in b.docs]
        self.counts, self.slots, self.stage = [], [], []
        sb = 0
        for d, ((idx, st), want) in zip(b.docs, self.wants):
            self.counts.append(0 if st else int(idx.size))
            self.stage.append(0 if want.error == 0 else 1 if st else 2)  # 0: well-formed, else the stage it fails at
            if want.error == 0:
                self.slots.append(int(want.tape.size))
                sb += len(want.strings)
            else:
                self.slots.append(0 if not b.laid_out else 2 if st else predicted_length(d))
        self.io = np.concatenate([[0], np.cumsum(self.counts)]).astype(np.int64)
        self.to = np.concatenate([[0], np.cumsum(self.slots)]).astype(np.int64)
        self.need_idx, self.need_tape = int(self.io[-1]) + 1, int(self.to[-1])
        self.sb_wellformed = sb
        self.all_wellformed = all(s == 0 for s in self.stage)


_expect = {}


def expect(name):
    if name not in _expect:
        _expect[name] = Expect(batch(name))
    return _expect[name]


# ---- the cuts: [(capacity, label)], ascending, each capacity once -----------------------------------------------------------------
def _cuts(pairs, lowest):
    seen, out = set(), []
    for c, label in sorted(pairs, key=lambda t: t[0]):
        if c >= lowest and c not in seen:
            seen.add(c)
            out.append((int(c), label))
    return out


def _three(b):
    """the first, a middle and the last document"""
    return [("first", b.roles["first"]), ("middle", b.roles.get("middle", len(b.docs) // 2)), ("last", b.roles["last"])]


def index_cuts(name):
    """need and need - 1; need - r for r in 2..33 (every residue of the cut modulo the 32 indexes of a line); index_offsets[k] - 1, + 0,
    + 1 of the first, a middle and the last document; 1 (the sentinel only) and 2.  (index_capacity 0 is an argument error.)"""
    b, e = batch(name), expect(name)
    pairs = [(e.need_idx, "need"), (e.need_idx - 1, "need - 1"), (1, "the sentinel only"), (2, "2")]
    pairs += [(e.need_idx - r, "need - %d" % r) for r in range(2, LINE_INDEXES + 2)]
    for role, k in _three(b):
        pairs += [(int(e.io[k]) + d, "index_offsets[%s] %+d" % (role, d)) for d in (-1, 0, 1)]
    return _cuts(pairs, 1)


def string_record_offsets(name):
    """the records of the `strings` document relative to its doc_string_offsets: -> [(first byte, first content byte, last byte)]
    for STRINGS_RECORDS -- a record is a 4-byte big-endian length and the bytes (sj_strings.h)"""
    e = expect(name)
    raw = bytes(e.wants[batch(name).roles["strings"]][1].strings)
    out, at = [], 0
    for want in STRINGS_RECORDS:
        n = int.from_bytes(raw[at:at + 4], "big")
        assert raw[at + 4:at + 4 + n] == want, (raw, at)
        out.append((at, at + 4, at + 4 + n - 1))
        at += 4 + n
    return out


def string_cuts(name, need_sb, dso):
    """need, need - 1 and 0; doc_string_offsets[k] - 1, + 0, + 1 of a middle and the last document; for the record without an escape
    and the one with: its first byte, inside its header, its first content byte, its last byte.  dso: doc_string_offsets of the roomy
    run (with failing documents in the batch the oracle has no batch-wide offsets; a well-formed document's records are its own)"""
    b = batch(name)
    pairs = [(need_sb, "need"), (need_sb - 1, "need - 1"), (0, "0")]
    for role, k in _three(b)[1:]:
        pairs += [(int(dso[k]) + d, "doc_string_offsets[%s] %+d" % (role, d)) for d in (-1, 0, 1)]
    if "strings" in b.roles:
        base = int(dso[b.roles["strings"]])
        for what, (first, content, last) in zip(("plain", "escaped"), string_record_offsets(name)):
            pairs += [(base + first, what + " record: first byte"), (base + first + 2, what + " record: inside the header"),
                      (base + content, what + " record: first content byte"), (base + last, what + " record: last byte")]
    return _cuts(pairs, 0)


def slot_words(n):
    """the words of a slot of n words that get a cut: all of them up to 160; behind that 0..64, every 16th and the last 64"""
    if n <= 160:
        return list(range(n))
    return sorted(set(range(65)) | set(range(0, n, 16)) | set(range(n - 64, n)))


TAPE_ROLES = {"accepted": ("first", "last", "long", "listed", "fail_space", "blank"),
              "repaired": ("first", "last", "long", "listed", "fail_space", "s1_middle", "s1_front", "s1_end"),  # (the well-formed first and last)
              "packed": ("first", "last", "long", "listed", "fail_space", "s1_unclosed"),  # (a failing document's slot is empty there)
              "single": ("first",)}


def tape_cuts(name):
    """need, need - 1, 0 and 1; every word (slot_words) of the slots of TAPE_ROLES: the first and the last document, a token-walker
    document of more than 64 tokens, one on the exact walker's list, a stage-2-failing document's predicted slot, a two-word slot;
    packed: both sides of and inside the last document of the first PACK_DOCS chunk and the first of the second; single: 2 * count + 1,
    2 * count + 2, the true length, the true length - 1 and 16"""
    b, e = batch(name), expect(name)
    pairs = [(e.need_tape, "need"), (e.need_tape - 1, "need - 1"), (0, "0"), (1, "1")]
    for role in TAPE_ROLES[name]:
        k = b.roles[role]
        pairs += [(int(e.to[k]) + j, "%s + %d" % (role, j)) for j in slot_words(e.slots[k])]
    if name == "packed":
        for role in ("chunk0_last", "chunk1_first"):
            k = b.roles[role]
            for edge, at in (("start", int(e.to[k])), ("end", int(e.to[k + 1]))):
                pairs += [(at + d, "%s %s %+d" % (role, edge, d)) for d in (-1, 0, 1)]
    if name == "single":
        count = e.counts[0]
        pairs += [(2 * count + 1, "2 * count + 1"), (2 * count + 2, "2 * count + 2"), (e.slots[0], "the true length"),
                  (e.slots[0] - 1, "the true length - 1"), (16, "16")]
    return _cuts(pairs, 0)
