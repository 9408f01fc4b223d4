"""A seeded generator of documents and plans for the selector's tests, shared by the host simulation's suite
(tests/test_host_select_fuzz.py) and the GPU suite (tests/test_gpu_select.py).  Imports nothing from the product: what must come
out of a selection is decided by select_common.expected_columns alone; this file only decides what goes in, and counts what the
corpus covers (statistics()) from the documents and select_common.

corpus() -> [(name, [document bytes], [pointer bytes])].  A fuzz case is one random SCHEMA (a tree of objects and arrays with keys
from vocabulary()), a few dozen documents rendered from it with members dropped, shuffled, shifted by filler, duplicated and
replaced by scalars, the same number of documents of OTHER schemas shuffled in between (so that neighbours in a batch are unlike:
staged next to not staged, deep next to flat, 3 members next to 300), and one plan whose pointers were drawn by walking the
rendered documents -- hits and their near-misses.  The limit cases walk plans at the limits of include/sjmi.h."""
import functools
import json
import random
import struct

from tests import select_common as SC

SEED = 20261017
OBJECT_SIZES = [0, 1, 15, 16, 17, 31, 32, 33, 48]
WIDE_SIZES = [200, 300, 48, 33]
PLAN_SIZES = [1, 2, 5, 12, 20, 33, 48, 64]
N_SCHEMAS = 32
OWN_DOCS = 72      # documents rendered from a case's schema ...
FOREIGN_DOCS = 40  # ... and documents of other schemas between them
BYTE_POSITIONS = (0, 7, 8, -1)  # where the near-miss families differ: first byte, byte 7, byte 8, last byte
MAX_PATHS, MAX_STEPS, MAX_NAME_BYTES = 64, 16, 4096  # (tests/test_select_plan.py holds these against include/sjmi.h)
# the cases of corpus(), by name, for whoever parametrises over them without generating anything at collection time
CASE_IDS = ["fuzz_%d" % g for g in range(N_SCHEMAS)] + ["limit_64_children", "limit_full_name_table", "limit_key_of_4096_bytes", "limit_last_string_record"]

_FILL = b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGH"
LENGTH_KEYS = [(b"L%02d" % n + _FILL)[:n] for n in range(41)]  # one key of every length 0..40
LONG_KEYS = [(b"long%04d_" % n * (n // 9 + 1))[:n] for n in (100, 1000, 4096)]
FAMILY_BASE = b"abcdefghijklmnopqrst"


def _changed(key, pos):
    b = bytearray(key)
    b[pos] ^= 1
    return bytes(b)


def vocabulary():
    """the keys documents are made of: (all, the short ones a schema samples from)"""
    first8 = [b"prefix8_" + s for s in (b"alpha", b"alphb", b"blpha", b"x", b"")]
    first16 = [b"sharedprefix16__" + s for s in (b"tail0001", b"tail0002", b"uail0001", b"t", b"")]
    family = [FAMILY_BASE] + [_changed(FAMILY_BASE, p) for p in BYTE_POSITIONS]
    tokens = [b"0", b"10", b"01", b"-"]
    special = [b"a/b", b"m~n", b'q"r', b"b\\s", b"nu\x00l", "é".encode(), "k€y".encode(), b"~1", b"/", b"~"]
    short = LENGTH_KEYS + first8 + first16 + family + tokens + special + LONG_KEYS[:1]
    assert len(set(short)) == len(short)
    return short + LONG_KEYS[1:], short


def key_text(key, escaped=False):
    """the key as a JSON string: literally (what must be escaped, escaped), or every character as \\uXXXX"""
    s = key.decode("utf-8")
    if escaped:
        return ('"' + "".join("\\u%04x" % ord(c) for c in s) + '"').encode()
    return json.dumps(s, ensure_ascii=False).encode("utf-8")


def pointer(tokens):
    return b"".join(b"/" + SC.escape_token(t) for t in tokens)


_STRINGS = [b'"s"', b'""', b'"a\\nb"', b'"\\u00e9"', '"é€"'.encode(), b'"x\\u0000y"', b'"q\\"r\\\\"', b'"' + b"v" * 57 + b'"', b'"12345678"']
_NUMBERS = [b"0", b"-1", b"7", b"9223372036854775807", b"-9223372036854775808", b"1.5", b"-0.0", b"1e300", b"2.5e-3", b"123456789012"]


def scalar(rng):
    """a value of one tape word (an atom, a string) or two (an integer, a double), header-looking payloads among them"""
    r = rng.randrange(12)
    if r < 3:
        return (b"true", b"false", b"null")[r]
    if r < 5:
        return rng.choice(_NUMBERS)
    if r == 5:
        return b"%d" % rng.choice(SC.HEADER_LOOKING)
    if r == 6:
        return repr(struct.unpack("<d", struct.pack("<Q", rng.choice(SC.HEADER_LOOKING[:6])))[0]).encode()
    if r == 7:
        return b"%d" % rng.randrange(-1000, 100000)
    return rng.choice(_STRINGS)


# ---- schemas: ["s"] a scalar, ["a", [child]] an array, ["o", [[key, child]]] an object --------------------------------------
def _schema(rng, short, depth, size, as_array=False):
    def child():
        if depth < 5 and rng.random() < (0.35 if depth < 2 else 0.25) / (1 + size / 24):
            return _schema(rng, short, depth + 1, rng.choice([0, 1, 2, 3, 3, 5, 8]), rng.random() < 0.35)
        return ["s"]
    if as_array:
        return ["a", [child() for _ in range(size)]]
    keys = rng.sample(short, min(size, len(short)))
    keys += [b"w%03d" % i for i in range(size - len(keys))]  # (a wide object: more members than the vocabulary has short keys)
    rng.shuffle(keys)
    return ["o", [[k, child()] for k in keys]]


def _spine(rng, short, levels):
    """nesting of `levels` containers, objects and arrays mixed, with a few members beside the way down"""
    node = ["s"]
    for _ in range(levels):
        if rng.random() < 0.4:
            elems = [["s"] for _ in range(rng.randrange(3))]
            elems.insert(rng.randrange(len(elems) + 1), node)
            node = ["a", elems]
        else:
            keys = rng.sample(short, rng.choice([1, 2, 3, 4]))
            members = [[k, ["s"]] for k in keys]
            members[rng.randrange(len(members))][1] = node
            node = ["o", members]
    return node


def make_schema(rng, g):
    allk, short = vocabulary()
    if g % 4 == 0:
        node = _spine(rng, short, rng.choice([12, 15, 16, 17, 20]))
    elif g % 4 == 1:
        node = _schema(rng, short, 0, WIDE_SIZES[(g // 4) % len(WIDE_SIZES)])
    else:
        node = _schema(rng, short, 0, OBJECT_SIZES[(g // 2) % len(OBJECT_SIZES)] if g % 8 != 6 else 17, as_array=g % 8 == 6)
    if node[0] == "o" and node[1] and g % 5 == 0:  # a long key now and then (every document of the schema pays its bytes)
        node[1][rng.randrange(len(node[1]))][0] = LONG_KEYS[1 + (g // 5) % 2]
    return node


# ---- documents --------------------------------------------------------------------------------------------------------------
def _render(node, rng, pad=None):
    if node[0] == "s":
        return scalar(rng)
    if node[0] == "a":
        elems = [_render(c, rng) for c in node[1]]
        r = rng.random()
        if r < 0.2 and elems:
            del elems[rng.randrange(len(elems)):]  # (an index the plan holds is now the length, or behind it)
        elif r < 0.3:
            elems += [scalar(rng) for _ in range(rng.choice([1, 15, 16, 17, 33]))]
        if pad is not None:
            elems += [b"true"] * pad
        return b"[" + b",".join(elems) + b"]"
    members = []  # [key, text]
    for key, child in node[1]:
        r = rng.random()
        if r < 0.12:
            continue
        if r < 0.17:
            child = ["s"]  # a scalar where paths go on
        elif r < 0.20:
            child = ["a", [["s"], ["s"]]]
        members.append([key, _render(child, rng)])
    if rng.random() < 0.5:
        rng.shuffle(members)
    # filler in one block: moves the members behind it to positions 15, 16, 17, 31, 32 ... of the object
    at = rng.randrange(len(members) + 1)
    members[at:at] = [[b"f%d" % i, scalar(rng)] for i in range(rng.choice([0, 0, 0, 1, 2, 14, 15, 16, 17, 30, 31, 32]))]
    # a duplicate key: in the same round, 16 members on, or behind a member the walk descends into
    if members and rng.random() < 0.45:
        i = rng.randrange(len(members))
        dup = [members[i][0], rng.choice([b'"second"', b"2", b'{"x":"second"}', b"[2]", b"null"])]
        how = rng.randrange(3)
        if how == 0:
            members.insert(min(len(members), i + 1 + rng.randrange(3)), dup)
        elif how == 1:
            members += [[b"g%d" % k, scalar(rng)] for k in range(i + 16 - len(members))]
            members.insert(i + 16, dup)
        else:
            behind = [j for j in range(i + 1, len(members)) if members[j][1][:1] in (b"{", b"[")]
            if behind:
                members.insert(rng.choice(behind) + 1, dup)
    if pad is not None:
        members.insert(rng.choice([0, len(members)]), [b"pad", b"[" + b",".join([b"true"] * pad) + b"]"])
    return b"{" + b",".join(key_text(k, len(k) < 48 and rng.random() < 0.2) + b":" + v for k, v in members) + b"}"


def render_document(schema, seed, target_words=None):
    """one document of the schema; target_words: padded with atoms to exactly that many tape words (None when it is larger already)"""
    if target_words is None:
        return _render(schema, random.Random(seed))
    from oracle import oracle as O
    have = len(O.parse(_render(schema, random.Random(seed), 0)).tape)
    if have > target_words:
        return None
    doc = _render(schema, random.Random(seed), target_words - have)
    assert len(O.parse(doc).tape) == target_words
    return doc


TRIVIAL = [b"[]", b"{}", b"5", b'"s"', b"null", b"-0.0", b'{"":1}', b"[[],{}]", b'{"a":{"b":{}}}', b"[1,2,3]"]


# ---- plans ------------------------------------------------------------------------------------------------------------------
def plan_fits(pointers):
    """what sel_compile accepts: the limits of include/sjmi.h, the name table counted per trie edge in 8-byte words"""
    if len(pointers) > MAX_PATHS:
        return False
    edges = set()
    for p in pointers:
        tokens = SC.pointer_tokens(p)
        if len(tokens) > MAX_STEPS:
            return False
        edges.update(tuple(tokens[:n + 1]) for n in range(len(tokens)))
    return sum((len(e[-1]) + 7) // 8 * 8 for e in edges) <= MAX_NAME_BYTES


def _walk(rng, root):
    """a random path of 1..16 steps through a to_python() tree -> (tokens, the containers stepped through, the value reached)"""
    tokens, through, cur = [], [], root
    for _ in range(rng.randint(1, MAX_STEPS)):
        if cur[0] == "o" and cur[2]:
            inner = [m for m in cur[2] if m[1][0] in "oa"]
            key, nxt = rng.choice(inner if inner and rng.random() < 0.6 else cur[2])
            tokens.append(bytes(key))
        elif cur[0] == "a" and cur[2]:
            k = rng.randrange(len(cur[2]))
            tokens.append(b"%d" % k)
            nxt = cur[2][k]
        else:
            break
        through.append(cur)
        cur = nxt
    return tokens, through, cur


def _near_miss(rng, tokens, through, reached):
    tokens = list(tokens)
    if not tokens:
        return [b"x"]
    s = rng.randrange(len(tokens))
    tok, how = tokens[s], rng.randrange(7)
    if how == 0 and tok:
        pos = rng.choice([p for p in BYTE_POSITIONS if p < len(tok)])
        tokens[s] = _changed(tok, pos)
    elif how == 1:
        tokens[s] = tok[:-1]
    elif how == 2:
        tokens[s] = tok + rng.choice([b"x", b"0", b"\x00"])
    elif how == 3 and through[s][0] == "a":
        tokens[s] = b"%d" % len(through[s][2])  # index = length
    elif how == 4 and through[s][0] == "a":
        tokens[s] = b"0" + tok  # a leading zero
    elif reached[0] not in "oa":
        tokens = (tokens + [rng.choice([b"x", b"0", b""])])[:MAX_STEPS + 1]  # a step through a scalar
        if len(tokens) > MAX_STEPS:
            tokens = tokens[:MAX_STEPS - 1] + [b"x"]
    else:
        tokens[s] = tok + b"~"
    return tokens


def draw_plan(rng, roots, n_paths):
    """n_paths pointers: hits of the documents `roots` (to_python() trees), their near-misses, repeats and the root"""
    out = []
    for _ in range(40 * n_paths):
        if len(out) == n_paths:
            break
        tokens, through, reached = _walk(rng, rng.choice(roots))
        r = rng.random()
        if r < 0.55:
            cand = pointer(tokens)
        elif r < 0.9:
            cand = pointer(_near_miss(rng, tokens, through, reached))
        elif r < 0.96 and out:
            cand = rng.choice(out)
        else:
            cand = b""
        if plan_fits(out + [cand]):
            out.append(cand)
    assert out
    return out


# ---- the limit cases ----------------------------------------------------------------------------------------------------------
def limit_cases():
    rng = random.Random(SEED ^ 0x11)
    allk, short = vocabulary()
    cases = []
    # 64 paths that are 64 children of the root, over objects that hold all, some and none of them in shuffled order
    kids = [k for k in short if len(k) <= 40][:MAX_PATHS]
    assert len(kids) == MAX_PATHS
    docs = []
    for n in (64, 64, 64, 40, 17, 16, 3, 1, 0, 0):
        for _ in range(2):
            members = [[k, scalar(rng)] for k in rng.sample(kids, n)] + [[b"f%d" % i, scalar(rng)] for i in range(rng.choice([0, 1, 16, 40]))]
            rng.shuffle(members)
            docs.append(b"{" + b",".join(key_text(k, rng.random() < 0.2) + b":" + v for k, v in members) + b"}")
    docs += [b"[" + b",".join(scalar(rng) for _ in range(12)) + b"]", b"{}", b"7"]
    cases.append(("limit: 64 children of the root", docs, [pointer([k]) for k in kids]))
    # a name table of exactly 4096 bytes: 32 paths x 16 steps of 8-byte tokens
    names = [[b"%07d%x" % (p, s) for s in range(16)] for p in range(32)]
    docs = []
    for _ in range(12):
        members = []
        for p in rng.sample(range(32), rng.choice([1, 3, 8, 32])):
            depth = rng.choice([16, 16, 15, 9, 1])
            text = scalar(rng)
            for s in range(depth - 1, -1, -1):
                side = b'"side":%s,' % scalar(rng) if rng.random() < 0.3 else b""
                text = b"{" + side + key_text(names[p][s]) + b":" + text + b"}"
            members.append(text[1:-1])
        docs.append(b"{" + b",".join(members) + b"}")
    full = [pointer(t) for t in names]
    assert plan_fits(full) and not plan_fits(full + [b"/x"])
    cases.append(("limit: a full name table", docs, full))
    # one token of 4096 bytes
    big = LONG_KEYS[2]
    assert len(big) == MAX_NAME_BYTES
    docs = [b"{" + key_text(big) + b":1}", b"{" + key_text(_changed(big, -1)) + b':1,"a":2}', b"{" + key_text(big[:-1]) + b":1," + key_text(big) + b':"found"}',
            b"{" + key_text(_changed(big, 0)) + b":1," + key_text(_changed(big, 4088)) + b":2," + key_text(big) + b":[3]," + key_text(big) + b":4}",
            b'{"a":1}', b'{"a":{' + key_text(big) + b":1}}"]
    cases.append(("limit: a key of 4096 bytes", docs, [pointer([big])]))
    # the last string record of a document: a key of every length (every load shape of sel_key_word) that the plan names, keys
    # whose first 8 / 16 bytes a name of the same length shares, and a selected string value
    keys = LENGTH_KEYS + LONG_KEYS[:1] + [b"prefix8_alpha", b"prefix8_alphb", b"sharedprefix16__tail0001", b"sharedprefix16__tail0002"] + \
        [FAMILY_BASE] + [_changed(FAMILY_BASE, p) for p in BYTE_POSITIONS]
    docs = [b'{"x":"first",' + key_text(k) + b":%d}" % i for i, k in enumerate(keys)]
    docs += [b"[1,{" + key_text(k) + b":[true]}]" for k in keys[:41:5]]
    docs += [b'{"x":"the last record"}', b'{"L":{"x":""}}', b'"root"']
    ptrs = [pointer([k]) for k in keys] + [b"/x", b"/L/x", b""]
    assert plan_fits(ptrs)
    cases.append(("limit: the last string record", docs, ptrs))
    return cases


# ---- the corpus ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus():
    from oracle import oracle as O
    S = SC.slice_words()
    own = []
    for g in range(N_SCHEMAS):
        rng = random.Random(SEED * 1000 + g)
        schema = make_schema(rng, g)
        docs = [render_document(schema, rng.getrandbits(48)) for _ in range(OWN_DOCS - 4)]
        # tapes on both sides of the slice (a document that is larger already stays as it is)
        for target in (S - 1, S, S + 1, 4 * S + 1 + rng.randrange(200)):
            seed = rng.getrandbits(48)
            docs.append(render_document(schema, seed, target) or render_document(schema, seed))
        own.append(docs)
    cases = []
    for g in range(N_SCHEMAS):
        rng = random.Random(SEED * 1000 + 500 + g)
        foreign = [rng.choice(own[rng.choice([h for h in range(N_SCHEMAS) if h != g])]) for _ in range(FOREIGN_DOCS - 4)] + rng.sample(TRIVIAL, 4)
        roots = [O.parse(d).to_python() for d in own[g][::6]]
        ptrs = draw_plan(rng, roots, PLAN_SIZES[g % len(PLAN_SIZES)])
        docs = own[g] + foreign
        rng.shuffle(docs)
        cases.append(("fuzz %d" % g, docs, ptrs))
    cases += limit_cases()
    assert len(cases) == len(CASE_IDS)
    return cases


# ---- what the corpus covers ---------------------------------------------------------------------------------------------------
def _trace(root, tokens):
    """the object steps the pointer matches in the document -> ([(tokens in front, member position, the object, descends)], present)"""
    out, cur = [], root
    for n, tok in enumerate(tokens):
        if cur[0] == "o":
            pos = next((i for i, (k, _) in enumerate(cur[2]) if k == tok), None)
            if pos is None:
                return out, False
            nxt = cur[2][pos][1]
            out.append((tuple(tokens[:n]), pos, cur, n + 1 < len(tokens) and nxt[0] in "oa"))
            cur = nxt
        elif cur[0] == "a" and SC._INDEX.fullmatch(tok) and int(tok) < len(cur[2]):
            cur = cur[2][int(tok)]
        else:
            return out, False
    return out, True


@functools.lru_cache(maxsize=None)
def parsed_corpus():
    """-> [(name, documents, pointers, [oracle.Parsed], expected_columns)]"""
    from oracle import oracle as O
    out = []
    for name, docs, ptrs in corpus():
        parsed = [O.parse(d) for d in docs]
        assert not any(p.error for p in parsed), name
        out.append((name, docs, ptrs, parsed, SC.expected_columns(parsed, ptrs)))
    return out


def statistics():
    """what the generator's own test asserts: counted from the documents and select_common, nothing of the product"""
    S = SC.slice_words()
    st = {"documents": 0, "pairs": 0, "present": 0, "matched_key_lengths": set(), "matched_positions": set(), "behind_a_descent": 0,
          "duplicates": {"same round": 0, "16 members apart": 0, "across a descent": 0}, "tape_words": set(), "plan_sizes": set(),
          "max_nesting": 0, "object_sizes": set(), "array_sizes": set(), "types": set(), "last_record_key_shapes": set(), "last_record_value": 0}

    def shape(v, depth):
        st["max_nesting"] = max(st["max_nesting"], depth)
        if v[0] == "o":
            st["object_sizes"].add(len(v[2]))
            for _, e in v[2]:
                shape(e, depth + 1)
        elif v[0] == "a":
            st["array_sizes"].add(len(v[2]))
            for e in v[2]:
                shape(e, depth + 1)
    for name, docs, ptrs, parsed, want in parsed_corpus():
        st["documents"] += len(docs)
        st["plan_sizes"].add(len(ptrs))
        tokens = [SC.pointer_tokens(p) for p in ptrs]
        for k, p in enumerate(parsed):
            root = p.to_python()
            shape(root, 0)
            st["tape_words"].add(len(p.tape))
            steps = []
            for n, t in enumerate(tokens):
                tr, present = _trace(root, t)
                assert present == (want[n][k][0] != SC.MISSING)
                st["pairs"] += 1
                st["present"] += present
                st["types"].add(want[n][k][0])
                steps += tr
            descents = {}
            for front, pos, obj, down in steps:
                st["matched_key_lengths"].add(len(obj[2][pos][0]))
                st["matched_positions"].add(pos)
                if down:
                    descents.setdefault(front, set()).add(pos)
            for front, pos, obj, down in set((f, q, id(o), d) for f, q, o, d in steps):
                st["behind_a_descent"] += any(d < pos for d in descents.get(front, ()))
            for front, pos, obj, down in steps:
                key, val = obj[2][pos]
                for j in range(pos + 1, len(obj[2])):
                    if obj[2][j][0] == key and obj[2][j][1] != val:  # first match wins, and a wrong winner would show
                        between = [d for d in descents.get(front, ()) if pos < d < j]
                        if between:
                            st["duplicates"]["across a descent"] += 1
                        elif j - pos == 16:
                            st["duplicates"]["16 members apart"] += 1
                        elif j - pos < 16 and pos not in descents.get(front, ()):
                            st["duplicates"]["same round"] += 1
            # the last record of the document's string buffer: a key the plan matches (by the load shape of sel_key_word), or a selected value
            words = last_record(p)
            if words is not None:
                off, ln, end = words
                rec = bytes(p.strings[off + 4:off + 4 + ln])
                for front, pos, obj, down in steps:
                    if bytes(obj[2][pos][0]) == rec and pos == len(obj[2]) - 1 and obj[2][pos][1][0] not in "soa":
                        st["last_record_key_shapes"].add("0" if ln == 0 else "1-3" if ln < 4 else "4-7" if ln < 8 else "whole words" if ln % 8 == 0 else "tail")
                for n in range(len(ptrs)):
                    t, payload = want[n][k]
                    st["last_record_value"] += t == ord('"') and payload == rec and _value_is_last(root, tokens[n])
    return st


def _value_is_last(root, tokens):
    """the value the pointer reaches is the last thing in the document (so a string there is the last record)"""
    cur = root
    for tok in tokens:
        if cur[0] == "o":
            if not cur[2] or cur[2][-1][0] != tok or any(k == tok for k, _ in cur[2][:-1]):
                return False
            cur = cur[2][-1][1]
        elif cur[0] == "a":
            if not cur[2] or tok != b"%d" % (len(cur[2]) - 1):
                return False
            cur = cur[2][-1]
        else:
            return False
    return True


def last_record(parsed):
    """-> (offset, length, end) of the record of parsed.strings that lies last, from the tape's string words; None without one"""
    t, best, i, n = parsed.tape, None, 1, len(parsed.tape) - 1
    while i < n:
        w = int(t[i])
        ty = w >> 56
        if ty == ord('"'):
            off = w & 0x00FFFFFFFFFFFFFF
            if best is None or off > best:
                best = off
        i += 2 if ty in (ord("l"), ord("d")) else 1
    if best is None:
        return None
    ln = int.from_bytes(parsed.strings[best:best + 4], "big")
    return best, ln, best + 4 + ln
