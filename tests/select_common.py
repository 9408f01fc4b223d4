"""What a selection must give, from the oracle alone: RFC 6901 pointers applied to oracle.Parsed.to_python() -- the oracle's
tape read by the oracle's own JsonValue walk (first matching key, the iterator chain's elements, raw double bits).  Shares no
code with the product.  Used by the host simulation's tests and the GPU tests; every (path, document) pair is compared."""
import re

MISSING = 0
_INDEX = re.compile(rb"0|[1-9][0-9]*")


def escape_token(key):
    """RFC 6901 section 3: a key (bytes) as a reference token."""
    return key.replace(b"~", b"~0").replace(b"/", b"~1")


def pointer_tokens(pointer):
    """RFC 6901 section 4: the reference tokens of a pointer (bytes), unescaped ('~1' first, then '~0')."""
    pointer = pointer.encode("utf-8") if isinstance(pointer, str) else bytes(pointer)
    if pointer == b"":
        return []
    assert pointer[:1] == b"/", pointer
    return [t.replace(b"~1", b"/").replace(b"~0", b"~") for t in pointer[1:].split(b"/")]


def _words(v):
    """tape words of a to_python() value (Tape.java:28-47: two for a number, a start and an end word for a container)"""
    t = v[0]
    if t in ("l", "d"):
        return 2
    if t == "a":
        return 2 + sum(_words(e) for e in v[2])
    if t == "o":
        return 2 + sum(1 + _words(e) for _, e in v[2])
    return 1


def _step(v, idx, token):
    """one JsonValue.get / arrayIterator step: -> (value, its tape index) or None"""
    if v[0] == "o":
        p = idx + 1
        for key, val in v[2]:
            if key == token:
                return val, p + 1  # the FIRST matching member (JsonValue.java:95-105)
            p += 1 + _words(val)
        return None
    if v[0] == "a":
        if not _INDEX.fullmatch(token):
            return None
        k, p = int(token), idx + 1
        if k >= len(v[2]):
            return None
        for e in v[2][:k]:
            p += _words(e)
        return v[2][k], p
    return None


def expected_one(root, pointer):
    """-> (type byte, payload): payload = the bytes for a string, else the uint64 the column must hold; (0, 0) = MISSING"""
    cur = (root, 1)  # the root value is tape word 1
    for token in pointer_tokens(pointer):
        cur = _step(cur[0], cur[1], token)
        if cur is None:
            return (MISSING, 0)
    v, idx = cur
    t = v[0]
    if t == "s":
        return (ord('"'), bytes(v[1]))
    if t == "l":
        return (ord("l"), v[1] & 0xFFFFFFFFFFFFFFFF)
    if t == "d":
        return (ord("d"), v[1])
    if t in "tfn":
        return (ord(t), 1 if t == "t" else 0)
    return (ord("[" if t == "a" else "{"), (v[1] << 32) | idx)


def expected_columns(parsed_docs, pointers):
    """parsed_docs: oracle.Parsed or None (a failed document) per document -> [path][document] of expected_one()"""
    roots = [None if p is None or p.error else p.to_python() for p in parsed_docs]
    return [[(MISSING, 0) if r is None else expected_one(r, ptr) for r in roots] for ptr in pointers]


def check_columns(types, values, sb, want, what=""):
    """types / values: [n_paths, n_docs] arrays as the selector wrote them, sb: the string buffer (bytes-like) the string
    values point into; want: expected_columns().  Compares EVERY pair; -> the number of pairs that are not MISSING."""
    sb = memoryview(sb)
    present = 0
    assert len(types) == len(want) and len(values) == len(want)
    for p, col in enumerate(want):
        assert len(types[p]) == len(col), (what, p)
        for k, (t, payload) in enumerate(col):
            got_t, got_v = int(types[p][k]), int(values[p][k]) & 0xFFFFFFFFFFFFFFFF
            assert got_t == t, "%s path %d document %d: type %r, want %r" % (what, p, k, chr(got_t) if got_t else 0, chr(t) if t else 0)
            if t == ord('"'):
                ln, off = got_v >> 32, got_v & 0xFFFFFFFF
                assert ln == len(payload) and bytes(sb[off:off + ln]) == payload, \
                    "%s path %d document %d: string %r, want %r" % (what, p, k, bytes(sb[off:off + ln]), payload)
                assert int.from_bytes(bytes(sb[off - 4:off]), "big") == ln
            else:
                assert got_v == payload, "%s path %d document %d: value 0x%x, want 0x%x" % (what, p, k, got_v, payload)
            present += t != MISSING
    return present


# ---------------------------------------------------------------------------------------------------------------------
# inputs shared by the host-simulation tests and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def slice_words():
    """SEL_SLICE_WORDS of csrc/sj_select.h: the tape words of a document that are staged on chip"""
    import os
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "simdjson-java_amd", "csrc", "sj_select.h")).read()
    return int(re.search(r"SEL_SLICE_WORDS\s*=\s*(\d+)", text).group(1))


def reserialised(name, pick):
    """the elements pick(document) of a fixture, one JSON text each, written by Python's json (non-ASCII as \\uXXXX escapes,
    so a key or value is compared in its unescaped form)"""
    import json
    from tests.conftest import load_fixture
    return [json.dumps(e).encode("ascii") for e in pick(json.loads(load_fixture(name)))]


TWITTER_POINTERS = ["/user/default_profile", "/user/screen_name", "", "/id", "/text", "/entities/hashtags/0/text",
                    "/entities/urls/0/indices/1", "/retweeted_status/user/name", "/metadata/iso_language_code", "/coordinates",
                    "/user/entities/url/urls/0/expanded_url", "/retweet_count", "/favorited", "/user", "/entities/user_mentions",
                    "/entities/user_mentions/1/screen_name", "/nope", "/user/nope/deeper", "/text/0", "/user/name"]
GITHUB_POINTERS = ["/type", "/actor/login", "/repo/name", "/payload/commits/0/author/name", "/payload/commits/1/sha", "/public",
                   "/created_at", "/payload/size", "/payload/issue/labels/0/name", "/payload/forkee/owner/id", "/id", "/org/login",
                   "/payload", "/payload/commits", "/payload/ref", "/actor/gravatar_id", "/payload/commits/-", "/payload/commits/00"]

HEADER_LOOKING = [0x5B00000000000005, 0x7B00000000000003, 0x2200000000000001, 0x6C00000000000000, 0x6400000000000000,
                  0x5B00000000000000, 0x7B00000000FFFFFF, 0x7200000000000002, 0x5D00000000000001, 0x7D00000000000001]


def _double_text(bits):
    import struct
    return repr(struct.unpack("<d", struct.pack("<Q", bits))[0])


def sized_document(target_words):
    """a document whose tape has exactly target_words words, with selected members at its very end"""
    from oracle import oracle as O
    for extra in ("", ",true"):  # (an integer makes two tape words, an atom one)
        m = max(0, (target_words - 40) // 2)
        while m < target_words:
            doc = ('{"pad":[%s%s],"t":true,"last":{"x":[10,20],"y":"end"}}' % (",".join(str(i) for i in range(m)), extra)).encode()
            n = len(O.parse(doc).tape)
            if n == target_words:
                return doc
            if n > target_words:
                break
            m += 1
    raise AssertionError("no document of %d tape words" % target_words)


def adversarial_cases():
    """-> [(name, [document bytes], [pointer str])]: everything section 1 of the selector's contract decides"""
    S = slice_words()
    ints = [str(v) for v in HEADER_LOOKING]
    dbls = [_double_text(v) for v in HEADER_LOOKING[:6]]
    deep = "7"
    for _ in range(16):
        deep = '{"a":%s,"b":[%s]}' % (deep, deep) if len(deep) < 4000 else '{"a":%s}' % deep
    mixed = '"leaf"'
    for i in range(16):
        mixed = '[0,%s]' % mixed if i % 2 else '{"k":%s}' % mixed
    cases = [
        ("duplicate keys", [b'{"a":1,"a":2,"b":{"c":1,"c":[2]},"a":{"x":1}}', b'{"b":{"c":"first","d":1,"c":"second"},"a":null}'],
         ["/a", "/b/c", "/a/x", "/b/c/0", "/b/d"]),
        ("escaped key", [b'{"\\u0061b":1,"ab":2}', b'{"a\\u0062":{"\\u0063":true},"x\\ny":3,"q\\"r":4,"b\\\\s":5}', b'{"\\u00e9":1,"\xc3\xa9":2}'],
         ["/ab", "/ab/c", "/x\ny", '/q"r', "/b\\s", "/\u00e9", "/a\\u0062"]),
        ("empty key", [b'{"":1}', b'{"a":0,"":{"":[5,{"":"deep"}]}}', b'{"a":1}', b'[]', b'""'],
         ["/", "//", "///1/", "", "/a", "///0"]),
        ("slash and tilde", [b'{"a/b":1,"m~n":2,"~1":3,"~":4,"/":5,"a":{"b":6},"~01":7,"m":{"n":8}}'],
         ["/a~1b", "/m~0n", "/~01", "/~0", "/~1", "/a/b", "/~001", "/m/n", "/~0~1", "/~1~0"]),
        ("zero on object and array", [b'{"0":"key"}', b'["elem"]', b'{"0":{"1":"k"},"1":["a","b"]}', b'[[0,1],{"0":"o","01":"p"}]', b'{"00":1,"-":2}'],
         ["/0", "/0/1", "/1/1", "/1/0", "/1/01", "/00", "/-"]),
        ("array tokens", [b'[10,11,12]', b'[[1,2],[3]]', b'[]', b'[{"a":[1,[2,3,{"b":null}]]}]', b'{"a":[1,2]}'],
         ["/0", "/2", "/3", "/01", "/-", "/1/0", "/0/1", "/0/2", "/0/a/1/2/b", "/0/a/1/2", "/0/a/1/3", "/a/1", "/a/2", "/a/-", "/a/+1",
          "/a/1e0", "/a/ 1", "/4294967296", "/18446744073709551616", "/99999999999999999999999999", "/0/99999999999999999999999999"]),
        ("through a scalar", [b'{"a":1,"b":"str","c":null,"d":true,"e":1.5}', b'5', b'"s"', b'null', b'false', b'-0.0', b'9223372036854775807',
                               b'-9223372036854775808'],
         ["/a/b", "/b/0", "/c/x", "/d/0", "/e/e", "", "/0", "/a", "/"]),
        ("roots and empties", [b'[]', b'{}', b'[[],{}]', b'{"a":[],"b":{}}', b'[1]', b'{"a":{"b":{}}}', b'1e300', b'true'],
         ["", "/0", "/1", "/a", "/b", "/a/0", "/b/x", "/0/0", "/1/a", "/a/b", "/a/b/c"]),
        ("sixteen steps", [deep.encode(), mixed.encode(), b'{"a":{"a":{"a":1}}}'],
         ["/a" * 16, "/a" * 15, "/a" * 15 + "/b", "/a" * 14 + "/b/0", "/a" * 3 + "/b/0" + "/a" * 10, "/a" * 9 + "/b/0/a/a/a/b/0",
          "".join("/1" if i % 2 else "/k" for i in range(15, -1, -1)), "".join("/1" if i % 2 else "/k" for i in range(15, 0, -1)),
          "/a/a/a", "/a/a/a/a"]),
        ("header-looking integers",
         [('{"n0":%s,"a":{"x":1},"n1":%s,"b":[%s,{"y":%s,"z":"in"},%s],"n2":%s,"c":"after","n3":[%s]}' %
           (ints[i % 10], ints[(i + 1) % 10], ints[(i + 2) % 10], ints[(i + 3) % 10], ints[(i + 4) % 10], ints[(i + 5) % 10], ",".join(ints))).encode()
          for i in range(10)] + [("[" + ",".join(ints) + ',{"k":"v"}]').encode()],
         ["/a/x", "/b/1/z", "/b/1/y", "/b/2", "/c", "/n0", "/n1", "/n2", "/n3/9", "/n3/10", "/b/0", "/10/k", "/0", "/9", "/b", "/n3"]),
        ("header-looking doubles",
         [('{"d0":%s,"a":{"x":1},"d1":%s,"b":[%s,{"y":%s,"z":"in"},%s],"c":"after","d3":[%s]}' %
           (dbls[i % 6], dbls[(i + 1) % 6], dbls[(i + 2) % 6], dbls[(i + 3) % 6], dbls[(i + 4) % 6], ",".join(dbls))).encode() for i in range(6)],
         ["/a/x", "/b/1/z", "/b/1/y", "/b/2", "/c", "/d0", "/d1", "/d3/5", "/d3/6", "/b/0", "/d3"]),
        ("around the slice", [sized_document(S - 1), sized_document(S), sized_document(S + 1), sized_document(2 * S + 1), b'{"last":{"y":1}}'],
         ["/last/x/1", "/last/y", "/pad/0", "/pad/%d" % ((S - 30) // 2), "/pad/%d" % S, "/t", "/last", "", "/pad"]),
        ("shared prefixes", [b'{"u":{"a":1,"b":{"c":2,"d":[3,4,{"e":5}]},"ab":6},"v":{"a":7},"u2":8}', b'{"u":{"b":{"d":[0]}},"u":{"a":"second"}}',
                             b'{"v":{"a":[1]},"u":[{"a":1}]}'],
         ["/u", "/u/a", "/u/b", "/u/b/c", "/u/b/d", "/u/b/d/0", "/u/b/d/2/e", "/u/ab", "/v/a", "/u2", "/u/a", "/u/b/d/2", "/v", "/u/0/a", "/v/a/0",
          "", "/u/b/d/1", "/u/b/c"]),
    ]
    return cases
