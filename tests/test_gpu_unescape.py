"""GPU parity tests of the batched string-unescape kernels (C ABI sjmi_unescape) against the oracle's
StringParser restatement: string_buffer[0,total) bit-identical, same first failing string and error code."""
import random

import numpy as np
import pytest

from oracle import oracle as O
from tests.conftest import load_fixture
from tests.golden import vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=64 * 1024 * 1024)
    yield c
    c.close()


def _check(ctx, doc):
    doc = bytes(doc)
    idx, st = ctx.stage1(doc)
    assert st == 0, "test documents must pass stage 1"
    padded = doc + b"\0" * 64
    want_sb, want_offs, want_feo, want_fec = O.unescape_all(padded, idx)
    got_sb, got_fei, got_fec = ctx.unescape(len(doc) + 4 * idx.size + 64)
    if want_feo < 0:
        assert got_fei is None and got_fec == 0
        assert got_sb == want_sb
    else:
        # oracle: ordinal among strings; GPU: position in indexes[]
        quote_positions = [i for i in range(idx.size) if doc[idx[i]] == 0x22]
        assert got_fei == quote_positions[want_feo]
        assert got_fec == want_fec
        assert got_sb[:len(want_sb)] == want_sb  # records before the failing string


@pytest.mark.parametrize("name", ["twitter.json", "github_events.json", "wide_bench.json"])
def test_reference_files(ctx, name):
    _check(ctx, load_fixture(name))


def test_every_code_point_escape(ctx):
    """StringParsingTest.java:51-70: every non-surrogate code point as \\uXXXX / surrogate pair."""
    parts = []
    for cp in list(range(0, 0x10000, 3)) + list(range(0x10000, 0x110000, 101)) + [0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10FFFF]:
        if 0xD800 <= cp <= 0xDFFF:
            continue
        if cp < 0x10000:
            parts.append('"\\u%04X"' % cp if cp % 2 else '"\\u%04x"' % cp)
        else:
            v = cp - 0x10000
            parts.append('"\\u%04X\\u%04X"' % (0xD800 + (v >> 10), 0xDC00 + (v & 0x3FF)))
    _check(ctx, ("[" + ",".join(parts) + "]").encode())


def test_random_strings(ctx):
    rng = random.Random(31337)
    esc = ['\\"', "\\\\", "\\/", "\\b", "\\f", "\\n", "\\r", "\\t", "\\u00e9", "\\uD83D\\uDE00", "\\u0000"]
    chars = ["a", "b", " ", "é", "€", "한", "😀", "x" * 70, "{", "]", ":", ","]
    parts = []
    for _ in range(20000):
        n = rng.choice([0, 1, 2, 5, 20, 63, 64, 65, 200])
        parts.append('"' + "".join(rng.choice(esc) if rng.random() < 0.2 else rng.choice(chars) for _ in range(n)) + '"')
    doc = ("[" + (",\n " .join(parts)) + "]").encode()
    _check(ctx, doc)
    _check(ctx, b'{"k" : "v" , "a":"b"   }')
    _check(ctx, b'"root string \\n"')
    _check(ctx, b'"root"   ')
    _check(ctx, b"[1,2,3]")
    _check(ctx, b"")


@pytest.mark.parametrize("case", [c for c in V.STRING_ERRORS if c[1] not in (V.MSG_TRAILING, V.MSG_UNCLOSED)],
                         ids=lambda c: repr(c[0]))
def test_reference_error_vectors(ctx, case):
    text, msg, cite = case
    doc = text.encode()
    _check(ctx, doc)
    idx, st = ctx.stage1(doc)
    _, fei, fec = ctx.unescape(len(doc) + 4 * idx.size + 64)
    assert fei is not None and O.error_message(fec).startswith(msg[:20]), cite


def test_first_error_is_the_lowest_position(ctx):
    good = '"ok\\n"'
    doc = ("[" + ",".join([good] * 500 + ['"\\uD800x"'] + [good] * 500 + ['"\\q"'] + [good] * 10) + "]").encode()
    _check(ctx, doc)
    for s in ['"\\uDC00"', '"\\uD800\\u0041"', '"\\u12G4"', '"\\x"']:
        _check(ctx, ("[" + ",".join([good] * 100 + [s] + [good] * 100) + "]").encode())


def test_window_boundaries_of_the_cooperative_path(ctx):
    """The string pass gives each lane a 64-byte block and each wave a granule of 64 blocks (4 KiB): every kind of escape,
    backslash runs, surrogate pairs and every error placed so that they straddle the block edges at 64 to 512 bytes; also
    closing quotes followed by long whitespace runs, long strings between structurals, and documents shorter than the
    16-byte halo in front of a block.  Granule edges are the business of tests/test_gpu_string_granules.py."""
    pieces = ["\\n", "\\\\", "\\\"", "\\u00e9", "\\u20AC", "\\uD83D\\uDE00", "\\\\\\\\\\\\", "\\/"]
    docs = []
    for boundary in (64, 128, 256, 512):
        for back in range(0, 13):
            for pc in pieces:
                s = "a" * (boundary - back) + pc + "tail"
                docs.append('"' + s + '"')
    good = "[" + ",\n".join(docs) + "]"
    _check(ctx, good.encode())
    # errors straddling a boundary: the first one (lowest structural) must win, with the reference's code
    for bad in ["\\uD83Dx", "\\uD83D\\u0041", "\\uDE00", "\\u12G4", "\\q", "\\uD83D\\uD83D", "\\u"]:
        for back in (0, 1, 2, 3, 5, 6, 7, 11):
            s = '"' + "b" * (64 - back) + bad + ' rest"'
            _check(ctx, ("[" + ",".join(['"ok\\t"'] * 3 + [s] + ['"\\q"']) + "]").encode())
    # whitespace runs after the closing quote (pretty-printed, deeper than the 16-byte tail window), long strings that
    # make a row of 64 structurals span more than the 2 KiB backslash map, tiny documents
    deep = '[\n' + ",\n".join('"v%d\\t"%s' % (i, " " * (i % 40)) for i in range(300)) + "\n" + " " * 37 + "]"
    _check(ctx, deep.encode())
    long_row = "[" + ",".join('"%s\\n%s"' % ("x" * (50 * (i % 9)), "y" * 300) for i in range(200)) + "]"
    _check(ctx, long_row.encode())
    for tiny in [b'""', b'"a"', b'"\\n"', b'["",""]', b'"\\u0041"', b' "x" ', b'"0123456789abc"', b'"0123456789abcd"',
                 b'"0123456789abcde"']:
        _check(ctx, tiny)


def test_packed_stream_of_short_escaped_strings(ctx):
    """Escaped strings of up to 256 bytes are unescaped together as one packed byte stream per 64 structurals
    (unescape_packed): token soups of every escape kind and of every length 1..300 (so that string boundaries, escapes,
    \\uXXXX and surrogate pairs fall on every position of the 64-byte windows of the STREAM, and long strings mix in),
    strings that end in backslash pairs in front of strings that begin with them, and every error of StringParser placed in
    one of many escaped strings of the same wave (the first by position wins, the strings in front of it are intact)."""
    rng = random.Random(4242)
    toks = ["a", "b", "Z", " ", "é", "€", "\\n", "\\t", "\\\\", "\\\"", "\\/", "\\b", "\\u0041", "\\u00e9", "\\u20AC", "\\uD83D\\uDE00",
            "\\\\\\\\", "\\\\\\\"", "\\u0000", "\\uFFFF", "\\uDBFF\\uDFFF"]

    def soup(n):
        out, size = [], 0
        while size < n:
            t = rng.choice(toks)
            out.append(t)
            size += len(t.encode())
        return "".join(out)
    for _ in range(12):
        parts = ['"%s"' % soup(rng.randint(1, rng.choice([8, 30, 70, 300]))) for _ in range(rng.randint(100, 700))]
        sep = rng.choice([",", ", ", ",\n  "])
        _check(ctx, ("[" + sep.join(parts) + "]").encode())
    # every length, escapes at both ends
    _check(ctx, ("[" + ",".join('"\\\\%s\\\\"' % ("x" * n) for n in range(0, 300)) + "]").encode())
    _check(ctx, ("[" + ",".join('"%s\\uD83D\\uDE00"' % ("y" * n) for n in range(0, 200)) + "]").encode())
    _check(ctx, ('{' + ",".join('"k\\\\":"\\\\v%d\\\\\\\\"' % i for i in range(500)) + "}").encode())
    # errors: one failing string among escaped neighbours, at every lane phase; two failing strings -> the first
    bads = ["\\uD83Dx", "\\uD83D\\u0041", "\\uDE00", "\\u12G4", "\\q", "\\uD83D\\uD83D", "\\u", "\\uD83D", "\\u00"]
    for k, bad in enumerate(bads):
        for where in (0, 1, 5, 17, 62, 63, 64, 65, 130):
            parts = ['"n%d\\n"' % i for i in range(where)] + ['"%s%s%s"' % ("p" * (k + where % 7), bad, "s" * (where % 5))]
            parts += ['"t%d\\t"' % i for i in range(70)] + ['"\\q"'] + ['"u\\n"'] * 10
            _check(ctx, ("[" + ",".join(parts) + "]").encode())
