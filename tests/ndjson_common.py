"""What the NDJSON splitter (include/sjmi.h, sjmi_ndjson_offsets*) must give: the reference, the seeded fuzz inputs and the edge
cases, shared by the host simulation's tests (tests/test_host_ndjson.py) and the GPU's (tests/test_gpu_ndjson.py)."""
import numpy as np

TAIL_BLANK, OVERFLOW = 1, 2
ALPHABET = b'\n \t\ra"{'
CANARY = 0xC0FFEE0DDBA11AD5
PAD_FILL = b"\na"  # what the bytes around a buffer are filled with: any influence of the padding shows


def ndjson_reference(buf):            # -> (offsets, consumed, tail_blank)
    consumed = buf.rfind(b"\n") + 1
    starts, p = [], 0
    while p < consumed:
        e = buf.index(b"\n", p) + 1
        if buf[p:e].strip(b" \t\r\n"): starts.append(p)
        p = e
    if starts: starts[0] = 0
    return (starts + [consumed] if starts else [0]), consumed, not buf[consumed:].strip(b" \t\r")


def fuzz_input(rng, tile, length=None):
    """one input over ALPHABET: NL density 1/2 .. 1/4000, BLANK density 0 .. 0.99 of the other bytes, length 0 .. 3 tiles + 65"""
    n = int(rng.integers(0, 3 * tile + 66)) if length is None else length
    nl = 1.0 / float(np.exp(rng.uniform(np.log(2.0), np.log(4000.0))))
    blank = float(rng.choice([0.0, 0.5, 0.9, 0.99, rng.uniform(0.0, 0.99)]))
    r = rng.random(n)
    out = np.empty(n, dtype=np.uint8)
    is_nl = r < nl
    is_blank = ~is_nl & (rng.random(n) < blank)
    out[is_nl] = 10
    out[is_blank] = rng.choice(np.frombuffer(b" \t\r", dtype=np.uint8), int(is_blank.sum()))
    rest = ~is_nl & ~is_blank
    out[rest] = rng.choice(np.frombuffer(b'a"{', dtype=np.uint8), int(rest.sum()))
    return out.tobytes()


def fuzz_inputs(count, tile, seed):
    """`count` inputs from one seed; the first lengths are the small ones every split has to get right"""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 2, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 65]
    return [fuzz_input(rng, tile, fixed[i] if i < len(fixed) else None) for i in range(count)]


def edge_cases(T):
    """(name, bytes) for a tile of T bytes (placed for a buffer that begins on a tile edge)"""
    line = b'{"a":1}\n'
    cases = []
    for n in (0, 1, 63, 64, 65, T - 1, T, T + 1):
        body = (line * (n // len(line) + 1))[:n]
        cases.append(("len %d of lines" % n, body))
        cases.append(("len %d ending in NL" % n, body[:-1] + b"\n" if n else body))
    cases.append(("one NL", b"\n"))
    cases.append(("one byte of content", b"a"))
    cases.append(("no NL at all", b'{"a": 1}  ' * 40))
    cases.append(("no NL, all blank", b" \t\r" * 50))
    cases.append(("all lines blank", b"\n \n\t\r\n\r\n\n   \n" * 30))
    cases.append(("all lines blank, content in the tail", b"\n \n\r\n" * 30 + b"  x "))
    cases.append(("leading blank lines", b"\n\r\n  \n" + line * 3))
    cases.append(("form feed, vertical tab, NUL and a BOM are content", b"\f\n\v\n\0\n\xef\xbb\xbf\n \n"))
    a = bytearray(b"a" * (2 * T))
    a[T - 1] = 10
    cases.append(("NL as the last byte of a tile", bytes(a) + b"\n"))
    a = bytearray(b"a" * (2 * T))
    a[T] = 10
    cases.append(("NL as the first byte of a tile", bytes(a) + b"\n"))
    for at in (63, 64):
        a = bytearray(b" " * 200)
        a[at] = 10
        a[at + 1] = ord("x")
        a[190] = 10
        cases.append(("NL at byte %d of a block" % at, bytes(a)))
        a = bytearray(b"x" * 200)
        a[at] = 10
        cases.append(("NL at byte %d between content" % at, bytes(a) + b"\n"))
    a = bytearray((line * (T // len(line) + 1))[:T - 1] + b"\r\n" + line * 2)
    cases.append(("CR LF split across a tile edge", bytes(a)))
    a = bytearray(b" " * (T - 1) + b"\r\n" + b"\r\n" + line)
    a[0:2] = b"x\n"
    cases.append(("a blank CR LF line across a tile edge", bytes(a)))
    cases.append(("a blank run over three tiles, then content on the same line", line + b" " * (3 * T + 9) + b"x\n" + line))
    cases.append(("a blank run over three tiles from the start, then content", b"\t" * (3 * T) + b"x\ny\n"))
    cases.append(("a line of 3T + 5 with content in its first tile only", b"\n" + b"x" + b" " * (3 * T + 3) + b"\n" + line))
    cases.append(("a line of 3T + 5 with content in its last tile only", b"\n" + b" " * (3 * T + 3) + b"x" + b"\n" + line))
    cases.append(("a line of 3T + 5, all blank, between documents", line + b" " * (3 * T + 4) + b"\n" + line))
    cases.append(("the densest output", (b"1\n" * (T + 2))[:2 * T + 3]))
    cases.append(("the densest output, CR LF", (b"1\r\n" * T)[:2 * T + 3]))
    cases.append(("an unterminated tail over two tiles", line * 3 + b"y" * (2 * T)))
    cases.append(("a blank tail over two tiles", line * 3 + b" " * (2 * T)))
    return cases


def sparse_input(n_tiles, T, extra=37):
    """n_tiles tiles and a bit: short lines at the tile edges and a dense patch, long runs between them (cheap for the reference)"""
    a = np.full(n_tiles * T - T + extra, ord(" "), dtype=np.uint8)
    for t in range(0, n_tiles - 1):
        at = t * T
        if t % 3 == 0:
            a[at] = ord("x")
        if t % 5 != 4:
            a[at + T - 1 if t % 2 else at + 1] = 10
        if t % 7 == 3:
            a[at + T // 2:at + T // 2 + 6] = np.frombuffer(b"\n{}\r\n\n", dtype=np.uint8)
    a[-extra:-extra + 4] = np.frombuffer(b'1\n"a', dtype=np.uint8)
    return a.tobytes()


def expect(buf, capacity, ref=None):
    """-> (entries the call must have written, in order from 0; n_docs; consumed; flags); ref = ndjson_reference(buf) if at hand"""
    offs, consumed, tail_blank = ref or ndjson_reference(buf)
    n_docs = len(offs) - 1
    flags = (TAIL_BLANK if tail_blank else 0) | (OVERFLOW if capacity < n_docs + 1 else 0)
    return offs[:capacity], n_docs, consumed, flags


def check(what, buf, capacity, got_offsets, got_result, ref=None):
    """got_offsets: the capacity entries (canary-filled before the call) plus the canaries behind them"""
    want, n_docs, consumed, flags = expect(buf, capacity, ref)
    assert (int(got_result[0]), int(got_result[1]), int(got_result[2]) & 0xFFFFFFFF) == (n_docs, consumed, flags), \
        "%s: (n_docs, consumed, flags) = %s, want %s" % (what, [int(x) for x in got_result[:3]], (n_docs, consumed, flags))
    got = np.asarray(got_offsets, dtype=np.uint64)
    w = np.asarray(want, dtype=np.uint64)
    if not np.array_equal(got[:len(want)], w):
        bad = int(np.flatnonzero(got[:len(want)] != w)[0])
        raise AssertionError("%s: doc_offsets[%d] = %d, want %d (of %d)" % (what, bad, int(got[bad]), int(w[bad]), len(want)))
    assert (got[len(want):] == np.uint64(CANARY)).all(), "%s: an entry behind the %d valid ones was written" % (what, len(want))
    return n_docs
