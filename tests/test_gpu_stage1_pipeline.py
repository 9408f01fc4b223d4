"""The worker pipeline of the stage-1 kernel -- the ticket of the next granule and the prefix in front of the parked one are
requested ahead of their use, the next granule's first step is loaded while the current one is still classified -- at every
granule size, in both assignment modes, on the full grid and on the small one (debug flag 32: 32 worker waves, so that an input
of 33 granules reaches the ticket path and one of 130 makes every wave iterate four or more times).  Indexes and status,
bit-exact against oracle.stage1.

The inputs are seeded JSON-like text whose features sit ON the edges the pipeline hands values across:
  * every granule edge carries a feature, every other one inside a long string: consecutive granules are entered with different
    in-string parity, so a stale or wrong prefix moves or drops indexes;
  * backslash runs of 1 to 9, ending at the edge and split by it, and two-, three- and four-byte UTF-8 sequences split at every
    byte, at 64-byte block edges, 4 KiB step edges and granule edges (granules of one step: a step edge IS a granule edge);
  * the same sequences TRUNCATED at the three edges, one per input, so that a missed carry clears the status bit;
  * lengths of 1, 2, 3, 33 and 130 granules exactly (the last granule is then the tail block alone) and -1, +1, +63, +64, +65
    bytes from there.
The largest input is 130 granules of 16 KiB + 65 bytes (2.03 MiB)."""
import random

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 4)
SIZES = (1, 2, 3, 33, 130)       # granules
DELTAS = (0, -1, 1, 63, 64, 65)  # bytes from the granule edge
NG = SIZES[-1]
BROKEN_NG = 34                   # the truncated sequences sit at the edges of granule 33, the first one taken by ticket on the small grid
BROKEN_G = 33

_PARTS = ['"name"', '"va\\"lue"', '"x\\\\"', '"é€한😀"', "12345", "-1.5e10", "true", "false", "null", '"\\u00e9\\ud83d\\ude00"',
          '"' + "abc def " * 9 + '"', '""', "{", "}", "[", "]", ":", ",", " ", "\n", '{"k":[1,2,{"z":null}]}', '"\\\\\\\\"']


def _pool(rng):
    """String-complete chunks of JSON-like text: the filler between the features, which alone decide the parity at an edge."""
    chunks = []
    for _ in range(48):
        parts = [rng.choice(_PARTS) for _ in range(rng.randint(20, 90))]
        if rng.random() < 0.5:
            parts.append('"' + "".join(rng.choice("abcdefghij klmnop") for _ in range(rng.randint(0, 200))) + '"')
        chunks.append("".join(parts).encode())
    return chunks


def _cores():
    """(bytes, bytes in front of the edge): what straddles an edge."""
    cores = []
    for r in range(1, 10):
        tail = b'"' if r % 2 else b"x"  # (an odd run escapes the quote: the string goes on)
        cores.append((b"\\" * r + tail, r))  # the run ends at the edge, what it escapes lies behind it
        if r >= 2:
            cores.append((b"\\" * r + tail, r // 2))  # the edge splits the run
    for seq in ("é", "€", "😀"):
        b = seq.encode()
        for k in range(1, len(b)):
            cores.append((b, k))
    cores.append((b"xy", 1))
    cores.append((b"[]", 1))
    assert len(cores) % 2 == 1 and len(cores) % 3 != 0  # every core meets both wrappings and every step edge
    return cores


_TRUNCATED = [(b"\xc3a", 1), (b"\xe2\x82a", 1), (b"\xe2\x82a", 2), (b"\xf0\x9f\x98a", 1), (b"\xf0\x9f\x98a", 2), (b"\xf0\x9f\x98a", 3)]


def _feature(edge, core, k, wrapped):
    pre, post = (b'"' + b"w" * 39, b"w" * 20 + b'",') if wrapped else (b'"ab', b'",')
    return edge - k - len(pre), pre + core + post


def _edges(steps, g):
    """The three edges of granule g that carry a feature: its granule edge, one of its step edges, one of its block edges."""
    G = 4096 * steps
    step = g * G + 4096 * (1 + g % (steps - 1)) if steps > 1 else None
    return g * G, step, g * G + 64 * (2 + (7 * g) % 60)


def _text(steps, granules, pool, override=None):
    """granules * steps * 4 KiB (+ 128) bytes; override = {edge: (core, k)} in place of that edge's own feature."""
    rng = random.Random(7 + steps)
    cores = _cores()
    feats = []
    for g in range(0, granules):
        ge, se, be = _edges(steps, g)
        for n, e in enumerate((ge, se, be)):
            if e is None or e == 0:
                continue
            core, k = cores[(g + 9 * n) % len(cores)]
            if override and e in override:
                core, k = override[e]
            feats.append(_feature(e, core, k, wrapped=(g + n) % 2 == 1))  # (granule edges: every odd one lies inside a string)
    feats.sort()
    total = granules * 4096 * steps + 128
    out = bytearray()
    longest = max(len(c) for c in pool)
    for start, fb in feats + [(total, b"")]:
        assert start >= len(out), "features overlap"
        while len(out) + longest <= start:
            out += rng.choice(pool)
        out += b" " * (start - len(out))
        out += fb
    return np.frombuffer(bytes(out[:total]), dtype=np.uint8)


_cache = {}


def _inputs(steps):
    """[(name, text, length, reference indexes, reference status)], made once per granule size and shared by every setting."""
    if steps in _cache:
        return _cache[steps]
    G = 4096 * steps
    pool = _pool(random.Random(1))
    cases = []
    text = _text(steps, NG, pool)
    for size in SIZES:
        for delta in DELTAS:
            n = size * G + delta
            cases.append(("%dg%+d" % (size, delta), text, n) + O.stage1(text, n))
    # the whole text has no UTF-8 error: the sequences split at the edges are valid
    assert cases[-1][4] & O.ST_UTF8 == 0
    ge, se, be = _edges(steps, BROKEN_G)
    for what, e in (("granule", ge), ("step", se), ("block", be)):
        if e is None:
            continue
        for core, k in _TRUNCATED:
            t = _text(steps, BROKEN_NG, pool, {e: (core, k)})
            n = BROKEN_NG * G + 100
            want_idx, want_st = O.stage1(t, n)
            assert want_st & O.ST_UTF8, "the truncated sequence is this input's only UTF-8 error"
            cases.append(("trunc-%s-%d/%d" % (what, k, len(core) - 1), t, n, want_idx, want_st))
    _cache[steps] = cases
    return cases


@pytest.fixture(scope="module", params=[(m, f) for m in ("fast", "ticket") for f in (0, 32)], ids=lambda p: "%s-flags%d" % p)
def ctx(request):
    import simdjson_java_amd as S
    mode, flags = request.param
    c = S.Context(device=0, capacity=NG * 4096 * 4 + 4096)
    c.set_tile_mode(mode == "ticket")
    c.debug_set_flags(flags)
    yield c
    c.close()


@pytest.mark.parametrize("steps", STEPS)
def test_pipeline_edges(ctx, steps):
    ctx.set_tile_steps(steps)
    try:
        for name, text, n, want_idx, want_st in _inputs(steps):
            got_idx, got_st = ctx.stage1(text, n)
            assert got_st == want_st, (name, got_st, want_st)
            assert got_idx.size == want_idx.size, (name, got_idx.size, want_idx.size)
            if not np.array_equal(got_idx, want_idx):
                bad = int(np.nonzero(got_idx != want_idx)[0][0])
                raise AssertionError("%s: first index mismatch at %d: got %d want %d" % (name, bad, got_idx[bad], want_idx[bad]))
    finally:
        ctx.set_tile_steps(0)


def test_inputs_cover_the_edges():
    """The generator itself (no GPU work): every odd granule edge lies inside a string, every even one outside, so consecutive
    granules are entered with different parity."""
    for steps in STEPS:
        G = 4096 * steps
        text = _inputs(steps)[0][1]
        b = bytes(text)
        for g in range(1, NG):
            inside = b[g * G - 30:g * G - 10] == b"w" * 20  # the wrapping string's padding
            assert inside == (g % 2 == 1), (steps, g)
