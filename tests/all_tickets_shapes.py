"""Inputs for the stage-1 kernel's third assignment form (FLAG_ALL_TICKETS, debug flag 0x800: FAST mode with the scanner workgroup,
every granule by ticket, a wave's first one included), chosen by GRANULE COUNT: what can go wrong there depends on how many
granules stand against how many waves, ticket classes and scanner windows -- not on the bytes.  Pure Python (numpy), no GPU, no
oracle: tests/test_all_tickets_shapes.py holds this module against oracle.stage1, tests/test_gpu_all_tickets.py and
tests/test_gpu_context_threads.py run its cases on the device.

The launch geometry is restated from csrc/stage1.hip (granules_for, launch_mode, k_stage1):
    nblocks = len // 64 + 1                     one tail block, always
    ngran   = ceil(nblocks / (64 * steps))      a granule = steps * 4 KiB
    want    = ceil(ngran / 4) + 1               four worker waves per workgroup + the scanner workgroup
    grid    = min(want, resident)               resident = 9 under debug flag 32
    workers = (grid - 1) * 4,  NC = min(workers, 8) ticket classes,  retire rule on for grid >= 64
so with G = 4096 * steps every length in [(n - 1) * G, n * G - 1] has n granules and n * G has n + 1.

A case is (n, steps, kind): kind "top" = n * G - 1 bytes, "bottom" = (n - 1) * G, "ragged" = one length in between.  Its text is a
window of one seeded run of the _json_like generator of tests/test_gpu_stage1.py (newlines blanked, so that a text entered inside a
string holds no unescaped character), with a hazard on every granule boundary -- an escaped quote, two quotes, three backslashes and
a quote, a 3-byte and a 4-byte character straddling it, in turn -- and every other case begins with an open string, so that odd
parity runs down the whole chain of granules.  The module itself says what stage 1 must answer: status 0 for a text that ends
outside a string, SJMI_ST_UNCLOSED alone for one that ends inside (a case is made to end where its kind says by dropping its last
real quote if need be)."""
import random

import numpy as np

from tests.test_gpu_stage1 import _json_like

STEPS = (1, 2, 4)
TICKET_CLASSES = 8
SMALL_GRID = 9          # workgroups of a FAST launch under debug flag 32: 8 of workers (32 waves) + the scanner's
RETIRE_GRID = 64        # gridDim.x from which the workers on the scanner's CU retire
ST_UNCLOSED = 2
FLAG_ALL_TICKETS, FLAG_SMALL_GRID = 0x800, 32

# granule counts and why:
COUNTS = (1, 2, 3, 4, 5,            # one workgroup of workers; fewer granules than waves
          7, 8, 9,                  # around TICKET_CLASSES
          31, 32, 33, 63, 64, 65,   # around the 32 workers of the small grid, and twice that
          248, 249, 252, 253,       # gridDim.x 63, 64, 64, 65: the retire rule switches on
          255, 256, 257, 1024, 1025)  # the scanner's windows of 256 granules and its round of 1024
BIG_COUNT = 16384                   # beyond twice any resident worker count; steps = 1 (64 MiB): big_case()
KINDS = ("top", "bottom", "ragged")
HAZARDS = (b'\\"', b'""', b'\\\\\\"', "€".encode(), "\U0001F600".encode())
# (bytes of the hazard in front of the boundary)
_FRONT = (1, 1, 3, 1, 2)


def granules_for(length, steps):
    return (length // 64 + 1 + 64 * steps - 1) // (64 * steps)


def grid_for(ngran, resident):
    return min((ngran + 3) // 4 + 1, resident)


def workers_for(ngran, resident):
    return (grid_for(ngran, resident) - 1) * 4


def length_of(n, steps, kind):
    G = 4096 * steps
    if kind == "top":
        return n * G - 1
    if kind == "bottom":
        return (n - 1) * G
    return (n - 1) * G + 1 + random.Random(1000 * n + steps).randrange(G - 2)


class Case:
    __slots__ = ("n", "steps", "kind", "length", "open", "offset")

    def __init__(self, n, steps, kind, length, open_, offset):
        self.n, self.steps, self.kind, self.length, self.open, self.offset = n, steps, kind, length, open_, offset

    @property
    def name(self):
        return "n%d-s%d-%s%s" % (self.n, self.steps, self.kind, "-open" if self.open else "")

    @property
    def want_status(self):
        return ST_UNCLOSED if self.open else 0


_BASE_GRANULES = 1025 + 3
_base = None


def _base_text():
    """one run of the generator, long enough for the largest case at any window offset; no newlines"""
    global _base
    if _base is None:
        text = _json_like(random.Random(20800), _BASE_GRANULES * 4096 * 4).replace(b"\n", b" ")
        _base = np.frombuffer(text, dtype=np.uint8)
    return _base


def cases(steps):
    """the cases of one granule size, in a fixed order; every other one is entered inside a string"""
    out = []
    rng = random.Random(77 + steps)
    for n in COUNTS:
        for kind in KINDS:
            length = length_of(n, steps, kind)
            open_ = len(out) % 2 == 1 and length >= 2
            out.append(Case(n, steps, kind, length, open_, rng.randrange(3 * 4096 * 4 - 64)))
    return out


def _is_continuation(b):
    return 0x80 <= b < 0xC0


def _unescaped_quotes(a):
    """positions of the quotes of `a` that no odd run of backslashes stands in front of"""
    q = np.flatnonzero(a == 0x22)
    run = np.zeros(q.size, dtype=np.int64)
    live = np.ones(q.size, dtype=bool)
    k = 1
    while True:
        p = q - k
        live &= p >= 0
        live[live] = a[p[live]] == 0x5C
        if not live.any():
            break
        run[live] += 1
        k += 1
    return q[run % 2 == 0]


def ends_inside_string(a):
    return _unescaped_quotes(np.asarray(a)).size % 2 == 1


def text_of(case):
    """-> np.uint8 [length + 128]: the case's bytes and 128 blanks behind them (readable padding for the device forms)"""
    n, G, L = case.n, 4096 * case.steps, case.length
    base = _base_text()
    off = case.offset
    while _is_continuation(int(base[off])):
        off += 1
    d = np.full(L + 128, 0x20, dtype=np.uint8)
    d[:L] = base[off:off + L]
    # (a character cut by the window's end)
    if L:
        k = L - 1
        while k > 0 and _is_continuation(int(d[k])):
            k -= 1
        if d[k] >= 0xC0 and L - k < (2 if d[k] < 0xE0 else 3 if d[k] < 0xF0 else 4):
            d[k:L] = ord("a")
    if case.open:
        lo = 1
        while lo < L and _is_continuation(int(d[lo])):
            lo += 1
        d[0:lo] = ord("a")
        d[0] = 0x22
    for b in range(G, L - 8, G):  # every granule boundary with room on both sides
        h = (b // G) % len(HAZARDS)
        hz, front = HAZARDS[h], _FRONT[h]
        lo, hi = b - front, b - front + len(hz)
        wlo, whi = lo, hi
        while _is_continuation(int(d[wlo])):
            wlo -= 1
        while _is_continuation(int(d[whi])):
            whi += 1
        d[wlo:whi] = ord("a")
        d[lo:hi] = np.frombuffer(hz, dtype=np.uint8)
    uq = _unescaped_quotes(d[:L])
    if (uq.size % 2 == 1) != case.open:
        # the last real quote goes (never the opening one of an open case: that case then has an even number, two at least)
        d[uq[-1]] = ord("a")
    return d


def boundaries_with_hazards(case):
    G = 4096 * case.steps
    return list(range(G, case.length - 8, G))


def big_case(twitter):
    """BIG_COUNT granules of 4 KiB: twitter.json back to back and blanks up to one byte short of the granule edge.  Its expected
    indexes have a closed form (copy k's are copy 0's + k * len(twitter)), so no reference run over 64 MiB is needed.
    -> (np.uint8 [length + 128], length, copies)"""
    length = BIG_COUNT * 4096 - 1
    copies = length // len(twitter)
    d = np.full(length + 128, 0x20, dtype=np.uint8)
    one = np.frombuffer(twitter, dtype=np.uint8)
    d[:copies * one.size] = np.tile(one, copies)
    return d, length, copies


def big_expected(idx0, n0, copies):
    """the closed form: np.uint32 indexes of `copies` copies of a document of n0 bytes whose own indexes are idx0"""
    return (idx0.astype(np.int64)[None, :] + (np.arange(copies, dtype=np.int64) * n0)[:, None]).reshape(-1).astype(np.uint32)
