"""The per-block tape-word counts (SjBlockMasks::words of sj_block.h / sj_block32.h -- the blkw array of k_stage1_batch, which
k_doc_prepare sums into every document's tape slot) against an independent count from the oracle, on the CPU.

tests/host_sim/words_sim.cpp walks a buffer block by block with the real carries and the kernels' tail masking and returns `words`
from both forms of the block algebra.  The reference is tests/batch_layouts.oracle_block_words: per block, 1 for every structural of
oracle.stage1 whose byte is not ',' or ':', 1 more if it is '-' or a digit.  The count for the polarity in which the buffer itself
enters a block comes from oracle.stage1 of the buffer; the count for the other polarity from oracle.stage1 of the same bytes behind a
block of one quote and 63 blanks, which flips the string parity of every block and leaves the scalar and escape carries as they
are.  So both bytes of `words` are compared on every block of every input.

`words` has no precondition as a count of bytes: "number" means "a structural that begins with '-' or a digit" in the header and in
the reference alike.  (That such a primitive IS a number holds for well-formed documents only; this test does not need it.)"""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from tests import batch_layouts as BL
from tests.conftest import ROOT, load_fixture

SIM_DIR = os.path.join(ROOT, "tests", "host_sim")


def build_words_sim(src_dir=SIM_DIR):
    """libwords_sim.so from words_sim.cpp in src_dir and the two headers it includes by their path relative to itself
    (../../simdjson-java_amd/csrc): a copy of the tree with a changed header builds the same way"""
    so = os.path.join(src_dir, "libwords_sim.so")
    src = os.path.join(src_dir, "words_sim.cpp")
    csrc = os.path.normpath(os.path.join(src_dir, "..", "..", "simdjson-java_amd", "csrc"))
    deps = [src, os.path.join(csrc, "sj_block.h"), os.path.join(csrc, "sj_block32.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.sim_words.restype = C.c_int
    lib.sim_words.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return lib


def sim_words(lib, data):
    """-> words[nblocks, 2]: column 0 from sj_block, column 1 from sj_block32"""
    a = np.frombuffer(bytes(data) + b"\0" * 64, dtype=np.uint8)
    out = np.zeros((len(data) // 64 + 1, 2), dtype=np.uint32)
    assert lib.sim_words(a.ctypes.data, len(data), out.ctypes.data) == 0
    return out


class Tally:
    def __init__(self):
        self.blocks = self.entered_inside = self.differ = 0


def check_words(lib, data, tally=None, what=""):
    outside, inside, entered = BL.oracle_block_words(data)
    got = sim_words(lib, data)
    for col, form in ((0, "sj_block"), (1, "sj_block32")):
        for name, want, have in (("outside", outside, got[:, col] & 0xFF), ("inside", inside, (got[:, col] >> 8) & 0xFF)):
            if not np.array_equal(want, have):
                b = int(np.nonzero(want != have)[0][0])
                raise AssertionError("%s %s block %d entered %s a string (the buffer enters it %s): got %d words, the oracle %d; bytes %r" % (
                    what, form, b, name, "inside" if entered[b] else "outside", int(have[b]), int(want[b]), bytes(data[b * 64:b * 64 + 64])))
        assert not (got[:, col] >> 16).any()
    if tally is not None:
        tally.blocks += entered.size
        tally.entered_inside += int(entered.sum())
        tally.differ += int((outside != inside).sum())


def inputs():
    """the generators of tests/test_host_sim.py (JSON-like, quote / backslash, backslash runs, random bytes), the four fixture files,
    every layout of tests/batch_layouts.py"""
    rng = random.Random(5)
    alphabet = b'\\\\\\"""{}[]:, \t\n\r\x0c\x1a\x01abc019.-e'
    for it in range(4000):
        n = rng.choice([0, 1, 63, 64, 65, 127, 128, 129, rng.randint(0, 700)])
        mode = it % 4
        if mode == 0:
            d = bytes(rng.choice(alphabet) for _ in range(n))
        elif mode == 1:
            d = bytes(rng.choice(b'\\"a ') for _ in range(n))
        elif mode == 2:
            d = b"a" * rng.randint(0, 70) + b"\\" * rng.randint(1, 300) + rng.choice([b'"', b"x", b""]) + b'"x' * rng.randint(0, 40)
        else:
            d = bytes(rng.getrandbits(8) for _ in range(n))
        yield "fuzz %d" % it, d
    # (numbers and atoms behind every kind of byte, so that the number class meets structurals and non-structurals alike)
    words = [b"-", b"0", b"12", b"9", b"-3", b"true", b"n", b",", b":", b"[", b"]", b"{", b"}", b'"', b'\\"', b" ", b"\n", b"a", b"\x0c", b"\x1a"]
    for it in range(1500):
        yield "tokens %d" % it, b"".join(rng.choice(words) for _ in range(rng.randint(0, 200)))
    for name in ("twitter.json", "github_events.json", "wide_bench.json", "malformed.txt"):
        yield name, load_fixture(name)
    for fam in BL.FAMILIES:
        for layout in BL.family(fam):
            yield "layout " + layout.name, layout.render()[0]


@pytest.fixture(scope="module")
def lib():
    return build_words_sim()


def test_block_words_equal_the_oracles_count_in_both_polarities(lib):
    """Both forms, both polarities, every block.  The blocks that the inputs themselves enter inside a string (the polarity that is
    then counted on the unchanged buffer) are at least a third of all, and every block is compared in both polarities -- more than
    the third the conditions ask for; on at least a tenth of the blocks the two counts differ, so swapping them cannot pass."""
    t = Tally()
    for what, d in inputs():
        check_words(lib, d, t, what)
    print("\nblocks %d, entered inside a string by their own buffer %d, with different counts for the two polarities %d" % (
        t.blocks, t.entered_inside, t.differ))
    assert t.entered_inside * 3 >= t.blocks, (t.entered_inside, t.blocks)
    assert t.differ * 10 >= t.blocks, (t.differ, t.blocks)
