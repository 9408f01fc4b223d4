"""CPU-only: tests/all_tickets_shapes.py against its own claims and against oracle.stage1 -- every case has the granule count it
names, the list straddles every grid threshold of the ticketed-first-granule form under the full and the small grid, every
boundary it says it planted a hazard on holds one, and the oracle answers each text as the module says it must (0, or
SJMI_ST_UNCLOSED alone for a text that ends inside a string)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import all_tickets_shapes as A

FULL = 1 << 20  # (a resident count no case reaches: the grid is what the launch wants)


def test_lengths_have_the_granule_count_they_name():
    for steps in A.STEPS:
        G = 4096 * steps
        cases = A.cases(steps)
        assert [c.n for c in cases] == [n for n in A.COUNTS for _ in A.KINDS]
        for c in cases:
            assert A.granules_for(c.length, steps) == c.n, c.name
            assert A.granules_for(c.n * G, steps) == c.n + 1, c.name                    # one byte more than "top"
            if c.n > 1:
                assert A.granules_for((c.n - 1) * G - 1, steps) == c.n - 1, c.name      # one byte less than "bottom"
            if c.kind == "ragged":
                assert (c.n - 1) * G < c.length < c.n * G - 1, c.name
        assert sum(c.open for c in cases) >= len(cases) // 2 - 2
        assert {c.kind for c in cases if c.open} == set(A.KINDS)


def test_big_case_has_its_granule_count(twitter):
    d, length, copies = A.big_case(twitter)
    assert A.granules_for(length, 1) == A.BIG_COUNT and A.granules_for(length + 1, 1) == A.BIG_COUNT + 1
    assert d.size == length + 128 and copies * len(twitter) <= length < (copies + 1) * len(twitter)
    assert A.BIG_COUNT >= 2 * 256 * 4 * 8  # (twice the waves 256 CUs hold at the hardware's limit of 8 per SIMD; the kernel's LDS allows fewer)
    idx0, st0 = O.stage1(twitter)
    assert st0 == 0
    # the closed form on three copies against the oracle on three copies
    want, st = O.stage1(twitter * 3)
    assert st == 0 and np.array_equal(A.big_expected(idx0, len(twitter), 3), want)
    assert bytes(d[copies * len(twitter):]) == b" " * (d.size - copies * len(twitter))


def test_counts_straddle_the_grid_thresholds():
    counts = set(A.COUNTS) | {A.BIG_COUNT}
    # the full grid: one workgroup of workers with fewer granules than waves, exactly as many, one more
    assert {n for n in counts if A.workers_for(n, FULL) == 4} == {1, 2, 3, 4} and A.workers_for(5, FULL) == 8
    # the ticket classes: NC = min(workers, 8); fewer granules than classes, as many, one more
    assert {min(A.workers_for(n, FULL), A.TICKET_CLASSES) for n in counts} == {4, 8}
    assert {7, 8, 9} <= counts and A.workers_for(7, FULL) == 8
    # the retire rule: gridDim.x on both sides of 64
    grids = {A.grid_for(n, FULL) for n in counts}
    assert {A.RETIRE_GRID - 1, A.RETIRE_GRID, A.RETIRE_GRID + 1} <= grids
    assert [A.grid_for(n, FULL) for n in (248, 249, 252, 253)] == [63, 64, 64, 65]
    # the scanner: windows of 256 granules, rounds of 1024
    assert {255, 256, 257, 1024, 1025} <= counts
    # the small grid (debug flag 32): below its 9 workgroups, at them, and granules against its 32 workers and twice that
    small = {n: A.grid_for(n, A.SMALL_GRID) for n in counts}
    assert {g for g in small.values() if g < A.SMALL_GRID} >= {2, 3, 4} and small[31] == small[32] == small[33] == A.SMALL_GRID
    assert min(n for n, g in small.items() if g == A.SMALL_GRID) == 31 and small[9] < A.SMALL_GRID
    w = A.workers_for(33, A.SMALL_GRID)
    assert w == 32 and {w - 1, w, w + 1, 2 * w - 1, 2 * w, 2 * w + 1} <= counts
    assert A.BIG_COUNT > 2 * w and A.workers_for(A.BIG_COUNT, A.SMALL_GRID) == w


@pytest.mark.parametrize("steps", A.STEPS)
def test_oracle_answers_as_the_module_says(steps):
    G = 4096 * steps
    seen = set()
    for c in A.cases(steps):
        d = A.text_of(c)
        assert d.size == c.length + 128 and bytes(d[c.length:]) == b" " * 128, c.name
        assert A.ends_inside_string(d[:c.length]) == c.open, c.name
        assert not c.open or d[0] == 0x22, c.name
        idx, st = O.stage1(d, c.length)
        assert st == c.want_status == (A.ST_UNCLOSED if c.open else 0), (c.name, st)
        assert idx.size > c.length // 64 or c.length < 64, c.name  # (dense text, not blanks)
        bounds = A.boundaries_with_hazards(c)
        assert len(bounds) == max(0, c.n - 1 - (1 if c.length - (c.n - 1) * G <= 8 else 0)), c.name
        for b in bounds[:8] + bounds[-8:]:
            h = (b // G) % len(A.HAZARDS)
            hz, front = A.HAZARDS[h], A._FRONT[h]
            assert bytes(d[b - front:b - front + len(hz)]) == hz and 0 < front < len(hz), (c.name, b)
            seen.add(h)
    assert seen == set(range(len(A.HAZARDS)))
