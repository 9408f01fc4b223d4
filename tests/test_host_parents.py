"""CPU check of the parent columns' passes (simdjson-java_amd/csrc/sj_parents.h, which csrc/parents.hip compiles verbatim) against
the reference of tests/parents_common.py: tests/host_sim/parents_sim.cpp runs the dense and the sparse pass with a sequential
workgroup, chunks of 64, 128 and 1024 rows in three orders, every buffer ending at an unreadable page; a stand-alone program runs
them under ASan and UBSan.  All results are integers: every comparison is an equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import host_sim_lib
from tests import parents_common as PC
from tests.members_common import header_constant

CHUNKS = (64, 128, 1024)
ORDERS = (0, 1, 2)


def load_sim():
    """tests/host_sim/parents_sim.cpp (tests/host_sim_lib.py builds it) with its signatures"""
    lib = host_sim_lib.load("parents", ("sj_parents.h", "sj_fieldcol.h"))
    lib.sim_parent_columns.restype = C.c_int
    lib.sim_parent_columns.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sim_parent_chunk_rows.restype = lib.sim_parent_max_cols.restype = C.c_uint32
    for f in (lib.sim_parent_count_wave, lib.sim_parent_count_lane):
        f.restype, f.argtypes = C.c_uint64, [C.c_void_p, C.c_uint64, C.c_uint64]
    return lib


@pytest.fixture(scope="module")
def lib():
    lib = load_sim()
    assert lib.sim_parent_max_cols() == header_constant("SJMI_PARENT_MAX_COLS") == PC.MAX_COLS
    assert header_constant("SJMI_PARENT_RESULT_WORDS") == PC.RESULT_WORDS and lib.sim_parent_chunk_rows() == 1024
    return lib


def ptr(buf):
    return None if buf is None else buf[0].ctypes.data + buf[1] * buf[0].itemsize


def sim_call(lib, chunk=0, order=0, guard=1):
    def call(off, n_docs, rows, n_rows, rc, types, values, n_cols, col_stride, pt, p, ot, ov, out_stride, result):
        return lib.sim_parent_columns(ptr(off), n_docs, ptr(rows), n_rows, ptr(rc), ptr(types), ptr(values), n_cols, col_stride, ptr(pt), ptr(p),
                                      ptr(ot), ptr(ov), out_stride, ptr(result), chunk, order, guard)
    return call


def every_schedule(lib, offsets, n_rows, **kw):
    first = None
    for chunk in CHUNKS:
        for order in ORDERS:
            got = PC.check(sim_call(lib, chunk, order), offsets, n_rows, what=(kw.get("what"), chunk, order), **{k: v for k, v in kw.items() if k != "what"})
            first = got if first is None else first
            assert (got[0] == first[0]).all() and got[1] == first[1]
    return first


def test_both_searches_count_the_offsets_at_or_below_a_row(lib):
    rng = np.random.default_rng(3)
    for n_docs in (0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 70000):
        offsets = PC.offsets_of(PC.random_counts(n_docs, n_docs, empty=0.5))
        total = int(offsets[-1])
        xs = [0, 1, total - 1, total, total + 1, 1 << 40, (1 << 64) - 1] + [int(v) for v in rng.integers(0, total + 2, size=40)]
        xs += [int(v) for v in offsets[1:][:20]] + [int(v) - 1 for v in offsets[1:][:20] if v]
        for x in xs:
            if x < 0:
                continue
            want = int(np.searchsorted(offsets[1:], np.uint64(x), side="right"))
            assert lib.sim_parent_count_wave(offsets.ctypes.data, n_docs, x) == want, (n_docs, x)
            assert lib.sim_parent_count_lane(offsets.ctypes.data, n_docs, x) == want, (n_docs, x)


@pytest.mark.parametrize("live", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1])
def test_dense_rows_at_every_edge(lib, live):
    """the rows of an explode: exactly `live` rows over documents of which a third have none, with carried columns"""
    counts = PC.random_counts(max(live // 3, 1), live)
    counts[-1] += max(live - int(counts.sum()), 0)
    while int(counts.sum()) > live:
        counts[int(np.flatnonzero(counts)[0])] -= 1
    offsets = PC.offsets_of(counts)
    assert int(offsets[-1]) == live
    cols = PC.doc_columns(2, counts.size, counts.size + 3, live)
    every_schedule(lib, offsets, live, cols=cols, what=live)
    every_schedule(lib, offsets, live + 70, cols=cols, row_count=live, out_stride=live + 75, what=("row count", live))


def test_documents_without_rows_in_front_behind_and_between(lib):
    for counts in ([0, 0, 0, 5, 0, 0, 2, 0, 0, 0], [3] + [0] * 3000 + [4], [0] * 200 + [1] * 130 + [0] * 200, [0] * 3000 + [1], [1] + [0] * 3000):
        offsets = PC.offsets_of(counts)
        n = int(offsets[-1])
        cols = PC.doc_columns(1, len(counts), len(counts), 5)
        want, _ = every_schedule(lib, offsets, n, cols=cols, what=counts[:12])
        assert set(want.tolist()) == {k for k, c in enumerate(counts) if c}


def test_one_document_over_three_chunks_and_starts_at_the_edges(lib):
    """the middle chunk of a long document has no document start and takes its seed alone; documents that begin exactly at a
    wave edge (64) and at a chunk edge (1024, and the small chunks' 128)"""
    for counts in ([10, 3 * 1024 + 5, 7], [64, 64, 0, 896, 1024, 1, 1023], [128, 0, 128, 768, 2048], [1023, 1, 1, 1023]):
        offsets = PC.offsets_of(counts)
        every_schedule(lib, offsets, int(offsets[-1]), cols=PC.doc_columns(3, len(counts), len(counts) + 1, 9), what=counts)


def test_no_row_no_document_one_document(lib):
    cols1 = PC.doc_columns(2, 1, 4, 1)
    for counts, cols in (([0] * 40, PC.doc_columns(2, 40, 40, 2)), ([], cols1), ([0], cols1), ([5], cols1), ([1500], cols1)):
        offsets = PC.offsets_of(counts)
        for n_rows in (0, 1, 70, 1500, 1601):
            want, result = every_schedule(lib, offsets, n_rows, cols=cols, what=(counts[:3], n_rows))
            assert result[1] == max(0, n_rows - int(offsets[-1]))
            every_schedule(lib, offsets, n_rows, rows=np.arange(n_rows)[::-1].copy(), cols=cols, what=("sparse", counts[:3], n_rows))


def test_the_row_count_is_read_where_it_lies(lib):
    offsets = PC.offsets_of(PC.random_counts(500, 4))
    total = int(offsets[-1])
    cols = PC.doc_columns(2, 500, 500, 4)
    for row_count in (0, 1, 64, total - 1, total, total + 5, 1 << 50):
        for n_rows in (total, total + 40, total - 100):
            every_schedule(lib, offsets, n_rows, row_count=row_count, cols=cols, what=(row_count, n_rows))
            PC.check(sim_call(lib), offsets, n_rows, rows=np.arange(n_rows)[::-1].copy(), row_count=row_count, cols=cols)


def test_the_sparse_form(lib):
    offsets = PC.offsets_of(PC.random_counts(3000, 8))
    total = int(offsets[-1])
    cols = PC.doc_columns(3, 3000, 3001, 8)
    rng = np.random.default_rng(8)
    ascending = np.flatnonzero(rng.random(total) < 0.1)  # (a filter's selection vector)
    ranked = rng.permutation(total)[:2048]  # (a top k's rows: any order)
    duplicates = rng.integers(0, total, size=1500) // 7 * 7
    edges = np.array([0, total - 1, total, 1 << 40, total + 1, (1 << 64) - 1, 0, total - 1], dtype=np.uint64)
    for rows in (ascending, ranked, duplicates, edges):
        want, result = every_schedule(lib, offsets, rows.size, rows=rows.astype(np.uint64), cols=cols)
    with_rows = np.flatnonzero(np.diff(offsets))
    assert want.tolist() == [with_rows[0], with_rows[-1], -1, -1, -1, -1, with_rows[0], with_rows[-1]] and result[1] == 4


def test_each_output_is_optional_and_strides_may_be_wider(lib):
    offsets = PC.offsets_of(PC.random_counts(700, 6))
    total = int(offsets[-1])
    cols = PC.doc_columns(2, 700, 900, 6)
    for kw in (dict(cols=None), dict(cols=cols, with_parents=False, with_types=False), dict(cols=cols, with_parents=False),
               dict(cols=cols, with_types=False), dict(cols=cols, out_stride=total + 300), dict(cols=cols, shift=3), dict(cols=cols, shift=1)):
        every_schedule(lib, offsets, total + 9, **kw)
        PC.check(sim_call(lib), offsets, 300, rows=np.arange(300, dtype=np.uint64) * 3, **kw)


def test_64_carried_columns(lib):
    offsets = PC.offsets_of(PC.random_counts(300, 2))
    every_schedule(lib, offsets, int(offsets[-1]) + 3, cols=PC.doc_columns(64, 300, 301, 2))
    for n_cols in (1, 3, 4, 5, 63):
        PC.check(sim_call(lib, 128, 2), offsets, int(offsets[-1]), cols=PC.doc_columns(n_cols, 300, 300, n_cols))


def test_wild_offsets_end_and_touch_nothing_outside(lib):
    """offsets that are not monotone, or far above the rows: the parents mean nothing, but the run ends, the record is written,
    and with every buffer at an unreadable page nothing outside was read or written"""
    rng = np.random.default_rng(12)
    n_docs, n_rows = 5000, 6000
    for shape in range(4):
        offsets = rng.integers(0, n_rows * 2, size=n_docs + 1).astype(np.uint64)
        if shape == 1:
            offsets[::5] = np.uint64((1 << 64) - 1)
        elif shape == 2:
            offsets = np.sort(offsets)[::-1].copy()
        elif shape == 3:
            offsets[:] = 17
        types, values = PC.doc_columns(2, n_docs, n_docs, shape)
        for chunk in CHUNKS:
            for order in ORDERS:
                for rows in (None, rng.integers(0, n_rows * 3, size=n_rows).astype(np.uint64)):
                    p = np.full(n_rows + 2, PC.CANARY, dtype=np.uint64)
                    pt = np.full(n_rows + 2, PC.CANARY_BYTE, dtype=np.uint8)
                    ov = np.full(2 * n_rows + 2, PC.CANARY, dtype=np.uint64)
                    ot = np.full(2 * n_rows + 2, PC.CANARY_BYTE, dtype=np.uint8)
                    result = np.zeros(3, dtype=np.uint64)
                    got = lib.sim_parent_columns(offsets.ctypes.data, n_docs, None if rows is None else rows.ctypes.data, n_rows, None,
                                                 types.ctypes.data, values.ctypes.data, 2, n_docs, pt[1:].ctypes.data, p[1:].ctypes.data,
                                                 ot[1:].ctypes.data, ov[1:].ctypes.data, n_rows, result.ctypes.data, chunk, order, 1)
                    assert got == 0 and result[0] == n_rows and result[1] <= n_rows and result[2] == 0
                    assert p[0] == p[-1] == ov[0] == ov[-1] == PC.CANARY and pt[0] == pt[-1] == ot[0] == ot[-1] == PC.CANARY_BYTE
                    parents = p[1:-1].view(np.int64)
                    assert ((parents >= -1) & (parents < n_docs)).all()


def test_argument_errors(lib):
    ok = np.zeros(64, dtype=np.uint64)
    off, ty, va = np.array([0, 2, 4], dtype=np.uint64), np.zeros(16, dtype=np.uint8), np.zeros(9, dtype=np.uint64)
    p = lambda a, o=0: a.ctypes.data + o
    PT, PP, OT, OV, S = p(ok), p(ok, 64), p(ok, 128), p(ok, 256), p(ok, 448)

    def f(o=p(off), n_docs=2, rows=None, n=4, rc=None, t=p(ty), v=p(va), n_cols=1, cs=2, pt=PT, pp=PP, ot=OT, ov=OV, os_=4, res=S):
        return lib.sim_parent_columns(o, n_docs, rows, n, rc, t, v, n_cols, cs, pt, pp, ot, ov, os_, res, 0, 0, 0)

    assert f() == 0
    assert f(o=None) == -2 and f(res=None) == -2
    assert f(n_cols=65, cs=2, os_=4) == -2
    assert f(t=None) == -2 and f(v=None) == -2 and f(ot=None) == -2 and f(ov=None) == -2
    assert f(t=None, v=None, ot=None, ov=None, n_cols=0) == 0
    assert f(cs=1) == -2 and f(os_=3) == -2 and f(cs=1, os_=3, n_cols=0, t=None, v=None, ot=None, ov=None) == 0
    assert f(n=1 << 32, os_=1 << 32) == -2 and f(n_docs=1 << 32, cs=1 << 32) == -2
    assert f(pt=None) == 0 and f(pp=None) == 0 and f(pt=None, pp=None) == 0
    assert f(t=p(ty, 3), pt=PT + 3, ot=OT + 5) == 0  # (types: any alignment)
    assert f(o=p(off, 4)) == -2 and f(rows=p(ok, 4)) == -2 and f(rc=p(ok, 4)) == -2 and f(v=p(va, 4)) == -2
    assert f(pp=PP + 4) == -2 and f(ov=OV + 4) == -2 and f(res=S + 4) == -2
    assert f(n=0, n_docs=0, cs=0, os_=0) == 0


def test_the_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """tests/host_sim/parents_asan_main.cpp: random shapes in heap blocks of exactly their size, every schedule, all runs compared
    with a plain loop.  Run as a child process."""
    exe = str(tmp_path / "parents_asan")
    src = os.path.join(host_sim_lib.SIM_DIR, "parents_asan_main.cpp")
    # (the sanitizers' runtimes linked INTO the program: it does not depend on what else the process loads, or in which order)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", "-o", exe, src])
    done = subprocess.run([exe, "150"], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all runs agree" in done.stdout
