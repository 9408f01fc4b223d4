"""The reference, the shapes and the checked call of the parent columns (include/sjmi.h, sjmi_parent_columns_device), shared by
tests/test_host_parents.py (the host simulation) and tests/test_gpu_parents.py (libsjmi.so).  The reference is numpy's
searchsorted on the row offsets; every result is an integer and every comparison an equality."""
import numpy as np

CANARY = 0xC0FFEE0DDF00D5
CANARY_BYTE = 0xC5
PAD = 8  # canary entries in front of and behind every output
RESULT_WORDS, MAX_COLS = 3, 64
ORPHAN = -1
TYPE_BYTES = np.frombuffer(b'ld"tfn[{\0', dtype=np.uint8)


def offsets_of(counts):
    """rows per document -> the row offsets an explode writes, uint64 [n_docs + 1]"""
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.uint64))]).astype(np.uint64)


def expected_parents(offsets, x):
    """row indices x -> their documents, int64, ORPHAN where x >= offsets[-1]"""
    x = np.asarray(x, dtype=np.uint64)
    k = np.searchsorted(offsets[1:], x, side="right").astype(np.int64)
    k[x >= offsets[-1]] = ORPHAN
    return k


def doc_columns(n_cols, n_docs, col_stride, seed):
    """n_cols document columns col_stride cells apart: any type byte, any value word -> (types uint8, values uint64), 2-D"""
    rng = np.random.default_rng(seed)
    types = TYPE_BYTES[rng.integers(0, TYPE_BYTES.size, size=(n_cols, col_stride))]
    types[:, ::3] = TYPE_BYTES[0]  # (plenty of longs)
    values = rng.integers(0, 1 << 63, size=(n_cols, col_stride), dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # (never 0: an orphan's 0 shows)
    assert col_stride >= n_docs
    return types, values


def random_counts(n_docs, seed, empty=0.3, high=9):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, high, size=n_docs)
    counts[rng.random(n_docs) < empty] = 0
    return counts


def check(call, offsets, n_rows, rows=None, row_count=None, cols=None, out_stride=None, with_parents=True, with_types=True, shift=0, what=""):
    """One call with canaries in front of and behind every output, and in every entry the call does not have to write (slots at
    or behind the live ones, the cells between out_stride-wide columns), compared with the reference.
    call(offsets, n_docs, rows, n_rows, row_count, types, values, n_cols, col_stride, parent_types, parents, out_types,
    out_values, out_stride, result) -> status, where every buffer is None or (a flat numpy array, the element at which the call's
    pointer begins); the call leaves its outputs in these arrays.  cols: None or (types, values) of doc_columns().  shift: the
    type pointers (document, parent and out) begin at this odd byte.  -> (parents int64 [live], result)"""
    n_docs = offsets.size - 1
    live = n_rows if row_count is None else min(n_rows, row_count)
    x = np.arange(n_rows, dtype=np.uint64) if rows is None else np.asarray(rows[:n_rows], dtype=np.uint64)
    want = expected_parents(offsets, x[:live])
    n_cols = 0 if cols is None else cols[0].shape[0]
    col_stride = 0 if cols is None else cols[0].shape[1]
    out_stride = (n_rows if out_stride is None else out_stride) if n_cols else 0
    rc = None if row_count is None else (np.array([row_count], dtype=np.uint64), 0)
    in_types = None if cols is None else (np.concatenate([np.zeros(shift, dtype=np.uint8), cols[0].reshape(-1)]), shift)
    in_values = None if cols is None else (np.ascontiguousarray(cols[1]).reshape(-1), 0)
    p = np.full(PAD + n_rows + PAD, CANARY, dtype=np.uint64)
    pt = np.full(PAD + shift + n_rows + PAD, CANARY_BYTE, dtype=np.uint8)
    ov = np.full(PAD + n_cols * out_stride + PAD, CANARY, dtype=np.uint64)
    ot = np.full(PAD + shift + n_cols * out_stride + PAD, CANARY_BYTE, dtype=np.uint8)
    result = np.full(1 + RESULT_WORDS + 1, CANARY, dtype=np.uint64)
    status = call((offsets, 0), n_docs, None if rows is None else (np.asarray(rows, dtype=np.uint64), 0), n_rows, rc, in_types, in_values, n_cols,
                  col_stride, (pt, PAD + shift) if with_types else None, (p, PAD) if with_parents else None,
                  (ot, PAD + shift) if n_cols else None, (ov, PAD) if n_cols else None, out_stride, (result, 1))
    assert status == 0, (what, status)
    assert result[0] == CANARY and result[-1] == CANARY
    n_orphans = int((want == ORPHAN).sum())
    assert [int(v) for v in result[1:-1]] == [live, n_orphans, 0], (what, result[1:-1], live, n_orphans)
    # the parents: a typed long column
    assert (p[:PAD] == CANARY).all() and (p[PAD + (live if with_parents else 0):] == CANARY).all(), (what, "a parent outside [0, live) was written")
    assert (pt[:PAD + shift] == CANARY_BYTE).all() and (pt[PAD + shift + (live if with_types else 0):] == CANARY_BYTE).all(), what
    if with_parents:
        got = p[PAD:PAD + live].view(np.int64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, "row", int(bad[0]), "parent", int(got[bad[0]]), "expected", int(want[bad[0]]))
    if with_types:
        assert (pt[PAD + shift:PAD + shift + live] == np.where(want == ORPHAN, 0, ord("l"))).all(), what
    # the carried cells
    assert (ov[:PAD] == CANARY).all() and (ov[PAD + n_cols * out_stride:] == CANARY).all(), what
    assert (ot[:PAD + shift] == CANARY_BYTE).all() and (ot[PAD + shift + n_cols * out_stride:] == CANARY_BYTE).all(), what
    if n_cols:
        gv = ov[PAD:PAD + n_cols * out_stride].reshape(n_cols, out_stride)
        gt = ot[PAD + shift:PAD + shift + n_cols * out_stride].reshape(n_cols, out_stride)
        assert (gv[:, live:] == CANARY).all() and (gt[:, live:] == CANARY_BYTE).all(), (what, "a cell at or behind the live rows was written")
        has = want != ORPHAN
        k = np.where(has, want, 0)
        assert (gv[:, :live] == np.where(has, cols[1][:, k], 0)).all(), what
        assert (gt[:, :live] == np.where(has, cols[0][:, k], 0)).all(), what
    return want, [int(v) for v in result[1:-1]]
