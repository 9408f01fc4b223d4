"""tools/bench_parents.py's command line: bad arguments are refused before any work (no device, no library is touched); its shapes
are what it says they are; and the torch route it measures against -- the calls a user has today -- gives, on the CPU, the
reference's parents and cells."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_parents.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--steps >= 1"), (("--rows", "0"), "--rows and --docs must be in [1, 2^32)"),
                       (("--rows", str(1 << 32)), "--rows and --docs must be in"), (("--docs", "0"), "--rows and --docs must be in"),
                       (("--docs", str(1 << 32)), "--rows and --docs must be in"), (("--warmup", "-1"), "--warmup >= 0"),
                       (("--shapes", "dense,nope"), "--shapes: a list of dense, dense_empty, dense_skewed, sparse_ranked, sparse_tenth"),
                       (("--shapes", ""), "--shapes"), (("--cols", "1,65"), "--cols: a list of column counts in [0, 64]"), (("--cols", "x"), "--cols"),
                       (("--cols", "-1"), "--cols"), (("--cols", ""), "--cols")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_shapes_and_the_torch_route():
    import torch
    from tests import parents_common as PC
    from tools import bench_parents as B
    n_rows, n_docs = 50000, 6000
    types, values = PC.doc_columns(3, n_docs, n_docs, 3)
    for shape in B.SHAPES:
        counts = B.bench_counts(n_rows, n_docs, shape)
        assert counts.size == n_docs and int(counts.sum()) == n_rows and (counts >= 0).all()
        if shape == "dense_empty":
            assert 0.85 < float((counts == 0).mean()) < 0.95
        if shape == "dense_skewed":
            assert int(counts.max()) >= n_rows // 2
        offsets = PC.offsets_of(counts)
        rows = B.bench_rows(n_rows, shape)
        assert (rows is None) == shape.startswith("dense")
        if shape == "sparse_ranked":
            assert rows.size == 2048 and (np.diff(rows) < 0).any()
        if shape == "sparse_tenth":
            assert 0.08 * n_rows < rows.size < 0.12 * n_rows and (np.diff(rows) > 0).all()
        x = np.arange(n_rows, dtype=np.int64) if rows is None else rows
        want = PC.expected_parents(offsets, x)
        assert (want >= 0).all()
        k, out_types, out_values = B.torch_route(torch, torch.from_numpy(offsets.view(np.int64)), torch.from_numpy(x), torch.from_numpy(types),
                                                 torch.from_numpy(values.view(np.int64)))
        assert k.numpy().tolist() == want.tolist()
        for c in range(3):
            assert (out_types[c].numpy() == types[c, want]).all() and (out_values[c].numpy().view(np.uint64) == values[c, want]).all()
