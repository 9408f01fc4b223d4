"""tools/bench_sortrows.py's command line: bad arguments are refused before any work (no device, no library is touched); and the
torch route it measures against -- masks, an order-preserving key, torch.sort(stable=True), index_select -- gives, on the CPU, the
reference's rows and carried cells for every case, the two-key chain included."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_sortrows.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--steps >= 1"), (("--rows", "0"), "--rows: a list of counts in [1, 2^32)"), (("--rows", str(1 << 32)), "--rows"),
                       (("--rows", "x"), "--rows"), (("--rows", ""), "--rows"), (("--warmup", "-1"), "--warmup >= 0"),
                       (("--cases", "counters,nope"), "--cases: a list of counters, longs, doubles, chain, carried"), (("--cases", ""), "--cases")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_torch_route_gives_the_references_rows():
    import torch
    from tests import sortrows_common as SO
    from tests import toprows_common as TC
    from tools import bench_sortrows as B
    n = 5000
    carry_ty, carry_va = TC.carried(2, n, n, 3)
    for case in B.CASES:
        keys = B.bench_keys(n, case, seed=3)
        assert len(keys) == (2 if case == "chain" else 1)
        want_rows, want = SO.chain([(ty, None, va, kind, desc) for ty, va, kind, desc in keys], n)
        assert all(3500 < w[1] <= n and w[0] == n for w in want) and want[-1][7] == {"longs": 8, "doubles": 8}.get(case, 2)
        t_keys = [(torch.from_numpy(ty), torch.from_numpy(va.view(np.int64)), kind, desc) for ty, va, kind, desc in keys]
        rows, cells = B.torch_chain(torch, t_keys, torch.from_numpy(carry_va.view(np.int64)))
        assert rows.numpy().tolist() == want_rows.astype(np.int64).tolist()
        assert (cells.numpy().view(np.uint64) == carry_va[:, want_rows.astype(np.int64)]).all()
    # one key, descending, and doubles with longs among them, NaNs and both zeros: the typed column of the operator's own tests
    for what, kind in (("doubles", TC.DOUBLE), ("counters", TC.LONG)):
        ty, va = TC.typed_column(n, 9, what)
        for descending in (False, True):
            want_rows, _, _ = SO.expected(ty, None, va, None, n, n, kind, descending)
            rows, _ = B.torch_route(torch, torch.from_numpy(ty), torch.from_numpy(va.view(np.int64)), kind == TC.DOUBLE, descending)
            assert rows.numpy().tolist() == want_rows.astype(np.int64).tolist()
