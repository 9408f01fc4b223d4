"""tools/bench_toprows.py's command line: bad arguments are refused before any work (no device, no library is touched); and the
torch route it measures against -- the calls a user has today -- gives, on the CPU, the reference's values in the reference's
order (not its rows: torch.topk leaves the order of ties unspecified)."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_toprows.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--steps >= 1"), (("--rows", "0"), "--rows must be in [1, 2^32)"), (("--rows", str(1 << 32)), "--rows must be in"),
                       (("--warmup", "-1"), "--warmup >= 0"), (("--columns", "uniform,nope"), "--columns: a list of uniform, counters, equal, doubles"),
                       (("--columns", ""), "--columns"), (("--ks", "8,0"), "--ks: a list of k in [1, 2048]"), (("--ks", "x"), "--ks"),
                       (("--ks", "2049"), "--ks"), (("--ks", ""), "--ks")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_torch_route_gives_the_references_values():
    import torch
    from tests import toprows_common as TC
    from tools import bench_toprows as B
    n = 5000
    carry_ty, carry_va = TC.carried(1, n, n, 3)
    for what in B.COLUMNS:
        ty, va, kind = B.bench_column(n, what, seed=3)
        column = va.view(np.float64) if kind == TC.DOUBLE else va.view(np.int64)
        for k in (1, 100, 2048):
            for largest in (True, False):
                want_rows, want = TC.expected(ty, None, va, n, kind, largest, k)
                assert 3500 < want[1] < 4500 and want[6] == k  # (80 % candidates)
                top, rows, cells = B.torch_route(torch, torch.from_numpy(ty), torch.from_numpy(va.view(np.int64)),
                                                 torch.from_numpy(carry_va.view(np.int64)), k, kind == TC.DOUBLE, largest)
                assert top.numpy().tolist() == column[want_rows].tolist() == column[rows.numpy()].tolist()
                assert (cells.numpy().view(np.uint64)[0] == carry_va[0, rows.numpy()]).all()
