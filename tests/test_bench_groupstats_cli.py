"""tools/bench_groupstats.py's command line: bad arguments are refused before any work (no device, no library is touched); and the
torch route it measures against -- the calls a user has today -- gives, on the CPU, what the reference gives where no sum wraps."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_groupstats.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--steps >= 1"), (("--rows", "0"), "--rows must be in [1, 2^32)"), (("--rows", str(1 << 32)), "--rows must be in"),
                       (("--warmup", "-1"), "--warmup >= 0"), (("--values", "all_long,nope"), "--values: a list of all_long, half_double"),
                       (("--values", ""), "--values"), (("--keys", "8,0"), "--keys: a list of key counts"), (("--keys", "x"), "--keys"),
                       (("--keys", str((1 << 20) + 1)), "--keys")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_torch_route_gives_what_the_reference_gives():
    import torch
    from tests import groupstats_common as GC
    from tools import bench_groupstats as B
    n_rows, n_keys = 3000, 7
    ix, words, bits = GC.keys_column(n_rows, n_keys, 4, "uniform")
    ty, va = GC.value_column(n_rows, 4, "exact")  # (longs below 2^40: no int64 sum wraps)
    want, _ = GC.expected(ix, bits, ty, va, n_keys, n_rows)
    got = [t.numpy() for t in B.torch_route(torch, torch.from_numpy(ix), torch.from_numpy(bits), torch.from_numpy(ty), torch.from_numpy(va.view(np.int64)),
                                            n_keys)]
    for k, w in enumerate(want):
        assert [int(got[j][k]) for j in range(4)] == [w["n_long"], w["n_double"], w["n_other"], w["sum_long"]]
        assert float(got[4][k]) == w["sum_double"] and (int(got[5][k]), int(got[6][k])) == (w["min_long"], w["max_long"])
        assert (float(got[7][k]), float(got[8][k])) == (w["min_double"], w["max_double"])
