"""tools/bench_joinrows.py's command line: bad arguments are refused before any work (no device, no library is touched); and the
torch route it measures against -- masks, torch.sort(stable=True), two torch.searchsorted, repeat_interleave, index_select --
gives, on the CPU, the reference's pairs and carried cells for every case."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_joinrows.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--steps >= 1"), (("--rows", "0"), "--rows: a list of counts in [1, 2^32)"), (("--rows", str(1 << 32)), "--rows"),
                       (("--rows", "x"), "--rows"), (("--rows", ""), "--rows"), (("--warmup", "-1"), "--warmup >= 0"),
                       (("--cases", "zipf,nope"), "--cases: a list of dim64k_100, dim64k_10, dim1m_100, dim1m_10, zipf, carried"), (("--cases", ""), "--cases")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_torch_route_gives_the_references_pairs():
    import torch
    from tests import joinrows_common as JO
    from tests import toprows_common as TC
    from tools import bench_joinrows as B
    n = 6000
    for case in B.CASES:
        (lt, lv), (rt, rv), n_cols = B.bench_sides(n, case, seed=3, scale=16)
        assert n_cols == (4 if case == "carried" else 0) and rt.size == {"dim1": 1 << 16, "zipf": B.ZIPF_BUILD // 16}.get(case[:4], 1 << 12)
        lref = JO.left_classes(lt, None, lv, None, n, n)
        order, record, build_keys = JO.build_set(rt, None, rv)
        want_l, want_r, _, want = JO.expected_by_searchsorted(JO.INNER, lref, order, record[1], build_keys)
        by_dict = JO.expected(JO.INNER, lref, order, record[1], build_keys)
        assert (by_dict[0] == want_l).all() and (by_dict[1] == want_r).all() and by_dict[3] == want
        assert 0.9 * n < lref[2].sum() < n and 0.9 * rt.size < record[1] < rt.size and want[4] + want[5] == n - lref[2].sum()
        rate = want[3] / lref[2].sum()
        assert (0.85 < rate < 0.99) if case.endswith("_100") or case == "carried" else (0.07 < rate < 0.12) if case.endswith("_10") else want[2] > 2 * n
        l_cells, r_cells = TC.carried(2, n, n, 3), TC.carried(2, rt.size, rt.size, 4)
        t = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x)
        left_rows, right_rows, lc, rc = B.torch_route(torch, t(lt), t(lv), t(rt), t(rv), t(l_cells[1]), t(r_cells[1]))
        assert left_rows.numpy().tolist() == want_l.astype(np.int64).tolist() and right_rows.numpy().tolist() == want_r.astype(np.int64).tolist()
        assert (lc.numpy().view(np.uint64) == l_cells[1][:, want_l.astype(np.int64)]).all()
        assert (rc.numpy().view(np.uint64) == r_cells[1][:, want_r.astype(np.int64)]).all()
