"""tools/bench_members.py's command line: bad arguments are refused before any work (no device, no library is touched); and its
host route -- the numpy walk of the member chains that the device route is measured against -- counts what Python's own parse
counts, on tapes made by the oracle."""
import os
import subprocess
import sys

import numpy as np

from tests.conftest import ROOT

TOOL = os.path.join(ROOT, "tools", "bench_members.py")


def _run(*args):
    return subprocess.run([sys.executable, TOOL] + list(args), capture_output=True, text=True, timeout=120, cwd=ROOT)


def test_bad_arguments_are_refused_before_any_work():
    for args, text in ((("--steps", "0"), "--docs, --rows and --steps must be >= 1"), (("--docs", "0"), "must be >= 1"), (("--warmup", "-1"), "--warmup >= 0"),
                       (("--sections", "explode,nope"), "--sections: a list of explode, census, discover"), (("--sections", ""), "--sections")):
        out = _run(*args)
        assert out.returncode == 2 and text in out.stderr, (args, out.stderr[-500:])


def test_the_host_route_counts_what_python_counts():
    from oracle import oracle as O
    from tests import explode_common as EC
    from tests import members_common as MC
    from tools import bench_members as B
    docs = [b"{" + b",".join(b'"' + k + b'":' + v for k, v in zip(B.pool_keys(i), B.pool_values(i))) + b"}" for i in (3, 20, 3, 100)]
    docs += [b'{}', b'[1,2]', b'{"id":{"id":1,"x":[1,{"y":2}]},"":null,"id":false}', b'7']
    tape, toffs, errs, sb, _, _ = EC.pack([O.parse(d) for d in docs])
    got = B.host_discover(tape, toffs.astype(np.int64), sb)
    assert got == MC.python_key_census([MC.resolve_pairs(MC.loads_pairs(d), "") for d in docs])
    assert got[0] == (b"id", [4, 0, 0, 1, 0, 0, 1, 0]) and (b"", [0, 0, 0, 0, 1, 0, 0, 0]) in got
