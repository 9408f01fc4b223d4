"""The host simulations of the column operators (tests/host_sim/<name>_sim.cpp) as shared libraries: one build step for the
tests/test_host_*.py that load one."""
import ctypes
import os
import subprocess

from tests.conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "host_sim")
CSRC_DIR = os.path.join(ROOT, "simdjson-java_amd", "csrc")


def load(name, csrc_headers):
    """tests/host_sim/<name>_sim.cpp as lib<name>sim.so, built with g++ when it is older than its source, the csrc headers it
    compiles verbatim, or what every one of these sims includes (seq_group.h, and sj_block.h behind it).  The library is
    written under another name and renamed: a test process never loads half of one."""
    so = os.path.join(SIM_DIR, "lib%ssim.so" % name)
    src = os.path.join(SIM_DIR, "%s_sim.cpp" % name)
    deps = [src, os.path.join(SIM_DIR, "seq_group.h")] + [os.path.join(CSRC_DIR, h) for h in ("sj_block.h",) + tuple(csrc_headers)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", tmp, src])
        os.replace(tmp, so)
    return ctypes.CDLL(so)
