"""CPU test of SimdJsonParser::parseBatch (csrc/host/simdjson_parser.cpp, batch_stages.h) without a GPU, under the sanitizers:
tests/host_sim/parse_batch_main.cpp is the real parser over a CPU engine made of the oracle's C.  It checks every document of
every batch against the oracle itself -- several thread and sub-batch counts, batches of changing shape on one parser, an engine
call failing in a feeder -- and exits non-zero on a mismatch; here it is built twice, once with ThreadSanitizer (the feeder /
pool / slab hand-offs are the project's only concurrent host code) and once with AddressSanitizer + UBSan, and run as a child
process.  The sanitizers' runtimes are linked INTO the program: it does not depend on what else the process loads, or in which order."""
import os
import platform
import re
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_sim", "parse_batch_main.cpp")
ORACLE_C = os.path.join(ROOT, "oracle", "sj_oracle.c")
# (threads, sub-batches) -> FNV over tapes, offsets, errors and string lengths of every batch of the run: what the program
# printed before parseBatch was cut into its parts, and prints since
DIGESTS = {(1, 1): "de1c8bde9975792e", (3, 2): "bc3afdee4ee5dbfb", (8, 3): "63b5ec389e034fbf", (2, 64): "bced82e58b19d4be"}


def _build(tmp_path, name, flags):
    obj, exe = str(tmp_path / ("oracle_%s.o" % name)), str(tmp_path / ("parse_batch_%s" % name))
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11"] + flags + ["-c", "-o", obj, ORACLE_C])
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-o", exe, SRC, obj])
    return exe


def _digests(stdout):
    return {(int(t), int(j)): d for t, j, d in re.findall(r"^parse_batch threads=(\d+) sub-batches=(\d+) digest=([0-9a-f]{16})$", stdout, flags=re.M)}


@pytest.mark.parametrize("name,flags", [
    ("tsan", ["-fsanitize=thread", "-static-libtsan"]),
    ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]),
])
def test_parse_batch_program_is_clean(tmp_path, name, flags):
    cmd = [_build(tmp_path, name, flags)]
    if name == "tsan" and shutil.which("setarch"):
        # this compiler's ThreadSanitizer expects program and libraries inside its fixed address map and gives up at start ("unexpected
        # memory mapping") where the kernel randomises addresses over more bits than it was written for: this child runs without
        # address randomisation (its own personality flag, nothing of the host's)
        cmd = ["setarch", platform.machine(), "-R"] + cmd
    env = {k: v for k, v in os.environ.items() if not k.startswith("SJMI_")}
    done = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert done.returncode == 0, done.stdout + done.stderr
    assert "all configurations agree with the oracle" in done.stdout
    for word in ("Sanitizer", "runtime error", "FAIL"):
        assert word not in done.stderr, done.stderr
    assert _digests(done.stdout) == DIGESTS, done.stdout
