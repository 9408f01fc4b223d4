"""CPU-only: the native sources read only the environment variables and test only the SJMI_* macros listed here.

An experiment's switch (a preprocessor branch that picks a rejected alternative, an ablation, a trace hook) does not
stay in the product: build the variant from an edited copy of the source instead (tools/build_variant.sh,
VARIANT_FILE=).  A new entry in either list needs a reason that holds for the product."""
import os
import re

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "simdjson-java_amd", "csrc")

# getenv("...") names: runtime switches that tests or users rely on
GETENV_ALLOWED = {
    "SJMI_TILE_MODE": "start contexts in SAFE tile assignment (stage 1's fall-back mode, also for callers who want it)",
    "SJMI_ZERO_COPY": "0 turns off zero-copy reads of host buffers (tests compare both placements)",
    "SJMI_BATCH_OPTIMISTIC": "0 turns off the optimistic batch pipeline (tests run both batch paths)",
    "SJMI_BATCH_REPAIR": "0 turns off the repair pass of rejected batches (tests run both)",
    "SJMI_TOKEN_WALK": "0 walks batches with the exact walker only (tests compare the two walkers)",
    "SJMI_TS_RUN_DOCS": "forces the stream walker's documents per run (tests reach every run size)",
    "SJMI_PARSE_THREADS": "host threads of the C++ SimdJsonParser shim",
    "SJMI_PARSE_PIPELINE": "sub-batches per batch of the C++ SimdJsonParser shim",
    "SJMI_PARSE_TIMING": "per-stage timing printout of the C++ SimdJsonParser shim",
}

# SJMI_* names in #if / #ifdef / #ifndef / #elif: measured tuning numbers, one code path each
IF_ALLOWED = {
    "SJMI_S1_SORT_MIN": "stage 1: indexes per 4 KiB step above which the expansion sorts its half masks",
    "SJMI_S1_PLAIN_WAVES": "stage 1: waves per SIMD of k_stage1",
    "SJMI_S1_BATCH_WAVES": "stage 1: waves per SIMD of k_stage1_batch",
    "SJMI_SSCAN_K": "string pass: the scanner's window, in 64-granule units",
    "SJMI_STR_CLASSES": "string pass: ticket counters",
    "SJMI_CW_GROUP_BIAS": "chunked walker: chunks are grouped by ~sqrt(chunks / bias)",
    "SJMI_TS_RUN": "stream walker: the most documents per run",
    "SJMI_TS_WAVES": "stream walker: waves per SIMD of k_tok_stream",
}


def _sources():
    out = {}
    for d, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f.endswith((".hip", ".h", ".hpp", ".cpp", ".cc", ".c")):
                path = os.path.join(d, f)
                out[os.path.relpath(path, ROOT)] = open(path, encoding="utf-8").read()
    assert any(p.endswith("stage1.hip") for p in out), "no sources found under %s" % CSRC
    return out


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def test_getenv_names_are_allowed():
    seen, bad = set(), []
    for path, text in _sources().items():
        code = _strip_comments(text)
        for m in re.finditer(r"\bgetenv\s*\(\s*([^)]*)\)", code):
            arg = m.group(1).strip()
            lit = re.fullmatch(r'"([^"]*)"', arg)
            line = code.count("\n", 0, m.start()) + 1
            if not lit:
                bad.append("%s:%d: getenv(%s): not a literal name" % (path, line, arg))
            elif lit.group(1) not in GETENV_ALLOWED:
                bad.append("%s:%d: getenv(\"%s\") is not in GETENV_ALLOWED" % (path, line, lit.group(1)))
            else:
                seen.add(lit.group(1))
    assert not bad, "\n".join(bad)
    assert seen == set(GETENV_ALLOWED), "allowed but no longer read: %s" % sorted(set(GETENV_ALLOWED) - seen)


def test_preprocessor_switches_are_allowed():
    seen, bad = set(), []
    for path, text in _sources().items():
        code = _strip_comments(text)
        for m in re.finditer(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b([^\n]*)", code, flags=re.M):
            line = code.count("\n", 0, m.start()) + 1
            for name in re.findall(r"\bSJMI_[A-Za-z0-9_]+", m.group(1)):
                if name in IF_ALLOWED:
                    seen.add(name)
                else:
                    bad.append("%s:%d: #if on %s, which is not in IF_ALLOWED" % (path, line, name))
    assert not bad, "\n".join(bad)
    assert seen == set(IF_ALLOWED), "allowed but no longer tested: %s" % sorted(set(IF_ALLOWED) - seen)
