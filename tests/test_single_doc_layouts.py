"""The conditions of the corpus of tests/single_doc_layouts.py, asserted on the CPU with the oracle alone: what
tests/test_gpu_single_doc_layouts.py can notice about sjmi_parse_document's walk depends on them -- that the restated switches
are the sources', that every member has the structurals and bytes its name says and takes the way through the dispatch it was
built for, that every way is taken in both byte bands, and that the reference's default limits admit every member."""
import os
import re

import numpy as np

from oracle import oracle as O
from tests import single_doc_layouts as L
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "simdjson-java_amd", "csrc")
STAGE1_CODES = (1, 2, 3)  # SJMI_E_UTF8, _UNCLOSED_STRING, _UNESCAPED_CHARS
CAPACITY_CODES = (28, 29, 100)  # SJMI_E_DEPTH, _CAPACITY, _INTERNAL
_facts = {}


def facts(m):
    """(the structurals' first bytes, the oracle's parse) of a member, computed once"""
    if m.name not in _facts:
        idx, _ = O.stage1(m.doc)
        sb = np.frombuffer(m.doc, dtype=np.uint8)[idx].tobytes() if idx.size else b""
        _facts[m.name] = (sb, O.parse(m.doc))
    return _facts[m.name]


def members():
    return [m for name in L.FAMILIES for m in L.family(name)]


def test_constants_are_the_sources():
    src = open(os.path.join(CSRC, "coop_walk.hip"), encoding="utf-8").read()

    def value(pattern):
        found = re.findall(pattern, src, flags=re.M)
        assert len(found) == 1, (pattern, found)
        return eval(found[0].replace("u", ""), {"__builtins__": {}})  # "256u << 10", "1536"
    got = {
        "COOP_CHUNK_MIN": value(r"^constexpr uint64_t COOP_CHUNK_MIN = ([0-9u <]+);"),
        "COOP_OPTIMISTIC_MIN": value(r"^constexpr uint64_t COOP_OPTIMISTIC_MIN = ([0-9u <]+);"),
        "CW_SINGLE_N": value(r"^constexpr uint64_t CW_SINGLE_N = ([0-9u <]+);"),
        "CW_SMALL_N": value(r"^constexpr uint64_t CW_SMALL_N = ([0-9u <]+);"),
        "CW_GROUP_BIAS": value(r"^#define SJMI_CW_GROUP_BIAS ([0-9]+)"),
        "CW_BIAS": value(r"^constexpr int CW_BIAS = ([0-9]+);"),
        "CW_LEVELS": value(r"^constexpr int CW_LEVELS = ([0-9]+);"),
    }
    assert set(got) == set(L.CONSTANTS)
    assert got == {name: getattr(L, name) for name in L.CONSTANTS}
    # the forms of the comparisons the restatement copies
    for text in ("count_bound > COOP_CHUNK_MIN", "count_bound > COOP_OPTIMISTIC_MIN", "to - from <= CW_SINGLE_N", "n <= CW_SMALL_N ? 128u : 512u",
                 "(uint64_t)g * g * SJMI_CW_GROUP_BIAS < nchunks", "hmin < 0 || hmax >= CW_LEVELS", "s.H + r.d >= CW_LEVELS"):
        assert text in src, text
    api = open(os.path.join(CSRC, "sjmi_api.hip"), encoding="utf-8").read()
    assert "const uint64_t bound = len + 1;" in api  # (the count bound of sjmi_parse_document: its byte length + 1)


def test_dispatch_restatement():
    assert [L.band(n) for n in (0, 1534, 1535, 1536, 16382, 16383, 16384, 1 << 20)] == \
        ["sweep", "sweep", "sweep", "queued", "queued", "queued", "optimistic", "optimistic"]
    assert [L.chunk_of(n) for n in (513, 262144, 262145)] == [128, 128, 512]
    assert [L.group_of(c) for c in (1, 256, 257, 1024, 1025, 4096, 4097)] == [8, 8, 16, 16, 32, 32, 64]
    assert L.path(b"[" + b"0," * 300, 1534) == "sweep" and L.path(b"[0]", 5000) == "short"
    flat = b"[" + b"0," * 400 + b"0]"
    assert L.path(flat, 5000) == "chunks"
    # (601 structurals in front: the run of opening brackets begins at the 89th structural of a chunk of 128; 768 in front of the closing ones)
    assert L.path(b"[" + b"0," * 300 + b"[" * 32 + b"]" * 32 + b",0" * 100 + b"]", 5000) == "chunks"   # the highest bracket at relative level 63
    assert L.path(b"[" + b"0," * 300 + b"[" * 33 + b"]" * 33 + b",0" * 100 + b"]", 5000) == "swing"
    assert L.path(b"[0,0," * 40 + b"0," * 284 + b"]" * 31 + b",0" * 100, 5000) == "chunks"                 # the lowest container level 0
    assert L.path(b"[0,0," * 40 + b"0," * 284 + b"]" * 32 + b",0" * 100, 5000) == "swing"


def test_byte_lengths_stay_small():
    # (about half a megabyte at the most; the structured flavour of the largest counts takes 1.6 bytes per structural)
    for m in members():
        assert len(m.doc) <= 530000 or (m.family == "counts" and "/structured/" in m.name and len(m.doc) <= 850000), m.name


def test_members_are_what_their_names_say():
    seen = set()
    for m in members():
        sb, want = facts(m)
        n, length = re.fullmatch(r".*/n(\d+)/len(\d+)", m.name).groups()
        assert len(sb) == int(n) == m.n, (m.name, len(sb))
        assert len(m.doc) == int(length), m.name
        assert want.n_structurals == m.n or m.kind == "stage1", (m.name, want.n_structurals)
        assert m.name not in seen
        seen.add(m.name)
    assert len(seen) > 300


def test_members_take_the_path_they_were_built_for():
    for m in members():
        sb, _ = facts(m)
        assert L.path(sb, len(m.doc)) == m.cell, m.name
        if m.cell in ("chunks", "spike"):
            # ... and nothing else declines them: the chunk walkers do walk these
            p = L.profile(sb)
            assert not p.group_window and not p.group_end_deep, (m.name, p)
        if m.name.startswith("bands/spike_") or m.name.startswith("bands/control_"):
            want_depth = int(m.name.split("/")[1].split("_")[1])
            assert L.profile(sb).max_depth == want_depth, m.name
        if m.name.startswith("bands/deep_end_mid_group") and m.cell != "sweep":
            # chunks END at 64 levels and more, and neither the chunk summaries, the group summaries nor the groups' ends show it
            p = L.profile(sb)
            assert p.deep_end and not (p.swing or p.group_window or p.group_end_deep), (m.name, p)


def test_every_cell_is_inhabited():
    cells, chunks, groups = set(), set(), set()
    for m in members():
        cells.add((L.band(len(m.doc)), m.cell))
        if m.cell not in ("sweep", "short"):
            chunks.add(L.chunk_of(m.n))
            groups.add(L.group_of(L.nchunks_of(m.n)))
    want = {("sweep", "sweep")} | {(b, p) for b in ("queued", "optimistic") for p in L.PATHS if p != "sweep"}
    assert cells == want, (sorted(want - cells), sorted(cells - want))
    assert chunks == {128, 512}
    assert {8, 16, 32} <= groups
    # every kind of `bands` at every length, the listed cells aside
    have = {(len(m.doc), m.name.split("/")[1]) for m in L.family("bands")}
    kinds = {k for _, k in have}
    assert {(length, k) for length in L.BAND_LENGTHS for k in kinds} - have == set(L.BAND_LEFT_OUT)
    assert sorted(L.BAND_LEFT_OUT) == sorted((length, k) for length in (1535, 1536)
                                             for k in ("control_63", "deep_end_1000", "deep_end_mid_group", "spike_64", "spike_71"))
    assert {len(m.doc) for m in L.family("bands")} == set(L.BAND_LENGTHS)
    for d in L.poison_documents():
        assert L.band(len(d)) == "optimistic"
    bad_utf8, declined = L.poison_documents()
    assert O.parse(bad_utf8).stage1_status & 1 and O.parse(declined).error == 0
    idx, _ = O.stage1(declined)
    assert L.path(np.frombuffer(declined, dtype=np.uint8)[idx].tobytes(), len(declined)) == "swing"


def test_counts_family_is_complete():
    names = {m.name.rsplit("/n", 1)[0] for m in L.family("counts")}
    for s in L.COUNTS:
        for form in L.FORMS:
            assert "counts/flat/s%d/%s" % (s, form) in names
            assert ("counts/structured/s%d/%s" % (s, form) in names) == (form == "plain" or s not in L.COUNTS[-8:])
    assert L.COUNTS == sorted(L.COUNTS) and L.COUNTS[-8] == L.CW_SMALL_N
    for m in L.family("counts"):
        if "/structured/" in m.name:
            assert m.doc.count(L.UNIT.encode()) >= (m.n - 32) // 28 >= 17, m.name


def test_phases_put_every_position_of_the_unit_on_a_chunk_edge():
    for k in L.PHASE_UNITS:
        firsts = set()
        for shift in L.PHASE_SHIFTS:
            m = [x for x in L.family("phases") if x.name.startswith("phases/units%d/shift%d/" % (k, shift))]
            assert len(m) == 1
            sb, _ = facts(m[0])
            chunk = L.chunk_of(m[0].n)
            assert chunk == (128 if k == 50 else 512)
            for j in range(k):
                at = L.phase_first_structural(shift, j)
                assert sb[at:at + 28] == b'{":",":[],":{},":[1,{":n}]},'
                for p in range(28):
                    if (at + p) % chunk == 0:
                        firsts.add(p)
        assert firsts == set(range(28)), (k, sorted(firsts))


def test_edge_pairs_sit_on_their_edges():
    firsts = {"[": b"[", "]": b"]", "{": b"{", "}": b"}", ",": b",", ":": b":", "1": b"1", '"k"': b'"'}
    large = 0
    for m in L.family("edge_pairs"):
        sb, _ = facts(m)
        what, e = m.name.split("/")[1:3]
        e = int(e[1:])
        assert e % L.chunk_of(m.n) == 0 and (m.n > L.CW_SMALL_N) == (e == L.EDGE_LARGE[0]), m.name
        large += m.n > L.CW_SMALL_N
        pair = [p for name, _, p, _, _ in L.PAIRS if name == what]
        if pair:
            assert sb[e - 1:e + 1] == b"".join(firsts[t] for t in pair[0]), m.name
        elif what == "root_close_last_then_trailing":
            assert sb[e - 1:e + 1] == b"]7" and sb.count(b"[") - sb[:e - 1].count(b"]") == 1 and sb[-1:] == b"]", m.name
        else:
            assert sb[e:e + 1] == b"]" and sb.count(b"[") - sb[:e - 1].count(b"]") == 1 and sb[-1:] == b"]", m.name
            assert (m.n == e + 1) == (what == "root_close_first_ends")
    assert large == len(L.LARGE_PAIRS) == 4
    assert {L.band(len(m.doc)) for m in L.family("edge_pairs")} == {"queued", "optimistic"}


def test_two_errors_differ_by_their_order():
    by_name = {m.name: m for m in L.family("two_errors")}
    pairs = 0
    for m in by_name.values():
        partner = L.two_error_partner(m.name)
        if partner:
            # the same two errors in the other order: picking the second one of either document would be the other's code
            assert facts(m)[1].error != facts(by_name[partner])[1].error, m.name
            pairs += 1
    assert pairs == len(by_name) - 4
    for m in by_name.values():
        if "/abutting/" in m.name:
            sb, want = facts(m)
            e = int(m.name.split("/")[2][1:])
            assert sb[e - 2:e + 1] == b"{11" and want.error == 12, m.name  # SJMI_E_OBJECT_NO_KEY at e - 1; e fails too (no comma)
            assert O.parse(m.doc.replace(b"{1 1}", b'{"a":1 1}')).error not in (0, 12)


def test_second_opinion_of_the_chunk_model():
    """whether a chunk is out of range: tools/chunk_scan_model.py's Summary over the same chunks"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import chunk_scan_model as M
    kinds = {ord(c): c for c in "[]{},:"}
    kinds[ord('"')] = "s"
    checked = out = 0
    for m in members():
        if m.n > 20000 or m.n == 0:
            continue
        sb, _ = facts(m)
        tokens = [kinds.get(c, "n" if c == ord("-") or 48 <= c <= 57 else "a") for c in sb]
        chunk = L.chunk_of(m.n)
        model = any(M.Summary(tokens[a:a + chunk]).out_of_range for a in range(0, len(tokens), chunk))
        assert model == L.profile(sb).swing, m.name
        checked += 1
        out += model
    assert checked > 200 and out >= 9


def test_the_reference_admits_every_member():
    for m in members():
        sb, want = facts(m)
        assert L.profile(sb).max_depth <= 1023, m.name
        if m.kind == "valid":
            assert want.error == 0 and want.stage1_status == 0, (m.name, want.error)
        elif m.kind == "error":
            assert want.error > 0 and want.stage1_status == 0 and want.error not in STAGE1_CODES + CAPACITY_CODES, (m.name, want.error)
        else:
            assert want.stage1_status != 0 and want.error in STAGE1_CODES, (m.name, want.error)
