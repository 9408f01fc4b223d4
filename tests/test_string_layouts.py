"""CPU checks of the granule-edge string layouts (tests/string_layouts.py): every layout passes stage 1 and has its features where
its label says; the oracle's StringParser restatement agrees with an independent reference (Python's json module) on every
string of every layout; and the host simulation of the string pass's block algebra (tests/host_sim/str_sim.cpp, both shortcut
settings) reproduces the oracle's records on them."""
import functools
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import string_layouts as L
from tests.test_host_strings import check_against_oracle, expected_records, sim_runners


@functools.lru_cache(None)
def layouts(family):
    return L.FAMILIES[family](False) if family == 8 else L.FAMILIES[family]()


FAMILIES = sorted(L.FAMILIES)


def literals(doc):
    """every string literal the string pass sees (an unescaped opening quote: quote & inString), as (position, literal bytes
    including both quotes)"""
    _, _, masks = O.index_blocks(doc, want_masks=True)
    quotes = []
    for b in range(masks.shape[0]):
        q = int(masks[b, 1])
        while q:
            low = q & -q
            quotes.append(64 * b + low.bit_length() - 1)
            q ^= low
    opens = {p for p in quotes if (int(masks[p // 64, 2]) >> (p % 64)) & 1}
    out = []
    for i, p in enumerate(quotes):
        if p in opens:
            out.append((p, doc[p:quotes[i + 1] + 1]))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_layouts_pass_stage1_and_sit_where_labelled(family):
    for lay in layouts(family):
        idx, st = O.stage1(lay.doc)
        assert st == 0, (lay.label, st)
        for pos, want in lay.marks:
            assert lay.doc[pos:pos + len(want)] == want, (lay.label, pos, lay.doc[pos:pos + len(want)], want)
        # every opening quote is a structural, except in family 7, where that is the point
        structural = set(int(x) for x in idx)
        opens = [p for p, _ in literals(lay.doc)]
        if family == 7:
            assert any(p not in structural for p in opens), lay.label
        else:
            assert all(p in structural for p in opens), lay.label


def test_layout_offsets_and_counts():
    """the claims the labels make about edges and \\u item counts, recomputed"""
    for lay in layouts(1):  # opening quotes at granule offsets 4093..4097, closing ones at the first / last 3 bytes
        opens, closes = lay.marks[0::2], lay.marks[1::2]
        assert sorted({p % L.G for p, _ in opens}) == [0, 1, 4093, 4094, 4095]
        assert sorted({p % L.G for p, _ in closes}) == [0, 1, 2, 4093, 4094, 4095]
        assert all(c // L.G - o // L.G in L.SPANS for (o, _), (c, _) in zip(opens, closes))
    for lay in layouts(3):  # the backslash 1..12 bytes in front of a block / granule edge
        step = L.G if "granule" in lay.label else L.BLK
        backs = {(-p) % step for p, _ in lay.marks}
        assert backs <= set(L.BACKS) and (len(lay.marks) < 12 or backs == set(L.BACKS)), lay.label
        if step == L.BLK:
            assert all((p + b) % L.G for p, _ in lay.marks for b in [(-p) % step])
    for lay in layouts(4):  # the run's last backslash at -1, 0, +1 of a block / granule start
        step = L.G if "granule" in lay.label else L.BLK
        ends = {((p + len(m) - 1) % step + 1) % step - 1 for p, m in lay.marks if m[:1] == b"\\"}
        assert len(ends) == 1 and ends <= {-1, 0, 1}, lay.label
        assert {len(m) for p, m in lay.marks if m[:1] == b"\\"} == set(L.RUNS)

    def items_per_granule(content, base):
        """\\uXXXX items by the granule of their last hex digit (a surrogate pair is one item, at its low half)"""
        n, i = {}, 0
        while i < len(content):
            if content[i:i + 2] == b"\\u":
                hi = int(content[i + 2:i + 6], 16)
                j = i + 6
                if 0xD800 <= hi <= 0xDBFF and content[j:j + 2] == b"\\u":
                    j += 6
                g = (base + j - 1) // L.G
                n[g] = n.get(g, 0) + 1
                i = j
            else:
                i += 1
        return n
    for counts in ([127], [128], [129], [L.U_MAX], [128, 129], [L.U_MAX, 127]):
        content = b"".join(L.u_granule(c, seed=k, only_short=(c == L.U_MAX)) for k, c in enumerate(counts))
        assert items_per_granule(content, 0) == {g: c for g, c in enumerate(counts)}
    assert 10 + 6 * L.U_MAX == L.G  # the densest granule: nothing but 6-byte items behind 10 plain bytes
    for lay in layouts(6):
        if "4096 quotes" in lay.label or "granule of quotes" in lay.label:
            assert lay.doc.count(b'"') % 2 == 0 and any(m == b'"' * L.G for _, m in lay.marks)
    for g, t in L.size_list(big=False):
        assert len(L.sized(g * L.G + t, 0)) == g * L.G + t


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_records_against_json(family):
    """The oracle's record of every string (sjo_parse_string, the StringParser restatement) against Python's json module: an
    accepted string's payload is json.loads(literal) in UTF-8; a rejected one is rejected by json.loads or decodes to a lone
    surrogate, which has no UTF-8 form (StringParser pairs surrogates itself and throws on a lone one)."""
    n_ok = n_bad = 0
    for lay in layouts(family):
        recs = expected_records(lay.doc)
        lits = literals(lay.doc)
        assert [p for p, _ in lits] == [r[0] for r in recs], lay.label
        for (pos, lit), (_, rec, code) in zip(lits, recs):
            try:
                ref = json.loads(lit.decode("utf-8")).encode("utf-8")
            except (ValueError, UnicodeEncodeError):
                ref = None
            if rec is None:
                assert ref is None, (lay.label, pos, lit[:80], code)
                n_bad += 1
            else:
                assert ref is not None, (lay.label, pos, lit[:80])
                assert rec[:4] == len(ref).to_bytes(4, "big") and rec[4:] == ref, (lay.label, pos, lit[:80])
                n_ok += 1
    assert n_ok > 0
    if family in (2, 3, 5, 7):
        assert n_bad > 0


@pytest.fixture(scope="module")
def sim():
    return sim_runners()


@pytest.mark.parametrize("family", FAMILIES)
def test_host_simulation_on_layouts(sim, family):
    for lay in layouts(family):
        for run in sim:
            check_against_oracle(lay.doc, run)
