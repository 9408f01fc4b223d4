"""The corpus of tests/grammar_sweep.py, held to the oracle alone (no GPU): the families' sizes, the oracle's code histogram of each
-- so that the GPU sweeps compare what they are meant to: every stage-2 code, 14 and 15 included, the deferred literal's codes 21 /
22 both winning over and losing to a grammar fault, the three stage-1 verdicts against everything else, the depth limit's code 28
-- and the vectorised helpers against their plain forms."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import grammar_sweep as G
from tests.tok_stream_layouts import predicted_length

HISTOGRAMS = {
    "short9": {0: 41, 10: 59049, 11: 59049, 12: 6498, 13: 824, 14: 3, 15: 26, 16: 2433, 17: 201235, 18: 268712},
    "short13": {0: 49, 10: 28561, 11: 28561, 12: 2186, 13: 183, 15: 1, 16: 867, 17: 155138, 18: 124397, 21: 31145, 22: 31145},
    "short12s": {0: 10, 1: 6516, 2: 4362, 3: 3809, 10: 757, 11: 757, 12: 79, 13: 11, 16: 27, 17: 2859, 18: 3433},
}
EDITS_5_UNITS = {0: 140, 10: 3, 11: 25, 12: 420, 13: 665, 14: 444, 15: 766, 16: 789, 17: 22, 18: 496, 21: 102, 22: 102}


@pytest.mark.parametrize("name", list(HISTOGRAMS))
def test_family_sizes_and_the_oracles_codes(name):
    docs = G.family(name)
    errors, parsed = G.answers(name)
    assert len(docs) == G.COUNTS[name] == len(set(docs)) == errors.size
    assert G.histogram(errors) == HISTOGRAMS[name]
    assert sorted(parsed) == np.nonzero(errors == 0)[0].tolist()
    # the C loop behind answers() is the same restatement as oracle.parse, document by document
    for k in range(0, len(docs), 997):
        assert O.parse(docs[k] + b"\n").error == int(errors[k]), (k, docs[k])


def test_short9_bytes_and_rare_codes():
    docs = G.family("short9")
    errors, _ = G.answers("short9")
    assert sum(len(d) + 1 for d in docs) == 8976371
    # six tokens is the shortest length at which code 14 occurs at all; code 15 once up to five tokens
    short = G.histogram(errors[:G.SHORT9_UP_TO_5])
    assert G.SHORT9_UP_TO_5 == 66429 and 14 not in short and short[15] == 1
    assert docs[:G.SHORT9_UP_TO_5] == G.short9(5)


def test_short13_two_faults():
    """a bad literal and another fault in one document: the literal's code wins in 62,258 documents, another code in 162,788"""
    docs = G.family("short13")
    errors, _ = G.answers("short13")
    two = G.two_faults(docs, errors)
    literal = (errors == 21) | (errors == 22)
    assert int((two & literal).sum()) == 62258 and int((two & ~literal).sum()) == 162788
    assert not (two & (errors == 0)).any()


@pytest.mark.parametrize("max_depth,hist,upto5", [
    (2, {0: 36, 10: 59049, 11: 59049, 12: 5740, 13: 729, 14: 3, 15: 22, 16: 2120, 17: 201232, 18: 268363, 28: 1527}, 165),
    (3, {0: 41, 10: 59049, 11: 59049, 12: 6411, 13: 814, 14: 3, 15: 26, 16: 2399, 17: 201235, 18: 268674, 28: 169}, 17)])
def test_short9_under_a_depth_limit(max_depth, hist, upto5):
    errors, parsed = G.answers("short9", max_depth)
    assert G.histogram(errors) == hist
    assert int((errors[:G.SHORT9_UP_TO_5] == 28).sum()) == upto5
    docs = G.family("short9")
    for k in np.nonzero(errors == 28)[0][::97]:
        assert O.parse(docs[k] + b"\n", max_depth=max_depth).error == 28 and O.parse(docs[k] + b"\n").error != 28


def test_edits():
    docs = G.family("edits")
    errors, parsed = G.answers("edits")
    sizes = [len(G.edits_of(G.edit_base(u))) for u in G.EDIT_UNITS]
    assert [len(G.edit_base(u)) for u in G.EDIT_UNITS] == [31, 61, 91, 151]
    assert sizes == [826, 1613, 2400, 3974] and len(docs) == sum(sizes) == errors.size
    assert G.histogram(errors[-3974:]) == EDITS_5_UNITS
    for u in G.EDIT_UNITS:
        assert O.parse(b" ".join(G.edit_base(u)) + b"\n").error == 0
    # the kept edits give the tape comparison something to compare: more than a hundred documents of 150 tokens
    assert sum(1 for k in parsed if k >= len(docs) - 3974) == 140 and len(parsed) >= 300


def test_predicted_lengths_equal_the_plain_form():
    for name, stride in (("short9", 1009), ("short13", 811), ("short12s", 13), ("edits", 7)):
        docs = G.family(name)
        got = G.predicted_lengths(docs, G.answers(name)[0])
        assert got.size == len(docs)
        for k in range(0, len(docs), stride):
            want = predicted_length(docs[k] + b"\n")
            assert int(got[k]) == (-1 if want is None else want), (name, k, docs[k])
    few = G.family("short12s")[::29]
    assert np.array_equal(G.predicted_lengths(few), G.predicted_lengths(G.family("short12s"), G.answers("short12s")[0])[::29])


def test_shuffled_and_pack():
    docs = G.family("short12s")
    perm, moved = G.shuffled(docs, 5)
    assert sorted(perm.tolist()) == list(range(len(docs))) and moved == [docs[i] for i in perm] and moved != docs
    assert np.array_equal(perm, G.shuffled(docs, 5)[0]) and not np.array_equal(perm, G.shuffled(docs, 6)[0])
    buf, offs = G.pack(moved)
    assert buf == b"".join(d + b"\n" for d in moved) and offs[0] == 0 and int(offs[-1]) == len(buf)
    assert all(buf[int(offs[k]):int(offs[k + 1])] == moved[k] + b"\n" for k in range(0, len(moved), 101))
