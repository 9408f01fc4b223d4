"""The conditions of the corpus of tests/stream_fuzz.py, asserted on the CPU with oracle.stage1 on the whole document as the only
truth: what tests/test_gpu_stream_fuzz.py can notice depends on them, so a change of a seed or a size that loses one fails here.
Prints the statistics (pytest -s shows them; profiles/r11/README.md records them)."""
from oracle import oracle as O
from tests import stream_fuzz as F


def test_the_corpus_covers_what_it_claims():
    st = F.statistics()
    print()
    print(F.format_statistics(st))
    docs = F.corpus()
    assert all(256 <= len(d) <= F.MAX_DOC for d in docs)
    # (a) every hazard class meets a chunk edge at every one of its split positions in some (document, chunking)
    assert not st["unmet"], st["unmet"]
    default = st["halo_64"]
    # (b) the keep copy's overlap branch: a chunk shorter than the bytes kept in front of it, in at least 30 % of the pairs
    assert default["short_pairs"] >= 0.30 * st["pairs"], (default["short_pairs"], st["pairs"])
    assert default["overlap_pairs"] >= default["short_pairs"]
    assert default["have_eq_keep"] > 0 and default["have_grows_in_steps"] > 0
    # (c) every escalation depth: 64 -> 256 -> 1024 -> 4096
    assert set(default["depths"]) == {0, 1, 2, 3}, default["depths"]
    # (d) a run that fills everything that is kept: resolved because the halo reaches offset 0, and reported
    for halo in F.STREAM_HALOS:
        h = st["halo_%d" % (halo or 64)]
        assert h["filled_from_start"] > 0, halo
        assert (h["filled_reported"] > 0) == ((halo or 64) < 8192), halo  # (the longest run, 4200 bytes, fits into 8 KiB of halo)
    # (e) every verdict the classes can produce
    assert set(st["status_counts"]) == set(range(8)), st["status_counts"]
    # (f) neither mostly valid nor mostly broken
    assert 0.25 * st["documents"] <= st["accepted"] <= 0.75 * st["documents"], (st["accepted"], st["documents"])
    # every last length of the issue occurs, and one test function stays at about 3,000 pushes
    assert set(st["last_lengths"]) == set(F.LAST_LENGTHS) | {"rest"}, st["last_lengths"]
    assert min(st["last_lengths"].values()) >= 20, st["last_lengths"]
    assert max(st["slice_pushes"]) <= 3300, st["slice_pushes"]
    assert st["split_shards_reporting_halo"] > 0


def test_the_hazards_are_what_their_classes_say():
    """spot checks of the generator against the oracle: the filler alone is clean, and a class that must break a document does"""
    import random
    b = F._Builder(random.Random(5), "filler")
    for n in (0, 5, 8, 9, 63, 64, 65, 700, 5000):
        b.fill(n)
    assert O.stage1(bytes(b.buf))[1] == 0
    by_name = {d.name: d for d in F.corpus()}
    for name, d in by_name.items():
        st = O.stage1(d.data)[1]
        if name.startswith("utf8_mid:") or name.startswith("utf8_end:"):
            assert st & O.ST_UTF8 and not st & O.ST_UNESCAPED, (name, st)
        elif name.startswith("ctrl_in_string"):
            assert st == O.ST_UNESCAPED, (name, st)
        elif name.startswith("lone_quote") or name == "one_string":
            assert st == O.ST_UNCLOSED, (name, st)
        elif name.startswith("combo_"):
            assert st == int(name[6:]), (name, st)
        elif name.startswith("valid_") or name.startswith("leading_run"):
            assert st == 0, (name, st)
        elif name.startswith("bsrun_end"):
            assert st in (0, O.ST_UNCLOSED), (name, st)
    for d in by_name.values():
        for cls, key, edge in d.hazards:
            assert edge % 64 == 0 and 0 < edge <= len(d), (d.name, cls, key, edge)
            if cls.startswith("bsrun_") and cls != "bsrun_then_quote":  # the run ends exactly at the edge
                assert d.data[edge - key:edge] == b"\\" * key and (key == edge or d.data[edge - key - 1] != F.BS), (d.name, cls, key)
            if cls.startswith("utf8_mid:"):
                seq = next(s for n, s, _ in F.V.UTF8_INVALID_MID if "utf8_mid:" + n == cls)
                assert d.data[edge - key:edge - key + len(seq)] == seq, (d.name, cls, key)


def test_the_model_of_what_a_stream_keeps():
    """model_stream on hand-made streams: the figures follow from sjmi_stream_push's text, not from running it"""
    run = b"\\" * 4200 + b'"x"' + b" " * 21  # 4224 bytes
    # all 64-byte chunks, halo 64: every chunk inside the run has a filled halo; while the stream is shorter than 4 KiB the
    # escalation ends at the stream's first byte; the chunk at 4160 sees 4096 kept bytes of backslashes and no beginning
    m = F.model_stream(run, list(range(0, len(run) + 1, 64)), 0)
    assert [p["error"] for p in m] == [False] * 65 + [True] and m[-1]["a"] == 4160 and m[-1]["have"] == 4096
    assert [p["depth"] for p in m[:6]] == [0, 0, 1, 1, 1, 2] and all(p["from_start"] for p in m[:65])
    assert [p["have"] for p in m[:4]] == [0, 64, 128, 192] and all(p["overlap"] for p in m[1:65]) and not m[0]["overlap"]
    # 8 KiB of halo keep 8 KiB: the same stream is exact
    m = F.model_stream(run, list(range(0, len(run) + 1, 64)), 8192)
    assert len(m) == len(run) // 64 and not any(p["error"] for p in m) and all(p["from_start"] for p in m[:66])
    # a run of 64 in the middle: one step of escalation, and a quote as its last byte is the same
    for tail in (b"\\" * 64, b"\\" * 63 + b'"'):
        d = b" " * 4096 + b'"' + b"a" * 127 + tail + b'" '
        m = F.model_stream(d, [0, 4096, 4096 + 192, len(d)], 0)
        assert [(p["depth"], p["h"], p["error"]) for p in m] == [(0, 0, False), (0, 64, False), (1, 256, False)]
    assert F.halo_filled(b"x" + b"\\" * 64, 65, 64) and not F.halo_filled(b"xx" + b"\\" * 63 + b"a", 66, 64)
