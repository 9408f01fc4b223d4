"""Single documents for sjmi_parse_document at every switch of its device walk, and a restatement of that dispatch in plain
Python (no import of the product: the constants are compared with the sources by tests/test_single_doc_layouts.py).

How one document is walked depends on its BYTE length (coop_walk_launch, csrc/coop_walk.hip: only the single-wave sweep below
COOP_CHUNK_MIN bytes, the chunk kernels with the sweep queued behind them below COOP_OPTIMISTIC_MIN, from there on the chunk
kernels alone and a second round trip for a document they decline), on its STRUCTURAL count (at most CW_SINGLE_N: the sweep
after all; chunks of 128 structurals up to CW_SMALL_N, of 512 beyond; groups of 8 .. 64 chunks) and on its DEPTH profile (a
chunk that leaves its window of relative levels, a chunk end at 64 levels or more, 64 levels reached inside a chunk only).
FAMILIES builds documents on both sides of each switch; every Member says in its name how many structurals and bytes it has
and carries the cell of the dispatch it was built for.  tests/test_single_doc_layouts.py holds the corpus to that with the
oracle alone, tests/test_gpu_single_doc_layouts.py sends every member through sjmi_parse_document."""
from collections import namedtuple

# ---- the switches (csrc/coop_walk.hip) -----------------------------------------------------------------------------------
COOP_CHUNK_MIN = 1536        # bytes + 1 above it: the chunk kernels run
COOP_OPTIMISTIC_MIN = 16384  # bytes + 1 above it: k_chunk_finish ends the call, the sweep is queued after a round trip
CW_SINGLE_N = 512            # at most this many structurals: "a short document after all"
CW_SMALL_N = 256 << 10       # at most this many structurals: chunks of 128, else of 512
CW_GROUP_BIAS = 4            # SJMI_CW_GROUP_BIAS: groups of g chunks while g * g * bias < chunks
CW_BIAS = 32                 # relative level of a chunk's first structural
CW_LEVELS = 64               # levels of the register stack
CONSTANTS = ("COOP_CHUNK_MIN", "COOP_OPTIMISTIC_MIN", "CW_SINGLE_N", "CW_SMALL_N", "CW_GROUP_BIAS", "CW_BIAS", "CW_LEVELS")

BANDS = ("sweep", "queued", "optimistic")
PATHS = ("sweep", "short", "chunks", "swing", "deep_end", "spike")


def band(length):
    if length + 1 <= COOP_CHUNK_MIN:
        return "sweep"
    return "queued" if length + 1 <= COOP_OPTIMISTIC_MIN else "optimistic"


def chunk_of(n):
    return 128 if n <= CW_SMALL_N else 512


def group_of(nchunks):
    g = 8
    while g * g * CW_GROUP_BIAS < nchunks:
        g <<= 1
    return g


def nchunks_of(n):
    return (n + chunk_of(n) - 1) // chunk_of(n)


Profile = namedtuple("Profile", "swing deep_end max_depth group_window group_end_deep")


def profile(structural_bytes):
    """A plain loop over the structurals' first bytes, chunk by chunk as k_chunk_summary and the scan see them: swing = some
    chunk is out of range (relative to CW_BIAS at its start an opening bracket would sit at relative level >= CW_LEVELS, or
    some structural's container level would be < 0), deep_end = the depth at some chunk's end is >= CW_LEVELS, max_depth = the
    most containers open at once.  Two more, for the members that are to stay on the chunk path: group_window = k_group_summary's
    conditions (inside a group of chunks, relative to CW_BIAS at the group's start: a chunk end at relative level >= CW_LEVELS,
    a depth below relative level 1), group_end_deep = the depth at some GROUP's end is >= CW_LEVELS (k_top_scan)."""
    sb = bytes(structural_bytes)
    n = len(sb)
    chunk = chunk_of(n)
    g = group_of(nchunks_of(n))
    swing = deep_end = group_window = group_end_deep = False
    depth = max_depth = 0
    for k, a in enumerate(range(0, n, chunk)):
        if k % g == 0:
            group_rel = CW_BIAS
        h = CW_BIAS
        min_after = 0
        for c in sb[a:a + chunk]:
            if c == 0x5B or c == 0x7B:
                if h < 1 or h >= CW_LEVELS:
                    swing = True
                h += 1
                if depth + h - CW_BIAS > max_depth:
                    max_depth = depth + h - CW_BIAS
            else:
                if h < 1:
                    swing = True
                if c == 0x5D or c == 0x7D:
                    h -= 1
            if h - CW_BIAS < min_after:
                min_after = h - CW_BIAS
        if group_rel + min_after < 1 or group_rel + h - CW_BIAS >= CW_LEVELS:
            group_window = True
        group_rel = max(0, group_rel + h - CW_BIAS)
        depth = max(0, depth + h - CW_BIAS)
        if depth >= CW_LEVELS:
            deep_end = True
            if k % g == g - 1 or a + chunk >= n:
                group_end_deep = True
    return Profile(swing, deep_end, max_depth, group_window, group_end_deep)


def path(structural_bytes, length):
    """which way a document of these structurals and this byte length takes through coop_walk_launch"""
    if band(length) == "sweep":
        return "sweep"
    if len(structural_bytes) <= CW_SINGLE_N:
        return "short"
    p = profile(structural_bytes)
    if p.swing:
        return "swing"
    if p.deep_end:
        return "deep_end"
    return "spike" if p.max_depth >= CW_LEVELS else "chunks"


# ---- documents from tokens -------------------------------------------------------------------------------------------------
# A document is a list of tokens, ONE structural each; two scalars in a row are kept apart by a space (a scalar directly behind
# a scalar is no structural), everything else abuts: n structurals = n tokens, and the token at index i is structural i.
Member = namedtuple("Member", "name doc n cell kind family")  # kind: "valid" | "error" | "stage1"
OPS = "[]{},:"
UNIT = '{"k":"v\\n","e":[],"o":{},"n":[1,{"x":null}]},'
UNIT_TOKENS = ["{", '"k"', ":", '"v\\n"', ",", '"e"', ":", "[", "]", ",", '"o"', ":", "{", "}", ",", '"n"', ":", "[", "1", ",", "{", '"x"', ":",
               "null", "}", "]", "}", ","]
assert "".join(UNIT_TOKENS) == UNIT and len(UNIT_TOKENS) == 28


def join(tokens):
    out = []
    prev_scalar = False
    for t in tokens:
        scalar = t[0] not in OPS
        if scalar and prev_scalar:
            out.append(" ")
        out.append(t)
        prev_scalar = scalar
    return "".join(out).encode()


def pad_to(doc, length, at=1):
    """whitespace between two structurals (in front of byte `at`) up to `length` bytes; None if the document is longer"""
    if len(doc) > length:
        return None
    return doc[:at] + b" " * (length - len(doc)) + doc[at:]


def member(family, what, doc, n, cell, kind):
    return Member("%s/%s/n%d/len%d" % (family, what, n, len(doc)), doc, n, cell, kind, family)


def simple_cell(n, length):
    """the cell of a document whose depth stays within a few levels"""
    return "sweep" if band(length) == "sweep" else ("short" if n <= CW_SINGLE_N else "chunks")


def flat_prefix(t):
    """t tokens of a flat array, the last one a comma (or the root's bracket): a value is due next.  t odd, or even and >= 4."""
    assert t >= 1 and (t % 2 == 1 or t >= 4), t
    return ["["] + (["[", "]", ","] if t % 2 == 0 else []) + ["0", ","] * ((t - (4 if t % 2 == 0 else 1)) // 2)


def flat_close(tokens, n):
    """continues a flat array (a value is due) to exactly n tokens, the root's closing bracket last"""
    room = n - len(tokens)
    assert room >= 2, (len(tokens), n)
    if room % 2:
        assert room >= 5, (len(tokens), n)
        tokens = tokens + ["[", "]", ","]
        room -= 3
    return tokens + ["0", ","] * ((room - 2) // 2) + ["0", "]"]


def with_structurals(s):
    """tests/test_gpu_coop_walk.py's flat document: "[0,0,...,0]" has 2k + 3 structurals; one "[]," in front adds 3"""
    even = s % 2 == 0
    k = (s - 3 - (3 if even else 0)) // 2
    return ("[" + ("[]," if even else "") + "0," * k + "0]").encode()


def unit_prefix(shift):
    """`shift` structurals in front of the units: "0," pairs, and one "[]," for an odd shift"""
    assert shift == 0 or shift >= 2
    return ("[]," if shift % 2 else "") + "0," * ((shift - (3 if shift % 2 else 0)) // 2)


def structured(s):
    """exactly s structurals: "[" + prefix + UNIT * k + "0]" """
    k = (s - 3) // 28
    p = s - 3 - 28 * k
    if p == 1:
        k, p = k - 1, p + 28
    assert k >= 1
    return ("[" + unit_prefix(p) + UNIT * k + "0]").encode()


# ---- counts ------------------------------------------------------------------------------------------------------------
COUNTS = [511, 512, 513, 514, 639, 640, 641, 768, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769, 131071, 131072, 131073,
          262143, 262144, 262145, 262144 + 511, 262144 + 512, 262144 + 513, 524287, 524288, 524289]
FORMS = ("plain", "unclosed", "trailing")


def _form(d, s, form):
    """-> (document, structurals, valid)"""
    if form == "plain":
        return d, s, "valid"
    return (d[:-1], s - 1, "error") if form == "unclosed" else (d + b" 7", s + 1, "error")


def counts():
    """Documents with EXACTLY s structurals, flat and built from UNIT (keys, an escaped string, both empty pairs, nesting: all of
    them straddle chunk edges); each also unclosed and with trailing content.  The eight largest counts take the structured
    flavour in its plain form only."""
    out = []
    for s in COUNTS:
        for flavour, build in (("flat", with_structurals), ("structured", structured)):
            for form in FORMS:
                if flavour == "structured" and form != "plain" and s in COUNTS[-8:]:
                    continue
                d, n, kind = _form(build(s), s, form)
                out.append(member("counts", "%s/s%d/%s" % (flavour, s, form), d, n, simple_cell(n, len(d)), kind))
    return out


# ---- phases ------------------------------------------------------------------------------------------------------------
PHASE_SHIFTS = (0, 2, 3, 5)
PHASE_UNITS = (50, 9400)  # ~1,400 structurals: chunks of 128; ~263,200: chunks of 512


def phase_first_structural(shift, j):
    """index of the first structural of unit j"""
    return 1 + shift + 28 * j


def phases():
    out = []
    for k in PHASE_UNITS:
        for shift in PHASE_SHIFTS:
            d = ("[" + unit_prefix(shift) + UNIT * k + "0]").encode()
            n = 1 + shift + 28 * k + 2
            out.append(member("phases", "units%d/shift%d" % (k, shift), d, n, simple_cell(n, len(d)), "valid"))
    return out


# ---- edge_pairs ----------------------------------------------------------------------------------------------------------
# (name, tokens in front, the pair, tokens behind, kind): after a flat prefix a value is due; `behind` leaves one due again
_IN_OBJECT = ["{", '"a"', ":", "1"]
PAIRS = [
    ("empty_array", [], ["[", "]"], [","], "valid"),
    ("empty_object", [], ["{", "}"], [","], "valid"),
    ("key_colon", ["{"], ['"k"', ":"], ["1", "}", ","], "valid"),
    ("comma_key", _IN_OBJECT, [",", '"k"'], [":", "2", "}", ","], "valid"),
    ("colon_value", ["{", '"k"'], [":", "1"], ["}", ","], "valid"),
    ("no_comma", [], ["1", "1"], [","], "error"),
    ("missing_colon", ["{"], ['"k"', "1"], ["}", ","], "error"),
    ("no_key", [], ["{", "1"], ["}", ","], "error"),
    ("comma_close_array", ["[", "1"], [",", "]"], [","], "error"),
    ("comma_close_object", _IN_OBJECT, [",", "}"], [","], "error"),
    ("wrong_close", [], ["[", "}"], [","], "error"),
    ("key_missing", _IN_OBJECT, [",", "1"], ["}", ","], "error"),
]
LARGE_PAIRS = ("no_comma", "missing_colon", "comma_close_array", "wrong_close")
EDGE_N = 1300                 # structurals of the small members: the last chunk edge is 1280
EDGE_SMALL = (128, 512, 1280)
EDGE_LARGE = (512 * 300, CW_SMALL_N + 1000)  # (edge, structurals)
EDGE_LENGTHS = (2048, 16384)  # the queued and the optimistic band


def edge_pair_tokens(front, pair, behind, e, n):
    """a flat array of n structurals in which structurals e - 1 and e are `pair`"""
    tokens = flat_prefix(e - 1 - len(front)) + front + pair + behind
    assert tokens[e - 1:e + 1] == pair
    return flat_close(tokens, n)


def root_close_tokens(e, n, last_of_chunk):
    """the root's closing bracket as structural e - 1 with trailing content from e on (last_of_chunk), or as structural e: the
    document's last one (n == e + 1), or with trailing content behind it"""
    at = e - 1 if last_of_chunk else e
    tokens = flat_prefix(at - 1) + ["0", "]"]
    assert tokens[at] == "]" and len(tokens) == at + 1
    if n == len(tokens):
        return tokens
    # (behind the root's end: a scalar, then what keeps the document's last structural the root's kind of closing bracket)
    tokens = tokens + ["7", ","]
    room = n - len(tokens)
    if room % 2 == 0:
        tokens, room = tokens + ["7"], room - 1
    return tokens + ["0", ","] * ((room - 1) // 2) + ["]"]


def edge_pairs():
    out = []

    def add(what, tokens, kind, lengths):
        for length in lengths:
            d = join(tokens)
            d = pad_to(d, length) if length else d
            out.append(member("edge_pairs", what, d, len(tokens), simple_cell(len(tokens), len(d)), kind))
    for e in EDGE_SMALL:
        for name, front, pair, behind, kind in PAIRS:
            add("%s/e%d" % (name, e), edge_pair_tokens(front, pair, behind, e, EDGE_N), kind, EDGE_LENGTHS)
        add("root_close_last_then_trailing/e%d" % e, root_close_tokens(e, EDGE_N, True), "error", EDGE_LENGTHS)
        add("root_close_first_then_trailing/e%d" % e, root_close_tokens(e, EDGE_N, False), "error", EDGE_LENGTHS)
        add("root_close_first_ends/e%d" % e, root_close_tokens(e, e + 1, False), "valid", EDGE_LENGTHS)
    e, n = EDGE_LARGE
    for name, front, pair, behind, kind in PAIRS:
        if name in LARGE_PAIRS:
            add("%s/e%d" % (name, e), edge_pair_tokens(front, pair, behind, e, n), kind, (0,))
    return out


# ---- two_errors ------------------------------------------------------------------------------------------------------------
# a grammar error of its own code each, as tokens that take a due value and leave one due
ERRORS = {
    "no_comma": ["1", "1", ","],                 # NO_COMMA_ARRAY at the second scalar
    "no_key": ["{", "1", "}", ","],              # OBJECT_NO_KEY
    "wrong_close": ["[", "}", ","],              # a bracket of the wrong kind
    "bad_escape": ['"\\q"', ","],                # StringParser: a malformed escape
}
TWO_ERROR_PAIRS = (("no_comma", "no_key"), ("no_key", "wrong_close"), ("bad_escape", "no_comma"), ("bad_escape", "wrong_close"))


def two_error_tokens(first, at_first, second, at_second, n):
    tokens = flat_prefix(at_first | 1) + ERRORS[first]
    fill = at_second - len(tokens)
    assert fill >= 3
    if fill % 2:
        tokens, fill = tokens + ["[", "]", ","], fill - 3
    return flat_close(tokens + ["0", ","] * (fill // 2) + ERRORS[second], n)


def two_errors():
    """Two different errors in two different chunks, each pair in both orders (the first by POSITION wins); in neighbouring
    chunks, in chunks that k_chunk_finish's lanes 2 and 1 look at (chunks 2 and 65), a malformed escape in front of and behind
    a grammar error, and an error at the last structural of a chunk with another at the first structural of the next."""
    out = []
    for a, b in TWO_ERROR_PAIRS:
        for x, y in ((a, b), (b, a)):
            for what, p, q, n, lengths in (("near", 128 * 2 + 40, 128 * 7 + 9, 1300, EDGE_LENGTHS), ("lanes", 128 * 2 + 40, 128 * 65 + 9, 128 * 70 + 5, (0, 20000))):
                t = two_error_tokens(x, p, y, q, n)
                for length in lengths:
                    d = join(t)
                    d = pad_to(d, length) if length else d
                    out.append(member("two_errors", "%s/%s_then_%s" % (what, x, y), d, n, simple_cell(n, len(d)), "error"))
    # structural e - 1 fails (a scalar where an object wants a key) and structural e fails as well (no comma behind it)
    for e in (512, 1280):
        t = flat_close(flat_prefix(e - 2) + ["{", "1", "1", "}", ","], EDGE_N)
        assert t[e - 2:e + 1] == ["{", "1", "1"]
        for length in EDGE_LENGTHS:
            d = pad_to(join(t), length)
            out.append(member("two_errors", "abutting/e%d" % e, d, EDGE_N, simple_cell(EDGE_N, len(d)), "error"))
    return out


def two_error_partner(name):
    """the member with the same two errors in the other order, or None"""
    head, _, tail = name.partition("_then_")
    if not tail:
        return None
    what, x = head.rsplit("/", 1)
    y, rest = tail.split("/", 1)
    return "%s/%s_then_%s/%s" % (what, y, x, rest)


# ---- bands -----------------------------------------------------------------------------------------------------------------
BAND_LENGTHS = (1535, 1536, 16383, 16384)
STEP = ["0", ",", "0", ",", "["]  # one level of a staircase: 5 structurals, fewer than 32 levels per chunk of 128
LEVEL = ["0", ","] * 20 + ["["]   # one level of a slow one: 41 structurals, fewer than 32 levels per group of 8 chunks
LEVEL_DOWN = ["]"] + [",", "0"] * 20


def stairs(depth, top, behind=()):
    """climbs to `depth` open containers one STEP at a time, `top` at the top, and comes back the same way"""
    return ["["] + STEP * (depth - 1) + list(top) + ["]", ",", "0", ",", "0"] * (depth - 1) + list(behind) + ["]"]


def spike_tokens(base, peak):
    """climbs slowly to `base` levels, idles to the 40th structural of a chunk, then opens up to `peak` levels and closes them at
    once: no chunk is out of range, no group of chunks either, and every chunk ends at `base` levels or fewer"""
    up = ["["] + LEVEL * (base - 1)
    idle = ["0", ","] * ((128 - len(up) % 128 + 40) // 2)
    return up + idle + ["["] * (peak - base) + ["7"] + ["]"] * (peak - base) + [",", "0"] * 20 + LEVEL_DOWN * (base - 1) + ["]"]


def deep_mid_group_tokens(base, peak):
    """climbs slowly to `base` levels, then -- from the second chunk of a group of 8 on -- to `peak` levels STEP by STEP, stays
    there over two chunk edges and is back at `base` levels well in front of the group's end: chunks END at `peak` >= CW_LEVELS
    levels, yet no chunk and no group of chunks leaves its window and every group ends below CW_LEVELS"""
    up = ["["] + LEVEL * (base - 1)
    idle = ["0", ","] * ((1024 - len(up) % 1024 + 128) // 2)
    return (up + idle + STEP * (peak - base) + ["0", ","] * 100 + ["0"] + ["]", ",", "0", ",", "0"] * (peak - base) + [",", "0"] * 20 +
            LEVEL_DOWN * (base - 1) + ["]"])


def _band_kinds():
    """name -> (tokens or bytes, cell beyond the sweep band, kind, where padding goes)"""
    flat = flat_close(["["], 601)
    k = {}
    k["chunks_flat"] = (flat, "chunks", "valid")
    k["chunks_units"] = (["["] + UNIT_TOKENS * 20 + ["0", "]"], "chunks", "valid")
    k["short_few"] = (flat_close(["["], 401), "short", "valid")
    k["swing_opens"] = (flat_close(flat_prefix(301) + ["["] * 40 + ["7"] + ["]"] * 40 + [","], 701), "swing", "valid")
    k["swing_closes"] = (["["] + STEP * 40 + ["0", ","] * 30 + ["7"] + ["]"] * 40 + [",", "0"] * 150 + ["]"], "swing", "valid")
    k["swing_stray_closes"] = (flat + ["]"] * 40, "swing", "error")
    k["deep_end_70"] = (stairs(70, ["0", ","] * 70 + ["7"]), "deep_end", "valid")
    k["deep_end_1000"] = (stairs(1000, ["7"]), "deep_end", "valid")
    k["deep_end_mid_group"] = (deep_mid_group_tokens(50, 70), "deep_end", "valid")
    k["spike_64"] = (spike_tokens(50, 64), "spike", "valid")
    k["spike_71"] = (spike_tokens(50, 71), "spike", "valid")
    k["control_63"] = (spike_tokens(50, 63), "chunks", "valid")
    k["error_last_chunk"] = (flat[:-4] + ["0", "0", ",", "0", "]"], "chunks", "error")
    return k


# What 1,535 and 1,536 bytes cannot hold: the staircase to 1,000 levels (9,993 structurals), and whatever has to climb SLOWLY --
# fewer than 32 levels per group of 8 chunks, or the group summaries decline the document before a chunk walker sees it: the
# spikes and their control (4,100 structurals and more) and the deep chunk ends in the middle of a group.
BAND_LEFT_OUT = [(length, what) for length in (1535, 1536)
                 for what in ("deep_end_1000", "deep_end_mid_group", "spike_64", "spike_71", "control_63")]


def bands():
    out = []
    kinds = _band_kinds()
    for length in BAND_LENGTHS:
        sweep = band(length) == "sweep"
        for what, (tokens, cell, kind) in kinds.items():
            d = pad_to(join(tokens), length)
            if d is None:
                assert (length, what) in BAND_LEFT_OUT, (length, what)
                continue
            assert (length, what) not in BAND_LEFT_OUT
            out.append(member("bands", what, d, len(tokens), "sweep" if sweep else cell, kind))
        # a few structurals around one long string; one structural; none at all
        few = b'{"k":"' + b"x" * (length - 29) + b'","n":[1,2,{"a":null}]}'
        one = b'"' + b"z" * (length - 2) + b'"'
        for what, d, n, kind in (("short_long_string", few, 19, "valid"), ("short_one", one, 1, "valid"), ("short_none", b" " * length, 0, "error")):
            assert len(d) == length
            out.append(member("bands", what, d, n, "sweep" if sweep else "short", kind))
        # stage 1 fails: a byte that is no UTF-8 inside a string, a string that never closes (its quote is the last structural)
        flat = join(flat_close(["["], 601))
        utf8 = pad_to(flat[:-1] + b',"\xff"]', length)
        unclosed = pad_to(flat[:-1] + b',"abc', length)
        out.append(member("bands", "stage1_utf8", utf8, 603, "sweep" if sweep else "chunks", "stage1"))
        out.append(member("bands", "stage1_unclosed_string", unclosed, 602, "sweep" if sweep else "chunks", "stage1"))
    return out


def poison_documents():
    """documents of the optimistic band, parsed in front of a member: one that fails UTF-8 validation, one that falls back"""
    flat = join(flat_close(["["], 601))
    swing = join(_band_kinds()["swing_opens"][0])
    return pad_to(flat[:-1] + b',"\xff"]', 17000), pad_to(swing, 17000)


FAMILIES = {"counts": counts, "phases": phases, "edge_pairs": edge_pairs, "two_errors": two_errors, "bands": bands}
_built = {}


def family(name):
    """the members of one family (built once: a later caller gets the same list and must leave it unchanged)"""
    if name not in _built:
        _built[name] = FAMILIES[name]()
        names = [m.name for m in _built[name]]
        assert len(set(names)) == len(names), "member names are not unique in %s" % name
    return _built[name]
