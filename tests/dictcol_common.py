"""What dictionary-encoding a string column must give (include/sjmi.h, sjmi_dictionary_column_device), in numpy, bytes and a
Python dict alone: shares no code with the product.  reference() is the expected encoding -- the dictionary in the order of
first occurrence, which is what a Python dict keeps --, check() compares everything a call wrote, and that it wrote nothing
else; dc_hash() restates the product's hash so that the tests can BUILD strings that collide in the table; the builders make
columns whose NULL rows carry value words that would be wild offsets.  Used by the host simulation's tests
(tests/test_host_dictcol.py) and the GPU tests (tests/test_gpu_dictcol.py)."""
import functools

import numpy as np

from tests import strcol_common as SC

STRING = SC.STRING
OVERFLOW, BYTES_OVERFLOW = 1, 2                        # SJMI_DICT_OVERFLOW, SJMI_DICT_BYTES_OVERFLOW
MAX_ENTRIES = 1 << 20                                  # SJMI_DICT_MAX_ENTRIES
CANARY = SC.CANARY
CANARY_WORD = SC.CANARY_WORD
CANARY_INDEX = 0x45C5C5C5                              # (positive as an int32: no entry number of these tests)
GUARD = 4                                              # canary entries in front of and behind every output
GUARD_BYTES = 37
ALL_NULL_TYPES = SC.NULL_TYPES + SC.OTHER_TYPES

M64 = (1 << 64) - 1
DC_SEED, DC_LEN_MUL, DC_MUL, DC_MIX_MUL = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x9FB21C651E98DF25, 0xD6E8FEB86659FD93


def dc_hash(s):
    """sj_dictcol.h dc_hash over the bytes s"""
    s = bytes(s)
    h = DC_SEED ^ (len(s) * DC_LEN_MUL & M64)
    for k in range(0, len(s), 8):
        h = ((h ^ int.from_bytes(s[k:k + 8], "little")) * DC_MUL) & M64
        h ^= h >> 29
    for _ in range(2):
        h ^= h >> 32
        h = (h * DC_MIX_MUL) & M64
    return h ^ (h >> 32)


def dc_hash_words(words, length):
    """dc_hash of many strings of ONE length <= 8 at once: words = their little-endian numbers (uint64 array)"""
    assert 0 < length <= 8
    with np.errstate(over="ignore"):
        h = (np.uint64(DC_SEED ^ (length * DC_LEN_MUL & M64)) ^ words) * np.uint64(DC_MUL)
        h ^= h >> np.uint64(29)
        for _ in range(2):
            h ^= h >> np.uint64(32)
            h *= np.uint64(DC_MIX_MUL)
        return h ^ (h >> np.uint64(32))


def slots_of(dict_capacity):
    s = 2
    while s < 2 * dict_capacity:
        s *= 2
    return s


def start_slot(s, slots):
    return dc_hash(s) & (slots - 1)


def tag(s):
    return dc_hash(s) >> 40


@functools.lru_cache(maxsize=None)
def strings_starting_at(slot, slots, count, length=5):
    """`count` different strings of `length` letters whose probe starts at `slot` of a table of `slots`"""
    rng = np.random.default_rng(slot * 1000 + slots)
    out = []
    while len(out) < count:
        s = bytes(rng.integers(97, 123, size=length, dtype=np.uint8))
        if start_slot(s, slots) == slot and s not in out:
            out.append(s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tag_twins(slots=64, length=6, last_byte_only=False):
    """two different strings of `length` bytes with the same start slot in a table of `slots` AND the same 24-bit tag: 30 equal
    bits, a birthday among 2^16 strings or so.  last_byte_only: they differ in their last byte alone (among the 256 endings
    of one prefix a pair is rare: many prefixes are tried, 2^23 hashes at once in numpy)."""
    rng = np.random.default_rng(length * 7 + last_byte_only)
    slot_bits = slots.bit_length() - 1
    for _ in range(200):
        if last_byte_only:
            prefixes = rng.integers(0, 1 << (8 * (length - 1)), size=1 << 15, dtype=np.uint64)
            words = (prefixes[:, None] | (np.arange(256, dtype=np.uint64) << np.uint64(8 * (length - 1)))[None, :]).reshape(-1)
            group = np.repeat(np.arange(prefixes.size, dtype=np.uint64), 256)
        else:
            words = np.unique(rng.integers(0, 1 << (8 * length), size=1 << 18, dtype=np.uint64))
            group = np.zeros(words.size, dtype=np.uint64)
        h = dc_hash_words(words, length)
        keys = (group << np.uint64(24 + slot_bits)) | ((h >> np.uint64(40)) << np.uint64(slot_bits)) | (h & np.uint64(slots - 1))
        order = np.argsort(keys)
        k, w = keys[order], words[order]
        hit = np.flatnonzero((k[1:] == k[:-1]) & (w[1:] != w[:-1]))
        if hit.size:
            a, b = (int(w[hit[0]]).to_bytes(8, "little")[:length], int(w[hit[0] + 1]).to_bytes(8, "little")[:length])
            assert a != b and start_slot(a, slots) == start_slot(b, slots) and tag(a) == tag(b)
            assert not last_byte_only or a[:-1] == b[:-1]
            return a, b
    raise AssertionError("no twins found")


# ---------------------------------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------------------------------
def column_of(rng, cells, sb_gap=3, place=None):
    """cells: bytes for a VALID row, None for a NULL row (a type drawn from every NULL type, a WILD value word).  Every
    occurrence gets bytes of its own in the string buffer, `sb_gap` random bytes apart at most; place = {row: offset modulo 8}
    puts that row's string at such an address.  -> (types uint8, values uint64, sb uint8)"""
    n = len(cells)
    types = np.empty(n, dtype=np.uint8)
    values = np.empty(n, dtype=np.uint64)
    sb = bytearray()
    for r, cell in enumerate(cells):
        if cell is None:
            types[r] = ALL_NULL_TYPES[int(rng.integers(0, len(ALL_NULL_TYPES)))]
            values[r] = SC.WILD[int(rng.integers(0, len(SC.WILD)))]
            continue
        sb += bytes(rng.integers(0, 256, size=int(rng.integers(0, sb_gap + 1)), dtype=np.uint8))
        if place and r in place:
            while len(sb) % 8 != place[r]:
                sb.append(0x7E)
        types[r] = STRING
        values[r] = (len(cell) << 32) | len(sb)
        sb += cell
    return types, values, np.frombuffer(bytes(sb) if sb else b"\0", dtype=np.uint8).copy()


def big_column(rng, n, vocabulary, p_null=0.1):
    """n rows drawn from `vocabulary` (a list of bytes) without a Python loop over the rows: the string buffer holds `copies` of
    every word at different alignments and a row points at one of them"""
    copies = 8
    sb = bytearray()
    where = np.empty((len(vocabulary), copies), dtype=np.uint64)
    for i, word in enumerate(vocabulary):
        for j in range(copies):
            sb += b"#" * ((i + j) % 3)
            where[i, j] = (len(word) << 32) | len(sb)
            sb += word
    pick = rng.integers(0, len(vocabulary), size=n)
    values = where[pick, rng.integers(0, copies, size=n)]
    pool = np.array(ALL_NULL_TYPES, dtype=np.uint8)
    null = rng.random(n) < p_null
    types = np.where(null, pool[rng.integers(0, pool.size, size=n)], np.uint8(STRING)).astype(np.uint8)
    wild = np.array(SC.WILD, dtype=np.uint64)[rng.integers(0, len(SC.WILD), size=n)]
    return types, np.where(null, wild, values), np.frombuffer(bytes(sb), dtype=np.uint8).copy()


def mixed_cells(rng, n, vocabulary, p_null=0.25):
    """n cells drawn from the vocabulary with NULL rows mixed in"""
    return [None if rng.random() < p_null else vocabulary[int(rng.integers(0, len(vocabulary)))] for _ in range(n)]


NINE = [b"", b"a", b"PushEvent", b"CreateEvent", b"en", b"ja", b"\xe6\x97\xa5\xe6\x9c\xac", b"a much longer value of forty bytes, here", b"PushEvenu"]


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
class Ref:
    pass


def reference(types, values, sb, live=None):
    """the encoding of rows [0, live): indices int32 [live], validity words, dict_rows, dict_offsets int64 [n_distinct + 1], the
    dictionary's bytes, n_valid, n_other"""
    types = np.asarray(types, dtype=np.uint8)
    values = np.asarray(values).view(np.uint64) if np.asarray(values).dtype == np.int64 else np.asarray(values, dtype=np.uint64)
    live = types.size if live is None else min(int(live), types.size)
    sb = bytes(np.asarray(sb, dtype=np.uint8))
    cells = []
    for r in range(live):
        if types[r] == STRING:
            v = int(values[r])
            assert (v & 0xFFFFFFFF) + (v >> 32) <= len(sb)
            cells.append(sb[v & 0xFFFFFFFF:(v & 0xFFFFFFFF) + (v >> 32)])
        else:
            cells.append(None)
    ref = reference_from_cells([(STRING if c is not None else int(types[r]), c) for r, c in enumerate(cells)])
    return ref


def contention_column(rng, n):
    """n rows over three values -- whole chunks and waves on three slots -- with the LAST row a fourth, new value: (types, values,
    sb, the reference).  The reference is made without a Python loop over the rows: the four values differ in length."""
    words = [b"PushEvent", b"en", b"a value of a little more than thirty-two bytes"]
    t, v, sb = big_column(rng, n, words, p_null=0.05)
    new = np.frombuffer(b"new in the last row", dtype=np.uint8)
    t[-1] = STRING
    v[-1] = (new.size << 32) | sb.size
    sb = np.concatenate([sb, new])
    valid = t == STRING
    _, first_index, inverse = np.unique(v[valid] >> np.uint64(32), return_index=True, return_inverse=True)
    order = np.argsort(first_index)
    rank = np.empty(order.size, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    ref = Ref()
    ref.live, ref.n_distinct, ref.n_valid = n, 4, int(valid.sum())
    ref.n_other = int(np.count_nonzero(~valid & (t != 0) & (t != ord("n"))))
    ref.indices = np.zeros(n, dtype=np.int32)
    ref.indices[valid] = rank[inverse]
    ref.dict_rows = np.flatnonzero(valid)[first_index[order]].astype(np.int64)
    ref.values = [bytes(sb[int(v[r]) & 0xFFFFFFFF:(int(v[r]) & 0xFFFFFFFF) + (int(v[r]) >> 32)]) for r in ref.dict_rows]
    assert sorted(ref.values) == sorted(words + [bytes(new)]) and ref.dict_rows[-1] == n - 1
    ref.dict_bytes = b"".join(ref.values)
    ref.dict_offsets = np.cumsum([0] + [len(e) for e in ref.values]).astype(np.int64)
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = valid
    ref.validity = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    return t, v, sb, ref


def reference_from_cells(cells):
    """the same from [(type byte, payload)] (tests/select_common.expected_columns), the payload of a string its bytes"""
    ref = Ref()
    n = len(cells)
    entries = {}
    ref.indices = np.zeros(n, dtype=np.int32)
    valid = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    rows = []
    for r, (t, payload) in enumerate(cells):
        if t != STRING:
            continue
        valid[r] = 1
        payload = bytes(payload)
        if payload not in entries:
            entries[payload] = len(entries)
            rows.append(r)
        ref.indices[r] = entries[payload]
    ref.live = n
    ref.validity = np.packbits(valid, bitorder="little").view("<u8").astype(np.uint64)
    ref.dict_rows = np.array(rows, dtype=np.int64)
    ref.values = list(entries)
    ref.dict_offsets = np.zeros(len(entries) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in entries], out=ref.dict_offsets[1:])
    ref.dict_bytes = b"".join(entries)
    ref.n_valid = int(valid.sum())
    ref.n_other = sum(1 for t, _ in cells if t not in (STRING, SC.MISSING, ord("n")))
    ref.n_distinct = len(entries)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# outputs with canaries all around, and their check
# ---------------------------------------------------------------------------------------------------------------------
class Out:
    """the output arrays of one call: every one GUARD canary entries longer at both ends (the bytes: bytes_front canary bytes in
    front -- so that a caller can put d_dict_bytes that many bytes into an allocation -- and GUARD_BYTES behind); .indices,
    .validity, .dict_rows, .dict_offsets, .dict_bytes, .result are the views a call is given"""

    def __init__(self, n_rows, dict_capacity, byte_capacity, bytes_front=GUARD_BYTES):
        self.n_rows, self.dict_capacity, self.byte_capacity, self.bytes_front = n_rows, dict_capacity, byte_capacity, bytes_front
        self.indices_store = np.full(n_rows + 2 * GUARD, CANARY_INDEX, dtype=np.int32)
        self.validity_store = np.full((n_rows + 63) // 64 + 2 * GUARD, CANARY_WORD, dtype=np.uint64)
        self.dict_rows_store = np.full(dict_capacity + 2 * GUARD, CANARY_WORD, dtype=np.uint64)
        self.dict_offsets_store = np.full(dict_capacity + 1 + 2 * GUARD, CANARY_WORD, dtype=np.uint64)
        self.dict_bytes_store = np.full(bytes_front + byte_capacity + GUARD_BYTES, CANARY, dtype=np.uint8)
        self.result_store = np.full(6 + 2 * GUARD, CANARY_WORD, dtype=np.uint64)

    STORES = ("indices", "validity", "dict_rows", "dict_offsets", "dict_bytes", "result")

    def guard(self, name):
        """canary entries in front of the view"""
        return self.bytes_front if name == "dict_bytes" else GUARD

    def guard_behind(self, name):
        return GUARD_BYTES if name == "dict_bytes" else GUARD

    def view(self, name):
        store = getattr(self, name + "_store")
        return store[self.guard(name):store.size - self.guard_behind(name)]


def check(what, out, ref, dict_capacity, byte_capacity, validity=True, dict_rows=True):
    """out: an Out a call has filled (with validity / dict_rows False: the call got NULL for it); ref = reference(...) over the
    LIVE rows"""
    live, nd = ref.live, ref.n_distinct
    overflow = nd > dict_capacity
    r = out.view("result")
    got = dict(n_rows=int(r[0]), n_valid=int(r[1]), n_other=int(r[2]), n_distinct=int(r[3]), dict_bytes=int(r[4]), flags=int(r[5]) & 0xFFFFFFFF,
               reserved=int(r[5]) >> 32)
    print("%s: %r" % (what, got))
    assert (got["n_rows"], got["n_valid"], got["n_other"], got["reserved"]) == (live, ref.n_valid, ref.n_other, 0), (what, got)
    assert bool(got["flags"] & OVERFLOW) == overflow and not got["flags"] & ~(OVERFLOW | BYTES_OVERFLOW), (what, got)
    words = (live + 63) // 64
    if validity:
        assert np.array_equal(out.view("validity")[:words], ref.validity[:words]), "%s: validity differs" % what
    # canaries: in front of and behind every array, and inside it behind what the call owns
    for name in Out.STORES:
        store, g, b = getattr(out, name + "_store"), out.guard(name), out.guard_behind(name)
        canary = {"indices": CANARY_INDEX, "dict_bytes": CANARY}.get(name, CANARY_WORD)
        assert np.all(store[:g] == canary) and np.all(store[store.size - b:] == canary), "%s: written outside %s" % (what, name)
    assert np.all(out.view("indices")[live:] == CANARY_INDEX), "%s: an index at or above the live rows is written" % what
    assert np.all(out.view("validity")[words if validity else 0:] == CANARY_WORD), "%s: a validity word behind the live rows is written" % what
    if not dict_rows:
        assert np.all(out.view("dict_rows") == CANARY_WORD), "%s: dict_rows written without one" % what
    if overflow:
        assert got["n_distinct"] > dict_capacity, (what, got)
        assert np.all(out.view("dict_bytes") == CANARY), "%s: a dictionary byte is copied under OVERFLOW" % what
        return got
    assert got["n_distinct"] == nd and got["dict_bytes"] == len(ref.dict_bytes), (what, got)
    assert bool(got["flags"] & BYTES_OVERFLOW) == (len(ref.dict_bytes) > byte_capacity), (what, got)
    assert np.array_equal(out.view("indices")[:live], ref.indices), \
        "%s: indices differ first at row %d" % (what, int(np.flatnonzero(out.view("indices")[:live] != ref.indices)[0]))
    if dict_rows:
        assert np.array_equal(out.view("dict_rows")[:nd].view(np.int64), ref.dict_rows), "%s: dict_rows differ" % what
        assert np.all(out.view("dict_rows")[nd:] == CANARY_WORD), "%s: dict_rows written behind n_distinct" % what
    assert np.array_equal(out.view("dict_offsets")[:nd + 1].view(np.int64), ref.dict_offsets), "%s: dict_offsets differ" % what
    assert np.all(out.view("dict_offsets")[nd + 1:] == CANARY_WORD), "%s: dict_offsets written behind n_distinct" % what
    below = min(len(ref.dict_bytes), byte_capacity)
    assert bytes(out.view("dict_bytes")[:below]) == ref.dict_bytes[:below], "%s: the dictionary's bytes differ" % what
    assert np.all(out.view("dict_bytes")[below:] == CANARY), "%s: written at or behind the byte capacity, or behind the last byte" % what
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the shapes of the issue, shared by the host simulation's tests and the GPU tests: (name, cells, dict_capacity, place)
# ---------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)


def late_first_cells():
    """the first VALID row is row 1024 (chunk 1); values whose first rows are the last lane of a wave (1087) and the first lane
    of the next chunk (2048)"""
    cells = [None] * 2100
    cells[1024] = b"first"
    for r in range(1025, 2100):
        cells[r] = b"first" if r % 3 else None
    cells[1087] = b"last lane of a wave"
    cells[2048] = b"first lane of chunk 2"
    cells[2050] = b"last lane of a wave"
    cells[2099] = b"first lane of chunk 2"
    return cells


def uniform_cases():
    n = 1025
    return [("everything NULL", [None] * n, n), ("everything one value", [b"same"] * n, n), ("everything the empty string", [b""] * n, n),
            ("every row distinct", [b"row %d" % r for r in range(n)], n)]


def collision_cases():
    """dict_capacity 32 -> 64 slots.  -> [(name, cells, place)]"""
    out = []
    chain = list(strings_starting_at(17, 64, 12))
    out.append(("a probe chain of 12 from slot 17", chain * 3 + chain[::-1], None))
    wrap = list(strings_starting_at(63, 64, 9))
    out.append(("a chain from slot 63 that wraps to slot 0", wrap + wrap[::-1] + wrap, None))
    a, b = tag_twins(64, 6, False)
    out.append(("tag twins of one length", [a, b, b, a, None, a, b], None))
    c, d = tag_twins(64, 6, True)
    out.append(("tag twins that differ in the last byte", [c, d, d, c, None, d, c], None))
    out.append(("tag twins, one astride a word boundary at an odd offset", [c, d, d, c, None, d, c], {1: 5, 2: 3, 3: 7}))
    exact = list(strings_starting_at(5, 64, 8)) + [b"value %d" % k for k in range(24)]
    out.append(("32 values in 64 slots", exact + exact[::-1], None))
    return out
