"""What gathering a string column must give (include/sjmi.h, sjmi_string_column_device), in numpy and bytes alone: shares no
code with the product.  reference() is the expected column, check() compares everything a call wrote -- and that it wrote
nothing else --, the builders make synthetic columns whose NULL rows carry value words that would be wild offsets.  Used by the
host simulation's tests (tests/test_host_strcol.py) and the GPU tests (tests/test_gpu_strcol.py)."""
import numpy as np

STRING = ord('"')
MISSING = 0
NULL_TYPES = [MISSING, ord("n")]                       # NULL rows that are no schema mismatch
OTHER_TYPES = [ord(c) for c in "ldtf[{"]               # ... and those that are (n_other)
OVERFLOW = 1                                           # SJMI_STRCOL_OVERFLOW
CANARY = 0xC5
CANARY_WORD = 0xC5C5C5C5C5C5C5C5
CANARY_ENTRIES = 4                                     # canary entries behind offsets[n_rows] and behind the last validity word
CANARY_BYTES = 37                                      # ... and bytes behind byte_capacity
# value words of NULL rows: every one of them would be a wild offset or a wild length
WILD = [0xFFFFFFFFFFFFFFFF, (1 << 63) | 0, (1 << 31) << 32, ((1 << 31) << 32) | 0xFFFFFFF0, 0x00000001FFFFFFFF, 0xFFFFFFFF00000000]


def reference(types, values, sb):
    """-> (offsets int64 [n + 1], validity words uint64 [ceil(n / 64)], data bytes, n_valid, n_other)"""
    types = np.asarray(types, dtype=np.uint8)
    values = np.asarray(values).view(np.uint64) if np.asarray(values).dtype == np.int64 else np.asarray(values, dtype=np.uint64)
    n = types.size
    assert values.size == n
    valid = types == STRING
    lens = np.where(valid, values >> np.uint64(32), np.uint64(0)).astype(np.int64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = valid
    words = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    sb = memoryview(sb)
    data = b"".join(bytes(sb[int(v & 0xFFFFFFFF):int(v & 0xFFFFFFFF) + int(v >> 32)]) for v in (int(x) for x in values[valid]))
    assert len(data) == int(offsets[n])  # (no string of the column runs past the buffer)
    n_other = int(np.count_nonzero(~valid & (types != MISSING) & (types != ord("n"))))
    return offsets, words, data, int(np.count_nonzero(valid)), n_other


def reference_from_cells(cells):
    """the same from the cells of tests/select_common.expected_columns / explode_common.expected_explode: [(type byte, payload)],
    the payload of a string its bytes"""
    n = len(cells)
    valid = np.array([t == STRING for t, _ in cells], dtype=bool).reshape(n)
    lens = np.array([len(p) if t == STRING else 0 for t, p in cells], dtype=np.int64).reshape(n)
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    bits = np.zeros((n + 63) // 64 * 64, dtype=np.uint8)
    bits[:n] = valid
    words = np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)
    data = b"".join(p for t, p in cells if t == STRING)
    n_other = sum(1 for t, _ in cells if t not in (STRING, MISSING, ord("n")))
    return offsets, words, data, int(valid.sum()), n_other


def out_buffers(n_rows, byte_capacity, validity=True):
    """the output arrays of one call, canaries all over: (offsets uint64, validity uint64 or None, data uint8, result uint64 [4])"""
    offsets = np.full(n_rows + 1 + CANARY_ENTRIES, CANARY_WORD, dtype=np.uint64)
    words = np.full((n_rows + 63) // 64 + CANARY_ENTRIES, CANARY_WORD, dtype=np.uint64) if validity else None
    data = np.full(byte_capacity + CANARY_BYTES, CANARY, dtype=np.uint8)
    return offsets, words, data, np.full(4, CANARY_WORD, dtype=np.uint64)


def check(what, got_offsets, got_validity, got_data, got_result, ref, byte_capacity, canaries=True):
    """got_*: what a call left in out_buffers() (got_validity None: it was called without one); ref = reference(...).
    canaries=False: the arrays end where their contents end (tensors a wrapper allocated exactly)."""
    offsets, words, data, n_valid, n_other = ref
    n = offsets.size - 1
    got_offsets = np.asarray(got_offsets).view(np.uint64)
    assert np.array_equal(got_offsets[:n + 1].view(np.int64), offsets), \
        "%s: offsets differ first at row %d" % (what, int(np.flatnonzero(got_offsets[:n + 1].view(np.int64) != offsets)[0]))
    if got_validity is not None:
        got_validity = np.asarray(got_validity).view(np.uint64)
        assert np.array_equal(got_validity[:words.size], words), \
            "%s: validity differs first in word %d" % (what, int(np.flatnonzero(got_validity[:words.size] != words)[0]))
    total = len(data)
    below = min(total, byte_capacity)
    got_data = np.asarray(got_data, dtype=np.uint8)
    want = np.frombuffer(data, dtype=np.uint8)[:below]
    assert np.array_equal(got_data[:below], want), \
        "%s: bytes differ first at %d of %d (capacity %d)" % (what, int(np.flatnonzero(got_data[:below] != want)[0]), total, byte_capacity)
    r = np.asarray(got_result).view(np.uint64)
    got = (int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 0xFFFFFFFF, int(r[3]) >> 32)
    assert got == (total, n_valid, n_other, OVERFLOW if total > byte_capacity else 0, 0), (what, got, (total, n_valid, n_other))
    if canaries:
        assert got_offsets.size == n + 1 + CANARY_ENTRIES and np.all(got_offsets[n + 1:] == CANARY_WORD), "%s: written behind offsets[n_rows]" % what
        if got_validity is not None:
            assert got_validity.size == words.size + CANARY_ENTRIES and np.all(got_validity[words.size:] == CANARY_WORD), \
                "%s: written behind the last validity word" % what
        # bytes between the column's end and the capacity are not the column's: they stay as they were, too
        assert got_data.size == byte_capacity + CANARY_BYTES and np.all(got_data[below:] == CANARY), \
            "%s: written at or behind the capacity, or behind the column's last byte" % what


def capacities(total):
    """the byte capacities of the issue: total + 3, total, total - 1, the middle, 1 and the sizing call"""
    return sorted({total + 3, total, max(total - 1, 0), total // 2, 1, 0}, reverse=True)


# ---------------------------------------------------------------------------------------------------------------------
# builders of synthetic columns
# ---------------------------------------------------------------------------------------------------------------------
def string_buffer(rng, size):
    return rng.integers(0, 256, size=size, dtype=np.uint8)


def column(rng, kinds, lengths, sb_size, src_align=None, at_end=()):
    """kinds[r]: a type byte; lengths[r]: the length of a STRING row.  A STRING row's bytes lie at a random place of the buffer
    (src_align: at that alignment modulo 16; rows listed in at_end: so that they END the buffer); a NULL row gets a WILD value
    word.  -> (types uint8, values uint64)"""
    kinds = np.asarray(kinds, dtype=np.uint8)
    n = kinds.size
    values = np.empty(n, dtype=np.uint64)
    for r in range(n):
        if kinds[r] == STRING:
            ln = int(lengths[r])
            assert ln <= sb_size
            if r in at_end:
                off = sb_size - ln
            elif src_align is None:
                off = int(rng.integers(0, sb_size - ln + 1))
            else:
                assert src_align + ln <= sb_size
                off = src_align + 16 * int(rng.integers(0, (sb_size - ln - src_align) // 16 + 1))
            values[r] = (ln << 32) | off
        else:
            values[r] = WILD[int(rng.integers(0, len(WILD)))]
    return kinds, values


def random_kinds(rng, n, p_string=0.6):
    """rows drawn from STRING, MISSING, 'n' and the other types"""
    pool = np.array(NULL_TYPES + OTHER_TYPES, dtype=np.uint8)
    kinds = pool[rng.integers(0, pool.size, size=n)]
    kinds[rng.random(n) < p_string] = STRING
    return kinds


def big_column(rng, n, max_len, sb_size, p_string=0.6):
    """random_column without a Python loop over the rows (for a million of them)"""
    kinds = random_kinds(rng, n, p_string)
    lengths = rng.integers(0, max_len + 1, size=n).astype(np.uint64)
    offs = rng.integers(0, sb_size - max_len + 1, size=n).astype(np.uint64)
    wild = np.array(WILD, dtype=np.uint64)[rng.integers(0, len(WILD), size=n)]
    return kinds, np.where(kinds == STRING, (lengths << np.uint64(32)) | offs, wild)


def random_column(rng, n, max_len, sb_size=4096, p_string=0.6, src_align=None):
    kinds = random_kinds(rng, n, p_string)
    lengths = rng.integers(0, max_len + 1, size=n)
    return column(rng, kinds, lengths, sb_size, src_align)


EDGE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
LONG = 70000


def length_cases(rng, sb_size):
    """(name, types, values): every edge length and one long string, each among empty VALID rows, among NULL rows, and with 300
    short rows in front of it (so that a wave's span begins and ends inside a trip); the row also placed last and first"""
    out = []
    for ln in EDGE_LENGTHS + (LONG,):
        for name, front, back in (("among empty strings", [(STRING, 0)] * 70, [(STRING, 0)] * 70),
                                  ("among NULL rows", [(MISSING, 0), (ord("n"), 0), (ord("l"), 0)] * 23, [(ord("{"), 0), (MISSING, 0)] * 35),
                                  ("behind 300 short rows", [(STRING, 1 + k % 5) for k in range(300)], [(STRING, 2), (STRING, 0), (STRING, 3)]),
                                  ("first", [], [(STRING, 1)] * 3), ("last", [(STRING, 3)] * 65, [])):
            rows = front + [(STRING, ln)] + back
            kinds = [k for k, _ in rows]
            lengths = [l for _, l in rows]
            t, v = column(rng, kinds, lengths, sb_size, at_end=(len(front),))
            out.append(("length %d %s" % (ln, name), t, v))
    return out


def shape_cases(rng, sb_size):
    """an all-NULL column, an all-empty-but-VALID column, one VALID row at the very end"""
    out = []
    for n in (1, 64, 200):
        out.append(("all NULL, %d rows" % n,) + column(rng, random_kinds(rng, n, p_string=0.0), np.zeros(n, int), sb_size))
        out.append(("all empty but VALID, %d rows" % n,) + column(rng, [STRING] * n, np.zeros(n, int), sb_size))
        kinds = list(random_kinds(rng, n - 1, p_string=0.0)) + [STRING]
        out.append(("one VALID row at the very end, %d rows" % n,) + column(rng, kinds, [0] * (n - 1) + [77], sb_size, at_end=(n - 1,)))
    return out
