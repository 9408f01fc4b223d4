"""What the tests of the fixed-width Arrow column exports share (tests/arrowcol_common.py, tests/timecol_common.py): the cell
types, the CANARY-filled output buffers of a call and their comparison, the live rows of a case and the row counts and strides
the cases are made with.  A Case of either has fields, types, values, n_rows, row_count, data_stride, validity_stride; a Ref has
data / validity (per field the words the call owns) and records (per field a tuple of ints, the live rows first).  check()
compares everything a call owns word for word and everything it must not touch: the words between the live rows and the
stride, the slack between fields, the words in front of and behind both blocks."""
import numpy as np

MISSING, NULL, LONG, DOUBLE, TRUE, FALSE, STRING = 0, ord("n"), ord("l"), ord("d"), ord("t"), ord("f"), ord('"')
ALL_TYPES = [MISSING] + [ord(c) for c in 'nldtf"[{']
MASK = (1 << 64) - 1
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
CANARY_WORD = 0xC5C5C5C5C5C5C5C5
FRONT, BACK = 3, 5                                      # canary words in front of and behind each output block


def encode(fields, dtype, whats, flags):
    """tuples (column, what[, flag ...]) -> the 16-byte field array of `dtype`: the C form, for the host simulation"""
    enc = np.zeros(len(fields), dtype=dtype)
    for k, field in enumerate(fields):
        enc[k] = (field[0], whats[field[1]], sum(flags[f] for f in field[2:]), 0)
    return enc


def pack_bits(bits):
    return [sum(1 << t for t, b in enumerate(bits[w:w + 64]) if b) for w in range(0, len(bits), 64)]


def live_rows(case):
    return case.n_rows if case.row_count is None else min(case.n_rows, case.row_count)


def live_counts(n):
    """what *d_row_count holds, for n_rows = n: absent, 0, 1, n - 1, n, n + 5 (clamped) and a count that ends inside a wave of a
    middle chunk (of a middle wave, where there is but one chunk)"""
    inside = 1024 + 64 + 7 if n > 1100 else n // 128 * 64 + 7 if n >= 128 else None
    out = [None]
    for rc in (0, 1, n - 1, n, n + 5, inside):
        if rc is not None and rc >= 0 and rc not in out:
            out.append(rc)
    return out


def strides(n_rows, slack):
    """(data_stride, validity_stride) of a case; slack: how far they lie above their minimum (0: the minimum)"""
    return n_rows + (7 if slack else 0), (n_rows + 63) // 64 + (2 if slack else 0)


def out_buffers(case, record_words, data=True, validity=True):
    """the output arrays of one call, canaries all over: (data or None, validity or None, results), the blocks FRONT words
    behind the beginning of their arrays and BACK words in front of their ends"""
    n_fields = len(case.fields)
    d = np.full(FRONT + n_fields * case.data_stride + BACK, CANARY_WORD, dtype=np.uint64) if data else None
    b = np.full(FRONT + n_fields * case.validity_stride + BACK, CANARY_WORD, dtype=np.uint64) if validity else None
    return d, b, np.full(record_words * n_fields, CANARY_WORD, dtype=np.uint64)


def _expect(owned, n_fields, stride):
    want = np.full(FRONT + n_fields * stride + BACK, CANARY_WORD, dtype=np.uint64)
    for f, words in enumerate(owned):
        assert len(words) <= stride
        want[FRONT + f * stride:FRONT + f * stride + len(words)] = np.array(words, dtype=np.uint64)
    return want


def _same(what, block, got, want, stride):
    got = np.asarray(got).view(np.uint64).reshape(-1)
    assert got.size == want.size, (what, block, got.size, want.size)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        where = "in front of the block" if at < FRONT else "behind the block" if at >= want.size - BACK else \
            "field %d, word %d" % ((at - FRONT) // max(stride, 1), (at - FRONT) % max(stride, 1))
        raise AssertionError("%s: %s differs first at %s: got %#x, want %#x (%#x: not to be touched)" % (what, block, where, int(got[at]), int(want[at]), CANARY_WORD))


def check(what, got_data, got_validity, got_results, case, ref):
    """got_*: what a call left in out_buffers() (None: called without it), whole arrays with their canaries"""
    n_fields = len(case.fields)
    got = np.asarray(got_results).view(np.uint64).reshape(n_fields, len(ref.records[0])).tolist()
    assert [tuple(r) for r in got] == ref.records, (what, got, ref.records)
    if got_data is not None:
        _same(what, "data", got_data, _expect(ref.data, n_fields, case.data_stride), case.data_stride)
    if got_validity is not None:
        _same(what, "validity", got_validity, _expect(ref.validity, n_fields, case.validity_stride), case.validity_stride)


def run_sim(sim, common, case, chunk, data=True, validity=True, type_shift=0, words=1, expect=0, fields=None, **over):
    """one call of a host simulation (sim_arrowcol, or sim_timecol for a case with a string buffer: `words` is its fetch form)
    into out_buffers(); over: arguments given otherwise than the case has them; -> the whole arrays, canaries included"""
    n_cols, stride = case.types.shape
    store = np.zeros(n_cols * stride + 16, dtype=np.uint8)  # the type columns at an odd address: a slice of a larger array
    t = store[type_shift:type_shift + n_cols * stride]
    t[:] = case.types.reshape(-1)
    values = np.ascontiguousarray(case.values, dtype=np.uint64)
    sb = np.ascontiguousarray(case.sb, dtype=np.uint8) if hasattr(case, "sb") else None
    enc = common.encode(case.fields) if fields is None else fields
    d, b, res = common.out_buffers(case, data, validity)
    rc = np.array([0 if case.row_count is None else case.row_count], dtype=np.uint64)
    args = dict(n_cols=n_cols, col_stride=stride, n_rows=case.n_rows, readable=(n_cols - 1) * stride + live_rows(case),
                data_stride=case.data_stride if data else 0, validity_stride=case.validity_stride, results=res.ctypes.data,
                sb=sb.ctypes.data if sb is not None else None)
    args.update(over)
    strings, fetch = ((), ()) if sb is None else ((args["sb"], sb.size), (words,))
    got = sim(enc.ctypes.data if len(enc) else None, len(enc), t.ctypes.data, values.ctypes.data, args["n_cols"], args["col_stride"], args["n_rows"],
              args["readable"], rc.ctypes.data if case.row_count is not None else None, *strings, chunk, *fetch,
              d[FRONT:].ctypes.data if data else None, args["data_stride"], len(enc) * case.data_stride if data else 0,
              b[FRONT:].ctypes.data if validity else None, args["validity_stride"], len(enc) * case.validity_stride if validity else 0, args["results"])
    assert got == expect, (case.name, got)
    return d, b, res
