"""Multi-GPU batched mode: shard documents across ranks, gather per-shard counts.

The path shards by DOCUMENT (independent units): rank r gets a contiguous, byte-balanced range of
documents, runs the same single-GPU kernels on it, and keeps its outputs local.  The only collective is one
all_gather of 4 x int64 per rank -- {documents, structurals, string bytes, failed documents} -- so that every rank
knows the global output offsets (north_star: "RCCL over xGMI only as a gather of per-shard counts").  On GPUs the
process group is "nccl" (= RCCL); the CPU tests run the same code over "gloo".
"""
import numpy as np


def partition_documents(doc_offsets, world_size):
    """Contiguous, byte-balanced document ranges: -> list of (first_doc, last_doc_exclusive) per rank.
    doc_offsets has n+1 entries (doc k = [offsets[k], offsets[k+1]))."""
    offs = np.asarray(doc_offsets, dtype=np.uint64)
    n = offs.size - 1
    total = int(offs[-1] - offs[0])
    bounds = [0]
    for r in range(1, world_size):
        target = int(offs[0]) + (total * r) // world_size
        k = int(np.searchsorted(offs, np.uint64(target), side="left"))
        k = min(max(k, bounds[-1]), n)
        bounds.append(k)
    bounds.append(n)
    return [(bounds[r], bounds[r + 1]) for r in range(world_size)]


def gather_counts(local_counts, device=None):
    """all_gather of the per-shard {docs, structurals, string_bytes, failed_docs}; -> int64 tensor [world, 4].
    With a single process (no initialised process group) returns the local row."""
    import torch
    import torch.distributed as dist
    row = torch.tensor([int(x) for x in local_counts], dtype=torch.int64, device=device)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return row[None, :]
    out = torch.empty(dist.get_world_size() * row.numel(), dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(out, row)
    return out.view(dist.get_world_size(), row.numel())


def global_offsets(gathered):
    """Exclusive prefix over ranks of the gathered counts: row r = where rank r's outputs start globally."""
    import torch
    g = gathered.to(torch.int64)
    return torch.cumsum(g, dim=0) - g


# stage-1 status bits of a result record, as include/sjmi.h names them
SJMI_ST_CAPACITY, SJMI_ST_INTERNAL, SJMI_ST_HALO, SJMI_ST_REJECTED = 0x100, 0x200, 0x400, 0x800


def _on_gpu(device):
    """(the CPU tests' stub engines are synchronous and have no streams)"""
    return str(device) != "cpu"


def _upload(data, device, pad):
    """bytes or a uint8 tensor -> a uint8 tensor on `device`: the data, then `pad` zero bytes"""
    import torch
    if not hasattr(data, "numel"):
        return torch.frombuffer(bytearray(data) + bytearray(pad), dtype=torch.uint8).to(device)
    buf = torch.zeros(int(data.numel()) + pad, dtype=torch.uint8, device=device)
    buf[:int(data.numel())] = data
    return buf


def _ptr(tensor, entries):
    """the tensor's pointer, or NULL when it has no entries for the call (an empty tensor's own pointer may be anything)"""
    return tensor.data_ptr() if entries else 0


def _column_pair(types, values):
    """the 1-D (types uint8, values int64) pair of one column -> n_rows"""
    import torch
    assert types.dim() == 1 and values.dim() == 1 and types.numel() == values.numel()
    assert types.dtype == torch.uint8 and values.dtype == torch.int64 and types.is_contiguous() and values.is_contiguous()
    return int(types.numel())


def _column_set(types, values, n_rows):
    """the 2-D [n_cols, stride] (types uint8, values int64) pair of a set of columns -> n_cols, stride, n_rows (default: the stride)"""
    import torch
    assert types.dim() == 2 and values.dim() == 2 and types.shape == values.shape
    assert types.dtype == torch.uint8 and values.dtype == torch.int64 and types.is_contiguous() and values.is_contiguous()
    n_cols, stride = int(types.shape[0]), int(types.shape[1])
    n_rows = stride if n_rows is None else int(n_rows)
    assert n_cols >= 1 and 0 <= n_rows <= stride
    return n_cols, stride, n_rows


def _key_column(key_types, key_values, key_validity, n_rows):
    """the 1-D key column of top_rows() / sort_rows() (types uint8 or None, values int64, validity int64 words or None) with at
    least n_rows rows (default: all of key_values) -> n_rows"""
    import torch
    assert key_values.dim() == 1 and key_values.dtype == torch.int64 and key_values.is_contiguous()
    n_rows = int(key_values.numel()) if n_rows is None else int(n_rows)
    assert 0 <= n_rows <= int(key_values.numel())
    assert key_types is None or (key_types.dim() == 1 and key_types.dtype == torch.uint8 and key_types.is_contiguous() and
                                 int(key_types.numel()) >= n_rows)
    assert key_validity is None or (key_validity.dtype == torch.int64 and key_validity.is_contiguous() and
                                    int(key_validity.numel()) >= (n_rows + 63) // 64)
    return n_rows


def _check_row_count(row_count, types):
    import torch
    if row_count is not None:
        assert row_count.dtype == torch.int64 and row_count.numel() == 1 and row_count.device == types.device


GROUP_STATS_WORDS = 10  # SJMI_GROUP_STATS_WORDS
TOP_KINDS = {"long": 1, "double": 2}  # SJMI_TOP_LONG, SJMI_TOP_DOUBLE
TOP_SMALLEST, TOP_MAX_K, TOP_RESULT_WORDS = 1, 2048, 9  # SJMI_TOP_SMALLEST, SJMI_TOP_MAX_K, SJMI_TOP_RESULT_WORDS
SORT_DESCENDING, SORT_BAD_ROW, SORT_RESULT_WORDS = 1, 1, 9  # SJMI_SORT_DESCENDING, SJMI_SORT_BAD_ROW, SJMI_SORT_RESULT_WORDS (the kinds: TOP_KINDS)
PARENT_MAX_COLS, PARENT_RESULT_WORDS = 64, 3  # SJMI_PARENT_MAX_COLS, SJMI_PARENT_RESULT_WORDS
JOIN_HOWS = {"inner": 0, "left": 1, "semi": 2, "anti": 3}  # SJMI_JOIN_INNER, SJMI_JOIN_LEFT, SJMI_JOIN_SEMI, SJMI_JOIN_ANTI
JOIN_OVERFLOW, JOIN_BAD_ROW, JOIN_BAD_ORDER, JOIN_RESULT_WORDS = 1, 2, 4, 9  # SJMI_JOIN_<FLAG>, SJMI_JOIN_RESULT_WORDS


def decode_group_stats(stats):
    """The stats of BatchShard.group_stats() on the host (a numpy array of shape [n_keys, 10], int64 or uint64) -> one dict per
    key with Python values: n_long, n_double, n_other, sum_long (an int built from the 128 bits), sum_double, min_long, max_long,
    min_double, max_double.  The minima and maxima of a class without a row are None."""
    words = np.ascontiguousarray(stats).view(np.uint64).reshape(-1, GROUP_STATS_WORDS)
    signed, floats = words.view(np.int64), words.view(np.float64)
    out = []
    for k in range(words.shape[0]):
        n_long, n_double = int(words[k, 0]), int(words[k, 1])
        out.append({
            "n_long": n_long, "n_double": n_double, "n_other": int(words[k, 2]),
            "sum_long": (int(signed[k, 4]) << 64) + int(words[k, 3]),
            "sum_double": float(floats[k, 5]),
            "min_long": int(signed[k, 6]) if n_long else None, "max_long": int(signed[k, 7]) if n_long else None,
            "min_double": float(floats[k, 8]) if n_double else None, "max_double": float(floats[k, 9]) if n_double else None,
        })
    return out


class BatchShard:
    """One rank's contiguous share of a batch of documents, resident on its device, and everything one step of the
    batched path needs: outputs sized once, then `step()` queues sjmi_parse_batch_device (isolated stage 1 -> string
    records -> GPU walk; no host round trip) on the given stream.  `engine` is a binding.Context (or, in the CPU tests,
    a stub with the same parse_batch_device signature); tensors are plain torch tensors on `device`."""

    def __init__(self, engine, shard_bytes, local_offsets, device, max_depth=1024, index_ratio=1, string_ratio=1.0,
                 tape_ratio=1.0, device_offsets=None):
        """device_offsets: the documents' offsets as an int64 tensor of n_docs + 1 entries that is already on `device` (from_ndjson:
        they were made there and never leave it); local_offsets is then not looked at.  They must cover the shard exactly."""
        import torch
        self.engine = engine
        self.device = device
        self.n = int(shard_bytes.numel()) if hasattr(shard_bytes, "numel") else len(shard_bytes)
        if device_offsets is None:
            offs = np.ascontiguousarray(local_offsets, dtype=np.uint64)
            assert offs[0] == 0 and int(offs[-1]) == self.n  # (the documents cover the shard exactly: include/sjmi.h, sjmi_parse_batch_device)
            self.n_docs = offs.size - 1
        else:
            self.n_docs = int(device_offsets.numel()) - 1
        self.buf = _upload(shard_bytes, device, 128)
        self.offs = torch.from_numpy(offs.view(np.int64).copy()).to(device) if device_offsets is None else device_offsets
        # the defaults cover the worst cases (one structural per byte: "[[[[", one tape word per byte: "[1,1,1"); real
        # JSON has one structural per 5-11 bytes, so a caller that knows its data passes tighter ratios (bench.py) -- a
        # shortfall is reported by the kernels (never overrun) and check() raises
        self.index_capacity = self.n // index_ratio + self.n_docs + 16
        self.idx = torch.empty(self.index_capacity, dtype=torch.int32, device=device)
        self.index_offsets = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=device)
        self.doc_status = torch.zeros(max(self.n_docs, 1), dtype=torch.int32, device=device)
        self.sb_capacity = int(self.n * string_ratio) + 4 * self.index_capacity + 64
        self.sb = torch.empty(self.sb_capacity, dtype=torch.uint8, device=device)
        self.doc_string_offsets = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=device)
        self.tape_capacity = int(self.n * tape_ratio) + 2 * self.n_docs + 8
        self.tape = torch.empty(self.tape_capacity, dtype=torch.int64, device=device)
        self.tape_offsets = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=device)
        self.doc_errors = torch.zeros(max(self.n_docs, 1), dtype=torch.int32, device=device)
        self.result = torch.zeros(9, dtype=torch.int64, device=device)  # sjmi_batch_result
        self.max_depth = max_depth
        self._ndocs = torch.tensor([self.n_docs], dtype=torch.int64, device=device)
        # what check() latches for step() (bench.py resets the first two between its sections)
        self.rejected_steps, self.format_rejected, self.unrepairable = 0, False, False
        # the last step's stream, and the select / explode queued behind it, for check() to queue again
        self._last_stream, self._sel_pending, self._exp_pending = 0, None, None
        self._sel_plan = self._exp_plan = self._exp_capacity = None  # what sel_* / exp_* are allocated for
        self._side_stream = None  # sharded_step's, made on first use
        self.ndjson_consumed, self.ndjson_flags = None, 0  # (from_ndjson)

    @classmethod
    def from_ndjson(cls, engine, shard_bytes, device, **kwargs):
        """A shard from the bytes of a file of newline-delimited JSON (bytes or a uint8 tensor): the bytes are uploaded and split
        into documents ON the device (sjmi_ndjson_offsets_device; blank lines belong to the document in front of them), the
        24-byte result record is read back -- the one host synchronisation of the path -- and the shard is built over
        [0, consumed) with the offsets never leaving the device.  The unterminated tail, if any, is not part of the shard:
        .ndjson_consumed says where it begins and .ndjson_flags bit 0 (SJMI_NDJSON_TAIL_BLANK) whether it is blank; a caller
        at the end of its file appends one '\\n' first.  kwargs as for the constructor."""
        import torch
        n = int(shard_bytes.numel()) if hasattr(shard_bytes, "numel") else len(shard_bytes)
        raw = _upload(shard_bytes, device, 64)  # (SJMI_PADDING readable bytes)
        result = torch.zeros(3, dtype=torch.int64, device=device)  # sjmi_ndjson_result
        offs = torch.empty(n // 2 + 1, dtype=torch.int64, device=device)  # (a document is at least one byte and its NL)
        stream = torch.cuda.current_stream(device).cuda_stream if _on_gpu(device) else 0
        engine_stream = _on_gpu(device) and not stream  # (handle 0 names the engine's own stream, which torch's do not order)
        if engine_stream:
            torch.cuda.synchronize(device)  # (the upload has to be done before it starts)
        engine.ndjson_offsets_device(raw.data_ptr(), n, offs.data_ptr(), offs.numel(), result.data_ptr(), stream)
        if engine_stream:
            torch.cuda.synchronize(device)
        r = result.cpu().numpy()
        n_docs, consumed, flags = int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF
        assert not (flags & 2), "n // 2 + 1 offsets always suffice"
        # (without a document, blank lines have nothing in front of them to belong to: the shard is empty)
        shard = cls(engine, raw[:consumed if n_docs else 0], None, device, device_offsets=offs[:n_docs + 1], **kwargs)
        shard.ndjson_consumed, shard.ndjson_flags = consumed, flags
        return shard

    def step(self, stream=0, exact=False, rejected=False):
        """One step, queued on `stream`.  Default: sjmi_parse_batch_device_optimistic -- only the optimistic pipeline (eight queue
        entries); a batch it cannot take (a document fails stage 1, a separator is missing) comes back with SJMI_ST_REJECTED in
        its result record and check() makes the call for rejected batches then (sjmi_parse_batch_device_rejected: per-document
        verdicts + the pipeline over a sanitized copy), off the hot path.  exact=True: sjmi_parse_batch_device, everything
        queued, every document decided on its own whatever the batch contains."""
        # Latched by check(): data that was rejected once does not take the optimistic-only call again (a step whose record says
        # REJECTED has no valid counts for the gather).  Rejected although every document passed stage 1 = rejected for its FORMAT
        # (no control-character separators): the next batch will be too, so it goes straight to the call for rejected batches;
        # rejected for a document that fails stage 1: the exact call, which tries the plain pass first.
        rejected = rejected or (not exact and self.format_rejected and not self.unrepairable)
        exact = exact or self.rejected_steps > 0
        # (an engine from before an entry point existed makes the exact call in its place)
        if rejected and hasattr(self.engine, "parse_batch_device_rejected"):
            call = self.engine.parse_batch_device_rejected
        elif exact or rejected or not hasattr(self.engine, "parse_batch_device_optimistic"):
            call = self.engine.parse_batch_device
        else:
            call = self.engine.parse_batch_device_optimistic
        self._last_stream = stream
        self._sel_pending = None  # (a select queued behind an earlier step does not belong to this one)
        self._exp_pending = None
        call(self.buf.data_ptr(), self.n, self.offs.data_ptr(), self.n_docs, self.idx.data_ptr(), self.index_capacity,
             self.index_offsets.data_ptr(), self.doc_status.data_ptr(), self.sb.data_ptr(), self.sb_capacity,
             self.doc_string_offsets.data_ptr(), self.max_depth, self.tape.data_ptr(), self.tape_capacity,
             self.tape_offsets.data_ptr(), self.doc_errors.data_ptr(), self.result.data_ptr(), stream)

    def select(self, plan, stream=0):
        """Every path of `plan` (a binding.SelectPlan) on every document of the shard: sjmi_select_batch_device, queued on
        `stream` behind the step() that was queued there -- no host synchronisation, the tapes never leave the device.
        -> (sel_types [n_paths, n_docs] uint8, sel_values [n_paths, n_docs] int64), allocated once per plan and overwritten
        by every call: types 0 = MISSING, else the tape type byte; values as include/sjmi.h lays them out (string values
        point into self.sb).  A step that came back SJMI_ST_REJECTED has no valid outputs, so the columns are valid only for
        a step check() has accepted: when check() runs the step again through the call for rejected batches (or the exact
        call), it queues this select again behind it, and the columns then belong to that run.  A document that failed
        (doc_errors[k] != 0) is MISSING on every path."""
        import torch
        if self._sel_plan is not plan:
            self.sel_types = torch.zeros((plan.n_paths, self.n_docs), dtype=torch.uint8, device=self.device)
            self.sel_values = torch.zeros((plan.n_paths, self.n_docs), dtype=torch.int64, device=self.device)
            self._sel_plan = plan
        self._sel_pending = (plan, stream)
        self.engine.select_batch_device(plan, self.tape.data_ptr(), self.tape_offsets.data_ptr(), self.doc_errors.data_ptr(),
                                        self.sb.data_ptr(), self.n_docs, self.sel_types.data_ptr(), self.sel_values.data_ptr(), stream)
        return self.sel_types, self.sel_values

    def explode(self, plan, row_capacity, stream=0):
        """The base array of `plan` (a binding.ExplodePlan) of every document of the shard as rows, every element pointer on
        every element: sjmi_explode_batch_device, queued on `stream` behind the step() that was queued there -- no host
        synchronisation.  -> (exp_row_offsets [n_docs + 1] int64, exp_types [n_paths, row_capacity] uint8, exp_values
        [n_paths, row_capacity] int64), allocated once per (plan, row_capacity) and overwritten by every call.  A MEMBERS plan
        (ExplodePlan(..., members=True)) takes the base OBJECT's members as rows and has plan.n_columns = n_paths + 1 columns:
        the element pointers on the member's value, and the member's key -- a string cell -- in the last one.  The offsets
        are always complete (exp_row_offsets[n_docs] = the total number of rows); rows at or behind row_capacity are not
        written.  row_capacity 0: the offsets only (the columns are empty).  As for select(), the outputs are valid only for
        a step check() has accepted, and check() queues the explode again behind a step it had to run again."""
        import torch
        row_capacity = int(row_capacity)
        if self._exp_plan is not plan or self._exp_capacity != row_capacity:
            self.exp_row_offsets = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=self.device)
            n_columns = getattr(plan, "n_columns", plan.n_paths)
            self.exp_types = torch.zeros((n_columns, row_capacity), dtype=torch.uint8, device=self.device)
            self.exp_values = torch.zeros((n_columns, row_capacity), dtype=torch.int64, device=self.device)
            self._exp_plan, self._exp_capacity = plan, row_capacity
        self._exp_pending = (plan, row_capacity, stream)
        cells = int(self.exp_types.numel())
        self.engine.explode_batch_device(plan, self.tape.data_ptr(), self.tape_offsets.data_ptr(), self.doc_errors.data_ptr(),
                                         self.sb.data_ptr(), self.n_docs, self.exp_row_offsets.data_ptr(), row_capacity,
                                         _ptr(self.exp_types, cells), _ptr(self.exp_values, cells), stream)
        return self.exp_row_offsets, self.exp_types, self.exp_values

    def string_column(self, types, values, byte_capacity=None, stream=0):
        """ONE string column as Arrow large_utf8: sjmi_string_column_device on a 1-D (types uint8, values int64) tensor pair -- a
        row of sel_types / sel_values, or a row of exp_types / exp_values cut to the rows present -- whose string cells point
        into self.sb.  -> (offsets [n_rows + 1] int64, validity [ceil(n_rows / 64)] int64 words (LSB first), data uint8, result
        [4] int64 = total_bytes, n_valid, n_other, flags), new tensors every call.  Rows that are not strings (MISSING -- a
        failed document's among them --, null, numbers, booleans, containers) are NULL; result[2] counts those of them that are
        neither MISSING nor null.  byte_capacity=None: a sizing call, the 32-byte record read back -- the one host
        synchronisation -- `data` allocated exactly and the second call made.  With a byte_capacity nothing synchronises: bytes
        at or behind it are not written and result[3] & 1 (SJMI_STRCOL_OVERFLOW) says so; the offsets are complete either way.
        Call it on a step that check() has accepted: unlike select() and explode(), it is not queued again behind a step that
        check() had to run again."""
        import torch
        n_rows = _column_pair(types, values)
        offsets = torch.empty(n_rows + 1, dtype=torch.int64, device=self.device)
        validity = torch.empty((n_rows + 63) // 64, dtype=torch.int64, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)  # sjmi_strcol_result (every call writes all of it)
        call = lambda data, capacity: self.engine.string_column_device(
            _ptr(types, n_rows), _ptr(values, n_rows), n_rows, self.sb.data_ptr(), offsets.data_ptr(), _ptr(validity, n_rows),
            _ptr(data, capacity), capacity, result.data_ptr(), stream)
        return offsets, validity, self._sized_bytes(call, result, 0, byte_capacity), result

    def _sized_bytes(self, call, record, word, byte_capacity):
        """The byte buffer of string_column() and dictionary_column(), filled by call(data, capacity).  byte_capacity=None: the
        sizing call (no buffer, capacity 0), record[word] read back behind a synchronisation, the buffer allocated exactly and
        the second call made -- none for 0 bytes; with a byte_capacity the one call and nothing synchronises."""
        import torch
        if byte_capacity is None:
            call(None, 0)
            if _on_gpu(self.device):
                torch.cuda.synchronize(self.device)  # (`stream` need not be the one torch's copy is queued on)
            byte_capacity = int(record.cpu()[word])
            if not byte_capacity:
                return torch.empty(0, dtype=torch.uint8, device=self.device)
        data = torch.empty(int(byte_capacity), dtype=torch.uint8, device=self.device)
        call(data, int(byte_capacity))
        return data

    def filter(self, plan, types, values, n_rows=None, out_capacity=None, stream=0):
        """The rows on which every term of `plan` (a binding.FilterPlan) is true, and the columns compacted to them:
        sjmi_filter_columns_device on a 2-D [n_cols, stride] (types uint8, values int64) tensor pair -- sel_types / sel_values, or
        exp_types / exp_values with n_rows = the rows present (default: the stride) -- whose string cells point into self.sb.
        -> (rows [out_capacity] int64, out_types [n_cols, out_capacity] uint8, out_values [n_cols, out_capacity] int64, keep
        [ceil(n_rows / 64)] int64 words (LSB first), result [2] int64 = n_kept, flags), new tensors every call.  Entries at or
        behind result[0] are not written: the caller slices by it after its own synchronisation; a row of out_types / out_values
        so cut is a column for string_column().  out_capacity=None: n_rows, which always suffices -- nothing synchronises either
        way; with a smaller one result[1] & 1 (SJMI_FILTER_OVERFLOW) says that rows were left out, and 0 is the sizing call.
        Call it on a step that check() has accepted: like string_column(), it is not queued again behind a step that check() had
        to run again."""
        import torch
        n_cols, stride, n_rows = _column_set(types, values, n_rows)
        out_capacity = n_rows if out_capacity is None else int(out_capacity)
        rows = torch.empty(out_capacity, dtype=torch.int64, device=self.device)
        out_types = torch.empty((n_cols, out_capacity), dtype=torch.uint8, device=self.device)
        out_values = torch.empty((n_cols, out_capacity), dtype=torch.int64, device=self.device)
        keep = torch.empty((n_rows + 63) // 64, dtype=torch.int64, device=self.device)
        result = torch.empty(2, dtype=torch.int64, device=self.device)  # sjmi_filter_result (every call writes all of it)
        self.engine.filter_columns_device(plan, _ptr(types, n_rows), _ptr(values, n_rows), n_cols, stride, n_rows, self.sb.data_ptr(),
                                          _ptr(keep, n_rows), _ptr(rows, out_capacity), out_capacity, _ptr(out_types, out_capacity),
                                          _ptr(out_values, out_capacity), result.data_ptr(), stream)
        return rows, out_types, out_values, keep, result

    def arrow_columns(self, fields, types, values, n_rows=None, row_count=None, stream=0):
        """Typed columns as Arrow int64 / float64 / bool arrays: sjmi_arrow_columns_device on a 2-D [n_cols, stride] (types uint8,
        values int64) tensor pair -- sel_types / sel_values, exp_types / exp_values, or the compacted pair of filter().  fields:
        tuples (column, "int64" | "float64" | "bool"[, "integral_doubles"]), at most 64; two may name one column.  n_rows sizes
        the launch and the outputs (default: the stride); row_count is an optional 1-element int64 DEVICE tensor -- result[0:1]
        of filter(), exp_row_offsets[n_docs:] of explode() -- that the kernels read: the live rows are min(n_rows, row_count[0])
        and nothing synchronises.  -> (data [n_fields, n_rows] int64, validity [n_fields, ceil(n_rows / 64)] int64 words (LSB
        first), results [n_fields, 4] int64 = live rows, n_valid, n_other, n_inexact), new tensors every call.  A float64
        field's row of `data` is read with .view(torch.float64); a bool field's is a bitmap in its first ceil(live / 64) words.
        Rows at or above the live rows, and the words behind them, are not written: the caller slices by results[:, 0] after
        its own synchronisation.  Call it on a step that check() has accepted: like string_column() and filter(), it is not
        queued again behind a step that check() had to run again."""
        return self._field_columns(self.engine.arrow_columns_device, 4, (), fields, types, values, n_rows, row_count, stream)

    def timestamp_columns(self, fields, types, values, n_rows=None, row_count=None, stream=0):
        """RFC 3339 string columns as Arrow timestamp arrays: sjmi_time_columns_device on a 2-D [n_cols, stride] (types uint8,
        values int64) tensor pair -- sel_types / sel_values, exp_types / exp_values, or the compacted pair of filter() -- whose
        string cells point into self.sb.  fields: tuples (column, "s" | "ms" | "us" | "ns"[, "naive_utc"]), at most 64; two may
        name one column.  n_rows sizes the launch and the outputs (default: the stride); row_count is an optional 1-element int64
        DEVICE tensor -- result[0:1] of filter(), exp_row_offsets[n_docs:] of explode() -- that the kernels read: the live rows
        are min(n_rows, row_count[0]) and nothing synchronises.  -> (data [n_fields, n_rows] int64 at the field's unit since
        1970-01-01T00:00:00Z, validity [n_fields, ceil(n_rows / 64)] int64 words (LSB first), results [n_fields, 6] int64 = live
        rows, n_valid, n_other, n_malformed, n_range, n_inexact), new tensors every call.  Rows at or above the live rows, and
        the words behind them, are not written: the caller slices by results[:, 0] after its own synchronisation.  Call it on a
        step that check() has accepted: like arrow_columns(), it is not queued again behind a step that check() had to run
        again."""
        return self._field_columns(self.engine.time_columns_device, 6, (self.sb.data_ptr(),), fields, types, values, n_rows, row_count, stream)

    def _field_columns(self, call, record_words, strings, fields, types, values, n_rows, row_count, stream):
        """arrow_columns() and timestamp_columns(): the checks of the tensor pair, the outputs and the call; `strings` is () or
        (the string buffer's pointer,), record_words the width of a field's record"""
        import torch
        n_cols, stride, n_rows = _column_set(types, values, n_rows)
        _check_row_count(row_count, types)
        n_fields, words = len(fields), (n_rows + 63) // 64
        data = torch.empty((n_fields, n_rows), dtype=torch.int64, device=self.device)
        validity = torch.empty((n_fields, words), dtype=torch.int64, device=self.device)
        results = torch.empty((n_fields, record_words), dtype=torch.int64, device=self.device)  # (every call writes all of it)
        call(fields, _ptr(types, n_rows), _ptr(values, n_rows), n_cols, stride, n_rows, _ptr(row_count, row_count is not None), *strings,
             _ptr(data, n_rows), n_rows, _ptr(validity, n_rows), words, results.data_ptr(), stream)
        return data, validity, results

    def dictionary_column(self, types, values, dict_capacity, byte_capacity=None, row_count=None, stream=0):
        """ONE string column as an Arrow dictionary array: sjmi_dictionary_column_device on a 1-D (types uint8, values int64)
        tensor pair, as string_column() takes it, whose string cells point into self.sb.  The dictionary holds at most
        dict_capacity distinct values (at most 2^20), in the order of their first occurrence.  row_count is an optional 1-element
        int64 DEVICE tensor -- result[0:1] of filter(), exp_row_offsets[n_docs:] of explode() -- that the kernels read: the live
        rows are min(n_rows, row_count[0]).  -> (indices [n_rows] int32, validity [ceil(n_rows / 64)] int64 words (LSB first),
        dict_rows [dict_capacity] int64, dict_offsets [dict_capacity + 1] int64, dict_bytes uint8, result [6] int64 = live rows,
        n_valid, n_other, n_distinct, dict_bytes, flags), new tensors every call.  Indices and validity words at or above the live
        rows, and dictionary entries at or above result[3], are not written: the caller slices by the record.  byte_capacity=
        None: a sizing call, the record read back -- the one host synchronisation -- dict_bytes allocated exactly and the second
        call made.  With a byte_capacity nothing synchronises: bytes at or behind it are not written and result[5] & 2
        (SJMI_DICT_BYTES_OVERFLOW) says so.  result[5] & 1 (SJMI_DICT_OVERFLOW): more distinct values than dict_capacity; only
        the counts and the validity mean anything then.  Call it on a step that check() has accepted, like string_column()."""
        import torch
        n_rows = _column_pair(types, values)
        _check_row_count(row_count, types)
        dict_capacity = int(dict_capacity)
        indices = torch.empty(n_rows, dtype=torch.int32, device=self.device)
        validity = torch.empty((n_rows + 63) // 64, dtype=torch.int64, device=self.device)
        dict_rows = torch.empty(dict_capacity, dtype=torch.int64, device=self.device)
        dict_offsets = torch.empty(dict_capacity + 1, dtype=torch.int64, device=self.device)
        result = torch.empty(6, dtype=torch.int64, device=self.device)  # sjmi_dict_result (every call writes all of it)
        one = torch.empty(1, dtype=torch.int32, device=self.device)  # (d_indices must not be NULL, not even without rows)
        call = lambda data, capacity: self.engine.dictionary_column_device(
            _ptr(types, n_rows), _ptr(values, n_rows), n_rows, _ptr(row_count, row_count is not None), self.sb.data_ptr(),
            indices.data_ptr() if n_rows else one.data_ptr(), _ptr(validity, n_rows), dict_capacity, _ptr(dict_rows, dict_capacity),
            dict_offsets.data_ptr(), _ptr(data, capacity), capacity, result.data_ptr(), stream)
        return indices, validity, dict_rows, dict_offsets, self._sized_bytes(call, result, 4, byte_capacity), result

    def key_census(self, indices, validity, types, n_keys, row_count=None, stream=0):
        """The rows per dictionary entry and value type: sjmi_key_census_device on the (indices [n_rows] int32, validity words) of
        dictionary_column() -- validity None: every live row counts -- and a 1-D types uint8 tensor with the same rows, normally
        the "" element pointer's row of a members explode.  n_keys is the number of dictionary entries (at most 2^20); row_count
        as for dictionary_column().  -> (counts [n_keys, 8] int64: per entry the rows whose type is 'l', 'd', '"', 't' or 'f',
        'n', '[', '{', anything else; result [4] int64 = live rows, n_counted, n_out_of_range, flags), new tensors every call,
        every word of them written.  A valid row whose index is outside [0, n_keys) -- the indices of an overflowed dictionary
        -- is counted in result[2] only.  Nothing synchronises.  Call it on a step that check() has accepted: like
        dictionary_column(), it is not queued again behind a step that check() had to run again."""
        import torch
        n_rows, n_keys = int(indices.numel()), int(n_keys)
        assert indices.dim() == 1 and indices.dtype == torch.int32 and indices.is_contiguous()
        assert types.dim() == 1 and types.dtype == torch.uint8 and types.is_contiguous() and int(types.numel()) == n_rows
        assert validity is None or (validity.dtype == torch.int64 and validity.is_contiguous() and int(validity.numel()) >= (n_rows + 63) // 64)
        _check_row_count(row_count, types)
        counts = torch.empty((n_keys, 8), dtype=torch.int64, device=self.device)
        result = torch.empty(4, dtype=torch.int64, device=self.device)  # sjmi_census_result (every call writes all of it)
        self.engine.key_census_device(_ptr(indices, n_rows), _ptr(validity, validity is not None and n_rows), _ptr(types, n_rows), n_rows,
                                      _ptr(row_count, row_count is not None), n_keys, _ptr(counts, n_keys), result.data_ptr(), stream)
        return counts, result

    def group_stats(self, indices, validity, types, values, n_keys, row_count=None, stream=0):
        """Count, sum, minimum and maximum of ONE column per dictionary entry: sjmi_group_stats_device on the (indices [n_rows]
        int32, validity words) of dictionary_column() -- validity None: every live row counts -- and a 1-D (types uint8, values
        int64) pair with the same rows: a row of sel_* / exp_*, or of filter()'s compacted pair.  n_keys is the number of
        dictionary entries (at most 2^20), n_rows below 2^32; row_count as for dictionary_column().  -> (stats [n_keys, 10] int64:
        per entry n_long, n_double, n_other, sum_long_lo, sum_long_hi, the bits of sum_double, min_long, max_long, the bits of
        min_double and max_double -- decode_group_stats() reads them on the host --; result [5] int64 = live rows, n_grouped,
        n_out_of_range, n_nan, flags), new tensors every call, every word of them written.  The long words are exact and the same
        in every run; sum_double is summed in an unspecified order.  Nothing synchronises.  Call it on a step that check() has
        accepted: like key_census(), it is not queued again behind a step that check() had to run again."""
        import torch
        n_rows, n_keys = int(indices.numel()), int(n_keys)
        assert indices.dim() == 1 and indices.dtype == torch.int32 and indices.is_contiguous()
        assert _column_pair(types, values) == n_rows
        assert validity is None or (validity.dtype == torch.int64 and validity.is_contiguous() and int(validity.numel()) >= (n_rows + 63) // 64)
        _check_row_count(row_count, types)
        stats = torch.empty((n_keys, GROUP_STATS_WORDS), dtype=torch.int64, device=self.device)
        result = torch.empty(5, dtype=torch.int64, device=self.device)  # sjmi_group_result (every call writes all of it)
        self.engine.group_stats_device(_ptr(indices, n_rows), _ptr(validity, validity is not None and n_rows), _ptr(types, n_rows),
                                       _ptr(values, n_rows), n_rows, _ptr(row_count, row_count is not None), n_keys, _ptr(stats, n_keys),
                                       result.data_ptr(), stream)
        return stats, result

    def top_rows(self, key_types, key_values, k, kind="long", largest=True, key_validity=None, types=None, values=None, n_rows=None,
                 row_count=None, stream=0):
        """ORDER BY one column, LIMIT k: sjmi_top_rows_device on the 1-D key column (key_types uint8 or None, key_values int64) --
        with types a row of sel_* / exp_* or of filter()'s compacted pair; without types and with key_validity (int64 words, LSB
        first) a data row of arrow_columns() / timestamp_columns(); with both, both must pass.  kind "long": 'l' cells (without
        types: every valid row) as int64; "double": 'd' cells and 'l' cells converted as arrow_columns() converts them (without
        types: every valid row as the bits of a double), NaNs counted and left out.  k at most TOP_MAX_K = 2048; largest=False
        takes the k smallest.  types / values: a 2-D [n_cols, stride] pair of columns to carry along, or None.  n_rows (default:
        all of key_values; at most the stride, below 2^32) and row_count as for arrow_columns().  -> (rows [k] int64: the row
        indices in rank order, equal values by ascending row, the ties at the cut decided the same way; out_types [n_cols, k]
        uint8 and out_values [n_cols, k] int64: the carried cells of these rows, the layout of filter()'s compacted pair; result
        [9] int64 = live rows, n_candidates, n_null, n_other, n_nan, n_inexact, n_out, kth_bits, flags), new tensors every call;
        only the first n_out = min(k, n_candidates) entries of a row are written.  Everything is a function of the input alone.
        Nothing synchronises.  Call it on a step that check() has accepted: like group_stats(), it is not queued again behind a
        step that check() had to run again."""
        import torch
        assert kind in TOP_KINDS, "top_rows(): kind is 'long' or 'double'"
        n_rows, k = _key_column(key_types, key_values, key_validity, n_rows), int(k)
        assert 0 <= k <= TOP_MAX_K
        _check_row_count(row_count, key_values)
        n_cols = stride = 0
        if types is not None:
            n_cols, stride, _ = _column_set(types, values, n_rows)
        rows = torch.empty(k, dtype=torch.int64, device=self.device)
        out_types = torch.empty((n_cols, k), dtype=torch.uint8, device=self.device)
        out_values = torch.empty((n_cols, k), dtype=torch.int64, device=self.device)
        result = torch.empty(TOP_RESULT_WORDS, dtype=torch.int64, device=self.device)  # sjmi_top_result (every call writes all of it)
        self.engine.top_rows_device(_ptr(key_types, key_types is not None and n_rows), _ptr(key_validity, key_validity is not None and n_rows),
                                    _ptr(key_values, n_rows), n_rows, _ptr(row_count, row_count is not None), TOP_KINDS[kind],
                                    0 if largest else TOP_SMALLEST, k, _ptr(types, n_cols), _ptr(values, n_cols), n_cols, stride, _ptr(rows, k),
                                    _ptr(out_types, n_cols * k), _ptr(out_values, n_cols * k), result.data_ptr(), stream)
        return rows, out_types, out_values, result

    def sort_rows(self, keys, types=None, values=None, rows=None, n_rows=None, row_count=None, stream=0):
        """ORDER BY one or several columns, all rows: a chain of sjmi_sort_rows_device calls, a stable sort each, from the LAST key
        to the first.  keys: a list of (key_types, key_values, kind, descending[, key_validity]), most significant first -- each
        a 1-D key column as top_rows() takes it, all with the same number of source rows, kind "long" or "double".  rows=None:
        position i is source row i and n_rows defaults to the source rows; with rows (1-D int64: filter()'s selection vector, in
        any order, duplicates legal) position i is row rows[i] and n_rows defaults to rows.numel(); an entry outside the source
        rows is a BAD position, counted and ordered with the nulls.  row_count as for arrow_columns(): the live positions are
        min(n_rows, row_count[0]).  types / values: a 2-D [n_cols, stride] pair of columns to carry along (stride at least the
        source rows), or None; they are gathered by the last call only.  -> (rows [n_rows] int64: the source row at every
        output place -- the candidates by value, then NaN, OTHER, NULL and BAD positions, equal ones in input order --;
        out_types [n_cols, n_rows] uint8 and out_values [n_cols, n_rows] int64: the carried cells of these rows, the layout of
        filter()'s compacted pair; records [len(keys), 9] int64: records[i] is the sjmi_sort_result of keys[i] = live positions,
        n_candidates, n_null, n_other, n_nan, n_inexact, n_bad, n_passes, flags), new tensors every call; entries at or behind
        the live positions are not written.  The calls exchange two row buffers of the shard's own making; `rows` is only read.
        Everything is a function of the input alone.  Nothing synchronises.  Call it on a step that check() has accepted: like
        top_rows(), it is not queued again behind a step that check() had to run again."""
        import torch
        assert len(keys) >= 1, "sort_rows(): at least one key"
        n_source = int(keys[0][1].numel())
        for key in keys:
            assert len(key) in (4, 5) and key[2] in TOP_KINDS, "sort_rows(): a key is (types, values, kind, descending[, validity])"
            assert _key_column(key[0], key[1], key[4] if len(key) == 5 else None, None) == n_source
        if rows is None:
            n_rows = n_source if n_rows is None else int(n_rows)
            assert 0 <= n_rows <= n_source
        else:
            assert rows.dim() == 1 and rows.dtype == torch.int64 and rows.is_contiguous()
            n_rows = int(rows.numel()) if n_rows is None else int(n_rows)
            assert 0 <= n_rows <= int(rows.numel())
        _check_row_count(row_count, keys[0][1])
        n_cols = stride = 0
        if types is not None:
            n_cols, stride, _ = _column_set(types, values, n_source)
        buffers = [torch.empty(n_rows, dtype=torch.int64, device=self.device) for _ in range(min(2, len(keys)))]
        out_types = torch.empty((n_cols, n_rows), dtype=torch.uint8, device=self.device)
        out_values = torch.empty((n_cols, n_rows), dtype=torch.int64, device=self.device)
        records = torch.empty((len(keys), SORT_RESULT_WORDS), dtype=torch.int64, device=self.device)  # (every call writes all of its own)
        source = rows
        for call, at in enumerate(range(len(keys) - 1, -1, -1)):
            key_types, key_values, kind, descending = keys[at][:4]
            key_validity = keys[at][4] if len(keys[at]) == 5 else None
            carry = n_cols if at == 0 else 0  # (the carried cells follow the final order only)
            out = buffers[call % 2]
            self.engine.sort_rows_device(_ptr(key_types, key_types is not None and n_source), _ptr(key_validity, key_validity is not None and n_source),
                                         _ptr(key_values, n_source), n_source, _ptr(source, source is not None and n_rows), n_rows,
                                         _ptr(row_count, row_count is not None), TOP_KINDS[kind], SORT_DESCENDING if descending else 0,
                                         _ptr(types, carry), _ptr(values, carry), carry, stride if carry else 0, _ptr(out, n_rows),
                                         _ptr(out_types, carry * n_rows), _ptr(out_values, carry * n_rows), n_rows if carry else 0,
                                         records[at].data_ptr(), stream)
            source = out
        return source, out_types, out_values, records

    def join_rows(self, left_key, right_key, how="inner", left=None, right=None, left_rows=None, n_left=None, left_count=None,
                  right_rows=None, n_right=None, right_count=None, right_sorted=None, pair_capacity=None, with_offsets=False, stream=0):
        """JOIN two row sets ON one long key a side: sjmi_join_rows_device, behind one sjmi_sort_rows_device (LONG, ascending, no
        carried columns) on the right key unless right_sorted is given.  left_key / right_key: (types, values[, validity]), a
        1-D key column each as top_rows() takes it (types or validity may be None).  how: "inner", "left" (every live left
        position at least once, an unmatched one with right row -1), "semi" (the left positions with a match, once) or "anti"
        (those without, NULL, OTHER and BAD keys included).  left / right: a 2-D [n_cols, stride] (types, values) pair of
        columns of the side's source rows to carry onto the pairs, or None; right must be None under "semi" and "anti".
        left_rows / n_left / left_count and right_rows / n_right / right_count: the positions of a side as sort_rows() takes
        rows / n_rows / row_count -- a filter's selection and its n_kept, an explode's last row offset.  right_sorted = the last
        element of an earlier call's result on the same right side: the sort is skipped -- build once, probe many -- and the
        right_* arguments are not read.  pair_capacity: the pairs the outputs hold (required).  -> (left_rows [pair_capacity]
        int64 and right_rows [pair_capacity] int64 (None under "semi" and "anti"): the source rows of every pair, by ascending
        left position and, inside one, ascending right position; left_types / left_values [n_left_cols, pair_capacity] and
        right_types / right_values [n_right_cols, pair_capacity]: the carried cells, MISSING and 0 without a row; pair_offsets
        [n_left + 1] int64 with with_offsets=True, else None: the pairs in front of every left position, explode's row_offsets
        with "left position = document" for parent_columns(); record [9] int64 = live left positions, n_build, n_pairs,
        n_matched, n_null, n_other, n_bad, n_right_bad, flags (JOIN_OVERFLOW: n_pairs > pair_capacity, call again with more);
        right_sorted), new tensors every call; only the first min(n_pairs, pair_capacity) pairs are written.  Everything is a
        function of the input alone.  Nothing synchronises.  Call it on a step that check() has accepted: like sort_rows(), it
        is not queued again behind a step that check() had to run again."""
        import torch
        assert how in JOIN_HOWS, "join_rows(): how is 'inner', 'left', 'semi' or 'anti'"
        assert pair_capacity is not None and int(pair_capacity) >= 0, "join_rows(): pair_capacity is required"
        pair_capacity = int(pair_capacity)
        keeps_right = how in ("inner", "left")
        assert right is None or keeps_right, "join_rows(): a semi or anti join carries no right columns"

        def side(key, rows, n, count):
            assert len(key) in (2, 3), "join_rows(): a key is (types, values[, validity])"
            validity = key[2] if len(key) == 3 else None
            n_source = _key_column(key[0], key[1], validity, None)
            if rows is None:
                n = n_source if n is None else int(n)
                assert 0 <= n <= n_source
            else:
                assert rows.dim() == 1 and rows.dtype == torch.int64 and rows.is_contiguous()
                n = int(rows.numel()) if n is None else int(n)
                assert 0 <= n <= int(rows.numel())
            _check_row_count(count, key[1])
            return key[0], validity, key[1], n_source, n

        def carried(columns, n_source):
            if columns is None:
                return None, None, 0, 0
            n_cols, stride, _ = _column_set(columns[0], columns[1], n_source)
            return columns[0], columns[1], n_cols, stride

        l_types, l_validity, l_values, l_source, n_left = side(left_key, left_rows, n_left, left_count)
        lc_types, lc_values, l_cols, l_stride = carried(left, l_source)
        if right_sorted is None:
            r_types, r_validity, r_values, r_source, n_right = side(right_key, right_rows, n_right, right_count)
            order = torch.empty(n_right, dtype=torch.int64, device=self.device)
            sort_record = torch.empty(SORT_RESULT_WORDS, dtype=torch.int64, device=self.device)
            self.engine.sort_rows_device(_ptr(r_types, r_types is not None and r_source), _ptr(r_validity, r_validity is not None and r_source),
                                         _ptr(r_values, r_source), r_source, _ptr(right_rows, right_rows is not None and n_right), n_right,
                                         _ptr(right_count, right_count is not None), TOP_KINDS["long"], 0, 0, 0, 0, 0, _ptr(order, n_right), 0, 0,
                                         0, sort_record.data_ptr(), stream)
            right_sorted = (order, sort_record)
        else:
            r_types, r_validity, r_values, r_source, _ = side(right_key, None, None, None)
            order, sort_record = right_sorted
            assert order.dim() == 1 and order.dtype == torch.int64 and order.is_contiguous()
            assert sort_record.dtype == torch.int64 and sort_record.is_contiguous() and int(sort_record.numel()) == SORT_RESULT_WORDS
            n_right = int(order.numel())
        rc_types, rc_values, r_cols, r_stride = carried(right, r_source)
        out_left = torch.empty(pair_capacity, dtype=torch.int64, device=self.device)
        out_right = torch.empty(pair_capacity, dtype=torch.int64, device=self.device) if keeps_right else None
        left_types = torch.empty((l_cols, pair_capacity), dtype=torch.uint8, device=self.device)
        left_values = torch.empty((l_cols, pair_capacity), dtype=torch.int64, device=self.device)
        right_types = torch.empty((r_cols, pair_capacity), dtype=torch.uint8, device=self.device)
        right_values = torch.empty((r_cols, pair_capacity), dtype=torch.int64, device=self.device)
        pair_offsets = torch.empty(n_left + 1, dtype=torch.int64, device=self.device) if with_offsets else None
        record = torch.empty(JOIN_RESULT_WORDS, dtype=torch.int64, device=self.device)  # sjmi_join_result (every call writes all of it)
        self.engine.join_rows_device(
            (_ptr(l_types, l_types is not None and l_source), _ptr(l_validity, l_validity is not None and l_source), _ptr(l_values, l_source),
             l_source, _ptr(lc_types, l_cols), _ptr(lc_values, l_cols), l_cols, l_stride),
            _ptr(left_rows, left_rows is not None and n_left), n_left, _ptr(left_count, left_count is not None),
            (_ptr(r_types, r_types is not None and r_source), _ptr(r_validity, r_validity is not None and r_source), _ptr(r_values, r_source),
             r_source, _ptr(rc_types, r_cols), _ptr(rc_values, r_cols), r_cols, r_stride),
            _ptr(order, n_right), n_right, _ptr(sort_record, n_right), JOIN_HOWS[how], pair_capacity, _ptr(out_left, pair_capacity),
            _ptr(out_right, keeps_right and pair_capacity), _ptr(left_types, l_cols * pair_capacity), _ptr(left_values, l_cols * pair_capacity),
            _ptr(right_types, r_cols * pair_capacity), _ptr(right_values, r_cols * pair_capacity), pair_capacity if l_cols or r_cols else 0,
            _ptr(pair_offsets, with_offsets), record.data_ptr(), stream)
        return out_left, out_right, left_types, left_values, right_types, right_values, pair_offsets, record, right_sorted

    def parent_columns(self, row_offsets, types, values, rows=None, n_rows=None, row_count=None, with_parents=True, stream=0):
        """The document of every exploded row, and that document's cells on the row (pandas.json_normalize's meta, SQL's UNNEST
        with the outer row's columns): sjmi_parent_columns_device on the row offsets of explode() ([n_docs + 1] int64) and the
        2-D [n_cols, stride] (types uint8, values int64) pair of DOCUMENT columns -- sel_types / sel_values; stride at least
        n_docs -- or None for both to get the parents only.  rows=None is the dense form: slot i is row i, n_rows is required
        (normally the explode's row_capacity) and row_count is normally row_offsets[n_docs:].  With rows (1-D int64: filter()'s
        or top_rows()' rows, in any order, duplicates legal) slot i is row rows[i] and n_rows defaults to rows.numel().
        row_count as for arrow_columns(): the live slots are min(n_rows, row_count[0]).  -> (parent_types [n_rows] uint8,
        parents [n_rows] int64 -- one typed long column: 'l' and the document, MISSING and -1 for a row at or above
        row_offsets[n_docs], an orphan; both None with with_parents=False --, out_types [n_cols, n_rows] uint8, out_values
        [n_cols, n_rows] int64: the layout of filter()'s compacted pair, an orphan's cells MISSING and 0; result [3] int64 = live
        slots, n_orphans, flags), new tensors every call; slots at or behind the live ones are not written.  Nothing
        synchronises.  Call it on a step that check() has accepted: like filter(), it is not queued again behind a step that
        check() had to run again."""
        import torch
        assert row_offsets.dim() == 1 and row_offsets.dtype == torch.int64 and row_offsets.is_contiguous() and int(row_offsets.numel()) >= 1
        n_docs = int(row_offsets.numel()) - 1
        if rows is None:
            assert n_rows is not None, "parent_columns(): the dense form needs n_rows"
            n_rows = int(n_rows)
        else:
            assert rows.dim() == 1 and rows.dtype == torch.int64 and rows.is_contiguous()
            n_rows = int(rows.numel()) if n_rows is None else int(n_rows)
            assert n_rows <= int(rows.numel())
        assert n_rows >= 0
        _check_row_count(row_count, row_offsets)
        n_cols = stride = 0
        if types is not None:
            n_cols, stride, _ = _column_set(types, values, n_docs)
            assert n_cols <= PARENT_MAX_COLS
        parent_types = torch.empty(n_rows, dtype=torch.uint8, device=self.device) if with_parents else None
        parents = torch.empty(n_rows, dtype=torch.int64, device=self.device) if with_parents else None
        # (without a slot or without a document cell there is nothing to carry, and an empty tensor has no pointer to give: every
        # cell of the outputs is then an orphan's)
        carry = n_cols if n_rows and stride else 0
        make = torch.empty if carry == n_cols else torch.zeros
        out_types = make((n_cols, n_rows), dtype=torch.uint8, device=self.device)
        out_values = make((n_cols, n_rows), dtype=torch.int64, device=self.device)
        result = torch.empty(PARENT_RESULT_WORDS, dtype=torch.int64, device=self.device)  # sjmi_parent_result (every call writes all of it)
        self.engine.parent_columns_device(row_offsets.data_ptr(), n_docs, _ptr(rows, rows is not None and n_rows), n_rows,
                                          _ptr(row_count, row_count is not None), _ptr(types, carry), _ptr(values, carry), carry, stride,
                                          _ptr(parent_types, with_parents and n_rows), _ptr(parents, with_parents and n_rows),
                                          _ptr(out_types, carry), _ptr(out_values, carry), n_rows, result.data_ptr(), stream)
        return parent_types, parents, out_types, out_values, result

    def explode_with_parents(self, plan, row_capacity, doc_types, doc_values, stream=0):
        """explode() joined with the documents' columns in ONE column set: sjmi_explode_batch_device into the first
        plan.n_columns rows of types / values [n_columns + n_doc_cols + 1, row_capacity], then, on the same stream,
        sjmi_parent_columns_device (dense, row count = the explode's last row offset, read on the device) into the rest: the
        n_doc_cols DOCUMENT columns doc_types / doc_values (a 2-D [n_doc_cols, stride] pair, sel_types / sel_values) carried
        onto the rows come next, and the parent-id column -- 'l' and the row's document -- comes last.  -> (row_offsets
        [n_docs + 1] int64, types uint8, values int64, result [3] int64 = live rows, n_orphans, flags), tensors of its own on
        every call: exp_* and what check() queues again are left alone.  The columns of rows at or behind row_offsets[n_docs]
        are not written.  Nothing synchronises.  Call it on a step that check() has accepted: like filter(), it is not queued
        again behind a step that check() had to run again."""
        import torch
        row_capacity = int(row_capacity)
        n_doc_cols, stride, _ = _column_set(doc_types, doc_values, self.n_docs)
        assert n_doc_cols <= PARENT_MAX_COLS
        n_columns = getattr(plan, "n_columns", plan.n_paths)
        row_offsets = torch.zeros(self.n_docs + 1, dtype=torch.int64, device=self.device)
        types = torch.zeros((n_columns + n_doc_cols + 1, row_capacity), dtype=torch.uint8, device=self.device)
        values = torch.zeros((n_columns + n_doc_cols + 1, row_capacity), dtype=torch.int64, device=self.device)
        result = torch.empty(PARENT_RESULT_WORDS, dtype=torch.int64, device=self.device)  # sjmi_parent_result
        self.engine.explode_batch_device(plan, self.tape.data_ptr(), self.tape_offsets.data_ptr(), self.doc_errors.data_ptr(),
                                         self.sb.data_ptr(), self.n_docs, row_offsets.data_ptr(), row_capacity,
                                         _ptr(types, row_capacity), _ptr(values, row_capacity), stream)
        head, last = n_columns * row_capacity, (n_columns + n_doc_cols) * row_capacity  # cells in front of the carried columns / the ids
        at = lambda t, cells: t.data_ptr() + cells * t.element_size() if row_capacity else 0
        carry = n_doc_cols if row_capacity and stride else 0  # (no row or no document cell: nothing to carry, the cells stay MISSING)
        self.engine.parent_columns_device(row_offsets.data_ptr(), self.n_docs, 0, row_capacity, row_offsets.data_ptr() + 8 * self.n_docs,
                                          _ptr(doc_types, carry), _ptr(doc_values, carry), carry, stride, at(types, last), at(values, last),
                                          at(types, head), at(values, head), row_capacity, result.data_ptr(), stream)
        return row_offsets, types, values, result

    def group_by_string(self, key_types, key_values, val_types, val_values, dict_capacity, row_count=None, stream=0):
        """"Total and largest <value> per <key>": dictionary_column() on the 1-D key column (its string cells point into self.sb),
        then group_stats() on the 1-D value column with the same rows.  A convenience with host readbacks (the dictionary's
        size and bytes, the results), in the manner of discover_keys(), on a step that check() has accepted; the C calls stay
        asynchronous.  -> ([(key bytes, decode_group_stats()'s dict)] in the order of first occurrence, the sjmi_dict_result [6]
        and the sjmi_group_result [5] (numpy int64)).  Rows whose key cell is no string belong to no key.  Raises RuntimeError
        naming dict_capacity when there are more distinct keys than it (SJMI_DICT_OVERFLOW)."""
        import torch
        sync = lambda: torch.cuda.synchronize(self.device) if _on_gpu(self.device) else None
        indices, validity, _, dict_offsets, dict_bytes, dres = self.dictionary_column(key_types, key_values, dict_capacity, row_count=row_count,
                                                                                       stream=stream)
        sync()
        d = dres.cpu().numpy()
        if int(d[5]) & 1:
            raise RuntimeError("group_by_string(): more distinct keys than dict_capacity = %d (SJMI_DICT_OVERFLOW)" % dict_capacity)
        n_keys = int(d[3])
        stats, gres = self.group_stats(indices, validity, val_types, val_values, n_keys, row_count=row_count, stream=stream)
        sync()
        ends, raw = dict_offsets[:n_keys + 1].cpu().numpy(), bytes(dict_bytes.cpu().numpy())
        decoded = decode_group_stats(stats.cpu().numpy())
        return [(raw[int(ends[j]):int(ends[j + 1])], decoded[j]) for j in range(n_keys)], d, gres.cpu().numpy()

    def discover_keys(self, base_pointer="", dict_capacity=4096, stream=0):
        """"Which keys are in here, and what types do they hold?" for the object at base_pointer of every document: a members
        explode with the one element pointer "" (a sizing call, then the full one), dictionary_column() on its key column and
        key_census() on its type column, both with the explode's last row offset as the device row count.  A convenience with
        host readbacks (the row total, the dictionary's byte size, the results), on a step that check() has accepted; the C
        calls stay asynchronous.  -> ([(key bytes, [8 counts by class])] in the order of first occurrence, the row offsets
        [n_docs + 1] (numpy), the sjmi_dict_result [6] and the sjmi_census_result [4] (numpy int64)).  Raises RuntimeError
        naming dict_capacity when there are more distinct keys than it (SJMI_DICT_OVERFLOW)."""
        import torch
        from .binding import ExplodePlan
        sync = lambda: torch.cuda.synchronize(self.device) if _on_gpu(self.device) else None
        plan = ExplodePlan(base_pointer, [""], members=True)
        try:
            offs = self.explode(plan, 0, stream)[0]
            sync()
            total = int(offs[self.n_docs].cpu())
            offs, types, values = self.explode(plan, total, stream)
            row_count = offs[self.n_docs:]
            indices, validity, _, dict_offsets, dict_bytes, dres = self.dictionary_column(types[1], values[1], dict_capacity, row_count=row_count,
                                                                                           stream=stream)
            sync()
            d = dres.cpu().numpy()
            if int(d[5]) & 1:
                raise RuntimeError("discover_keys(%r): more distinct keys than dict_capacity = %d (SJMI_DICT_OVERFLOW)" % (base_pointer, dict_capacity))
            n_keys = int(d[3])
            counts, cres = self.key_census(indices, validity, types[0], n_keys, row_count=row_count, stream=stream)
            sync()
            ends, raw = dict_offsets[:n_keys + 1].cpu().numpy(), bytes(dict_bytes.cpu().numpy())
            table = counts.cpu().numpy()
            keys = [(raw[int(ends[j]):int(ends[j + 1])], [int(x) for x in table[j]]) for j in range(n_keys)]
            return keys, offs.cpu().numpy(), d, cres.cpu().numpy()
        finally:
            self._exp_pending = None  # (the plan does not outlive this call: check() has nothing to queue again)
            self._exp_plan = None
            plan.close()

    def counts_tensor(self):
        """The per-shard row of the count gather, on the device, without a host copy:
        {documents, structurals, string bytes, failed + handed-back documents}."""
        import torch
        r = self.result
        return torch.cat([self._ndocs, r[0:1], r[2:3], r[6:7] + r[7:8]])

    def _record(self):
        """sjmi_batch_result on the host -> (the 9 words, stage-1 status, string-pass flags, walk flags)"""
        r = self.result.cpu().numpy()
        return r, int(r[1]) & 0xFFFFFFFF, int(r[4]) & 0xFFFFFFFF, int(r[8]) & 0xFFFFFFFF

    def check(self):
        """Host-side verdict of the last step (synchronise first): raises if a capacity was exceeded."""
        r, st1, sflags, wflags = self._record()
        if st1 & SJMI_ST_REJECTED:  # not a batch for the optimistic pipeline -- the exact call, here, off the hot path
            import torch
            pending, exp_pending = self._sel_pending, self._exp_pending
            self.rejected_steps += 1
            if not (st1 & 0xFF):
                self.format_rejected = True  # (a clean stage-1 verdict and still rejected: the separators)
            for entry in ({"rejected": True}, {"exact": True}):
                # the call for rejected batches (repair on the device); a batch it cannot take either -- documents that are not
                # separated AND let a scalar run on across a boundary -- says REJECTED once more and is the exact call's
                self.step(self._last_stream, **entry)
                if pending is not None:  # the select that was queued behind the rejected step read outputs that were not valid
                    self.select(*pending)
                if exp_pending is not None:  # ... and so did the explode
                    self.explode(*exp_pending)
                if _on_gpu(self.device):
                    torch.cuda.synchronize(self.device)
                r, st1, sflags, wflags = self._record()
                if not (st1 & SJMI_ST_REJECTED):
                    break
                self.format_rejected = False  # (... and so are the batches behind it: the latch below moves to the exact call)
                self.unrepairable = True
        if st1 & (SJMI_ST_CAPACITY | SJMI_ST_INTERNAL):
            raise RuntimeError("stage 1 of the shard: capacity / internal error (status 0x%x)" % st1)
        if sflags & 1:
            raise RuntimeError("string buffer capacity exceeded")
        if sflags & 2:  # (the walkers read record offsets by string ordinal: with the table short they walk nothing)
            raise RuntimeError("more strings than the record table holds: index capacity exceeded")
        if sflags & 0xC:
            raise RuntimeError("string pass: engine fault (flags 0x%x)" % sflags)
        if wflags & 1:
            raise RuntimeError("tape capacity exceeded")
        return {"documents": self.n_docs, "structurals": int(r[0]), "string_bytes": int(r[2]), "tape_words": int(r[5]),
                "host_documents": int(r[6]), "failed_documents": int(r[7]), "stage1_status": st1 & 0xFF}


def sharded_step(shard, stream=0, always_gather=False):
    """One step of the multi-GPU batched path on this rank: the shard's kernels, then the count gather (the ONLY
    collective, north_star).  -> gathered [world, 4] int64 tensor on the shard's device.  always_gather: issue the
    collective even in a group of one rank (bench.py --sharded: the RCCL call path on a single GPU)."""
    import torch
    import torch.distributed as dist
    side = None
    if not stream and _on_gpu(shard.device):
        # stream handle 0 means "the engine context's own stream" to the C ABI -- and it is also the handle of torch's legacy
        # default stream, so it cannot name that one.  The torch ops that read the result record below must be ordered behind
        # the kernels: the kernels go on a side stream of the shard's, fenced against the caller's current stream on both
        # sides with events (wait_stream) -- stream order only, no host synchronisation anywhere in the step.
        cur = torch.cuda.current_stream(shard.device)
        if cur.cuda_stream:
            stream = cur.cuda_stream
        else:
            side = shard._side_stream
            if side is None:
                side = shard._side_stream = torch.cuda.Stream(device=shard.device)
            side.wait_stream(cur)
            stream = side.cuda_stream
    shard.step(stream)
    if side is not None:
        torch.cuda.current_stream(shard.device).wait_stream(side)
    row = shard.counts_tensor()
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not always_gather):
        return row[None, :]
    out = torch.empty(dist.get_world_size() * 4, dtype=torch.int64, device=shard.device)
    dist.all_gather_into_tensor(out, row)
    return out.view(dist.get_world_size(), 4)


# ---------------------------------------------------------------------------------------------------------------------
# ONE document over several GPUs / as a stream of chunks
# ---------------------------------------------------------------------------------------------------------------------
def split_points(n_bytes, parts, align=64):
    """Contiguous byte ranges [(a, b)] covering [0, n_bytes): every boundary a multiple of `align` (stage 1 works in
    64-byte blocks; a shard that is not the last one has no tail block), about equal sizes."""
    bounds = [0]
    for r in range(1, parts):
        b = (n_bytes * r // parts) // align * align
        bounds.append(max(b, bounds[-1]))
    bounds.append(n_bytes)
    return [(bounds[r], bounds[r + 1]) for r in range(parts)]


class HaloTooShort(RuntimeError):
    """SJMI_ST_HALO: a backslash run fills the whole left halo of a shard / chunk -- repeat with a larger one"""


class DocumentShard:
    """One rank's shard [a, b) of a document, resident on its device together with `halo` bytes of the document in front
    of it (the carries stage 1 needs are re-derived from them; only the in-string parity has to come from the ranks in
    front).  `data` = the document's bytes [a - halo, b) (bytes or a uint8 tensor)."""

    def __init__(self, engine, data, halo, is_last, device, index_ratio=1, halo_from_start=False):
        import torch
        self.engine, self.device, self.halo, self.is_last = engine, device, int(halo), bool(is_last)
        self.halo_from_start = bool(halo_from_start)  # the halo begins at the document's first byte
        total = int(data.numel()) if hasattr(data, "numel") else len(data)
        self.length = total - self.halo
        assert self.halo % 64 == 0 and (self.is_last or self.length % 64 == 0)
        self.buf = _upload(data, device, 128)
        self.capacity = self.length // index_ratio + 66
        self.idx = torch.empty(self.capacity, dtype=torch.int32, device=device)
        self.result = torch.zeros(2, dtype=torch.int64, device=device)  # sjmi_stage1_result
        self.entry_parity = 0

    def run(self, entry_parity, stream=0):
        self.entry_parity = int(entry_parity)
        self.engine.stage1_shard_device(self.buf.data_ptr() + self.halo, self.length, self.halo, self.is_last, self.entry_parity,
                                        self.idx.data_ptr(), self.capacity, self.result.data_ptr(), stream,
                                        halo_from_start=self.halo_from_start)

    def outcome(self):
        """(synchronise first) -> (count, status bits without UNCLOSED, parity after the shard)"""
        r = self.result.cpu().numpy()
        st = int(r[1]) & 0xFFFFFFFF
        if st & (SJMI_ST_CAPACITY | SJMI_ST_INTERNAL):
            raise RuntimeError("stage 1 of the shard: capacity / internal error (status 0x%x)" % st)
        if st & SJMI_ST_HALO:
            raise HaloTooShort("a backslash run fills the %d bytes of halo in front of the shard" % self.halo)
        return int(r[0]), st & 0xFD, (st >> 1) & 1


def resolve_split_document(shard, sync):
    """The protocol of a document split over the ranks of the default process group (or a single process):
      1. every rank scans its shard as if it started outside a string;
      2. all_gather of one word per rank: does the shard flip the in-string parity?  (the first collective)
      3. a rank whose true entry parity is 1 (XOR of the flips in front of it) scans again with entry parity 1;
      4. all_gather of {count, status, parity after}: global index offsets, the document's verdict.
    `sync` = a callable that synchronises the rank's stream.  -> dict(entry_parity, count, offset, total, status)
    where status has SJMI_ST_UNCLOSED set iff the LAST shard ends inside a string."""
    import torch
    import torch.distributed as dist
    multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank = dist.get_rank() if multi else 0
    world = dist.get_world_size() if multi else 1
    shard.run(0)
    sync()
    _, _, flip = shard.outcome()  # entered with parity 0: the parity after IS the flip
    flips = torch.tensor([flip], dtype=torch.int64, device=shard.device)
    if multi:
        allf = torch.empty(world, dtype=torch.int64, device=shard.device)
        dist.all_gather_into_tensor(allf, flips)
    else:
        allf = flips
    entry = int(allf[:rank].sum().item()) & 1
    if entry:
        shard.run(1)
        sync()
    count, st, after = shard.outcome()
    row = torch.tensor([count, st, after], dtype=torch.int64, device=shard.device)
    if multi:
        allr = torch.empty(world * 3, dtype=torch.int64, device=shard.device)
        dist.all_gather_into_tensor(allr, row)
        allr = allr.view(world, 3)
    else:
        allr = row[None, :]
    a = allr.cpu().numpy()
    status = 0
    for r in range(world):
        status |= int(a[r, 1])
    if int(a[world - 1, 2]):
        status |= 2  # SJMI_ST_UNCLOSED: the document ends inside a string
    return {"entry_parity": entry, "count": count, "offset": int(a[:rank, 0].sum()), "total": int(a[:, 0].sum()), "status": status}


def stream_document(engine, device, chunks, halo=64):
    """Document-stream mode on ONE GPU: the chunks of a document (bytes; every chunk but the last a multiple of 64 long)
    are scanned one after the other, the in-string parity carried from chunk to chunk, each chunk seeing `halo` bytes of
    its predecessor.  -> (list of (base offset, indexes np.uint32 relative to the chunk), status)."""
    import numpy as np
    import torch
    out, status, parity, base, tail = [], 0, 0, 0, b""
    keep = max(halo, 4096)  # bytes of the stream kept for the halo (a chunk is repeated with more of them on SJMI_ST_HALO)
    for k, ch in enumerate(chunks):
        last = k == len(chunks) - 1
        want = halo
        while True:
            h = min(want, len(tail)) // 64 * 64
            sh = DocumentShard(engine, tail[len(tail) - h:] + ch if h else ch, h, last, device, halo_from_start=(h == base))
            sh.run(parity)
            torch.cuda.synchronize()
            try:
                count, st, after = sh.outcome()
                break
            except HaloTooShort:
                if h >= len(tail) // 64 * 64:
                    raise  # (everything that is kept of the stream is backslashes)
                want *= 4
        parity = after
        status |= st
        out.append((base, sh.idx[:count].cpu().numpy().view(np.uint32).copy()))
        base += len(ch)
        tail = (tail + ch)[-keep:]
    if parity:
        status |= 2
    return out, status
