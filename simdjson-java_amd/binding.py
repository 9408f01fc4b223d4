"""ctypes binding of libsjmi.so (C ABI: include/sjmi.h).  No compute happens in Python and nothing
here falls back to a CPU path: a missing library or GPU raises SjmiError."""
import atexit
import ctypes as C
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_CSRC = os.path.join(_HERE, "csrc")
_LIB = os.path.join(_HERE, "libsjmi.so")
SOURCES = ["stage1.hip", "strings.hip", "batch.hip", "walk.hip", "coop_walk.hip", "masks.hip", "select.hip", "explode.hip", "ndjson.hip", "strcol.hip", "filter.hip", "arrowcol.hip", "timecol.hip", "dictcol.hip", "census.hip", "groupstats.hip", "toprows.hip", "sortrows.hip", "parents.hip", "joinrows.hip", "sjmi_api.hip", "host/simdjson_parser.cpp"]

ST_UTF8, ST_UNCLOSED, ST_UNESCAPED, ST_CAPACITY, ST_INTERNAL = 1, 2, 4, 0x100, 0x200
PADDING = 64

_MESSAGES = {  # exact reference messages (Utf8Validator.java:166, StructuralIndexer.java:298,301)
    ST_UTF8: "The input is not valid UTF-8",
    ST_UNCLOSED: "Unclosed string. A string is opened, but never closed.",
    ST_UNESCAPED: "Unescaped characters. Within strings, there are characters that should be escaped.",
}


class SjmiError(RuntimeError):
    pass


def status_message(status):
    """Message of the JsonParsingException SimdJsonParser.stage1 would throw (first check wins)."""
    for bit in (ST_UTF8, ST_UNCLOSED, ST_UNESCAPED):
        if status & bit:
            return _MESSAGES[bit]
    return None


def lib_path():
    return _LIB


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> simdjson-java_amd/libsjmi.so (in-tree; cross-compiles without a GPU).  Under a file lock
    with the staleness check repeated behind it (N ranks of a node that find the library stale at the same time: one builds, the
    others wait and load its result); every source compiled to an object of its own (in parallel, only what changed), then linked
    into a temporary file that is renamed into place -- a process that loads the library never sees half of it."""
    import fcntl
    from concurrent.futures import ThreadPoolExecutor
    srcs = [os.path.join(_CSRC, s) for s in SOURCES]
    headers = [os.path.join(_CSRC, h) for h in os.listdir(_CSRC) if h.endswith(".h")] + \
        [os.path.join(_CSRC, "host", h) for h in os.listdir(os.path.join(_CSRC, "host")) if h.endswith(".h")] + \
        [os.path.join(_ROOT, "include", "sjmi.h")]
    newest = max(os.path.getmtime(d) for d in srcs + headers)
    fresh = lambda: os.path.exists(_LIB) and os.path.getmtime(_LIB) >= newest
    if not force and fresh():
        return _LIB
    objdir = os.path.join(_HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and fresh():
                return _LIB  # (another process built it while this one waited for the lock)
            newest_h = max(os.path.getmtime(h) for h in headers)
            flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-pthread", "-I", os.path.join(_ROOT, "include")]

            def compile_one(src):
                obj = os.path.join(objdir, os.path.basename(src) + ".o")
                if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), newest_h):
                    cmd = ["hipcc"] + flags + ["-c", src, "-o", obj]
                    if verbose:
                        print(" ".join(cmd))
                    subprocess.check_call(cmd)
                return obj

            with ThreadPoolExecutor(min(len(srcs), os.cpu_count() or 1)) as ex:
                objs = list(ex.map(compile_one, srcs))
            tmp = "%s.tmp.%d" % (_LIB, os.getpid())
            cmd = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-pthread"] + objs + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
            os.replace(tmp, _LIB)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return _LIB


_lib = None

# The C ABI, one line per function of include/sjmi.h, in the header's order: name -> (result, arguments).  lib() declares all of
# them on the loaded library, so a Python int always travels at the width the header says; tests/test_abi_exports.py holds the
# table against the header's prototypes.  P: any pointer (handles, buffers, out-parameters, a hipStream_t); PP: where a handle
# is returned; S: a C string.
P, PP, I, U32, U64, S = C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint64, C.c_char_p
_PARSE_BATCH = (P, P, U64, P, U64, P, U64, P, P, P, U64, P, I, P, U64, P, P, P, P)
ABI = {
    "sjmi_create": (I, (PP, I, U64)),
    "sjmi_destroy": (None, (P,)),
    "sjmi_last_error": (S, (P,)),
    "sjmi_version": (S, ()),
    "sjmi_stage1": (I, (P, P, U64, P, U64, P, P)),
    "sjmi_stage1_device": (I, (P, P, U64, P, U64, P, P)),
    "sjmi_stage1_masks": (I, (P, P, U64, P, U64, P)),
    "sjmi_stage1_masks_device": (I, (P, P, U64, P, U64, P)),
    "sjmi_stage1_shard_device": (I, (P, P, U64, U64, I, I, P, U64, P, P)),
    "sjmi_stage1_shard_device2": (I, (P, P, U64, U64, I, I, I, P, U64, P, P)),
    "sjmi_stream_open": (I, (P, U64, U64, PP)),
    "sjmi_stream_push": (I, (P, P, U64, I, P, U64, P, P, P)),
    "sjmi_stream_close": (None, (P,)),
    "sjmi_split_open": (I, (P, P, U64, U64, I, I, P, U64, PP)),
    "sjmi_split_scan": (I, (P, P, P, P)),
    "sjmi_split_resolve": (I, (P, I, P, P, P, P)),
    "sjmi_split_close": (None, (P,)),
    "sjmi_unescape_device": (I, (P, P, U64, P, U64, P, U64, P, P)),
    "sjmi_unescape": (I, (P, P, U64, P, P, P)),
    "sjmi_stage1_unescape": (I, (P, P, U64, P, U64, P, P, P, U64, P, P, P)),
    "sjmi_stage1_batch_device": (I, (P, P, U64, P, U64, P, U64, P, P, P)),
    "sjmi_stage1_batch": (I, (P, P, U64, P, U64, P, U64, P, P, P)),
    "sjmi_ndjson_offsets_device": (I, (P, P, U64, P, U64, P, P)),
    "sjmi_ndjson_offsets": (I, (P, P, U64, P, U64, P, P, P)),
    "sjmi_ndjson_tile_bytes": (U64, ()),
    "sjmi_stage1_batch_isolated_device": (I, (P, P, U64, P, U64, P, U64, P, P, P, P)),
    "sjmi_stage1_batch_isolated": (I, (P, P, U64, P, U64, P, U64, P, P, P, P)),
    "sjmi_unescape_batch": (I, (P, P, U64, P, P, P, P)),
    "sjmi_unescape_batch_device": (I, (P, P, U64, P, U64, P, P, U64, P, U64, P, P, P)),
    "sjmi_walk_batch_device": (I, (P, P, P, U64, P, U64, P, P, P, P, U64, I, P, U64, P, P, P, P)),
    "sjmi_parse_batch_device": (I, _PARSE_BATCH),
    "sjmi_parse_batch_device_optimistic": (I, _PARSE_BATCH),
    "sjmi_parse_batch_device_rejected": (I, _PARSE_BATCH),
    "sjmi_parse_document": (I, (P, P, U64, I, P, U64, P, P, U64, P, P, P)),
    "sjmi_parser_create": (I, (PP, I, I, I)),
    "sjmi_parser_destroy": (None, (P,)),
    "sjmi_parser_parse": (I, (P, P, U64, P, P, P, P, P)),
    "sjmi_parser_last_message": (S, (P,)),
    "sjmi_parser_set_gpu_walk": (I, (P, I)),
    "sjmi_parser_parse_batch": (I, (P, P, U64, P, U64, P, P, P, P, P)),
    "sjmi_parser_ondemand_init": (I, (P, P, U64, I)),
    "sjmi_od_skip_child": (I, (P, I)),
    "sjmi_od_get_boolean": (I, (P, I, I, P, P)),
    "sjmi_od_get_long": (I, (P, I, I, P, P)),
    "sjmi_od_get_integral": (I, (P, I, I, I, P, P)),
    "sjmi_od_get_double": (I, (P, I, I, P, P)),
    "sjmi_od_get_float": (I, (P, I, I, P, P)),
    "sjmi_od_get_char": (I, (P, I, I, P, P)),
    "sjmi_od_get_string": (I, (P, I, P, P, P)),
    "sjmi_od_get_field_name": (I, (P, P, P)),
    "sjmi_od_start_array": (I, (P, I, P)),
    "sjmi_od_next_array_element": (I, (P, P)),
    "sjmi_od_start_object": (I, (P, I, P)),
    "sjmi_od_next_object_field": (I, (P, P)),
    "sjmi_od_move_to_field_value": (I, (P,)),
    "sjmi_od_assert_no_more_values": (I, (P,)),
    "sjmi_od_depth": (I, (P,)),
    "sjmi_od_peek": (I, (P,)),
    "sjmi_parser_root": (I, (P, P)),
    "sjmi_parser_batch_root": (I, (P, U64, P)),
    "sjmi_value_type": (I, (P, P)),
    "sjmi_value_as_long": (I, (P, P, P)),
    "sjmi_value_as_double": (I, (P, P, P)),
    "sjmi_value_as_boolean": (I, (P, P, P)),
    "sjmi_value_as_string": (I, (P, P, P, U64, P)),
    "sjmi_value_get": (I, (P, P, P, U64, P)),
    "sjmi_value_size": (I, (P, P)),
    "sjmi_value_first": (I, (P, P, P)),
    "sjmi_value_next": (I, (P, P, P, P)),
    "sjmi_select_plan_compile": (I, (P, P, U64, PP)),
    "sjmi_select_plan_destroy": (None, (P,)),
    "sjmi_select_batch_device": (I, (P, P, P, P, P, P, U64, P, P, P)),
    "sjmi_explode_plan_compile": (I, (P, U64, P, P, U64, PP)),
    "sjmi_explode_plan_destroy": (None, (P,)),
    "sjmi_explode_members_plan_compile": (I, (P, U64, P, P, U64, PP)),
    "sjmi_explode_batch_device": (I, (P, P, P, P, P, P, U64, P, U64, P, P, P)),
    "sjmi_string_column_device": (I, (P, P, P, U64, P, P, P, P, U64, P, P)),
    "sjmi_filter_plan_compile": (I, (P, U64, P, U64, PP)),
    "sjmi_filter_plan_destroy": (None, (P,)),
    "sjmi_filter_columns_device": (I, (P, P, P, P, U64, U64, U64, P, P, P, U64, P, P, P, P)),
    "sjmi_arrow_columns_device": (I, (P, P, U64, P, P, U64, U64, U64, P, P, U64, P, U64, P, P)),
    "sjmi_time_columns_device": (I, (P, P, U64, P, P, U64, U64, U64, P, P, P, U64, P, U64, P, P)),
    "sjmi_dictionary_column_device": (I, (P, P, P, U64, P, P, P, P, U64, P, P, P, U64, P, P)),
    "sjmi_key_census_device": (I, (P, P, P, P, U64, P, U64, P, P, P)),
    "sjmi_group_stats_device": (I, (P, P, P, P, P, U64, P, U64, P, P, P)),
    "sjmi_top_rows_device": (I, (P, P, P, P, U64, P, U32, U32, U64, P, P, U64, U64, P, P, P, P, P)),
    "sjmi_sort_rows_device": (I, (P, P, P, P, U64, P, U64, P, U32, U32, P, P, U64, U64, P, P, P, U64, P, P)),
    "sjmi_parent_columns_device": (I, (P, P, U64, P, U64, P, P, P, U64, U64, P, P, P, P, U64, P, P)),
    "sjmi_join_rows_device": (I, (P, P, P, U64, P, P, P, U64, P, U32, U64, P, P, P, P, P, P, U64, P, P, P)),
    "sjmi_host_register": (I, (P, P, U64)),
    "sjmi_set_input_staging": (I, (P, P, U64)),
    "sjmi_host_unregister": (I, (P, P)),
    "sjmi_selftest": (I, (P, P)),
    "sjmi_set_tile_steps": (I, (P, I)),
    "sjmi_set_tile_mode": (I, (P, I)),
    "sjmi_set_auto_safe": (I, (P, I)),
    "sjmi_set_profiling": (I, (P, I)),
    "sjmi_debug_set_flags": (I, (P, U32)),
    "sjmi_debug_counters": (I, (P, P)),
    "sjmi_kernel_time": (I, (P, P, P)),
}
EXPORTS = list(ABI)


# Handles that are still open when the interpreter exits are closed HERE, in an atexit hook -- i.e. while the HIP runtime
# (PyTorch's instance) is still up.  Left to __del__ during interpreter finalisation they would call hipFree /
# hipStreamDestroy in an arbitrary order relative to the runtime's own teardown, which can abort the process after the
# work is done (seen once as a core dump at the end of a GPU test run).
_live = weakref.WeakSet()
_exiting = False


def _close_all_at_exit():
    global _exiting
    for obj in list(_live):
        try:
            obj.close()
        except Exception:
            pass
    _exiting = True


atexit.register(_close_all_at_exit)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise SjmiError("libsjmi.so is not built (run __graft_entry__.build()); there is no CPU fallback")
        try:
            # PyTorch-ROCm bundles its own libamdhip64; load it first so that libsjmi.so binds to the same
            # HIP runtime instance (two runtimes in one process cannot both own the GPU).
            import torch  # noqa: F401
        except ImportError:
            pass
        # (SJMI_LIB: an experiment build of the same sources, tools/build_variant.sh -- A/B measurements only)
        L = C.CDLL(os.environ.get("SJMI_LIB") or _LIB)
        for name, (restype, argtypes) in ABI.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, list(argtypes)
        _lib = L
    return _lib


def _fields(fields, dtype, what, whats, flag_bits):
    """the encoder under arrow_fields() and time_fields(): tuples (column, <what>[, flag ...]) -> the 16-byte field array of `dtype`"""
    if isinstance(fields, np.ndarray) and fields.dtype == dtype:
        return np.ascontiguousarray(fields)
    enc = np.zeros(len(fields), dtype=dtype)
    for k, field in enumerate(fields):
        column, name, flags = field[0], field[1], field[2:]
        if name not in whats or any(f not in flag_bits for f in flags) or not 0 <= int(column) < 1 << 32:
            raise ValueError("%s field %d: unknown %s or flag, or column out of range: %r" % (what[0], k, what[1], (field,)))
        bits = 0
        for f in flags:
            bits |= flag_bits[f]
        enc[k] = (int(column), whats[name], bits, 0)
    return enc


JOIN_HOWS = {"inner": 0, "left": 1, "semi": 2, "anti": 3}  # SJMI_JOIN_<HOW>
JOIN_INNER, JOIN_LEFT, JOIN_SEMI, JOIN_ANTI = 0, 1, 2, 3
JOIN_OVERFLOW, JOIN_BAD_ROW, JOIN_BAD_ORDER = 1, 2, 4    # SJMI_JOIN_<FLAG>: the flags of a sjmi_join_result
JOIN_NO_ROW, JOIN_RESULT_WORDS = 0xFFFFFFFFFFFFFFFF, 9  # SJMI_JOIN_NO_ROW (-1 as an int64), SJMI_JOIN_RESULT_WORDS
JOIN_SIDE = np.dtype([("d_key_types", "<u8"), ("d_key_validity", "<u8"), ("d_key_values", "<u8"), ("n_source_rows", "<u8"),
                      ("d_types", "<u8"), ("d_values", "<u8"), ("n_cols", "<u8"), ("col_stride", "<u8")])  # sjmi_join_side


def join_side(d_key_types, d_key_validity, d_key_values, n_source_rows, d_types=0, d_values=0, n_cols=0, col_stride=0):
    """one side of Context.join_rows_device as the C struct (a numpy record in host memory): the key column of n_source_rows rows
    as sort_rows_device takes it, and n_cols carried columns col_stride cells apart (None / 0 with n_cols 0)"""
    side = np.zeros(1, dtype=JOIN_SIDE)
    side[0] = (d_key_types or 0, d_key_validity or 0, d_key_values or 0, n_source_rows, d_types or 0, d_values or 0, n_cols, col_stride)
    return side


ARROW_KINDS = {"int64": 1, "float64": 2, "bool": 3}     # SJMI_ARROW_<KIND>
ARROW_FLAGS = {"integral_doubles": 1}                   # SJMI_ARROW_F_*
ARROW_FIELD = np.dtype([("column", "<u4"), ("kind", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])  # sjmi_arrow_field


def arrow_fields(fields):
    """(column, kind[, flag ...]) tuples -> the sjmi_arrow_field array of Context.arrow_columns_device (an array of that dtype is
    taken as it is: the library validates it).  ValueError for a kind or a flag that has no name here."""
    return _fields(fields, ARROW_FIELD, ("arrow", "kind"), ARROW_KINDS, ARROW_FLAGS)


TIME_UNITS = {"s": 0, "ms": 1, "us": 2, "ns": 3}        # SJMI_TIME_<UNIT>, under Arrow's names
TIME_FLAGS = {"naive_utc": 1}                           # SJMI_TIME_F_*
TIME_FIELD = np.dtype([("column", "<u4"), ("unit", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])  # sjmi_time_field


def time_fields(fields):
    """(column, unit[, flag ...]) tuples such as (0, "us") or (2, "ns", "naive_utc") -> the sjmi_time_field array of
    Context.time_columns_device (an array of that dtype is taken as it is: the library validates it).  ValueError for a unit or a
    flag that has no name here."""
    return _fields(fields, TIME_FIELD, ("time", "unit"), TIME_UNITS, TIME_FLAGS)


class Context:
    """One sjmi_ctx: the engine-side state of one SimdJsonParser (SimdJsonParser.java:19-26)."""

    def __init__(self, device=0, capacity=34 * 1024 * 1024):
        self._h = C.c_void_p()
        rc = lib().sjmi_create(C.byref(self._h), device, capacity)
        if rc != 0:
            self._h = C.c_void_p()
            raise SjmiError("sjmi_create failed (rc=%d): no usable MI355X / HIP device; there is no CPU fallback" % rc)
        self.capacity = capacity
        _live.add(self)
        if os.environ.get("SJMI_TICKET_MODE") == "1":  # several processes on ONE GPU (bench.py's oversubscribed test mode): the FAST
            self.set_tile_mode(True)                   # kernel's whole grid cannot be resident beside another process's -- SAFE mode from the start
        if os.environ.get("SJMI_TILE_STEPS"):  # (experiments: the granule size of every stage-1 launch, sjmi_set_tile_steps)
            self.set_tile_steps(int(os.environ["SJMI_TILE_STEPS"]))

    def close(self):
        if self._h:
            lib().sjmi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if _exiting:
            return
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise SjmiError("%s failed (rc=%d): %s" % (what, rc, lib().sjmi_last_error(self._h).decode()))

    def selftest(self):
        mm = C.c_uint32(1)
        self._check(lib().sjmi_selftest(self._h, C.addressof(mm)), "sjmi_selftest")
        return mm.value

    def set_tile_steps(self, steps):
        self._check(lib().sjmi_set_tile_steps(self._h, steps), "sjmi_set_tile_steps")

    def stage1(self, data, length=None, index_capacity=None, idx=None):
        """Host-buffer path (SimdJsonParser.stage1 + padIfNeeded): -> (indexes incl. sentinel stripped, status).
        idx: the caller's own np.uint32 index array (e.g. page-locked: the zero-copy path)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n = a.size if length is None else length
        cap = ((n + 2) if index_capacity is None else index_capacity) if idx is None else idx.size
        if idx is None:
            idx = np.empty(max(cap, 1), dtype=np.uint32)
        cnt = C.c_uint64(0)
        st = C.c_uint32(0)
        ptr = a.ctypes.data if a.size else None
        self._check(lib().sjmi_stage1(self._h, ptr, n, idx.ctypes.data, cap, C.addressof(cnt), C.addressof(st)),
                    "sjmi_stage1")
        assert idx[cnt.value] == 0, "sentinel missing"
        return idx[:cnt.value].copy(), st.value

    def parse_document(self, data, length=None, max_depth=1024):
        """sjmi_parse_document: all three stages on the GPU -> (tape np.uint64 or None, string buffer bytes, error code,
        stage-1 status)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        n = a.size if length is None else length
        tape = np.zeros(2 * n + 16, dtype=np.uint64)
        sb = np.zeros(n + 4 * (n // 2 + 2) + 64, dtype=np.uint8)
        tl, sl = C.c_uint64(0), C.c_uint64(0)
        err = C.c_int32(0)
        st = C.c_uint32(0)
        self._check(lib().sjmi_parse_document(self._h, a.ctypes.data if a.size else None, n, max_depth, tape.ctypes.data, tape.size,
                                              C.addressof(tl), sb.ctypes.data, sb.size, C.addressof(sl), C.addressof(err),
                                              C.addressof(st)), "sjmi_parse_document")
        return (tape[:tl.value].copy() if err.value == 0 else None), bytes(sb[:sl.value]), err.value, st.value

    def stage1_masks(self, data, length=None):
        """The reference's per-block masks (sjmi_stage1_masks): -> np.uint64 [len // 64 + 1, 6] =
        {escaped, quote, inString, op, whitespace, structurals} per 64-byte block."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n = a.size if length is None else length
        nb = n // 64 + 1
        masks = np.zeros((nb, 6), dtype=np.uint64)
        got = C.c_uint64(0)
        self._check(lib().sjmi_stage1_masks(self._h, a.ctypes.data if a.size else None, n, masks.ctypes.data, nb,
                                            C.addressof(got)), "sjmi_stage1_masks")
        assert got.value == nb
        return masks

    def stage1_masks_device(self, d_buf, length, d_masks, capacity_blocks, stream=0):
        self._check(lib().sjmi_stage1_masks_device(self._h, d_buf, length, d_masks, capacity_blocks, stream),
                    "sjmi_stage1_masks_device")

    def stage1_unescape(self, data, idx=None, sb=None):
        """Fused host path (sjmi_stage1_unescape): -> (indexes, status, string_buffer bytes, first_error_index, code)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else data
        n = a.size
        if idx is None:
            idx = np.empty(n + 2, dtype=np.uint32)
        if sb is None:
            sb = np.empty(n + 4 * (n // 2 + 2) + 64, dtype=np.uint8)
        cnt, total, fei = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        st, fec = C.c_uint32(0), C.c_uint32(0)
        self._check(lib().sjmi_stage1_unescape(self._h, a.ctypes.data if n else None, n, idx.ctypes.data, idx.size,
                                               C.addressof(cnt), C.addressof(st), sb.ctypes.data, sb.size, C.addressof(total),
                                               C.addressof(fei), C.addressof(fec)), "sjmi_stage1_unescape")
        return idx[:cnt.value], st.value, sb[:total.value], (None if fei.value == 2**64 - 1 else fei.value), fec.value

    def stage1_batch(self, data, doc_offsets):
        """Batched host path: -> (indexes, index_offsets[np.uint64 n+1], status)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        n = offs.size - 1
        cap = a.size + 2
        idx = np.empty(max(cap, 1), dtype=np.uint32)
        io = np.zeros(n + 1, dtype=np.uint64)
        cnt = C.c_uint64(0)
        st = C.c_uint32(0)
        self._check(lib().sjmi_stage1_batch(self._h, a.ctypes.data if a.size else None, a.size, offs.ctypes.data, n,
                                            idx.ctypes.data, cap, io.ctypes.data, C.addressof(cnt), C.addressof(st)),
                    "sjmi_stage1_batch")
        return idx[:cnt.value].copy(), io, st.value

    def stage1_batch_isolated(self, data, doc_offsets):
        """Isolated batched host path: -> (indexes, index_offsets[np.uint64 n+1], doc_status[np.uint32 n], status)."""
        a = np.frombuffer(bytes(data), dtype=np.uint8)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        n = offs.size - 1
        cap = a.size + 2
        idx = np.empty(max(cap, 1), dtype=np.uint32)
        io = np.zeros(n + 1, dtype=np.uint64)
        ds = np.zeros(max(n, 1), dtype=np.uint32)
        cnt = C.c_uint64(0)
        st = C.c_uint32(0)
        self._check(lib().sjmi_stage1_batch_isolated(self._h, a.ctypes.data if a.size else None, a.size, offs.ctypes.data, n,
                                                     idx.ctypes.data, cap, io.ctypes.data, ds.ctypes.data, C.addressof(cnt),
                                                     C.addressof(st)), "sjmi_stage1_batch_isolated")
        assert idx[cnt.value] == 0, "sentinel missing"
        return idx[:cnt.value].copy(), io, ds[:n], st.value

    def unescape(self, string_capacity):
        """Unescape every string of the document of the last stage1() call.
        -> (string_buffer bytes, first_error_index or None, first_error_code)."""
        sb = np.empty(max(string_capacity, 1), dtype=np.uint8)
        total = C.c_uint64(0)
        fei = C.c_uint64(0)
        fec = C.c_uint32(0)
        self._check(lib().sjmi_unescape(self._h, sb.ctypes.data, string_capacity, C.addressof(total), C.addressof(fei),
                                        C.addressof(fec)), "sjmi_unescape")
        idx = None if fei.value == 0xFFFFFFFFFFFFFFFF else fei.value
        return sb[:total.value].tobytes(), idx, fec.value

    def unescape_batch(self, string_capacity, n_docs):
        """Unescape the strings of the batch of the last stage1_batch*() call.
        -> (string_buffer bytes, doc_string_offsets[np.uint64 n_docs+1], first_error_index or None, first_error_code)."""
        sb = np.empty(max(string_capacity, 1), dtype=np.uint8)
        dso = np.zeros(n_docs + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        fei = C.c_uint64(0)
        fec = C.c_uint32(0)
        self._check(lib().sjmi_unescape_batch(self._h, sb.ctypes.data, string_capacity, dso.ctypes.data, C.addressof(total),
                                              C.addressof(fei), C.addressof(fec)), "sjmi_unescape_batch")
        idx = None if fei.value == 0xFFFFFFFFFFFFFFFF else fei.value
        return sb[:total.value].tobytes(), dso, idx, fec.value

    def unescape_device(self, d_buf, length, d_indexes, count, d_sb, sb_capacity, d_result, stream=0):
        self._check(lib().sjmi_unescape_device(self._h, d_buf, length, d_indexes, count, d_sb, sb_capacity, d_result,
                                               stream), "sjmi_unescape_device")

    def unescape_batch_device(self, d_buf, total_len, d_indexes, count, d_doc_offsets, d_index_offsets, n_docs, d_sb,
                              sb_capacity, d_doc_string_offsets, d_result, stream=0):
        self._check(lib().sjmi_unescape_batch_device(self._h, d_buf, total_len, d_indexes, count, d_doc_offsets, d_index_offsets,
                                                     n_docs, d_sb, sb_capacity, d_doc_string_offsets, d_result, stream),
                    "sjmi_unescape_batch_device")

    def walk_batch_device(self, d_buf, d_doc_offsets, n_docs, d_indexes, count, d_index_offsets, d_doc_status, d_sb,
                          d_doc_string_offsets, string_base, max_depth, d_tape, tape_capacity, d_tape_offsets, d_doc_errors,
                          d_result, stream=0):
        self._check(lib().sjmi_walk_batch_device(self._h, d_buf, d_doc_offsets, n_docs, d_indexes, count, d_index_offsets,
                                                 d_doc_status, d_sb, d_doc_string_offsets, string_base, max_depth, d_tape,
                                                 tape_capacity, d_tape_offsets, d_doc_errors, d_result, stream),
                    "sjmi_walk_batch_device")

    def parse_batch_device(self, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity, d_index_offsets,
                           d_doc_status, d_sb, sb_capacity, d_doc_string_offsets, max_depth, d_tape, tape_capacity,
                           d_tape_offsets, d_doc_errors, d_result, stream=0):
        """sjmi_parse_batch_device: isolated stage 1 -> string records -> GPU walk, queued without a host round trip;
        d_result = device sjmi_batch_result (9 x int64: count, status | strings total, first_error_inv, flags |
        tape words, host documents, failed documents, flags)."""
        self._check(lib().sjmi_parse_batch_device(self._h, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity,
                                                  d_index_offsets, d_doc_status, d_sb, sb_capacity, d_doc_string_offsets,
                                                  max_depth, d_tape, tape_capacity, d_tape_offsets, d_doc_errors, d_result,
                                                  stream), "sjmi_parse_batch_device")

    def parse_batch_device_optimistic(self, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity, d_index_offsets,
                                      d_doc_status, d_sb, sb_capacity, d_doc_string_offsets, max_depth, d_tape, tape_capacity,
                                      d_tape_offsets, d_doc_errors, d_result, stream=0):
        """sjmi_parse_batch_device_optimistic: ONLY the optimistic pipeline is queued (eight entries); stage1.status & 0x800
        (SJMI_ST_REJECTED) in d_result = nothing is valid, make the exact call (parse_batch_device)."""
        self._check(lib().sjmi_parse_batch_device_optimistic(self._h, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity,
                                                             d_index_offsets, d_doc_status, d_sb, sb_capacity, d_doc_string_offsets,
                                                             max_depth, d_tape, tape_capacity, d_tape_offsets, d_doc_errors, d_result,
                                                             stream), "sjmi_parse_batch_device_optimistic")

    def parse_batch_device_rejected(self, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity, d_index_offsets,
                                    d_doc_status, d_sb, sb_capacity, d_doc_string_offsets, max_depth, d_tape, tape_capacity,
                                    d_tape_offsets, d_doc_errors, d_result, stream=0):
        """sjmi_parse_batch_device_rejected: the call behind SJMI_ST_REJECTED -- per-document verdicts, the failing documents
        blanked in a copy, the optimistic pipeline over the copy (repair); the per-document passes only for a batch that cannot
        take either.  Outputs as parse_batch_device."""
        self._check(lib().sjmi_parse_batch_device_rejected(self._h, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity,
                                                           d_index_offsets, d_doc_status, d_sb, sb_capacity, d_doc_string_offsets,
                                                           max_depth, d_tape, tape_capacity, d_tape_offsets, d_doc_errors, d_result,
                                                           stream), "sjmi_parse_batch_device_rejected")

    def select_batch_device(self, plan, d_tape, d_tape_offsets, d_doc_errors, d_sb, n_docs, d_types, d_values, stream=0):
        """sjmi_select_batch_device: every path of `plan` (a SelectPlan) on every document of a parsed batch; d_types
        (uint8) / d_values (uint64) are path-major columns of n_docs entries each.  Asynchronous on `stream`."""
        self._check(lib().sjmi_select_batch_device(self._h, plan._h, d_tape, d_tape_offsets, d_doc_errors, d_sb, n_docs, d_types,
                                                   d_values, stream), "sjmi_select_batch_device")

    def explode_batch_device(self, plan, d_tape, d_tape_offsets, d_doc_errors, d_sb, n_docs, d_row_offsets, row_capacity, d_types,
                             d_values, stream=0):
        """sjmi_explode_batch_device: the base array of `plan` (an ExplodePlan; a members plan: the base object) of every document
        of a parsed batch as rows; d_row_offsets (uint64, n_docs + 1 entries) is always complete, d_types (uint8) / d_values
        (uint64) are plan.n_columns column-major columns strided by row_capacity (both None / 0 with row_capacity 0: the offsets
        only).  Asynchronous on `stream`."""
        self._check(lib().sjmi_explode_batch_device(self._h, plan._h, d_tape, d_tape_offsets, d_doc_errors, d_sb, n_docs, d_row_offsets,
                                                    row_capacity, d_types or None, d_values or None, stream), "sjmi_explode_batch_device")

    def ndjson_offsets_device(self, d_buf, length, d_doc_offsets, offset_capacity, d_result, stream=0):
        """sjmi_ndjson_offsets_device: the doc_offsets of a device-resident buffer of newline-delimited JSON (any alignment),
        d_doc_offsets = offset_capacity uint64 (None / 0 with capacity 0: size only), d_result = device sjmi_ndjson_result
        (3 x int64: n_docs, consumed, flags in the low half of the third).  Asynchronous on `stream`."""
        self._check(lib().sjmi_ndjson_offsets_device(self._h, d_buf or None, length, d_doc_offsets or None, offset_capacity, d_result,
                                                     stream), "sjmi_ndjson_offsets_device")

    def string_column_device(self, d_types, d_values, n_rows, d_sb, d_offsets, d_validity, d_bytes, byte_capacity, d_result, stream=0):
        """sjmi_string_column_device: ONE (types, values) column of a select or an explode as Arrow large_utf8 -- d_offsets
        (int64, n_rows + 1 entries, always complete), d_validity (uint64 words, LSB first; None / 0: not written), d_bytes
        (byte_capacity bytes; None / 0 with capacity 0: the sizing call), d_result = device sjmi_strcol_result (4 x int64:
        total_bytes, n_valid, n_other, flags in the low half of the fourth).  Asynchronous on `stream`."""
        self._check(lib().sjmi_string_column_device(self._h, d_types or None, d_values or None, n_rows, d_sb or None, d_offsets or None,
                                                    d_validity or None, d_bytes or None, byte_capacity, d_result or None, stream),
                    "sjmi_string_column_device")

    def filter_columns_device(self, plan, d_types, d_values, n_cols, col_stride, n_rows, d_sb, d_keep, d_rows, out_capacity, d_out_types,
                              d_out_values, d_result, stream=0):
        """sjmi_filter_columns_device: the rows of n_cols (types, values) columns strided by col_stride on which every term of
        `plan` (a FilterPlan) is true -- d_keep (uint64 words, LSB first), d_rows (int64 [out_capacity], the kept rows' indexes,
        ascending), d_out_types / d_out_values (the columns compacted, strided by out_capacity); each None / 0: not written, the
        last three together (with out_capacity 0: the sizing call); d_result = device sjmi_filter_result (2 x int64: n_kept,
        flags in the low half of the second).  Asynchronous on `stream`."""
        self._check(lib().sjmi_filter_columns_device(self._h, plan._h, d_types or None, d_values or None, n_cols, col_stride, n_rows,
                                                     d_sb or None, d_keep or None, d_rows or None, out_capacity, d_out_types or None,
                                                     d_out_values or None, d_result or None, stream), "sjmi_filter_columns_device")

    def arrow_columns_device(self, fields, d_types, d_values, n_cols, col_stride, n_rows, d_row_count, d_data, data_stride, d_validity,
                             validity_stride, d_results, stream=0):
        """sjmi_arrow_columns_device: n_cols (types, values) columns strided by col_stride as Arrow arrays, one per field.  fields:
        tuples (column, kind[, flag ...]) with kind "int64" / "float64" / "bool" and the flag "integral_doubles" (see
        arrow_fields()), or an encoded array.  d_row_count (None / 0: every row) = a device uint64 that holds the live rows;
        d_data (uint64 [n_fields * data_stride]; None / 0 with stride 0: the counting call), d_validity (uint64 words, LSB first,
        [n_fields * validity_stride]; None / 0: not written), d_results = device sjmi_arrow_field_result (n_fields x 4 int64:
        n_rows, n_valid, n_other, n_inexact).  Asynchronous on `stream`."""
        self._field_columns("sjmi_arrow_columns_device", arrow_fields(fields), d_types, d_values, n_cols, col_stride, n_rows, d_row_count, (), d_data,
                            data_stride, d_validity, validity_stride, d_results, stream)

    def time_columns_device(self, fields, d_types, d_values, n_cols, col_stride, n_rows, d_row_count, d_sb, d_data, data_stride, d_validity,
                            validity_stride, d_results, stream=0):
        """sjmi_time_columns_device: the RFC 3339 strings of n_cols (types, values) columns strided by col_stride as Arrow timestamp
        arrays, one per field.  fields: tuples (column, unit[, flag ...]) with unit "s" / "ms" / "us" / "ns" and the flag
        "naive_utc" (see time_fields()), or an encoded array.  d_row_count (None / 0: every row) = a device uint64 that holds the
        live rows; d_sb = the string buffer the cells point into; d_data (int64 [n_fields * data_stride]; None / 0 with stride 0:
        the counting call), d_validity (uint64 words, LSB first, [n_fields * validity_stride]; None / 0: not written), d_results =
        device sjmi_time_field_result (n_fields x 6 int64: n_rows, n_valid, n_other, n_malformed, n_range, n_inexact).
        Asynchronous on `stream`."""
        self._field_columns("sjmi_time_columns_device", time_fields(fields), d_types, d_values, n_cols, col_stride, n_rows, d_row_count, (d_sb or None,),
                            d_data, data_stride, d_validity, validity_stride, d_results, stream)

    def _field_columns(self, entry, enc, d_types, d_values, n_cols, col_stride, n_rows, d_row_count, strings, d_data, data_stride, d_validity,
                       validity_stride, d_results, stream):
        """the call under arrow_columns_device() and time_columns_device(): `strings` is () or (the string buffer,)"""
        self._check(getattr(lib(), entry)(self._h, enc.ctypes.data if enc.size else None, enc.size, d_types or None, d_values or None, n_cols, col_stride,
                                          n_rows, d_row_count or None, *strings, d_data or None, data_stride, d_validity or None, validity_stride,
                                          d_results or None, stream), entry)

    def dictionary_column_device(self, d_types, d_values, n_rows, d_row_count, d_sb, d_indices, d_validity, dict_capacity, d_dict_rows,
                                 d_dict_offsets, d_dict_bytes, dict_byte_capacity, d_result, stream=0):
        """sjmi_dictionary_column_device: ONE (types, values) column as an Arrow dictionary array, the dictionary in the order of
        first occurrence.  d_row_count (None / 0: every row) = a device uint64 that holds the live rows; d_indices (int32
        [n_rows]), d_validity (uint64 words, LSB first; None / 0: not written), d_dict_rows (int64 [dict_capacity]; None / 0: not
        written), d_dict_offsets (int64 [dict_capacity + 1]), d_dict_bytes (dict_byte_capacity bytes; None / 0 with capacity 0:
        the sizing call), d_result = device sjmi_dict_result (6 x int64: live rows, n_valid, n_other, n_distinct, dict_bytes,
        flags in the low half of the sixth).  Asynchronous on `stream`."""
        self._check(lib().sjmi_dictionary_column_device(self._h, d_types or None, d_values or None, n_rows, d_row_count or None, d_sb or None,
                                                        d_indices or None, d_validity or None, dict_capacity, d_dict_rows or None,
                                                        d_dict_offsets or None, d_dict_bytes or None, dict_byte_capacity, d_result or None,
                                                        stream), "sjmi_dictionary_column_device")

    def key_census_device(self, d_indices, d_validity, d_types, n_rows, d_row_count, n_keys, d_counts, d_result, stream=0):
        """sjmi_key_census_device: the rows per dictionary entry and value type.  d_indices (int32 [n_rows]) / d_validity (uint64
        words, LSB first; None / 0: every live row counts) as sjmi_dictionary_column_device wrote them, d_types (uint8 [n_rows]) a
        types column with the same rows; d_row_count (None / 0: every row) = a device uint64 that holds the live rows; d_counts
        (uint64 [n_keys * 8]: entry-major, class-minor), d_result = device sjmi_census_result (4 x int64: live rows, n_counted,
        n_out_of_range, flags in the low half of the fourth).  Asynchronous on `stream`."""
        self._check(lib().sjmi_key_census_device(self._h, d_indices or None, d_validity or None, d_types or None, n_rows, d_row_count or None,
                                                 n_keys, d_counts or None, d_result or None, stream), "sjmi_key_census_device")

    def group_stats_device(self, d_indices, d_validity, d_types, d_values, n_rows, d_row_count, n_keys, d_stats, d_result, stream=0):
        """sjmi_group_stats_device: count, sum, minimum and maximum of ONE (type, value) column per dictionary entry.  d_indices /
        d_validity / d_row_count / n_keys as key_census_device takes them; d_types (uint8 [n_rows]) and d_values (uint64
        [n_rows]) one column with the same rows; d_stats (uint64 [n_keys * 10], key-major: n_long, n_double, n_other, sum_long_lo,
        sum_long_hi, sum_double, min_long, max_long, min_double, max_double), d_result = device sjmi_group_result (5 x int64:
        live rows, n_grouped, n_out_of_range, n_nan, flags in the low half of the fifth).  n_rows < 2^32.  Asynchronous on
        `stream`."""
        self._check(lib().sjmi_group_stats_device(self._h, d_indices or None, d_validity or None, d_types or None, d_values or None, n_rows,
                                                  d_row_count or None, n_keys, d_stats or None, d_result or None, stream), "sjmi_group_stats_device")

    def top_rows_device(self, d_key_types, d_key_validity, d_key_values, n_rows, d_row_count, kind, flags, k, d_types, d_values, n_cols,
                        col_stride, d_rows, d_out_types, d_out_values, d_result, stream=0):
        """sjmi_top_rows_device: the k rows with the largest (flags = TOP_SMALLEST: smallest) value of ONE key column, in rank
        order, ties by ascending row.  d_key_types (uint8 [n_rows]; None / 0: every valid row is a number), d_key_validity (uint64
        words, LSB first; None / 0: every live row is valid), d_key_values (uint64 [n_rows]); d_row_count (None / 0: every row) =
        a device uint64 that holds the live rows; kind = TOP_LONG or TOP_DOUBLE; k <= TOP_MAX_K; d_types / d_values = n_cols
        carried columns col_stride cells apart (None / 0 with n_cols 0); d_rows (uint64 [k]), d_out_types (uint8 [n_cols * k]),
        d_out_values (uint64 [n_cols * k]), d_result = device sjmi_top_result (9 x int64: live rows, n_candidates, n_null,
        n_other, n_nan, n_inexact, n_out, kth_bits, flags in the low half of the ninth).  n_rows < 2^32.  Asynchronous on
        `stream`."""
        self._check(lib().sjmi_top_rows_device(self._h, d_key_types or None, d_key_validity or None, d_key_values or None, n_rows,
                                               d_row_count or None, kind, flags, k, d_types or None, d_values or None, n_cols, col_stride,
                                               d_rows or None, d_out_types or None, d_out_values or None, d_result or None, stream),
                    "sjmi_top_rows_device")

    def sort_rows_device(self, d_key_types, d_key_validity, d_key_values, n_source_rows, d_rows_in, n_rows, d_row_count, kind, flags,
                         d_types, d_values, n_cols, col_stride, d_rows, d_out_types, d_out_values, out_stride, d_result, stream=0):
        """sjmi_sort_rows_device: ALL live positions ordered by the value of ONE key column, a stable sort (equal values keep
        their input order: chain the calls, last key first, for several keys).  The key column of n_source_rows rows as
        top_rows_device takes it; d_rows_in (None / 0: position i is row i; else uint64 [n_rows] source rows, an entry at or above
        n_source_rows a BAD position that is ordered with the nulls); d_row_count (None / 0: every position) = a device uint64
        that holds the live positions; kind = SORT_LONG or SORT_DOUBLE, flags = 0 or SORT_DESCENDING; d_types / d_values = n_cols
        carried columns col_stride >= n_source_rows cells apart (None / 0 with n_cols 0); d_rows (uint64 [n_rows], not
        d_rows_in), d_out_types (uint8) / d_out_values (uint64), n_cols rows out_stride >= n_rows cells apart; d_result = device
        sjmi_sort_result (9 x int64: live positions, n_candidates, n_null, n_other, n_nan, n_inexact, n_bad, n_passes, flags in
        the low half of the ninth).  Both row counts < 2^32.  Asynchronous on `stream`."""
        self._check(lib().sjmi_sort_rows_device(self._h, d_key_types or None, d_key_validity or None, d_key_values or None, n_source_rows,
                                                d_rows_in or None, n_rows, d_row_count or None, kind, flags, d_types or None, d_values or None,
                                                n_cols, col_stride, d_rows or None, d_out_types or None, d_out_values or None, out_stride,
                                                d_result or None, stream), "sjmi_sort_rows_device")

    def join_rows_device(self, left, d_left_rows_in, n_left, d_left_count, right, d_right_order, n_right, d_right_sort_result, how,
                         pair_capacity, d_left_rows, d_right_rows, d_left_out_types, d_left_out_values, d_right_out_types,
                         d_right_out_values, out_stride, d_pair_offsets, d_result, stream=0):
        """sjmi_join_rows_device: the LEFT positions joined with a sorted RIGHT side on a long key.  left / right: the arguments of
        join_side() as a tuple (d_key_types, d_key_validity, d_key_values, n_source_rows[, d_types, d_values, n_cols,
        col_stride]).  d_left_rows_in (None / 0: position i is row i) and d_left_count (None / 0: every position) as
        sort_rows_device takes them; d_right_order / n_right / d_right_sort_result = d_rows, n_rows and the DEVICE record of a
        sort_rows_device call (SORT_LONG, ascending) on the right key; how = JOIN_INNER / LEFT / SEMI / ANTI; d_left_rows,
        d_right_rows (uint64 [pair_capacity]; JOIN_NO_ROW without a match; None / 0 allowed under SEMI and ANTI); the carried cells
        of both sides, n_cols rows out_stride >= pair_capacity cells apart; d_pair_offsets (None / 0, or uint64 [n_left + 1]);
        d_result = device sjmi_join_result (9 x int64: live left positions, n_build, n_pairs, n_matched, n_null, n_other, n_bad,
        n_right_bad, flags in the low half of the ninth).  Asynchronous on `stream`."""
        l, r = join_side(*left), join_side(*right)
        self._check(lib().sjmi_join_rows_device(self._h, l.ctypes.data, d_left_rows_in or None, n_left, d_left_count or None, r.ctypes.data,
                                                d_right_order or None, n_right, d_right_sort_result or None, how, pair_capacity,
                                                d_left_rows or None, d_right_rows or None, d_left_out_types or None, d_left_out_values or None,
                                                d_right_out_types or None, d_right_out_values or None, out_stride, d_pair_offsets or None,
                                                d_result or None, stream), "sjmi_join_rows_device")

    def parent_columns_device(self, d_row_offsets, n_docs, d_rows, n_rows, d_row_count, d_types, d_values, n_cols, col_stride,
                              d_parent_types, d_parents, d_out_types, d_out_values, out_stride, d_result, stream=0):
        """sjmi_parent_columns_device: the document of every exploded row, and that document's cells on the row.  d_row_offsets
        (uint64 [n_docs + 1], as explode_batch_device writes them); d_rows (None / 0: the dense form, slot i is row i; else uint64
        [n_rows] row indices in any order); d_row_count (None / 0: every row) = a device uint64 that holds the live rows; d_types
        / d_values = n_cols DOCUMENT columns col_stride >= n_docs cells apart (None / 0 with n_cols 0); d_parent_types (uint8
        [n_rows]) and d_parents (int64 [n_rows]), each None / 0 to leave it out: 'l' and the document, MISSING and -1 for a row at
        or above d_row_offsets[n_docs]; d_out_types (uint8) / d_out_values (uint64), n_cols rows out_stride >= n_rows cells
        apart; d_result = device sjmi_parent_result (3 x int64: live rows, n_orphans, flags in the low half of the third).
        n_rows and n_docs < 2^32, n_cols <= 64.  Asynchronous on `stream`."""
        self._check(lib().sjmi_parent_columns_device(self._h, d_row_offsets or None, n_docs, d_rows or None, n_rows, d_row_count or None,
                                                     d_types or None, d_values or None, n_cols, col_stride, d_parent_types or None,
                                                     d_parents or None, d_out_types or None, d_out_values or None, out_stride,
                                                     d_result or None, stream), "sjmi_parent_columns_device")

    def ndjson_offsets(self, data):
        """sjmi_ndjson_offsets (host form) -> (doc_offsets np.uint64 [n_docs + 1], consumed, flags): the documents are the
        non-blank lines of data[0, consumed), blank lines absorbed by the document in front of them."""
        a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        offs = np.zeros(a.size // 2 + 1, dtype=np.uint64)
        n, consumed, flags = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._check(lib().sjmi_ndjson_offsets(self._h, a.ctypes.data if a.size else None, a.size, offs.ctypes.data, offs.size,
                                              C.addressof(n), C.addressof(consumed), C.addressof(flags)), "sjmi_ndjson_offsets")
        return offs[:n.value + 1].copy(), consumed.value, flags.value

    def stage1_batch_device(self, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity, d_index_offsets,
                            d_result, stream=0):
        self._check(lib().sjmi_stage1_batch_device(self._h, d_buf, total_len, d_doc_offsets, n_docs, d_indexes,
                                                   index_capacity, d_index_offsets, d_result, stream),
                    "sjmi_stage1_batch_device")

    def stage1_batch_isolated_device(self, d_buf, total_len, d_doc_offsets, n_docs, d_indexes, index_capacity,
                                     d_index_offsets, d_doc_status, d_result, stream=0):
        self._check(lib().sjmi_stage1_batch_isolated_device(self._h, d_buf, total_len, d_doc_offsets, n_docs, d_indexes,
                                                            index_capacity, d_index_offsets, d_doc_status, d_result,
                                                            stream), "sjmi_stage1_batch_isolated_device")

    def stage1_device(self, d_buf, length, d_indexes, index_capacity, d_result, stream=0):
        """Device-resident path; arguments are raw device pointers (ints) and a hipStream_t handle."""
        self._check(lib().sjmi_stage1_device(self._h, d_buf, length, d_indexes, index_capacity, d_result, stream),
                    "sjmi_stage1_device")

    def stage1_shard_device(self, d_buf, length, halo_bytes, is_last, entry_parity, d_indexes, index_capacity, d_result, stream=0,
                            halo_from_start=False):
        """One shard / stream chunk of a longer document (sjmi_stage1_shard_device2)."""
        self._check(lib().sjmi_stage1_shard_device2(self._h, d_buf, length, halo_bytes, 1 if halo_from_start else 0,
                                                    1 if is_last else 0, 1 if entry_parity else 0,
                                                    d_indexes, index_capacity, d_result, stream), "sjmi_stage1_shard_device2")

    def stream(self, max_chunk_bytes, halo_bytes=0):
        """sjmi_stream_open: one document as a stream of chunks -> a Stream (push(chunk, is_last), close())."""
        return Stream(self, max_chunk_bytes, halo_bytes)

    def split(self, d_shard, length, halo_bytes, halo_from_start, is_last, d_indexes, index_capacity):
        """sjmi_split_open: one rank's shard of a document split over GPUs -> a Split (scan(), resolve(entry_parity), close())."""
        return Split(self, d_shard, length, halo_bytes, halo_from_start, is_last, d_indexes, index_capacity)

    def set_auto_safe(self, on):
        self._check(lib().sjmi_set_auto_safe(self._h, 1 if on else 0), "sjmi_set_auto_safe")

    def set_tile_mode(self, ticket):
        self._check(lib().sjmi_set_tile_mode(self._h, 1 if ticket else 0), "sjmi_set_tile_mode")

    def debug_set_flags(self, flags):
        self._check(lib().sjmi_debug_set_flags(self._h, flags), "sjmi_debug_set_flags")

    def debug_counters(self):
        """-> [stage-1 launches queued, those with every granule by ticket, repeats in SAFE mode, SAFE mode now (0 / 1)]"""
        out = (C.c_uint64 * 4)()
        self._check(lib().sjmi_debug_counters(self._h, C.addressof(out)), "sjmi_debug_counters")
        return [int(v) for v in out]

    def set_profiling(self, on):
        self._check(lib().sjmi_set_profiling(self._h, 1 if on else 0), "sjmi_set_profiling")

    def kernel_time(self):
        """-> (sum of stage-1 kernel durations in ms since profiling was enabled, number of launches)."""
        ms = C.c_double(0)
        n = C.c_uint32(0)
        self._check(lib().sjmi_kernel_time(self._h, C.addressof(ms), C.addressof(n)), "sjmi_kernel_time")
        return ms.value, n.value


class SelectPlan:
    """sjmi_select_plan: a set of RFC 6901 JSON Pointers (str or bytes) compiled once, on the host (no device needed), for
    Context.select_batch_device / BatchShard.select.  Raises ValueError for a malformed pointer or an exceeded limit
    (include/sjmi.h: SJMI_SELECT_MAX_*)."""

    MISSING = 0

    def __init__(self, pointers):
        self.pointers = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in pointers]
        self.n_paths = len(self.pointers)
        blob = np.frombuffer(b"".join(self.pointers) + b"\0", dtype=np.uint8)
        offs = np.zeros(self.n_paths + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(p) for p in self.pointers], dtype=np.uint64)
        self._h = C.c_void_p()
        rc = lib().sjmi_select_plan_compile(blob.ctypes.data, offs.ctypes.data, self.n_paths, C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise ValueError("sjmi_select_plan_compile failed (rc=%d): a malformed JSON Pointer or a plan limit exceeded" % rc)

    def close(self):
        if self._h:
            lib().sjmi_select_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ExplodePlan:
    """sjmi_explode_plan: a base pointer and a set of element pointers (RFC 6901, str or bytes) compiled once, on the host (no
    device needed), for Context.explode_batch_device / BatchShard.explode.  members=True: a MEMBERS plan -- the base is an
    object, a row is a member, and the member's key is one more column behind the element pointers' (n_columns = n_paths + 1).
    Raises ValueError for a malformed pointer or an exceeded limit (include/sjmi.h: SJMI_SELECT_MAX_*,
    SJMI_EXPLODE_MEMBERS_MAX_PATHS)."""

    MISSING = 0

    def __init__(self, base, pointers, members=False):
        self.members = bool(members)
        self.base = base.encode("utf-8") if isinstance(base, str) else bytes(base)
        self.pointers = [p.encode("utf-8") if isinstance(p, str) else bytes(p) for p in pointers]
        self.n_paths = len(self.pointers)
        base_blob = np.frombuffer(self.base + b"\0", dtype=np.uint8)
        blob = np.frombuffer(b"".join(self.pointers) + b"\0", dtype=np.uint8)
        offs = np.zeros(self.n_paths + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(p) for p in self.pointers], dtype=np.uint64)
        self._h = C.c_void_p()
        entry = "sjmi_explode_members_plan_compile" if self.members else "sjmi_explode_plan_compile"
        rc = getattr(lib(), entry)(base_blob.ctypes.data, len(self.base), blob.ctypes.data, offs.ctypes.data, self.n_paths, C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise ValueError("%s failed (rc=%d): a malformed JSON Pointer or a plan limit exceeded" % (entry, rc))

    @property
    def n_columns(self):
        """the columns an explode with this plan writes: the element pointers', and a members plan's key column behind them"""
        return self.n_paths + (1 if self.members else 0)

    def close(self):
        if self._h:
            lib().sjmi_explode_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FilterPlan:
    """sjmi_filter_plan: a conjunction of at most 16 terms (column, op, constant) compiled once, on the host (no device needed),
    for Context.filter_columns_device / BatchShard.filter.  op is "<kind>_<cmp>": "type_eq" / "type_ne" with a type byte (an int,
    or a one-character str or bytes; 0 = MISSING), "long_eq|ne|lt|le|gt|ge" with an int, "double_eq|..." with a float,
    "string_eq" / "string_ne" / "string_prefix" with bytes or str (UTF-8).  Raises ValueError for what include/sjmi.h lists as
    SJMI_ERR_ARG: an unknown op, a NaN, a limit exceeded (SJMI_FILTER_MAX_*)."""

    KINDS = {"type": 0, "long": 1, "double": 2, "string": 3}
    CMPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5, "prefix": 6}
    _TERM = np.dtype([("column", "<u4"), ("op", "<u4"), ("operand", "<u8")])

    def __init__(self, terms):
        import struct
        self.terms = [tuple(t) for t in terms]
        enc = np.zeros(len(self.terms), dtype=self._TERM)
        blob = b""
        for k, (column, op, const) in enumerate(self.terms):
            kind, _, cmp = str(op).partition("_")
            if kind not in self.KINDS or cmp not in self.CMPS:
                raise ValueError("filter term %d: unknown op %r" % (k, op))
            if kind == "type":
                operand = ord(const) if isinstance(const, (str, bytes)) else int(const)
            elif kind == "long":
                operand = int(const) & 0xFFFFFFFFFFFFFFFF
                if not -(1 << 63) <= int(const) < (1 << 63):
                    raise ValueError("filter term %d: %r is no int64" % (k, const))
            elif kind == "double":
                operand = struct.unpack("<Q", struct.pack("<d", float(const)))[0]
            else:
                const = const.encode("utf-8") if isinstance(const, str) else bytes(const)
                operand = (len(const) << 32) | len(blob)
                blob += const
            if not 0 <= operand < (1 << 64) or not 0 <= int(column) < (1 << 32):
                raise ValueError("filter term %d: operand or column out of range" % k)
            enc[k] = (int(column), (self.KINDS[kind] << 4) | self.CMPS[cmp], operand)
        self.n_terms = len(self.terms)
        consts = np.frombuffer(blob + b"\0", dtype=np.uint8)
        self._h = C.c_void_p()
        rc = lib().sjmi_filter_plan_compile(enc.ctypes.data if self.n_terms else None, self.n_terms, consts.ctypes.data if blob else None,
                                            len(blob), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise ValueError("sjmi_filter_plan_compile failed (rc=%d): an unknown op, a NaN or a plan limit exceeded" % rc)

    def close(self):
        if self._h:
            lib().sjmi_filter_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JsonParsingException(Exception):
    """org.simdjson.JsonParsingException (JsonParsingException.java:3-12); .code = SJMI_E_*."""

    def __init__(self, code, message, position=0):
        super().__init__(message)
        self.code = code
        self.position = position


class _Value(C.Structure):
    _fields_ = [("doc", C.c_uint64), ("tape_idx", C.c_uint64)]


class JsonValue:
    """org.simdjson.JsonValue (JsonValue.java:18-221) through the sjmi_value_* C ABI (which runs the C++ mirror class
    org_simdjson::JsonValue); valid until the next parse on its parser, like the reference's."""

    def __init__(self, parser, handle):
        self._p = parser
        self._v = handle

    def _call(self, fn, *args):
        rc = fn(self._p._h, C.byref(self._v), *args)
        if rc < 0:
            raise SjmiError("%s failed (rc=%d): wrong type or stale handle" % (fn.__name__, rc))
        return rc

    def type(self):
        return chr(self._call(lib().sjmi_value_type))

    def isArray(self):
        return self.type() == "["

    def isObject(self):
        return self.type() == "{"

    def isString(self):
        return self.type() == '"'

    def isLong(self):
        return self.type() == "l"

    def isDouble(self):
        return self.type() == "d"

    def isBoolean(self):
        return self.type() in "tf"

    def isNull(self):
        return self.type() == "n"

    def asLong(self):
        out = C.c_int64(0)
        self._call(lib().sjmi_value_as_long, C.byref(out))
        return out.value

    def asDouble(self):
        out = C.c_double(0)
        self._call(lib().sjmi_value_as_double, C.byref(out))
        return out.value

    def asBoolean(self):
        out = C.c_int(0)
        self._call(lib().sjmi_value_as_boolean, C.byref(out))
        return bool(out.value)

    def asString(self):
        n = C.c_uint64(0)
        buf = (C.c_uint8 * 256)()
        rc = lib().sjmi_value_as_string(self._p._h, C.byref(self._v), buf, 256, C.byref(n))
        if rc == -3:  # SJMI_ERR_CAPACITY: n holds the length
            buf = (C.c_uint8 * n.value)()
            rc = lib().sjmi_value_as_string(self._p._h, C.byref(self._v), buf, n.value, C.byref(n))
        if rc != 0:
            raise SjmiError("sjmi_value_as_string failed (rc=%d)" % rc)
        return bytes(buf[:n.value]).decode("utf-8")

    def get(self, name):
        """JsonValue.get(String): the field's value or None."""
        key = name.encode("utf-8")
        out = _Value()
        rc = self._call(lib().sjmi_value_get, key, len(key), C.byref(out))
        return None if rc == 1 else JsonValue(self._p, out)

    def getSize(self):
        return self._call(lib().sjmi_value_size)

    def _children(self):
        cur = _Value()
        rc = self._call(lib().sjmi_value_first, C.byref(cur))
        while rc == 0:
            yield JsonValue(self._p, cur)
            nxt = _Value()
            rc = lib().sjmi_value_next(self._p._h, C.byref(self._v), C.byref(cur), C.byref(nxt))
            if rc < 0:
                raise SjmiError("sjmi_value_next failed (rc=%d)" % rc)
            cur = nxt

    def arrayIterator(self):
        assert self.isArray()
        return self._children()

    def objectIterator(self):
        """-> (key str, JsonValue) pairs in document order."""
        assert self.isObject()
        it = self._children()
        for k in it:
            yield k.asString(), next(it)

    def to_python(self):
        """The whole subtree in the oracle's Parsed.to_python() notation (type tags, raw IEEE bits, UTF-8 bytes)."""
        t = self.type()
        if t == '"':
            return ("s", self.asString().encode("utf-8"))
        if t == "l":
            return ("l", self.asLong())
        if t == "d":
            import struct
            return ("d", struct.unpack("<Q", struct.pack("<d", self.asDouble()))[0])
        if t in "tfn":
            return (t,)
        if t == "[":
            return ("a", self.getSize(), [c.to_python() for c in self.arrayIterator()])
        return ("o", self.getSize(), [(k.encode("utf-8"), v.to_python()) for k, v in self.objectIterator()])


class ParsedDocument:
    """Tape + string buffer of one parse (views copied out of the parser)."""

    def __init__(self, tape, strings):
        self.tape = tape
        self.strings = strings


class SimdJsonParser:
    """Python handle on the C++ host mirror org_simdjson::SimdJsonParser (csrc/host/simdjson_parser.h):
    parse(buffer, len) = GPU stage 1 + GPU string unescape + host stage 2 (SimdJsonParser.java:35-40)."""

    DEFAULT_CAPACITY = 34 * 1024 * 1024
    DEFAULT_MAX_DEPTH = 1024

    def __init__(self, capacity=DEFAULT_CAPACITY, max_depth=DEFAULT_MAX_DEPTH, device=0, gpu_walk=None):
        self._h = C.c_void_p()
        rc = lib().sjmi_parser_create(C.byref(self._h), capacity, max_depth, device)
        if rc != 0:
            self._h = C.c_void_p()
            raise SjmiError("sjmi_parser_create failed (rc=%d): no usable MI355X; there is no CPU fallback" % rc)
        self._device = device
        if gpu_walk is not None:  # stage 2 on the GPU (True) / on the host (False); None: the library's default, by size
            lib().sjmi_parser_set_gpu_walk(self._h, 1 if gpu_walk else 0)
        _live.add(self)

    def close(self):
        if getattr(self, "_ndjson_ctx", None) is not None:  # (parse_ndjson's splitter)
            self._ndjson_ctx.close()
            self._ndjson_ctx = None
        if self._h:
            lib().sjmi_parser_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        if _exiting:
            return
        try:
            self.close()
        except Exception:
            pass

    def parse(self, buffer, length=None):
        a = np.frombuffer(bytes(buffer), dtype=np.uint8)
        n = a.size if length is None else length
        tape_p = C.POINTER(C.c_uint64)()
        sb_p = C.POINTER(C.c_uint8)()
        tape_len = C.c_uint64(0)
        sb_len = C.c_uint64(0)
        err_pos = C.c_uint64(0)
        rc = lib().sjmi_parser_parse(self._h, a.ctypes.data if a.size else None, n, C.byref(tape_p), C.byref(tape_len),
                                     C.byref(sb_p), C.byref(sb_len), C.byref(err_pos))
        if rc > 0:
            raise JsonParsingException(rc, lib().sjmi_parser_last_message(self._h).decode("utf-8"), err_pos.value)
        if rc < 0:
            raise SjmiError("sjmi_parser_parse failed (rc=%d): %s" % (rc, lib().sjmi_parser_last_message(self._h).decode()))
        tape = np.ctypeslib.as_array(tape_p, shape=(tape_len.value,)).copy()
        strings = bytes(np.ctypeslib.as_array(sb_p, shape=(max(sb_len.value, 1),))[:sb_len.value])
        return ParsedDocument(tape, strings)

    def ondemand(self, buffer, length=None):
        """The on-demand front end (OnDemandJsonIterator.java; csrc/host/ondemand.h): pad + GPU stage 1 + iterator.init -> the
        cursor.  One cursor per parser at a time, invalidated by the next parse / ondemand."""
        a = np.frombuffer(bytes(buffer), dtype=np.uint8)
        n = a.size if length is None else length
        rc = lib().sjmi_parser_ondemand_init(self._h, a.ctypes.data if a.size else None, n, 0)
        if rc > 0:
            raise JsonParsingException(rc, lib().sjmi_parser_last_message(self._h).decode("utf-8"))
        if rc < 0:
            raise SjmiError("sjmi_parser_ondemand_init failed (rc=%d): %s" % (rc, lib().sjmi_parser_last_message(self._h).decode()))
        return OnDemandIterator(self)

    def root(self):
        """JsonValue of the last parse() (what SimdJsonParser.parse returns in the reference)."""
        v = _Value()
        rc = lib().sjmi_parser_root(self._h, C.byref(v))
        if rc != 0:
            raise SjmiError("sjmi_parser_root failed (rc=%d): no successful parse on this parser" % rc)
        return JsonValue(self, v)

    def batch_root(self, doc):
        """JsonValue of document `doc` of the last parse_batch(); raises JsonParsingException with that document's code."""
        v = _Value()
        rc = lib().sjmi_parser_batch_root(self._h, doc, C.byref(v))
        if rc > 0:
            raise JsonParsingException(rc, "document %d of the batch failed with code %d" % (doc, rc))
        if rc < 0:
            raise SjmiError("sjmi_parser_batch_root failed (rc=%d)" % rc)
        return JsonValue(self, v)

    def parse_ndjson(self, data):
        """A buffer of newline-delimited JSON: one '\\n' is appended if the last byte is not one, the GPU splits it into its
        documents (sjmi_ndjson_offsets; blank lines belong to the document in front of them), and parse_batch parses them.
        -> what parse_batch returns."""
        data = bytes(data)
        if data and not data.endswith(b"\n"):
            data += b"\n"
        ctx = getattr(self, "_ndjson_ctx", None)
        if ctx is None or ctx.capacity < len(data):
            if ctx is not None:
                ctx.close()
            ctx = self._ndjson_ctx = Context(self._device, max(len(data), 1 << 20))
        offs, consumed, _ = ctx.ndjson_offsets(data)
        return self.parse_batch(data[:consumed], offs)

    def parse_batch(self, buffer, doc_offsets):
        """-> (list of per-document tapes (np.uint64) or None where errors[k] != 0, shared strings bytes, errors)."""
        a = np.frombuffer(bytes(buffer), dtype=np.uint8)
        offs = np.ascontiguousarray(doc_offsets, dtype=np.uint64)
        n = offs.size - 1
        tape_p = C.POINTER(C.c_uint64)()
        to_p = C.POINTER(C.c_uint64)()
        sb_p = C.POINTER(C.c_uint8)()
        err_p = C.POINTER(C.c_int32)()
        sb_len = C.c_uint64(0)
        rc = lib().sjmi_parser_parse_batch(self._h, a.ctypes.data if a.size else None, a.size, offs.ctypes.data, n,
                                           C.byref(tape_p), C.byref(to_p), C.byref(sb_p), C.byref(sb_len), C.byref(err_p))
        if rc > 0:
            raise JsonParsingException(rc, lib().sjmi_parser_last_message(self._h).decode("utf-8"))
        if rc < 0:
            raise SjmiError("sjmi_parser_parse_batch failed (rc=%d): %s" % (rc, lib().sjmi_parser_last_message(self._h).decode()))
        def view(ptr, count, dtype):  # (an empty result may come back as a NULL pointer)
            return np.ctypeslib.as_array(ptr, shape=(count,)).copy() if count and bool(ptr) else np.zeros(0, dtype=dtype)
        to = np.ctypeslib.as_array(to_p, shape=(n + 1,)).copy()
        errors = view(err_p, n, np.int32)
        alltape = view(tape_p, int(to[-1]), np.uint64)
        strings = bytes(view(sb_p, sb_len.value, np.uint8))
        tapes = [alltape[int(to[k]):int(to[k + 1])] if errors[k] == 0 else None for k in range(n)]
        return tapes, strings, errors


class Stream:
    """sjmi_stream_*: chunks of one document, scanned once each; push -> (base offset, indexes relative to the chunk, status so far)"""

    def __init__(self, ctx, max_chunk_bytes, halo_bytes=0):
        L = lib()
        self._ctx, self._max = ctx, int(max_chunk_bytes)
        h = C.c_void_p()
        ctx._check(L.sjmi_stream_open(ctx._h, self._max, halo_bytes, C.byref(h)), "sjmi_stream_open")
        self._h = h
        self._idx = np.empty(self._max + 70, dtype=np.uint32)

    def push(self, chunk, is_last):
        a = np.frombuffer(bytes(chunk), dtype=np.uint8)
        count, base, st = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._ctx._check(lib().sjmi_stream_push(self._h, a.ctypes.data if a.size else None, a.size, 1 if is_last else 0, self._idx.ctypes.data,
                                                self._idx.size, C.byref(count), C.byref(base), C.byref(st)), "sjmi_stream_push")
        return base.value, self._idx[:count.value].copy(), st.value

    def close(self):
        if self._h:
            lib().sjmi_stream_close(self._h)
            self._h = None


class Split:
    """sjmi_split_*: scan() -> (flips the parity?, status bits); resolve(entry_parity) -> (count, status bits, parity behind the shard)"""

    def __init__(self, ctx, d_shard, length, halo_bytes, halo_from_start, is_last, d_indexes, index_capacity):
        L = lib()
        self._ctx = ctx
        h = C.c_void_p()
        ctx._check(L.sjmi_split_open(ctx._h, d_shard, length, halo_bytes, 1 if halo_from_start else 0, 1 if is_last else 0, d_indexes,
                                     index_capacity, C.byref(h)), "sjmi_split_open")
        self._h = h

    def scan(self, stream=0):
        flips, st = C.c_int(0), C.c_uint32(0)
        self._ctx._check(lib().sjmi_split_scan(self._h, stream, C.byref(flips), C.byref(st)), "sjmi_split_scan")
        return flips.value, st.value

    def resolve(self, entry_parity, stream=0):
        count, st, after = C.c_uint64(0), C.c_uint32(0), C.c_int(0)
        self._ctx._check(lib().sjmi_split_resolve(self._h, 1 if entry_parity else 0, stream, C.byref(count), C.byref(st), C.byref(after)),
                         "sjmi_split_resolve")
        return count.value, st.value, after.value

    def close(self):
        if self._h:
            lib().sjmi_split_close(self._h)
            self._h = None


class OnDemandIterator:
    """Python face of the sjmi_od_* entry points: the methods of the reference's OnDemandJsonIterator (names as in
    oracle/ondemand.py, the checker).  Nullable getters return None where the reference returns null."""
    EMPTY, NULL, NOT_EMPTY = 0, 1, 2

    def __init__(self, parser):
        self._p = parser

    def _check(self, rc):
        if rc > 0:
            raise JsonParsingException(rc, lib().sjmi_parser_last_message(self._p._h).decode("utf-8"))
        if rc < 0:
            raise SjmiError("on-demand call failed (rc=%d): %s" % (rc, lib().sjmi_parser_last_message(self._p._h).decode()))

    def depth_value(self):
        return lib().sjmi_od_depth(self._p._h)

    def peek_byte(self):
        return lib().sjmi_od_peek(self._p._h)

    def skip_child(self, parent_depth=None):
        self._check(lib().sjmi_od_skip_child(self._p._h, -1 if parent_depth is None else parent_depth))

    def get_boolean(self, root=False, nullable=True):
        n, v = C.c_int(0), C.c_int(0)
        self._check(lib().sjmi_od_get_boolean(self._p._h, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        return None if n.value else bool(v.value)

    def get_long(self, root=False, nullable=True, bits=64):
        n, v = C.c_int(0), C.c_int64(0)
        if bits == 64:
            self._check(lib().sjmi_od_get_long(self._p._h, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        else:
            self._check(lib().sjmi_od_get_integral(self._p._h, bits, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        return None if n.value else v.value

    def get_double(self, root=False, nullable=True):
        n, v = C.c_int(0), C.c_double(0)
        self._check(lib().sjmi_od_get_double(self._p._h, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        return None if n.value else v.value

    def get_float(self, root=False, nullable=True):
        n, v = C.c_int(0), C.c_float(0)
        self._check(lib().sjmi_od_get_float(self._p._h, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        return None if n.value else v.value

    def get_char(self, root=False, nullable=True):
        n, v = C.c_int(0), C.c_uint16(0)
        self._check(lib().sjmi_od_get_char(self._p._h, int(root), int(nullable), C.addressof(n), C.addressof(v)))
        return None if n.value else v.value

    def _bytes(self, ptr, ln):
        return C.string_at(ptr.value, ln.value) if ln.value else b""

    def get_string(self, root=False):
        n, ptr, ln = C.c_int(0), C.c_void_p(), C.c_uint64(0)
        self._check(lib().sjmi_od_get_string(self._p._h, int(root), C.addressof(n), C.addressof(ptr), C.addressof(ln)))
        return None if n.value else self._bytes(ptr, ln)

    def get_field_name(self):
        ptr, ln = C.c_void_p(), C.c_uint64(0)
        self._check(lib().sjmi_od_get_field_name(self._p._h, C.addressof(ptr), C.addressof(ln)))
        return self._bytes(ptr, ln)

    def start_iterating_array(self, root=False):
        r = C.c_int(0)
        self._check(lib().sjmi_od_start_array(self._p._h, int(root), C.addressof(r)))
        return r.value

    def next_array_element(self):
        r = C.c_int(0)
        self._check(lib().sjmi_od_next_array_element(self._p._h, C.addressof(r)))
        return bool(r.value)

    def start_iterating_object(self, root=False):
        r = C.c_int(0)
        self._check(lib().sjmi_od_start_object(self._p._h, int(root), C.addressof(r)))
        return r.value

    def next_object_field(self):
        r = C.c_int(0)
        self._check(lib().sjmi_od_next_object_field(self._p._h, C.addressof(r)))
        return bool(r.value)

    def move_to_field_value(self):
        self._check(lib().sjmi_od_move_to_field_value(self._p._h))

    def assert_no_more_json_values(self):
        self._check(lib().sjmi_od_assert_no_more_values(self._p._h))
