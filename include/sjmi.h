/*
 * sjmi.h -- C ABI of libsjmi.so: the MI355X (gfx950) stage-1 engine behind
 * simdjson-java's SimdJsonParser.parse(byte[], int).
 *
 * The reference has no FFI: its narrowest seam is the private method
 *     SimdJsonParser.stage1(byte[] buffer, int length)
 *         /root/reference/src/main/java/org/simdjson/SimdJsonParser.java:55-58
 * whose only observable effects are (a) BitIndexes.indexes[0..writeIdx] (ascending byte
 * offsets + a 0 sentinel, BitIndexes.java:14-41,82-96) and (b) one of three
 * JsonParsingExceptions (Utf8Validator.java:165-167, StructuralIndexer.java:297-302).
 * Every entry point below is what a Panama/JNI binding of that seam calls; INTEGRATION.md
 * shows the Java side.  Plain pointers and sizes only; no callbacks; no exceptions.
 *
 * Return value: 0 = the call ran (JSON-level verdicts are in `status`), < 0 = infrastructure
 * error (HIP failure, bad argument, capacity) -- never conflated with a JSON error.
 */
#ifndef SJMI_H
#define SJMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SJMI_PADDING 64u /* readable bytes required after len; SimdJsonParser.java:5 (PADDING) */

/* status bits; the Java shim throws the lowest set bit first (reference order of checks) */
#define SJMI_ST_UTF8 1u       /* "The input is not valid UTF-8"                      Utf8Validator.java:165-167 */
#define SJMI_ST_UNCLOSED 2u   /* "Unclosed string. A string is opened, but never closed." StructuralIndexer.java:297-299 */
#define SJMI_ST_UNESCAPED 4u  /* "Unescaped characters. Within strings, ..."         StructuralIndexer.java:300-302 */
#define SJMI_ST_CAPACITY 0x100u /* index_capacity < count+1 (the reference throws AIOOBE here) */
#define SJMI_ST_INTERNAL 0x200u /* engine fault (look-back timeout); results invalid */
#define SJMI_ST_REJECTED 0x800u /* sjmi_parse_batch_device_optimistic only: the batch is not one the optimistic pipeline can take (a document
                                 * fails stage 1, a separator is missing, the offsets do not cover the buffer): NO output of the call is
                                 * valid -- call sjmi_parse_batch_device_rejected (or sjmi_parse_batch_device), which decide every document on its own */
#define SJMI_ST_HALO 0x400u     /* sjmi_stage1_shard_device / sjmi_stream_push: a backslash run fills the whole left halo, so whether the
                                   byte behind it is escaped cannot be told from what is readable; results invalid -- give more halo */

/* return codes */
#define SJMI_OK 0
#define SJMI_ERR_HIP (-1)
#define SJMI_ERR_ARG (-2)
#define SJMI_ERR_CAPACITY (-3)
#define SJMI_ERR_INTERNAL (-4)
#define SJMI_ERR_NO_DEVICE (-5)

/* string / stage-2 error codes (numbering follows oracle/sj_oracle.h so that parity tests compare ints) */
#define SJMI_E_ESCAPE_UNEXPECTED 4       /* "Escaped unexpected character: "     CharacterUtils.java:74-83 */
#define SJMI_E_INVALID_UNICODE_ESCAPE 5  /* "Invalid unicode escape sequence."   StringParser.java:127-129 */
#define SJMI_E_LOW_SURROGATE_RESERVED 6  /* StringParser.java:53-55 */
#define SJMI_E_LOW_SURROGATE_NO_U 7      /* StringParser.java:113-115 */
#define SJMI_E_LOW_SURROGATE_RANGE 8     /* StringParser.java:118-122 */
#define SJMI_E_UTF8 1
#define SJMI_E_UNCLOSED_STRING 2
#define SJMI_E_UNESCAPED_CHARS 3
#define SJMI_E_NO_STRUCTURAL 9           /* JsonIterator.java:27-29; 10..21: grammar errors JsonIterator.java / TapeBuilder.java */
#define SJMI_E_UNCLOSED_OBJECT 10
#define SJMI_E_UNCLOSED_ARRAY 11
#define SJMI_E_OBJECT_NO_KEY 12
#define SJMI_E_MISSING_COLON 13
#define SJMI_E_KEY_MISSING 14
#define SJMI_E_NO_COMMA_OBJECT 15
#define SJMI_E_NO_COMMA_ARRAY 16
#define SJMI_E_TRAILING_CONTENT 17
#define SJMI_E_UNRECOGNIZED_PRIMITIVE 18
#define SJMI_E_INVALID_TRUE 19
#define SJMI_E_INVALID_FALSE 20
#define SJMI_E_INVALID_NULL 21
#define SJMI_E_NUM_MINUS 22              /* 22..27: NumberParser.java:34-72, ExponentParser.java:27-29 */
#define SJMI_E_NUM_LEADING_ZERO 23
#define SJMI_E_NUM_DECIMAL_POINT 24
#define SJMI_E_NUM_EXPONENT 25
#define SJMI_E_NUM_FOLLOWED 26
#define SJMI_E_NUM_LONG_RANGE 27
#define SJMI_E_DEPTH 28                  /* the reference throws ArrayIndexOutOfBoundsException (JsonIterator.java:69-70) */
#define SJMI_E_CAPACITY 29
#define SJMI_E_INTERNAL 100              /* engine invariant violated (never for status == 0 input) */

typedef struct sjmi_ctx sjmi_ctx;

/* device-side result record of one stage-1 call */
typedef struct sjmi_stage1_result {
    uint64_t count;   /* BitIndexes.writeIdx */
    uint32_t status;  /* SJMI_ST_* */
    uint32_t reserved;
} sjmi_stage1_result;

/* One context per host thread (SimdJsonParser is not thread-safe either: SimdJsonParser.java:9-13
 * shares one BitIndexes).  capacity_bytes = largest document, as the reference's ctor argument
 * `capacity` (SimdJsonParser.java:19-26). Owns a HIP stream, device staging buffers and the
 * tile-state workspace. Fails with SJMI_ERR_NO_DEVICE when no gfx950 device is usable: there is
 * no CPU fallback. */
int sjmi_create(sjmi_ctx** out, int device, uint64_t capacity_bytes);
void sjmi_destroy(sjmi_ctx* ctx);
const char* sjmi_last_error(const sjmi_ctx* ctx);
const char* sjmi_version(void);

/* Replaces SimdJsonParser.stage1 (+ padIfNeeded) for HOST buffers: copies buf[0,len) to the
 * device (padding handled internally: bytes >= len are never read from `buf`), runs the fused
 * kernel, copies indexes[0..count] (sentinel included) and the verdict back.
 * indexes must hold index_capacity entries; needs index_capacity >= count+1.  Like BitIndexes.write's speculative
 * stores (BitIndexes.java:14-41: "garbage may follow the valid prefix"), the call may write ANY entry of
 * indexes[0, index_capacity) -- small documents are downloaded by their bound, not by their count -- so a caller
 * must not keep other data inside that range; only indexes[0..count] are meaningful.  The same holds for
 * string_buffer[0, string_capacity) of sjmi_stage1_unescape / sjmi_unescape (StringParser's over-copy, :33-34). */
int sjmi_stage1(sjmi_ctx* ctx, const uint8_t* buf, uint64_t len, uint32_t* indexes, uint64_t index_capacity,
                uint64_t* count, uint32_t* status);

/* Same path on DEVICE-resident data (roofline runs, pipelines that already hold the document in
 * HBM). d_buf must be 16-byte aligned with SJMI_PADDING readable bytes after len (contents
 * ignored); d_indexes (16-byte aligned) holds index_capacity u32; d_result is a device sjmi_stage1_result.
 * Asynchronous on `stream` (a hipStream_t, may be NULL = the context's stream). len < 2^32. */
int sjmi_stage1_device(sjmi_ctx* ctx, const void* d_buf, uint64_t len, void* d_indexes, uint64_t index_capacity,
                       void* d_result, void* stream);

/* Bit-mask parity entry point: the six 64-bit masks one iteration of the reference's stage-1 loop holds for every 64-byte
 * block (StructuralIndexer.java:210-252), masks[6*b + {0..5}] = {escaped, quote, inString, op, whitespace, structurals}
 * of block b, for all len / 64 + 1 blocks (the reference always processes one space-padded tail block, :255-294,305-309).
 * They are internal locals of the reference (never asserted by its tests); north_star asks for them bit-exact, so the
 * engine reconstructs them from its own per-block formulation + the resolved in-string parity (csrc/masks.hip).
 * Host form: copies buf[0,len) in, masks out; needs mask_capacity_blocks >= len / 64 + 1; *n_blocks = blocks written.
 * Device form: d_buf as for sjmi_stage1_device, d_masks holds 6 * (len / 64 + 1) uint64; asynchronous on `stream`. */
int sjmi_stage1_masks(sjmi_ctx* ctx, const uint8_t* buf, uint64_t len, uint64_t* masks, uint64_t mask_capacity_blocks,
                      uint64_t* n_blocks);
int sjmi_stage1_masks_device(sjmi_ctx* ctx, const void* d_buf, uint64_t len, void* d_masks, uint64_t mask_capacity_blocks,
                             void* stream);

/* ONE SHARD of a document that is split over several GPUs, or ONE CHUNK of a document stream (SURVEY.md 8(e) row 2, 8(f)
 * rank 4; the reference has no counterpart: one byte[] per parse).  d_buf points at the shard's first byte (16-byte
 * aligned), with halo_bytes (a multiple of 64, >= 64 unless the shard starts the document) of the document's preceding
 * bytes readable right in front of it: everything stage 1 carries from block to block except the in-string parity is
 * re-derived from those bytes (escape run, previous scalar, UTF-8 continuation -- a backslash run that fills the whole
 * halo is the only thing it cannot see through: the call then reports SJMI_ST_HALO and the caller repeats it with a larger
 * halo).  is_last = 0: the shard ends on a 64-byte boundary (len % 64 == 0) and has
 * no tail block -- what straddles the boundary is validated by the next shard.  entry_parity = 1: the shard starts
 * inside a string.  Indexes are relative to d_buf; result.status bit SJMI_ST_UNCLOSED = the parity AFTER the shard.
 * Protocol (sharding.py DocumentSplit): run every shard with entry_parity 0; exchange the parities (1 bit per shard: the
 * first collective); a shard whose true entry parity is 1 runs again with entry_parity 1; exchange the counts. */
int sjmi_stage1_shard_device(sjmi_ctx* ctx, const void* d_buf, uint64_t len, uint64_t halo_bytes, int is_last, int entry_parity,
                             void* d_indexes, uint64_t index_capacity, void* d_result, void* stream);
/* the same with one more fact: halo_from_document_start != 0 = the halo begins at the document's first byte (nothing is in
 * front of it, so a backslash run that fills it is complete and SJMI_ST_HALO is never reported) */
int sjmi_stage1_shard_device2(sjmi_ctx* ctx, const void* d_buf, uint64_t len, uint64_t halo_bytes, int halo_from_document_start,
                              int is_last, int entry_parity, void* d_indexes, uint64_t index_capacity, void* d_result, void* stream);

/* The same as a PRODUCT feature, with the protocol's state kept in C (no per-chunk allocation, nothing for a binding to
 * re-implement): ONE document as a stream of chunks on one GPU -- a document of any length (the 4 GiB - 1 of uint32 indexes
 * and the 2 GiB of a Java byte[] apply to a chunk, not to the stream).  sjmi_stream_open sizes the device buffers once
 * (max_chunk_bytes per push; halo_bytes, a multiple of 64, 0 = 64: how much of the stream in front of a chunk stage 1 looks
 * at; up to 4 KiB of the stream are kept on the device, and a chunk whose halo proves too short -- SJMI_ST_HALO -- is
 * repeated with more of them by the call itself).  sjmi_stream_push: chunk = host bytes, every chunk but the last a non-zero
 * multiple of 64 long; indexes[0..*count] = the chunk's structurals RELATIVE to the chunk (+ the sentinel), *base = the
 * chunk's offset in the stream; *status = the document's verdict so far (SJMI_ST_UNCLOSED only behind the last chunk).
 * The in-string parity is carried from chunk to chunk, so every chunk is scanned exactly once.
 * A push that returns SJMI_ERR_ARG or SJMI_ERR_CAPACITY (index_capacity < *count + 1; a backslash run longer than the bytes kept) took
 * nothing of the chunk and leaves the stream as it was: the same chunk may be pushed again, with a larger array for instance. */
typedef struct sjmi_stream sjmi_stream;
int sjmi_stream_open(sjmi_ctx* ctx, uint64_t max_chunk_bytes, uint64_t halo_bytes, sjmi_stream** out);
int sjmi_stream_push(sjmi_stream* s, const uint8_t* chunk, uint64_t len, int is_last, uint32_t* indexes, uint64_t index_capacity,
                     uint64_t* count, uint64_t* base, uint32_t* status);
void sjmi_stream_close(sjmi_stream* s);
/* ... and one rank's shard of a document split over several GPUs (arguments as sjmi_stage1_shard_device2; everything stays
 * on the device).  sjmi_split_scan: the shard as if it began outside a string; *flips_parity = does it flip the in-string
 * parity -- all_gather that bit (the first collective).  sjmi_split_resolve(entry_parity = XOR of the flips of the ranks in
 * front): scans again ONLY if the entry parity is 1; -> the shard's count / status bits / parity behind it -- all_gather
 * those (the second collective): global index offsets = prefix sums of the counts, the document is unclosed iff the LAST
 * shard's parity_after is 1.  (A shard entered inside a string costs a second scan: both polarities in one pass would double
 * the index stores of the hot kernel for everybody) */
typedef struct sjmi_split sjmi_split;
int sjmi_split_open(sjmi_ctx* ctx, const void* d_shard, uint64_t len, uint64_t halo_bytes, int halo_from_document_start, int is_last,
                    void* d_indexes, uint64_t index_capacity, sjmi_split** out);
int sjmi_split_scan(sjmi_split* s, void* stream, int* flips_parity, uint32_t* status);
int sjmi_split_resolve(sjmi_split* s, int entry_parity, void* stream, uint64_t* count, uint32_t* status, int* parity_after);
void sjmi_split_close(sjmi_split* s);

/* device-side result record of one unescape call */
typedef struct sjmi_unescape_result {
    uint64_t total_bytes;      /* bytes of [be32 length][unescaped bytes] records written */
    uint64_t first_error_inv;  /* 0 = every string is fine; else ~((p << 8) | SJMI_E_* code) of the first failing string, p = byte
                                  offset of the offending escape in the document (sjmi_unescape_device, sjmi_parse_*), or the
                                  string's position in indexes[] (sjmi_unescape_batch_device) */
    uint32_t flags;            /* bit 0: string_buffer capacity exceeded; bit 1: more strings than the record table holds
                                * (index_capacity - 1 + 64 entries: raise index_capacity; no tape is built); bits 2-3: engine fault (results invalid) */
    uint32_t n_strings;        /* string literals of the document (sjmi_unescape_device) */
} sjmi_unescape_result;

/* Batched replacement of the per-string StringParser.parseString calls (StringParser.java:18-68) that
 * the reference's stage 2 makes for every string (TapeBuilder.java:174-177): for every string literal of the
 * document, in order, appends [be32 length][unescaped UTF-8 bytes] to string_buffer, so that
 * record k starts at sum_{j<k}(4 + len_j) -- exactly the STRING tape payloads of a valid document, and byte for byte
 * the reference's stringBuffer.  One streaming pass over the document (csrc/strings.hip); the index array is not
 * read (it is part of the signature because the reference's loop is over the '"' structurals: every opening quote of a
 * document that passes stage 2 is one).  It starts from the in-string parity of every 64-byte block, which the last
 * sjmi_stage1*_device launch of this context over the same (d_buf, len) left on the device -- the bytes must not have
 * changed since; without one (another context indexed the document) the call derives them itself with one more pass.
 * A string StringParser would throw on gets the record header FF FF FF <SJMI_E_* code> (what follows it up to the next
 * record is unspecified), all other records are still exact and in place; the first such error is also reported in
 * d_result.  Requires a stage-1 status of 0 for this document (closed strings); string_capacity < 4 GiB.
 * Device-resident form, asynchronous on `stream`; d_buf 16-byte aligned; d_result is a device sjmi_unescape_result. */
int sjmi_unescape_device(sjmi_ctx* ctx, const void* d_buf, uint64_t len, const void* d_indexes, uint64_t count,
                         void* d_string_buffer, uint64_t string_capacity, void* d_result, void* stream);

/* Host form: unescapes the strings of the document given to the LAST sjmi_stage1 call on this context
 * (its bytes and indexes are still resident on the device) into string_buffer[0, *total_bytes).
 * *first_error_index = position in indexes[] of the first failing string or UINT64_MAX; *first_error_code = SJMI_E_*. */
int sjmi_unescape(sjmi_ctx* ctx, uint8_t* string_buffer, uint64_t string_capacity, uint64_t* total_bytes,
                  uint64_t* first_error_index, uint32_t* first_error_code);

/* SimdJsonParser.parse's GPU part in ONE call: sjmi_stage1 followed by sjmi_unescape of the same document, with two
 * host synchronisations instead of four (the unescape kernels read the structural count from the stage-1 result on
 * the device).  Outputs as in the two separate calls; the string outputs are meaningful only if *status == 0. */
int sjmi_stage1_unescape(sjmi_ctx* ctx, const uint8_t* buf, uint64_t len, uint32_t* indexes, uint64_t index_capacity,
                         uint64_t* count, uint32_t* status, uint8_t* string_buffer, uint64_t string_capacity,
                         uint64_t* total_bytes, uint64_t* first_error_index, uint32_t* first_error_code);

/* ---- batched documents ---------------------------------------------------------------------------------
 * n_docs documents packed in one buffer, document k at [doc_offsets[k], doc_offsets[k+1]), each followed by at
 * least one JSON whitespace byte inside its range (NDJSON style; doc_offsets[n_docs] = total length).
 * One stage-1 launch indexes the whole buffer; index_offsets[k] (n_docs+1 entries) then delimits document k's
 * indexes, which stay ABSOLUTE byte offsets (subtract doc_offsets[k] for the reference's per-document values).
 * status is the verdict of the whole batch (exact whenever every document passes stage 1; see batch.hip).
 * Device form, asynchronous on `stream`. */
int sjmi_stage1_batch_device(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_doc_offsets,
                             uint64_t n_docs, void* d_indexes, uint64_t index_capacity, void* d_index_offsets,
                             void* d_result, void* stream);
/* Host form: copies the batch in, returns indexes[0..count], index_offsets[0..n_docs], count and status. */
int sjmi_stage1_batch(sjmi_ctx* ctx, const uint8_t* buf, uint64_t total_len, const uint64_t* doc_offsets, uint64_t n_docs,
                      uint32_t* indexes, uint64_t index_capacity, uint64_t* index_offsets, uint64_t* count,
                      uint32_t* status);

/* ---- doc_offsets of a buffer of newline-delimited JSON, made on the device (csrc/ndjson.hip) --------------
 * NL is 0x0A; BLANK is 0x20, 0x09 and 0x0D and nothing else ('\f', '\v', NUL and a BOM are content).  A LINE is a maximal run
 * of non-NL bytes plus the NL that ends it; the TAIL, the bytes behind the last NL, is never a line and never a document;
 * consumed = the index behind the last NL (0 without one).  A line is blank when every byte before its NL is BLANK (empty lines,
 * "\r\n" lines); n_docs = the lines that are not.  With s_0 < s_1 < ... the start offsets of those lines: doc_offsets[0] = 0,
 * doc_offsets[k] = s_k for k >= 1, doc_offsets[n_docs] = consumed -- blank lines are trailing whitespace of the document in
 * front of them, leading ones leading whitespace of document 0, so the documents cover [0, consumed) exactly and each ends in
 * '\n': what sjmi_parse_batch_device_optimistic accepts.  With n_docs == 0 only doc_offsets[0] = 0 is written.  A raw NL inside
 * a string is illegal JSON: it splits the document into two malformed ones, as in every NDJSON reader.
 * d_buf may have ANY alignment and len any value, 0 included; SJMI_PADDING bytes behind len are readable (vector loads reach
 * into them; they never influence the result), and so are the bytes between d_buf and the 16-byte boundary below it (the same
 * allocation).  d_doc_offsets: offset_capacity uint64; d_result: a device sjmi_ndjson_result.  n_docs and consumed are ALWAYS
 * complete; with offset_capacity < n_docs + 1 (SJMI_NDJSON_OVERFLOW) only doc_offsets[0, offset_capacity) are written and nothing
 * behind them -- offset_capacity == 0 with a NULL d_doc_offsets is legal and is how a caller sizes its array (one read of the
 * input instead of two).  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but the
 * three kernels -- except that a call with a larger len than any before it on this context grows the context's per-tile scratch,
 * which waits for the device and may block.  That scratch is one per context: ndjson calls on ONE context must be ordered with
 * respect to each other (the same stream, or streams the caller orders with events); use a context per stream otherwise.
 * A caller that streams a large file parses [0, consumed) and carries [consumed, len) to the front of its next chunk; at the end
 * of the file it appends one '\n' if the last byte is not one (this call does not; the Python helper parse_ndjson does). */
#define SJMI_NDJSON_TAIL_BLANK 1u  /* every byte of [consumed, len) is BLANK (an empty tail included) */
#define SJMI_NDJSON_OVERFLOW   2u  /* offset_capacity < n_docs + 1 */
typedef struct sjmi_ndjson_result {
    uint64_t n_docs, consumed;
    uint32_t flags, reserved;
} sjmi_ndjson_result;
int sjmi_ndjson_offsets_device(sjmi_ctx* ctx, const void* d_buf, uint64_t len, void* d_doc_offsets, uint64_t offset_capacity,
                               void* d_result, void* stream);
/* Host form: copies buf[0, len) in (len <= the context's capacity), runs the device form, returns doc_offsets[0, min(n_docs + 1,
 * offset_capacity)), *n_docs, *consumed and *flags. */
int sjmi_ndjson_offsets(sjmi_ctx* ctx, const uint8_t* buf, uint64_t len, uint64_t* doc_offsets, uint64_t offset_capacity,
                        uint64_t* n_docs, uint64_t* consumed, uint32_t* flags);
uint64_t sjmi_ndjson_tile_bytes(void); /* the kernels' tile; tests place their edge cases by it */

/* ISOLATED batch: exact per document whatever the other documents contain.  One wave per document, every carry
 * (in-string parity, escape run, previous scalar, UTF-8 continuation) starts from zero at the document's first byte.
 * doc_status[k] = the SJMI_ST_* bits document k would get from sjmi_stage1 on its own; a document with a non-zero
 * status contributes NO indexes (index_offsets[k+1] == index_offsets[k], as the reference throws before its stage 2);
 * the others get exactly their own indexes (absolute byte offsets).  result.status = OR of the document statuses
 * (| SJMI_ST_CAPACITY), result.count = indexes written.  The plain batch above cannot attribute an error to a document,
 * and two documents with an unclosed string each cancel in its verdict.  This call tries it first all the same -- ONE
 * plain launch over the packed buffer -- and accepts it ON THE DEVICE when that is provably what the per-document passes
 * would give: every document ends in a control-character separator ('\n', '\r', '\t': an open string would turn it into
 * an unescaped character), doc_offsets[0] == 0 and doc_offsets[n_docs] == total_len, and the global verdict is clean.
 * The per-document passes are queued behind it and leave at once when it was accepted, so nothing comes back to the host.
 * Device form, asynchronous on `stream`; d_doc_status: n_docs uint32; d_buf and d_indexes 16-byte aligned for the
 * plain pass (else only the per-document passes run). */
int sjmi_stage1_batch_isolated_device(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_doc_offsets,
                                      uint64_t n_docs, void* d_indexes, uint64_t index_capacity, void* d_index_offsets,
                                      void* d_doc_status, void* d_result, void* stream);
/* Host form. */
int sjmi_stage1_batch_isolated(sjmi_ctx* ctx, const uint8_t* buf, uint64_t total_len, const uint64_t* doc_offsets,
                               uint64_t n_docs, uint32_t* indexes, uint64_t index_capacity, uint64_t* index_offsets,
                               uint32_t* doc_status, uint64_t* count, uint32_t* status);

/* sjmi_unescape for the batch given to the LAST sjmi_stage1_batch / sjmi_stage1_batch_isolated call on this context:
 * one string buffer for the whole batch (records in structural order), plus doc_string_offsets[k] (n_docs + 1 entries)
 * = offset of document k's first record, so that the stage 2 of every document can start at its own offset (documents
 * can then be walked by parallel host threads). */
int sjmi_unescape_batch(sjmi_ctx* ctx, uint8_t* string_buffer, uint64_t string_capacity, uint64_t* doc_string_offsets,
                        uint64_t* total_bytes, uint64_t* first_error_index, uint32_t* first_error_code);

/* Device-resident form of the same, asynchronous on `stream`: indexes / doc_offsets / index_offsets as given to and
 * produced by sjmi_stage1_batch[_isolated]_device (device pointers, n_docs + 1 uint64 entries each).  Unlike
 * sjmi_unescape_device it knows the document boundaries: in isolated mode a document that failed stage 1 has no
 * structurals, so the last string of the document in front of it must end at that document's end, not at the next
 * structural of the batch.  d_doc_string_offsets may be NULL. */
int sjmi_unescape_batch_device(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_indexes, uint64_t count,
                               const void* d_doc_offsets, const void* d_index_offsets, uint64_t n_docs,
                               void* d_string_buffer, uint64_t string_capacity, void* d_doc_string_offsets, void* d_result,
                               void* stream);

/* ---- stage 2 on the GPU for batches ---------------------------------------------------------
 * JsonIterator.walkDocument + TapeBuilder (JsonIterator.java:26-200, TapeBuilder.java:41-217) for every document of a
 * batch, one GPU wave per document (csrc/coop_walk.hip), from the outputs of sjmi_stage1_batch_isolated_device and
 * sjmi_unescape_batch_device (all device pointers; the string pass also leaves a table of record offsets by string
 * ordinal on the context, so both calls must come from this context, for the same d_indexes).  Produces the tapes back to
 * back in d_tape (Tape.java:5-47 word layout; document k: words [tape_offsets[k], tape_offsets[k+1]), its container words
 * relative to its own start, STRING payloads = string_base + offset of the record in d_string_buffer) and doc_errors[k]
 * (int32): 0, or the SJMI_E_* code of the document's first error (stage-1 verdicts and malformed escapes included) with an
 * empty tape, or SJMI_WALK_NEEDS_HOST with an empty tape.  The device decides everything the reference's defaults admit:
 * nesting up to 1024 open containers (SimdJsonParser.java:7) and every number literal, including floating-point literals
 * of more than 19 significant digits at a rounding boundary (exact big-integer comparison with the midpoint, DoubleParser.
 * java:205-330).  Handed back only: max_depth > 1024 and a document that uses it, more than 65,536 such boundary literals
 * in one launch, a single document of more than 2^31 - 256 structurals.  d_result: sjmi_walk_result, bit 0 of flags =
 * tape_capacity exceeded: tape_words and tape_offsets are valid and complete, nothing at or behind d_tape[tape_capacity] is
 * written, and the tapes are unspecified -- except where sjmi_parse_batch_device* laid them out before the walk (below): there
 * every well-formed document whose slot ends at or below tape_capacity has its tape.  d_buf needs 64 readable bytes after the batch (the
 * reference's padding, SimdJsonParser.java:42-48).  Asynchronous on `stream`. */
#define SJMI_WALK_NEEDS_HOST (-1)
typedef struct sjmi_walk_result {
    uint64_t tape_words;       /* total tape words = tape_offsets[n_docs] */
    uint64_t host_documents;   /* documents left to the host walker */
    uint64_t failed_documents; /* documents with a JSON error */
    uint32_t flags;
    uint32_t reserved;
} sjmi_walk_result;
int sjmi_walk_batch_device(sjmi_ctx* ctx, const void* d_buf, const void* d_doc_offsets, uint64_t n_docs, const void* d_indexes,
                           uint64_t count, const void* d_index_offsets, const void* d_doc_status,
                           const void* d_string_buffer, const void* d_doc_string_offsets, uint64_t string_base,
                           int max_depth, void* d_tape, uint64_t tape_capacity, void* d_tape_offsets, void* d_doc_errors,
                           void* d_result, void* stream);

/* The whole batched parse, device-resident, in ONE call and without a host round trip between the stages:
 * sjmi_stage1_batch_isolated_device -> sjmi_unescape_batch_device -> sjmi_walk_batch_device (string_base 0), the
 * structural count handed from stage to stage on the device.  Outputs as documented for the three calls; index_capacity
 * bounds the structural count (+ sentinel) and sizes the workspaces.  d_result: a device sjmi_batch_result.  This is
 * what one rank of the sharded multi-GPU batch runs per step (sharding.py); asynchronous on `stream`.
 * Stage 1 is first tried as ONE plain launch over the packed batch and accepted on the device when every document ends in
 * a control-character separator ('\n', '\r', '\t'), the documents cover the buffer exactly (doc_offsets[0] == 0 and
 * doc_offsets[n_docs] == total_len: bytes outside the documents would feed state into them) and the global verdict is
 * clean -- then it is exactly what the per-document passes give; otherwise those run (queued behind it, they leave at once
 * when it was accepted).  (Round 5: the separators are checked by k_doc_prepare, which visits every boundary anyway, so the
 * verdict falls behind the string pass: a rejected batch pays one string pass over the raw batch before its own begins.)
 * Tapes: when the plain pass was accepted the tapes are laid out BEFORE the documents are walked (a document's tape length
 * is a function of its structurals' first bytes: TapeBuilder.java:41-48,191-208, Tape.java:33-43) and written at their final
 * addresses.  A document that then fails stage 2 (doc_errors[k] != 0) keeps its slot: tape_offsets[k + 1] - tape_offsets[k] is
 * its PREDICTED length and the words there are unspecified; walk.tape_words counts the slots.  Every well-formed document's
 * tape is where and what it always was, and a batch without failing documents is packed exactly as before.  (When the plain
 * pass was rejected -- some document fails stage 1, a separator is missing -- the REPAIR stage described at
 * sjmi_parse_batch_device_rejected takes the batch and reports like an accepted one; only behind a batch it cannot take either are
 * the tapes packed behind the walk and a failing document's range empty, as with sjmi_walk_batch_device.) */
typedef struct sjmi_batch_result {
    sjmi_stage1_result stage1;
    sjmi_unescape_result strings;
    sjmi_walk_result walk;
} sjmi_batch_result;
int sjmi_parse_batch_device(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_doc_offsets, uint64_t n_docs,
                            void* d_indexes, uint64_t index_capacity, void* d_index_offsets, void* d_doc_status,
                            void* d_string_buffer, uint64_t string_capacity, void* d_doc_string_offsets, int max_depth,
                            void* d_tape, uint64_t tape_capacity, void* d_tape_offsets, void* d_doc_errors, void* d_result,
                            void* stream);
/* The same call with ONLY the optimistic pipeline queued (round 5): k_stage1_batch -> k_strings -> k_doc_prepare -> tape layout ->
 * the token walker (+ the exact walker and the boundary-literal kernel for the documents it lists) -- eight queue entries instead
 * of thirty, which is what a small batch (one rank's share of a strong-scaled run) is bounded by.  Whether the batch qualified is
 * decided on the device like before and reported in result.stage1.status: SJMI_ST_REJECTED set = NOTHING this call wrote is
 * valid; the caller then makes the exact call above (same arguments), off its hot path.  Without that bit the outputs are
 * exactly those of sjmi_parse_batch_device.  NDJSON whose documents all pass stage 1 is never rejected. */
int sjmi_parse_batch_device_optimistic(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_doc_offsets, uint64_t n_docs,
                                       void* d_indexes, uint64_t index_capacity, void* d_index_offsets, void* d_doc_status,
                                       void* d_string_buffer, uint64_t string_capacity, void* d_doc_string_offsets, int max_depth,
                                       void* d_tape, uint64_t tape_capacity, void* d_tape_offsets, void* d_doc_errors, void* d_result,
                                       void* stream);

/* The call to make after sjmi_parse_batch_device_optimistic came back with SJMI_ST_REJECTED (round 6; same arguments, same outputs as
 * sjmi_parse_batch_device -- which is this call behind one more attempt at the plain pass).  The reference isolates a malformed
 * document for free -- one JsonParsingException per SimdJsonParser.parse, SimdJsonParser.java:35-40, the neighbours never see it --
 * so a batch with ONE bad document in a million must not cost a multiple of a clean one.  On the device, no host round trip:
 * every document gets its own stage-1 verdict (16 lanes per document, all carries from zero), the documents that fail are
 * blanked in a sanitized copy, and the optimistic pipeline runs over that copy (REPAIR) -- exact, because every surviving
 * document begins and ends outside a string; documents that are not separated at all are taken too as long as no scalar can run
 * on across a boundary (the last byte of every document is whitespace, an operator or a quote).  A batch that fails that rule
 * (or whose document offsets do not cover the buffer) comes back with SJMI_ST_REJECTED ONCE MORE: sjmi_parse_batch_device then
 * serves it with the per-document index passes -- three levels, each cheaper than the next, the last one takes anything.  A repaired batch reports like an accepted one: a document that failed stage 1
 * has doc_status[k] / doc_errors[k] set, no structurals and a two-word tape slot with unspecified contents; stage1.status is the
 * OR of the documents' verdicts.  (SJMI_BATCH_REPAIR=0 switches the repair stage off.) */
int sjmi_parse_batch_device_rejected(sjmi_ctx* ctx, const void* d_buf, uint64_t total_len, const void* d_doc_offsets, uint64_t n_docs,
                                     void* d_indexes, uint64_t index_capacity, void* d_index_offsets, void* d_doc_status,
                                     void* d_string_buffer, uint64_t string_capacity, void* d_doc_string_offsets, int max_depth,
                                     void* d_tape, uint64_t tape_capacity, void* d_tape_offsets, void* d_doc_errors, void* d_result,
                                     void* stream);

/* One document, ALL stages on the GPU: stage 1, string records and the cooperative walker (csrc/coop_walk.hip: JsonIterator.
 * walkDocument + TapeBuilder as scans, JsonIterator.java:26-200, TapeBuilder.java:41-217); only the tape (Tape.java:5-47 word
 * layout, tape[0] = root) and the string buffer come back -- the structural indexes stay on the device.  *error = 0, or the
 * document's SJMI_E_* code (stage-1 verdicts included; no tape), or SJMI_WALK_NEEDS_HOST (see sjmi_walk_batch_device: not
 * for anything the reference's default limits admit; sjmi_parser_parse walks such a document on the host). */
int sjmi_parse_document(sjmi_ctx* ctx, const uint8_t* buf, uint64_t len, int max_depth, uint64_t* tape, uint64_t tape_capacity,
                        uint64_t* tape_len, uint8_t* string_buffer, uint64_t string_capacity, uint64_t* strings_len,
                        int32_t* error, uint32_t* stage1_status);

/* ---- whole parse: SimdJsonParser.parse(byte[], int) (SimdJsonParser.java:35-40) ----------------------------
 * GPU stage 1 + GPU string unescape + the host stage-2 tree builder (C++ mirror of JsonIterator / TapeBuilder /
 * Tape: simdjson-java_amd/csrc/host/simdjson_parser.h).  The tape (Tape.java:5-47 word layout) and string
 * buffer views stay valid until the next parse on this parser (like the reference's JsonValue).
 * Returns 0, or > 0 = SJMI_E_* JSON error (message: sjmi_parser_last_message, exact reference text), or < 0. */
typedef struct sjmi_parser sjmi_parser;
int sjmi_parser_create(sjmi_parser** out, int capacity, int max_depth, int device);
void sjmi_parser_destroy(sjmi_parser* p);
int sjmi_parser_parse(sjmi_parser* p, const uint8_t* buf, uint64_t len, const uint64_t** tape, uint64_t* tape_len,
                      const uint8_t** strings, uint64_t* strings_len, uint64_t* error_pos);
const char* sjmi_parser_last_message(const sjmi_parser* p);
/* Where stage 2 of sjmi_parser_parse runs: 0 = the host walker over the GPU-made indexes and string records, 1 = the
 * cooperative GPU walker (sjmi_parse_document): the tape comes from the device, and only a document that fails or is
 * handed back is walked again on the host (for the exact exception); < 0 (the default) = by size: the GPU walker for
 * documents of 128 KiB and more (twitter.json 0.148 vs 0.188 ms, 2.4 x faster at 1 MiB, 6 x from 16 MiB on), the host
 * walker below.  Identical results. */
int sjmi_parser_set_gpu_walk(sjmi_parser* p, int on);
/* Batched parse (BASELINE.json configs[3]/[4]): the batch goes through the GPU (isolated stage 1 + string records)
 * as a pipeline of sub-batches on two streams, the host stage 2 of the documents runs on a pool of threads
 * (SJMI_PARSE_THREADS, default min(64, cores)) while the GPU works on the next sub-batch.  Document k's tape is
 * tape[tape_offsets[k] .. tape_offsets[k+1]) (container words relative to its own start, STRING payloads = offsets
 * into the shared `strings` buffer, which has unused gaps between sub-batches) and errors[k] is 0 or document k's
 * own SJMI_E_* error -- stage-1 errors included (isolated batch mode: one broken document never affects another).
 * The call itself is made from one thread; the parser is not thread-safe (like the reference's). */
int sjmi_parser_parse_batch(sjmi_parser* p, const uint8_t* buf, uint64_t total_len, const uint64_t* doc_offsets,
                            uint64_t n_docs, const uint64_t** tape, const uint64_t** tape_offsets,
                            const uint8_t** strings, uint64_t* strings_len, const int32_t** errors);

/* ---- the on-demand front end --------------------------------------------------------------
 * OnDemandJsonIterator (OnDemandJsonIterator.java:7-675), the cursor SchemaBasedJsonIterator.java:29-132 drives with one
 * call per field of the schema: it walks the structural indexes of stage 1 and parses only the values it is asked for.
 * sjmi_parser_ondemand_init = SimdJsonParser.parse(buffer, len, Class) up to and including iterator.init (:31-41): pad and
 * GPU stage 1.  (`reserved` must be 0.  Rounds 2-4 built a GPU skip table here -- up[] / match[] per structural, skipChild as
 * a lookup -- that never paid: 0.256 against 0.159 ms per parse-and-select of twitter.json, because the scan it replaced costs
 * ~1 ns per structural on the host and the table two kernels plus 8 bytes per structural over PCIe.  Removed in round 5.)
 * The calls below mirror
 * the iterator's methods one to one (root != 0: the Root form; nullable == 0: the NonNull form; *is_null: the method
 * returned null); each returns 0, or > 0 = the SJMI_E_* code of the JsonParsingException the reference throws there
 * (exact text: sjmi_parser_last_message), or < 0.  Every getter of the class is here. */
#define SJMI_E_OD_NOT_ENOUGH_CLOSE 40    /* "Not enough close braces."                                   :80 */
#define SJMI_E_OD_EXPECTED_CHAR 41       /* "Expected 'x' but got: 'y'."                                 :662 */
#define SJMI_E_OD_EXPECTED_CHAR_END 42   /* "Expected 'x' but reached end of buffer."                    :660 */
#define SJMI_E_OD_BOOLEAN 43             /* "Unrecognized boolean value. Expected: 'true' or 'false'."   :88,:152 */
#define SJMI_E_OD_BOOLEAN_OR_NULL 44     /* "... Expected: 'true', 'false' or 'null'."                   :104,:167 */
#define SJMI_E_OD_STRING_OR_NULL 45      /* "Invalid value starting at N. Expected either string or 'null'."  :455,:470 */
#define SJMI_E_OD_FLOAT_PART_MISSING 46  /* "Invalid floating-point number. Fraction or exponent part is missing."  NumberParser.java:303 */
#define SJMI_E_OD_BYTE_RANGE 47          /* "Number value is out of byte range ([-128, 127])."            NumberParser.java:97 */
#define SJMI_E_OD_SHORT_RANGE 48         /* "... out of short range ([-32768, 32767])."                   :136 */
#define SJMI_E_OD_INT_RANGE 49           /* "... out of int range ([-2147483648, 2147483647])."           :175 */
#define SJMI_E_OD_STRING_EXPECTED 50     /* "Invalid value starting at N. Expected string."               :480,:505 */
#define SJMI_E_OD_CHAR_CODE_POINT 51     /* "Invalid code point. Should be within the range U+0000–U+D777 or U+E000–U+FFFF."  StringParser.java:78 */
#define SJMI_E_OD_CHAR_NOT_16BIT 52      /* "String cannot be deserialized to a char. Expected a single 16-bit code unit character."  :104 */
#define SJMI_E_OD_CHAR_NOT_SINGLE 53     /* "... Expected a single-character string."                    :107 */
#define SJMI_OD_EMPTY 0                  /* IteratorResult :672-674 */
#define SJMI_OD_NULL 1
#define SJMI_OD_NOT_EMPTY 2
int sjmi_parser_ondemand_init(sjmi_parser* p, const uint8_t* buf, uint64_t len, int reserved);
int sjmi_od_skip_child(sjmi_parser* p, int parent_depth);             /* skipChild(parentDepth) :47-81; < 0: skipChild() :43-45 */
int sjmi_od_get_boolean(sjmi_parser* p, int root, int nullable, int* is_null, int* value);     /* :83-109,:147-171 */
int sjmi_od_get_long(sjmi_parser* p, int root, int nullable, int* is_null, int64_t* value);    /* :321-358 */
/* the Byte :204-241 / Short :243-280 / Int :282-319 getters: bits = 8, 16, 32 (64 = sjmi_od_get_long) */
int sjmi_od_get_integral(sjmi_parser* p, int bits, int root, int nullable, int* is_null, int64_t* value);
int sjmi_od_get_double(sjmi_parser* p, int root, int nullable, int* is_null, double* value);   /* :383-428 */
int sjmi_od_get_float(sjmi_parser* p, int root, int nullable, int* is_null, float* value);     /* :360-381,:430-444 */
int sjmi_od_get_char(sjmi_parser* p, int root, int nullable, int* is_null, uint16_t* utf16_unit);  /* :474-520 */
/* getRootString / getString :446-472, getFieldName :646-652: the unescaped bytes, valid until the next of these calls */
int sjmi_od_get_string(sjmi_parser* p, int root, int* is_null, const uint8_t** bytes, uint64_t* len);
int sjmi_od_get_field_name(sjmi_parser* p, const uint8_t** bytes, uint64_t* len);
int sjmi_od_start_array(sjmi_parser* p, int root, int* result);       /* startIterating[Root]Array :522-566 -> SJMI_OD_* */
int sjmi_od_next_array_element(sjmi_parser* p, int* has_next);        /* :568-579 */
int sjmi_od_start_object(sjmi_parser* p, int root, int* result);      /* startIterating[Root]Object :581-623 */
int sjmi_od_next_object_field(sjmi_parser* p, int* has_next);         /* :625-636 */
int sjmi_od_move_to_field_value(sjmi_parser* p);                      /* :638-644 */
int sjmi_od_assert_no_more_values(sjmi_parser* p);                    /* :666-670 */
int sjmi_od_depth(const sjmi_parser* p);                              /* getDepth :654-656 */
#define SJMI_OD_END 256
int sjmi_od_peek(const sjmi_parser* p);   /* (extension for schema-less drivers) the byte of the next structural, SJMI_OD_END behind the last */

/* ---- JsonValue (JsonValue.java:18-221) over the C ABI: the DOM view of the last parse -------------------------------
 * A value is (document, tape index), like the reference's (tape, tapeIdx, stringBuffer) tuple (JsonValue.java:20-30);
 * handles stay valid until the next parse / parse_batch on the parser.  Every accessor runs the C++ mirror class
 * org_simdjson::JsonValue (csrc/host/simdjson_parser.h).  Return 0 = ok, 1 = "null" / no more elements (where Java
 * returns null or hasNext() is false), < 0 = wrong type or bad handle (where Java would throw). */
typedef struct sjmi_value {
    uint64_t doc;      /* UINT64_MAX = the document of the last sjmi_parser_parse; else document index of the last batch */
    uint64_t tape_idx;
} sjmi_value;
int sjmi_parser_root(const sjmi_parser* p, sjmi_value* out);                       /* TapeBuilder.createJsonValue :215-217 */
int sjmi_parser_batch_root(const sjmi_parser* p, uint64_t doc, sjmi_value* out);   /* > 0: that document's SJMI_E_* error */
int sjmi_value_type(const sjmi_parser* p, const sjmi_value* v);  /* '[' '{' '"' 'l' 'd' 't' 'f' 'n' (isArray() ... isString(), :32-59) */
int sjmi_value_as_long(const sjmi_parser* p, const sjmi_value* v, int64_t* out);   /* asLong :69-71 */
int sjmi_value_as_double(const sjmi_parser* p, const sjmi_value* v, double* out);  /* asDouble :73-75 */
int sjmi_value_as_boolean(const sjmi_parser* p, const sjmi_value* v, int* out);    /* asBoolean :77-79 */
/* asString :81-89: copies the UTF-8 bytes (no terminator); *len = their number even when dst_capacity is too small */
int sjmi_value_as_string(const sjmi_parser* p, const sjmi_value* v, uint8_t* dst, uint64_t dst_capacity, uint64_t* len);
int sjmi_value_get(const sjmi_parser* p, const sjmi_value* v, const uint8_t* name, uint64_t name_len, sjmi_value* out); /* get :91-107 */
int sjmi_value_size(const sjmi_parser* p, const sjmi_value* v);                    /* getSize :109-111; < 0 on error */
/* arrayIterator / objectIterator (:61-67,143-194): first element (or key), then the following one.  In an object the
 * sequence alternates key (a string value), value, key, value ... exactly as they lie on the tape. */
int sjmi_value_first(const sjmi_parser* p, const sjmi_value* container, sjmi_value* out);
int sjmi_value_next(const sjmi_parser* p, const sjmi_value* container, const sjmi_value* child, sjmi_value* out);

/* ---- selecting fields of a parsed batch on the device ----------------------------------------------------------------
 * JsonValue.get (JsonValue.java:91-107) and arrayIterator (:143-168) applied step by step along a path, for every path of
 * a PLAN and every document of a batch whose tapes are still in device memory (csrc/select.hip).
 *
 * A path is an RFC 6901 JSON Pointer: "" = the document's root value, "/a/b" = get("a").get("b"), "~0" = '~', "~1" = '/'.
 * The container at hand decides how a token is read.  Object: the token is a key, compared byte for byte with the unescaped
 * key records (Arrays.compare(...) == 0, :102); the FIRST matching member wins (:95-105), so duplicate keys resolve as in the
 * reference.  Array: the token must be "0" or a decimal without a leading zero, and names the k-th element of the iterator
 * chain (Tape.computeNextIndex, Tape.java:86-98), whose end is the matching index (:151), not the 24-bit scope count.
 * Anything else -- a scalar at hand, a token that is no index on an array ("-" included), an index past the end, a key that
 * is not there -- makes the path MISSING for that document.
 *
 * sjmi_select_plan_compile: n_paths pointers, pointer p = pointers[pointer_offsets[p], pointer_offsets[p + 1]) (n_paths + 1
 * offsets).  Host only: no device, no context.  The paths are compiled to a trie, so the members of a container are visited
 * once for all paths that pass through it; results never depend on that sharing.  SJMI_ERR_ARG: a pointer is not empty and
 * does not begin with '/'; a '~' is followed by anything but '0' or '1'; or a limit is exceeded: */
#define SJMI_SELECT_MAX_PATHS 64u       /* paths of one plan */
#define SJMI_SELECT_MAX_STEPS 16u       /* reference tokens of one path */
#define SJMI_SELECT_MAX_NAME_BYTES 4096u /* the distinct (prefix, token) pairs of the plan, each token's unescaped bytes rounded up to a
                                          * multiple of 8, together (the plan has to fit in LDS) */
typedef struct sjmi_select_plan sjmi_select_plan;
int sjmi_select_plan_compile(const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths, sjmi_select_plan** out);
void sjmi_select_plan_destroy(sjmi_select_plan* plan);
/* Every path of `plan` on every document: d_tape, d_tape_offsets, d_doc_errors, d_string_buffer are the outputs of
 * sjmi_parse_batch_device / _optimistic / _rejected or of sjmi_walk_batch_device with string_base 0 (read only here).
 * Outputs, path-major so that a column is contiguous: d_types[p * n_docs + k] (uint8) and d_values[p * n_docs + k] (uint64):
 *   type 0                  MISSING; value 0
 *   'l' 'd'                 the payload word: the int64, or the IEEE bits (Tape.getInt64Value, Tape.java:69-71; JsonValue.asDouble :73-75)
 *   't' 'f'                 1 / 0 (JsonValue.asBoolean :77-79)
 *   'n'                     0
 *   '"'                     (length << 32) | (record offset + 4): the unescaped bytes in d_string_buffer (JsonValue.getString :85-89)
 *   '[' '{'                 (Tape.getScopeCount << 32, Tape.java:82-84) | tape index of the value inside its document
 * A document with doc_errors[k] != 0 (a JSON error or SJMI_WALK_NEEDS_HOST) is MISSING on every path and its tape slot is never
 * read.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but the kernel; the first
 * call with a plan copies it to the context's device memory (one blocking upload), later calls with the same plan reuse it.
 * A context holds one plan at a time: a call with another plan first waits for the device, then uploads that one. */
int sjmi_select_batch_device(sjmi_ctx* ctx, const sjmi_select_plan* plan, const void* d_tape, const void* d_tape_offsets,
                             const void* d_doc_errors, const void* d_string_buffer, uint64_t n_docs, void* d_types, void* d_values,
                             void* stream);

/* ---- exploding one array of every parsed document into rows on the device ----------------------------------------------
 * JsonValue.arrayIterator (JsonValue.java:143-168) over ONE array per document, with JsonValue.get (:91-107) paths evaluated on
 * every element: Arrow's list<struct> shape (csrc/explode.hip).  An explode plan is a BASE pointer plus up to
 * SJMI_SELECT_MAX_PATHS ELEMENT pointers, all RFC 6901 with the token rules, limits (SJMI_SELECT_MAX_STEPS for the base and for
 * each element pointer; SJMI_SELECT_MAX_NAME_BYTES for the base and for the element pointers together) and SJMI_ERR_ARG cases
 * of sjmi_select_plan_compile.  Host only: no device, no context.
 *
 * For document k the base value is what sjmi_select_batch_device yields for the base pointer.  If it is an array ('['), its
 * elements are those of the iterator chain: from idx + 1 (:149), by Tape.computeNextIndex (Tape.java:86-98), to
 * getMatchingBraceIndex - 1 (:151) -- never the 24-bit scope count (Tape.getScopeCount, Tape.java:82-84), which saturates.
 * The document contributes 0 rows when the base is MISSING, a scalar, a string or an object, or when doc_errors[k] != 0 (its
 * tape slot is never read).  Row r = row_offsets[k] + j belongs to element j; cell (r, p) is element pointer p evaluated with
 * the element as the root ("" = the element itself, "/a/0" = get("a") then element 0), i.e. what sjmi_select_batch_device gives
 * document k for the pointer base + "/" + j + p, in the same (type, value) encoding, container values' tape indexes included. */
typedef struct sjmi_explode_plan sjmi_explode_plan;
int sjmi_explode_plan_compile(const uint8_t* base_pointer, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                              uint64_t n_paths, sjmi_explode_plan** out);
void sjmi_explode_plan_destroy(sjmi_explode_plan* plan);
/* A MEMBERS plan: JsonValue.objectIterator (JsonValue.java:170-194) over ONE object per document -- Arrow's map<utf8, struct>
 * shape, for objects whose keys differ from document to document.  The same plan type, destroyed by
 * sjmi_explode_plan_destroy, with the rules, limits and SJMI_ERR_ARG cases of sjmi_explode_plan_compile, except that n_paths is
 * at most SJMI_EXPLODE_MEMBERS_MAX_PATHS: the key takes the 64th cell of a row.
 * With such a plan sjmi_explode_batch_device gives document k rows iff its base value is an OBJECT ('{'): the members of the
 * iterator chain -- from idx + 1, the key one word at pos, the value at pos + 1, the next member at Tape.computeNextIndex of the
 * value, up to getMatchingBraceIndex - 1; never the 24-bit scope count --, the walk made to move forward and to stay inside the
 * document whatever the words hold.  A base that is an array, a scalar, a string or MISSING gives 0 rows, and so does a failed
 * document.  The members of nested objects are not rows.  Row row_offsets[k] + j is member j in tape order; DUPLICATE KEYS ARE
 * SEPARATE ROWS, as the iterator yields them (unlike get()'s first-match rule), and the empty key "" is a key of length 0.
 * The call writes n_paths + 1 columns strided by row_capacity: columns 0 .. n_paths - 1 are the element pointers evaluated with
 * the member's VALUE as the root (the encoding unchanged, container cells carry tape indexes inside the document), column
 * n_paths is the KEY: type '"', value (length << 32) | (record offset + 4) -- exactly a string cell, which
 * sjmi_string_column_device, sjmi_dictionary_column_device and STRING filter terms take unchanged.  Everything else (the
 * offsets always complete, the sizing call, the capacity rule, the plan slot, the scratch, the stream rules, the known limit) is
 * as stated below.  An array plan behaves on every input as it did before members plans existed. */
#define SJMI_EXPLODE_MEMBERS_MAX_PATHS (SJMI_SELECT_MAX_PATHS - 1u)
int sjmi_explode_members_plan_compile(const uint8_t* base_pointer, uint64_t base_len, const uint8_t* pointers,
                                      const uint64_t* pointer_offsets, uint64_t n_paths, sjmi_explode_plan** out);
/* Inputs as sjmi_select_batch_device.  d_row_offsets (uint64[n_docs + 1]) is the exclusive prefix sum of the documents' row
 * counts and is ALWAYS complete: d_row_offsets[n_docs] is the total number of rows, whatever row_capacity is.  Columns are
 * strided by row_capacity: d_types[p * row_capacity + r] (uint8), d_values[p * row_capacity + r] (uint64).  Rows r >=
 * row_capacity are not written and nothing past the n_paths * row_capacity elements is touched: a caller sees the overflow
 * from d_row_offsets[n_docs].  row_capacity == 0 with NULL d_types / d_values is legal and writes the offsets only, so that a
 * caller can size its columns.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but
 * the kernels -- except that the first call with a plan copies it to the context's device memory (one blocking upload; the
 * context keeps the explode plan in a slot of its own, so alternating select and explode calls do not evict each other's
 * plan), and that a call with more documents than any explode call before it on this context grows the context's
 * per-document scratch (row counts, base tape indexes, chunk sums), which waits for the device and may block.
 * That scratch is one per context: explode calls on ONE context must be ordered with respect to each other (the same stream, or
 * streams the caller orders with events); two of them running at the same time would share it.  Use a context per stream otherwise.
 * A document whose rows begin below row_capacity and run past it is walked only as far as its rows are stored.
 * One group of sixteen lanes walks all elements of its document: one very wide array among small ones serialises (4.9). */
int sjmi_explode_batch_device(sjmi_ctx* ctx, const sjmi_explode_plan* plan, const void* d_tape, const void* d_tape_offsets,
                              const void* d_doc_errors, const void* d_string_buffer, uint64_t n_docs, void* d_row_offsets,
                              uint64_t row_capacity, void* d_types, void* d_values, void* stream);

/* ---- one string column as Arrow offsets, validity and bytes, gathered on the device -------------------------------------
 * A string cell of a select or explode column is (length << 32) | offset into the batch's string buffer, which holds every
 * string of every document with record headers between them.  This call turns ONE such column into Arrow's large_utf8 shape:
 * int64 offsets, an LSB-first validity bitmap and the strings' bytes back to back (csrc/strcol.hip).  It reads
 * a finished (types, values) column and the string buffer and nothing else: no tape, no plan.
 *
 * INPUT COLUMN.  d_types (uint8, ANY alignment: it is loaded as bytes) and d_values (uint64, 8-byte aligned) are one column of
 * n_rows cells in the encoding of sjmi_select_batch_device.  A select column is d_types + p * n_docs (and d_values + p *
 * n_docs) with n_rows = n_docs; an explode column is d_types + p * row_capacity with n_rows = min(total rows, row_capacity).
 * VALIDITY.  Row r is VALID iff types[r] == '"'; its length is values[r] >> 32 and its bytes are d_string_buffer[values[r] &
 * 0xFFFFFFFF ...].  Every other row -- MISSING, 'n', numbers, booleans, containers -- is NULL with length 0, and the value word
 * of a NULL row is never used as an offset or a length (nor read at all), whatever it holds.  n_valid counts the VALID rows;
 * n_other counts the rows that are neither VALID nor MISSING nor 'n': a schema mismatch the caller sees without a second pass.
 * OFFSETS.  d_offsets is int64[n_rows + 1], the exclusive prefix sum of the lengths.  It is ALWAYS complete, whatever
 * byte_capacity is, and d_offsets[n_rows] == total_bytes.
 * VALIDITY BITMAP.  d_validity is uint64[ceil(n_rows / 64)] (8-byte aligned): bit r & 63 of word r >> 6 is set iff row r is
 * VALID -- Arrow's LSB-first bitmap on a little-endian host.  Bits at or above n_rows in the last word are 0.  d_validity may
 * be NULL: nothing is written for it then.
 * BYTES.  Byte i of the column, offsets[r] <= i < offsets[r + 1], is byte i - offsets[r] of row r.  It is written to d_bytes[i]
 * iff i < byte_capacity; nothing at or behind d_bytes + byte_capacity is touched.  d_bytes may have any alignment.
 * byte_capacity == 0 with d_bytes == NULL is the SIZING call: offsets, validity and the result record only, the copy kernel is
 * not launched.  total_bytes > byte_capacity sets SJMI_STRCOL_OVERFLOW (the sizing call of a column with bytes sets it too).
 * The bytes are what the string pass wrote: they are not validated again.
 * THE EMPTY COLUMN.  n_rows == 0 is legal: d_offsets[0] = 0, a zero result record, and no kernel is launched with an empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_offsets or d_result; NULL d_types or d_values with n_rows > 0; NULL d_bytes with
 * byte_capacity > 0; d_values, d_offsets, d_validity or d_result not 8-byte aligned; n_rows >= 2^40.
 * STREAM AND SCRATCH.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but four plain
 * kernels that the stream orders (chunk sums per 1024 rows, their scan by one workgroup, the offsets, the copy) -- except that
 * a call with more rows than any string-column call before it on this context grows the context's chunk-sum scratch, which
 * waits for the device and may block.  That scratch is a slot of its own (not explode's) and one per context: string-column
 * calls on ONE context must be ordered with respect to each other (the same stream, or streams the caller orders with events).
 * KNOWN LIMIT.  A wave copies the bytes of its 64 consecutive rows, 64 bytes per trip: one very long string among short ones is
 * copied by one wave. */
#define SJMI_STRCOL_OVERFLOW 1u            /* total_bytes > byte_capacity */
typedef struct sjmi_strcol_result {
    uint64_t total_bytes, n_valid, n_other;
    uint32_t flags, reserved;
} sjmi_strcol_result;
int sjmi_string_column_device(sjmi_ctx* ctx, const void* d_types, const void* d_values, uint64_t n_rows,
                              const void* d_string_buffer, void* d_offsets, void* d_validity,
                              void* d_bytes, uint64_t byte_capacity, void* d_result, void* stream);

/* ---- filtering the rows of typed columns on the device and compacting the kept rows ----------------------------------------
 * Which rows a caller wants, decided between select / explode and the string gather (csrc/filter.hip).  The call
 * reads finished (types, values) columns and the string buffer and nothing else: no tape, no select plan.
 *
 * A FILTER PLAN is a conjunction of at most SJMI_FILTER_MAX_TERMS terms, compiled on the host with no device and no context.  A
 * term looks at ONE column: the cell of column c, row r is types[c * col_stride + r] / values[c * col_stride + r] in the encoding
 * of sjmi_select_batch_device.  A term is TRUE only in the cases below; in particular every comparison is FALSE on a cell that
 * is not of the comparable type -- NE on a MISSING or null cell included, as SQL treats a comparison with NULL.
 *   TYPE_EQ / TYPE_NE      the type byte equals / differs from the operand (0 = MISSING, so TYPE_NE 0 is "present"; 't' 'f' 'n'
 *                          are tested this way)
 *   LONG_* / DOUBLE_*      the cell is 'l' or 'd', and the comparison (EQ NE LT LE GT GE) of the cell with the constant holds for
 *                          the two numbers AS REAL NUMBERS, exactly: int64 with int64 as integers, double with double as IEEE
 *                          doubles (-0.0 == 0.0), int64 with double without rounding either side (9007199254740993 is GT
 *                          9007199254740992.0, not EQ).  +-infinity is a legal constant and a legal cell; a NaN constant does not
 *                          compile, and NaN cells (the parser makes none) satisfy no comparison.
 *   STRING_EQ / _NE / _PREFIX   the cell is '"' with len = value >> 32 and its bytes at d_string_buffer + (value & 0xFFFFFFFF).
 *                          EQ: len == clen and the bytes are equal, byte for byte on the unescaped bytes (Arrays.compare(...) == 0,
 *                          JsonValue.java:102); NE: a string that is not EQ; PREFIX: len >= clen and the first clen bytes are
 *                          equal.  An empty constant is legal.
 * A row is KEPT iff every term is TRUE; a plan without terms keeps every row.
 * sjmi_filter_plan_compile: the string constants are bytes[offset, offset + length) of `bytes` (n_bytes of them; NULL with 0).
 * SJMI_ERR_ARG: more than SJMI_FILTER_MAX_TERMS terms, an unknown op, a type operand above 255, a NaN, a string constant outside
 * `bytes` or longer than SJMI_FILTER_MAX_STRING, n_bytes above SJMI_FILTER_MAX_CONST_BYTES, NULL terms / bytes with a count. */
#define SJMI_FILTER_MAX_TERMS 16u
#define SJMI_FILTER_MAX_CONST_BYTES 1024u   /* all string constants of a plan together (n_bytes) */
#define SJMI_FILTER_MAX_STRING 256u         /* one string constant */
#define SJMI_F_TYPE_EQ 0x00u
#define SJMI_F_TYPE_NE 0x01u
#define SJMI_F_LONG_EQ 0x10u
#define SJMI_F_LONG_NE 0x11u
#define SJMI_F_LONG_LT 0x12u
#define SJMI_F_LONG_LE 0x13u
#define SJMI_F_LONG_GT 0x14u
#define SJMI_F_LONG_GE 0x15u
#define SJMI_F_DOUBLE_EQ 0x20u
#define SJMI_F_DOUBLE_NE 0x21u
#define SJMI_F_DOUBLE_LT 0x22u
#define SJMI_F_DOUBLE_LE 0x23u
#define SJMI_F_DOUBLE_GT 0x24u
#define SJMI_F_DOUBLE_GE 0x25u
#define SJMI_F_STRING_EQ 0x30u
#define SJMI_F_STRING_NE 0x31u
#define SJMI_F_STRING_PREFIX 0x36u
typedef struct sjmi_filter_term {
    uint32_t column;    /* which of the call's n_cols columns the term looks at */
    uint32_t op;        /* SJMI_F_<KIND>_<CMP> */
    uint64_t operand;   /* TYPE: the type byte; LONG: the int64; DOUBLE: the IEEE bits; STRING: (length << 32) | offset into `bytes` */
} sjmi_filter_term;
typedef struct sjmi_filter_plan sjmi_filter_plan;
int sjmi_filter_plan_compile(const sjmi_filter_term* terms, uint64_t n_terms, const uint8_t* bytes, uint64_t n_bytes, sjmi_filter_plan** out);
void sjmi_filter_plan_destroy(sjmi_filter_plan* plan);
/* MEMORY.  A cell's value word is used as an offset or a length only behind the test type == '"', and as a number only behind
 * 'l' / 'd'.  Of a string cell only bytes inside [offset, offset + len) are read, and the length decides before a byte is touched.
 * OUTPUTS, each optional except d_result:
 *   d_keep        uint64[ceil(n_rows / 64)], LSB first: bit r is set iff row r is kept; bits at or above n_rows are 0
 *   d_rows        int64[out_capacity]: d_rows[j] = the index of the j-th kept row, ascending -- the selection vector, with which a
 *                 caller gathers anything else (a document id, through explode's row offsets, included)
 *   d_out_types / d_out_values   all n_cols columns compacted: for j < min(n_kept, out_capacity), out_types[c * out_capacity + j] =
 *                 types[c * col_stride + rows[j]] and the values likewise, word for word -- a (types, values) column set again,
 *                 of which sjmi_string_column_device takes a row unchanged
 *   d_result      n_kept is ALWAYS complete, whatever out_capacity is; n_kept > out_capacity sets SJMI_FILTER_OVERFLOW
 * Entries j >= out_capacity are not written, nor entries between n_kept and out_capacity, and nothing behind out_capacity entries
 * (times n_cols for the columns) is touched.  d_rows, d_out_types and d_out_values come together or not at all; out_capacity == 0
 * with all three NULL is the SIZING call (the emit kernel is not launched).  Outputs must not overlap inputs.
 * n_rows == 0 is legal: a zero result record, and no kernel is launched with an empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: a term's column >= n_cols; col_stride < n_rows; NULL d_result; NULL d_types or d_values with n_rows >
 * 0; NULL d_string_buffer when the plan has a STRING term and n_rows > 0; NULL d_rows, d_out_types or d_out_values with
 * out_capacity > 0; d_values, d_keep, d_rows, d_out_values or d_result not 8-byte aligned (d_types and d_out_types take any
 * alignment); n_rows >= 2^40.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but three plain
 * kernels that the stream orders (the terms per 1024 rows, the scan of the chunk counts by one workgroup, the emit).  The plan
 * is handed to the kernels by value as a launch argument: the call uploads nothing and the context holds no filter plan.  The
 * only state is a scratch slot of its own (the chunk counts, and the keep words of a call without d_keep), which grows on demand
 * with a device synchronisation; it is one per context, so filter calls on ONE context must be ordered with respect to each other. */
#define SJMI_FILTER_OVERFLOW 1u   /* n_kept > out_capacity */
typedef struct sjmi_filter_result {
    uint64_t n_kept;
    uint32_t flags, reserved;
} sjmi_filter_result;
int sjmi_filter_columns_device(sjmi_ctx* ctx, const sjmi_filter_plan* plan, const void* d_types, const void* d_values, uint64_t n_cols,
                               uint64_t col_stride, uint64_t n_rows, const void* d_string_buffer, void* d_keep, void* d_rows,
                               uint64_t out_capacity, void* d_out_types, void* d_out_values, void* d_result, void* stream);

/* ---- typed columns as Arrow int64, float64 and bool arrays, made on the device ------------------------------------------------
 * The end of the device-side pipeline for everything that is not a string: one call turns a set of finished (types, values)
 * columns into Arrow arrays -- a data buffer and an LSB-first validity bitmap per FIELD -- with a record of counts per field
 * (csrc/arrowcol.hip).  It reads the columns and nothing else: no tape, no string buffer, no plan object.
 *
 * INPUT.  The column set of sjmi_filter_columns_device: the cell of column c, row r is types[c * col_stride + r] / values[c *
 * col_stride + r] in the encoding of sjmi_select_batch_device; d_types is loaded as bytes and takes ANY alignment.  `fields` is a
 * HOST array of n_fields (1 .. SJMI_ARROW_MAX_FIELDS) entries: field f makes one output array of kind `kind` from column
 * `column`.  Two fields may name the same column (the same path once as INT64 and once as FLOAT64).
 * LIVE ROWS.  live = n_rows when d_row_count is NULL, else min(n_rows, *(const uint64_t*)d_row_count), read ON THE DEVICE by the
 * kernels: pointing d_row_count at sjmi_filter_result.n_kept, or at d_row_offsets + n_docs of an explode, chains the calls
 * without a host synchronisation.  n_rows only sizes the grid and the buffers.  Rows at or above live are not read, not counted
 * and not written.
 * CELLS.  VALID = the validity bit is 1.  A NULL row's data slot is written as 0.  A cell's value word is used only behind the
 * type tests named here; whatever it holds in other cells never shows in an output.
 *   INT64     'l' -> the int64.  With SJMI_ARROW_F_INTEGRAL_DOUBLES a 'd' cell converts too when its double is finite, has no
 *             fraction and lies in [-2^63, 2^63) -- exactly: -0.0 -> 0, -9223372036854775808.0 is VALID, 9223372036854775808.0
 *             is not.  Every other 'd' cell is NULL and counted in n_other.
 *   FLOAT64   'd' -> its IEEE bits unchanged (NaN and the infinities pass through); 'l' -> the int64 converted round to nearest,
 *             ties to even.  n_inexact counts the 'l' cells whose conversion is not exact (2^53 + 1 -> 2^53 is inexact, 2^53
 *             is exact, INT64_MIN is exact, INT64_MAX -> 2^63 is inexact).
 *   BOOL      't' / 'f' -> VALID; the data is a BITMAP in the first ceil(live / 64) words of the field's data row, LSB first, the
 *             bit set iff 't'.  NULL rows' bits and the bits at or above live in the last word are 0.  The value word of a
 *             boolean cell is not read: the type byte says it.
 *   NULL      in every kind: MISSING (0), 'n' and every type not named above.  n_other counts the NULL rows that are neither
 *             MISSING nor 'n' -- the schema mismatch, as in sjmi_strcol_result.
 * OUTPUTS.
 *   d_data      uint64[n_fields * data_stride]: field f, row r at f * data_stride + r (BOOL: word w of the bitmap at f *
 *               data_stride + w).  NULL together with data_stride == 0 is the COUNTING call: validity and records only.
 *   d_validity  uint64[n_fields * validity_stride]: field f owns the words f * validity_stride ...; bit r & 63 of word r >> 6 is
 *               set iff row r is VALID, bits at or above live in the last written word are 0 (the bitmap of
 *               sjmi_string_column_device).  May be NULL: nothing is written for it, the records alone give the null counts.
 *   d_results   sjmi_arrow_field_result[n_fields], ALWAYS complete.  n_rows of a record is live: the consumer learns the row
 *               count with the same readback.
 * Of a field exactly the data words [0, live) -- BOOL: [0, ceil(live / 64)) -- and the validity words [0, ceil(live / 64)) are
 * written; nothing else in the two blocks is touched, and nothing behind them.  Outputs must not overlap inputs.
 * THE EMPTY CASES.  n_rows == 0 or live == 0 is legal: records of zeros, no data or validity word written, and no kernel is
 * launched with an empty grid.  n_fields == 0 is SJMI_ERR_ARG.
 * ARGUMENTS.  SJMI_ERR_ARG: n_fields 0 or above SJMI_ARROW_MAX_FIELDS; a field with an unknown kind, a flag that is not defined
 * for its kind, reserved != 0 or column >= n_cols; col_stride < n_rows; data_stride < n_rows with d_data, or a data_stride
 * without one; validity_stride < ceil(n_rows / 64) with d_validity; NULL d_results; NULL d_types or d_values with n_rows > 0;
 * d_values, d_row_count, d_data, d_validity or d_results not 8-byte aligned; n_rows >= 2^40.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but two plain
 * kernels that the stream orders (the conversion per 1024 rows and field, the sum of the chunk counts per field).  The fields are
 * validated and handed to the kernels by value as a launch argument: the call uploads nothing and the context holds no schema.
 * The only state is a scratch slot of its own (one packed count word per field and 1024-row chunk), which grows on demand with
 * a device synchronisation; it is one per context, so arrow-column calls on ONE context must be ordered with respect to each
 * other. */
#define SJMI_ARROW_MAX_FIELDS 64u          /* = SJMI_SELECT_MAX_PATHS */
#define SJMI_ARROW_INT64   1u
#define SJMI_ARROW_FLOAT64 2u
#define SJMI_ARROW_BOOL    3u
#define SJMI_ARROW_F_INTEGRAL_DOUBLES 1u   /* INT64 fields only */
typedef struct sjmi_arrow_field {
    uint32_t column;    /* which of the call's n_cols columns the field is made of */
    uint32_t kind;      /* SJMI_ARROW_<KIND> */
    uint32_t flags;     /* SJMI_ARROW_F_* */
    uint32_t reserved;  /* 0 */
} sjmi_arrow_field;
typedef struct sjmi_arrow_field_result {
    uint64_t n_rows, n_valid, n_other, n_inexact;
} sjmi_arrow_field_result;
int sjmi_arrow_columns_device(sjmi_ctx* ctx, const sjmi_arrow_field* fields, uint64_t n_fields, const void* d_types, const void* d_values,
                              uint64_t n_cols, uint64_t col_stride, uint64_t n_rows, const void* d_row_count, void* d_data,
                              uint64_t data_stride, void* d_validity, uint64_t validity_stride, void* d_results, void* stream);

/* ---- RFC 3339 string columns as Arrow timestamp arrays, made on the device ----------------------------------------------------
 * JSON has no time type: a timestamp arrives as a string ("created_at":"2015-01-01T15:00:00Z").  This call parses the string
 * cells of finished (types, values) columns into Arrow timestamp arrays -- an int64 per row at the field's unit, counted from
 * 1970-01-01T00:00:00Z, an LSB-first validity bitmap and a record of counts per FIELD (csrc/timecol.hip).  It
 * reads the columns and the string buffer and nothing else: no tape, no plan object.
 * EPOCH NUMBERS need no call of their own: a column of 'l' cells is served by sjmi_arrow_columns_device's INT64, and an int64
 * array IS a timestamp array, by reinterpretation at the caller's unit (Arrow's timestamp is an int64 with a unit and a zone
 * in the type).  'l' and 'd' cells under a time field are therefore NULL and counted in n_other.
 *
 * INPUT, LIVE ROWS.  As sjmi_arrow_columns_device: the column set of sjmi_filter_columns_device, d_types loaded as bytes at ANY
 * alignment, `fields` a HOST array of n_fields (1 .. SJMI_TIME_MAX_FIELDS) entries of which two may name one column (the same
 * path at two units); live = n_rows when d_row_count is NULL, else min(n_rows, *(const uint64_t*)d_row_count) read ON THE
 * DEVICE, so that a filter's n_kept or an explode's last row offset chains the calls without a host synchronisation.  Rows at
 * or above live are not read, not counted and not written.  d_string_buffer is the buffer the string cells point into.
 * CELLS.  A cell's value word is read only behind type == '"'; the bytes of a string only behind that AND the test of its
 * length.  A '"' cell is the unescaped bytes [offset, offset + len) of d_string_buffer, value = (len << 32) | offset, which
 * must match the WHOLE of
 *       YYYY-MM-DD sep hh:mm:ss [ '.' 1 to 9 digits ] zone
 *   sep: 'T', 't' or ONE space.  zone: 'Z', 'z', or +hh:mm / -hh:mm.  Every digit is an ASCII digit.  Year 0000..9999, month
 *   01..12, a day that the month has in the proleptic Gregorian calendar (0000, 2000, 2024 are leap years; 1900, 2023 are not),
 *   hour 00..23, minute and second 00..59 (":60", a leap second, is malformed), offset hour 00..23 and offset minute 00..59;
 *   -00:00 is UTC.  Nothing may precede or follow, so len is 20..35.  With SJMI_TIME_F_NAIVE_UTC the zone may be absent -- the
 *   time is then taken as UTC -- and len is 19..35.  A string of any other length is malformed WITHOUT A BYTE OF IT BEING READ;
 *   date-only strings are malformed.
 *   VALUE  (days_from_civil(Y, M, D) * 86400 + hh * 3600 + mm * 60 + ss - offset_seconds) * 10^k + fraction, k = 0, 3, 6, 9 by
 *          unit, the fraction scaled to the unit with its surplus digits DROPPED -- a floor, since the fraction is positive:
 *          1969-12-31T23:59:59.5Z at SECOND is -1.  A VALID cell with a non-zero dropped digit counts in n_inexact.
 *   RANGE  a value that is not an int64 makes the cell NULL and counts in n_range; only NANO can do this:
 *          2262-04-11T23:47:16.854775807Z is INT64_MAX and VALID, 1677-09-21T00:12:43.145224192Z is INT64_MIN and VALID, one
 *          nanosecond further out is a range error.  Decided in integers on the seconds; nothing overflows on the way.
 *   NULL   a string that fails the grammar: counted in n_malformed.  MISSING (0) and 'n': counted nowhere.  Every other type --
 *          'l' and 'd' included --: counted in n_other, the schema mismatch as in sjmi_arrow_field_result.
 * OUTPUTS.  As sjmi_arrow_columns_device, every field an int64 one:
 *   d_data      uint64[n_fields * data_stride]: field f, row r at f * data_stride + r, a NULL row's word written as 0.  NULL
 *               together with data_stride == 0 is the COUNTING call: validity and records only.
 *   d_validity  uint64[n_fields * validity_stride], LSB first: bit r & 63 of word f * validity_stride + (r >> 6) is set iff row
 *               r of field f is VALID; bits at or above live in the last written word are 0.  May be NULL.
 *   d_results   sjmi_time_field_result[n_fields], ALWAYS complete, n_rows = live.
 * Of a field exactly the data words [0, live) and the validity words [0, ceil(live / 64)) are written; nothing else in the two
 * blocks is touched, and nothing behind them.  Outputs must not overlap inputs.
 * THE EMPTY CASES.  n_rows == 0 or live == 0 is legal: records of zeros, no data or validity word written, and no kernel is
 * launched with an empty grid.  n_fields == 0 is SJMI_ERR_ARG.
 * ARGUMENTS.  SJMI_ERR_ARG: n_fields 0 or above SJMI_TIME_MAX_FIELDS; a field with a unit above SJMI_TIME_NANO, a flag other
 * than SJMI_TIME_F_NAIVE_UTC, reserved != 0 or column >= n_cols; col_stride < n_rows; data_stride < n_rows with d_data, or a
 * data_stride without one; validity_stride < ceil(n_rows / 64) with d_validity; NULL d_results; NULL d_types, d_values or
 * d_string_buffer with n_rows > 0; d_values, d_row_count, d_data, d_validity or d_results not 8-byte aligned; n_rows >= 2^40.
 * MEMORY.  The string bytes are fetched as the naturally aligned 8-byte words that hold at least one byte of the string: such
 * a word lies in the same page, and so in the same allocation, as that byte, and what else it carries reaches no output.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but two plain
 * kernels that the stream orders (the parse per 256 rows and field, the sum of the chunk counts per field).  The fields are
 * validated and handed to the kernels by value as a launch argument: the call uploads nothing and the context holds no schema.
 * The only state is a scratch slot of its own (one packed count word per field and 256-row chunk), which grows on demand with
 * a device synchronisation; it is one per context, so time-column calls on ONE context must be ordered with respect to each
 * other.
 * NOT HERE.  date32 and time-of-day kinds, named zones, leap seconds, other formats. */
#define SJMI_TIME_MAX_FIELDS 64u           /* = SJMI_SELECT_MAX_PATHS */
#define SJMI_TIME_SECOND 0u
#define SJMI_TIME_MILLI  1u
#define SJMI_TIME_MICRO  2u
#define SJMI_TIME_NANO   3u
#define SJMI_TIME_F_NAIVE_UTC 1u           /* a string without an offset is taken as UTC */
typedef struct sjmi_time_field {
    uint32_t column;    /* which of the call's n_cols columns the field is made of */
    uint32_t unit;      /* SJMI_TIME_<UNIT> */
    uint32_t flags;     /* SJMI_TIME_F_* */
    uint32_t reserved;  /* 0 */
} sjmi_time_field;
typedef struct sjmi_time_field_result {
    uint64_t n_rows, n_valid, n_other, n_malformed, n_range, n_inexact;
} sjmi_time_field_result;
int sjmi_time_columns_device(sjmi_ctx* ctx, const sjmi_time_field* fields, uint64_t n_fields, const void* d_types, const void* d_values,
                             uint64_t n_cols, uint64_t col_stride, uint64_t n_rows, const void* d_row_count, const void* d_string_buffer,
                             void* d_data, uint64_t data_stride, void* d_validity, uint64_t validity_stride, void* d_results, void* stream);

/* ---- one string column as an Arrow dictionary array, encoded on the device -----------------------------------------------
 * Most string columns of real JSON are categorical.  This call turns ONE (types, values) column into Arrow's dictionary shape:
 * an int32 index per row, an LSB-first validity bitmap, and the dictionary -- one entry per distinct value -- as int64 offsets
 * and bytes (csrc/dictcol.hip).  It reads a finished column and the string buffer and nothing else.
 *
 * INPUT COLUMN.  d_types / d_values / d_string_buffer exactly as sjmi_string_column_device takes them: d_types is loaded as
 * bytes at any alignment, a value word is read only behind type == '"', and of a string only the naturally aligned 8-byte words
 * that hold at least one of its bytes are read (each lies in the page, and so in the allocation, of such a byte).
 * LIVE ROWS, as in sjmi_arrow_columns_device.  d_row_count == NULL: live = n_rows.  Else it points to a uint64 in DEVICE memory
 * that the kernels read: live = min(n_rows, *d_row_count) -- a filter's n_kept, an explode's last row offset.  Rows at or above
 * `live` are not read, counted or written.
 * MEANING.  Row r is VALID iff types[r] == '"'.  Two VALID rows are EQUAL iff they have the same length and the same bytes; the
 * empty string is a value of its own.  The dictionary holds one entry per distinct value IN THE ORDER OF FIRST OCCURRENCE:
 * entry j is the value whose first VALID row is the j-th smallest among the first rows -- the order of pyarrow's
 * dictionary_encode() and of pandas.factorize.  The output is therefore a function of the input alone, whatever the scheduling.
 * OUTPUTS.  d_indices: int32[n_rows], 4-byte aligned: the entry number of a VALID row, 0 for a NULL row; exactly [0, live) is
 * written.  d_validity: the bitmap of sjmi_string_column_device, may be NULL; words [0, ceil(live / 64)) are written, bits at or
 * above `live` are 0.  d_dict_rows: int64[dict_capacity], may be NULL: the row of each entry's first occurrence, ascending.
 * d_dict_offsets: int64[dict_capacity + 1], the exclusive scan of the entries' lengths; entries [0, n_distinct] are written.
 * d_dict_bytes (any alignment): the entries' bytes back to back, below dict_byte_capacity.  dict_byte_capacity == 0 with NULL
 * d_dict_bytes is the SIZING call: indices, offsets, rows and the record are complete, the copy is not launched.
 * d_result: sjmi_dict_result; n_rows = live, n_other as in sjmi_strcol_result.  SJMI_DICT_BYTES_OVERFLOW is set iff dict_bytes >
 * dict_byte_capacity (the sizing call of a dictionary with bytes sets it), SJMI_DICT_OVERFLOW iff there are more distinct
 * values than dict_capacity.
 * UNDER SJMI_DICT_OVERFLOW n_rows, n_valid, n_other, the validity bitmap and the flag are still exact; n_distinct is some number
 * above dict_capacity; the indices and the dictionary buffers hold unspecified values inside their stated extents (d_indices
 * [0, live), d_dict_rows [0, dict_capacity), d_dict_offsets[0]), nothing outside them is written, no dictionary byte is copied
 * (dict_bytes = 0), and the call completes.  dict_capacity == 0 is legal: an overflow unless no row is VALID.
 * THE EMPTY CASES.  n_rows == 0, or live == 0, is legal: d_dict_offsets[0] = 0, a zero record; no kernel is launched with an
 * empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: dict_capacity > SJMI_DICT_MAX_ENTRIES; NULL d_indices, d_dict_offsets or d_result; NULL d_types,
 * d_values or d_string_buffer with n_rows > 0; NULL d_dict_bytes with dict_byte_capacity > 0; d_values, d_row_count,
 * d_validity, d_dict_rows, d_dict_offsets or d_result not 8-byte aligned, d_indices not 4-byte aligned; n_rows >= 2^40.
 * STREAM AND SCRATCH.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, nothing queued but plain
 * kernels that the stream orders: one that clears the hash table (no memset node), the insert -- the only kernel with atomics:
 * agent-scope relaxed load / compare-exchange / fetch-min on the table's words; nothing spins or waits for another workgroup,
 * and a probe is bounded by the table's slots --, the count of first rows per 1024 rows, their scan by one workgroup (the
 * record), the ranks, the indices, and the four string-gather kernels over the dictionary (the copy only with a byte capacity).
 * With n_rows == 0 only the two one-workgroup kernels are queued.  The context owns a scratch slot of its own for this call: the
 * table (32 bytes per entry of dict_capacity, rounded up to a power of two), 4 bytes per row, the chunk counts and the compacted
 * dictionary column.  A call that needs more of it than any before it on this context grows it, which waits for the device and
 * may block.  It is one per context: dictionary calls on ONE context must be ordered with respect to each other.
 * KNOWN LIMITS.  One lane hashes and compares one row's string, eight bytes per trip: very long strings are slow.  A dictionary's
 * bytes are copied by the string gather's kernel, with its known limit. */
#define SJMI_DICT_MAX_ENTRIES (1u << 20)
#define SJMI_DICT_OVERFLOW 1u              /* more distinct values than dict_capacity */
#define SJMI_DICT_BYTES_OVERFLOW 2u        /* dict_bytes > dict_byte_capacity */
typedef struct sjmi_dict_result {
    uint64_t n_rows, n_valid, n_other, n_distinct, dict_bytes;
    uint32_t flags, reserved;
} sjmi_dict_result;
int sjmi_dictionary_column_device(sjmi_ctx* ctx, const void* d_types, const void* d_values, uint64_t n_rows, const void* d_row_count,
                                  const void* d_string_buffer, void* d_indices, void* d_validity, uint64_t dict_capacity, void* d_dict_rows,
                                  void* d_dict_offsets, void* d_dict_bytes, uint64_t dict_byte_capacity, void* d_result, void* stream);

/* ---- the key census: rows per dictionary entry and value type, counted on the device ----------------------------------------
 * "Which keys are in here, and what types do they hold?"  A members explode gives a key column and a column of value types,
 * sjmi_dictionary_column_device turns the keys into indices, and this call counts the rows per (index, type class): a group-by
 * of counts, nothing else -- no sums, minima or maxima (csrc/census.hip, csrc/sj_census.h).  Those are
 * sjmi_group_stats_device's, below.
 *
 * INPUTS.  d_indices: int32[n_rows], 4-byte aligned -- the indices of sjmi_dictionary_column_device.  d_validity: its LSB-first
 * bitmap (8-byte aligned words); NULL: every live row counts.  d_types: ONE uint8 column with the same rows, loaded as bytes at
 * any alignment -- normally the "" element pointer of a members explode, but any types column is legal.  LIVE ROWS as in
 * sjmi_arrow_columns_device: d_row_count == NULL: live = n_rows; else live = min(n_rows, *d_row_count), a uint64 in DEVICE
 * memory (8-byte aligned) that the kernels read.  Rows at or above `live` are not read.
 * CLASSES.  0 'l', 1 'd', 2 '"', 3 't' or 'f', 4 'n', 5 '[', 6 '{', 7 every other type byte (MISSING included).
 * MEANING.  A live row r whose validity bit is set and whose index lies in [0, n_keys) adds 1 to d_counts[indices[r] *
 * SJMI_CENSUS_CLASSES + class(types[r])]; d_counts is uint64[n_keys * SJMI_CENSUS_CLASSES], 8-byte aligned.  A valid live row
 * whose index lies outside [0, n_keys) -- the unspecified indices under SJMI_DICT_OVERFLOW: negatives, INT32_MIN, INT32_MAX -- is
 * counted in n_out_of_range and touches nothing else.  The record: n_rows = live, n_counted = the rows that were added,
 * n_out_of_range, flags = 0; always complete.  Exactly d_counts[0, n_keys * 8) is written, every word, zeros included; nothing
 * before or behind it is touched.  The outputs are exact integer sums: a function of the input alone.
 * THE EMPTY CASES.  n_rows == 0, live == 0 and n_keys == 0 are legal: the counts are zeroed, the record is zero but for n_rows
 * and, with n_keys == 0, n_out_of_range; no kernel is launched with an empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_result; NULL d_indices or d_types with n_rows > 0; NULL d_counts with n_keys > 0; n_keys >
 * SJMI_DICT_MAX_ENTRIES; d_indices not 4-byte aligned; d_validity, d_row_count, d_counts or d_result not 8-byte aligned;
 * n_rows >= 2^40.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node: a kernel that
 * clears the counts and the record, then ONE kernel over the rows, which the stream orders.  The context keeps NO state for
 * this call -- no scratch, nothing to grow, nothing that two calls could share: census calls on one context need no ordering
 * among themselves beyond what their buffers ask.
 * KERNELS.  n_keys <= SJMI_CENSUS_LDS_KEYS: a workgroup takes chunks of 1024 rows in a grid stride, counts into 32-bit bins in
 * LDS with LDS atomics (it takes fewer than 2^32 rows, so a bin cannot overflow) and adds its NON-ZERO bins to d_counts once,
 * with agent-scope relaxed 64-bit atomic adds.  Larger n_keys: such adds go straight to d_counts, the rows of a wave that fall
 * into the same bin merged into one add first.  The record's counts are summed the same way.  Nothing spins or waits for another workgroup; the counts are read across the kernel boundary
 * only.
 * KNOWN LIMIT.  Above SJMI_CENSUS_LDS_KEYS equal bins are merged inside a wave only: a column whose rows all fall into one bin
 * still sends one add per 64 rows to one address, and is slower there than below the threshold (4.16). */
#define SJMI_CENSUS_CLASSES 8u
#define SJMI_CENSUS_LDS_KEYS 1024u         /* 8192 32-bit bins = 32 KiB of LDS per workgroup */
typedef struct sjmi_census_result {
    uint64_t n_rows, n_counted, n_out_of_range;
    uint32_t flags, reserved;
} sjmi_census_result;
int sjmi_key_census_device(sjmi_ctx* ctx, const void* d_indices, const void* d_validity, const void* d_types, uint64_t n_rows,
                           const void* d_row_count, uint64_t n_keys, void* d_counts, void* d_result, void* stream);

/* ---- group statistics per dictionary key: count, sum, minimum and maximum, on the device ----------------------------------
 * "Total and largest /payload/size per /type": sjmi_dictionary_column_device turns the key column into indices, and this call
 * aggregates ONE (type, value) column with the same rows per index (csrc/groupstats.hip, csrc/sj_groupstats.h).
 *
 * INPUTS.  d_indices, d_validity, n_rows, d_row_count, n_keys exactly as sjmi_key_census_device takes them: int32 indices (4-byte
 * aligned), the LSB-first bitmap or NULL for "every live row", live = min(n_rows, *d_row_count) read on the device.  d_types (uint8,
 * any alignment) and d_values (uint64, 8-byte aligned) are ONE (type, value) column with the same rows: a row of sel_* or exp_*, or
 * of a filter's compacted pair.  A row's value word is loaded only behind the type test, and only for 'l' and 'd': what lies
 * behind any other type byte is never read.  Rows at or above `live` are not read.
 * MEANING.  A valid live row with 0 <= index < n_keys belongs to that key, and its cell counts as long ('l'), as double ('d') or
 * as other (every other type byte, MISSING included).  A valid row with any other index is counted in n_out_of_range and touches
 * nothing else (its type and value are not read).  A 'd' cell of a key that is a NaN is counted in the record's n_nan and nowhere
 * else -- not in n_other, not in n_grouped; such cells are outside the parser's output.  Longs and doubles are never mixed: a
 * caller who wants one total adds the two sums and owns that rounding.
 * OUTPUT.  d_stats: uint64[n_keys * SJMI_GROUP_STATS_WORDS], key-major, 8-byte aligned; per key the words
 *     0 n_long  1 n_double  2 n_other  3 sum_long_lo  4 sum_long_hi  5 sum_double  6 min_long  7 max_long  8 min_double  9 max_double
 * sum_long_hi:sum_long_lo is the 128-bit two's-complement sum of the key's 'l' cells: exact, no wrap, no overflow flag.  min_long /
 * max_long are int64; a key without an 'l' cell has INT64_MAX / INT64_MIN.  sum_double, min_double and max_double are the bits of
 * doubles.  min_double / max_double are exact under IEEE totalOrder restricted to non-NaN values, so -0.0 < +0.0; a key without a
 * 'd' cell has +inf / -inf.  sum_double is the sum of the key's 'd' cells IN AN UNSPECIFIED ORDER: IT IS THE ONE OUTPUT WORD THAT
 * MAY DIFFER BETWEEN TWO RUNS ON THE SAME INPUT (in its last bits: |sum_double - the exact sum| <= gamma(n_double - 1) * sum|x|,
 * gamma(k) = k u / (1 - k u), u = 2^-53, for every order).  Infinite cells follow IEEE addition (+inf and -inf in one key: NaN);
 * the sign of a zero sum is unspecified.  Every other word, and the record, is a function of the input alone.  The call writes
 * exactly d_stats[0, n_keys * 10), every word, and nothing before or behind them.
 * The record, sjmi_group_result, 40 bytes, always complete: n_rows = live, n_grouped = the rows that belong to a key (the sum of
 * all n_long, n_double and n_other), n_out_of_range, n_nan, flags = 0.
 * WHY n_rows < 2^32.  The 128-bit sum is accumulated as two 64-bit words: the unsigned sum of the cells' low 32 bits, each below
 * 2^32, so below 2^32 * 2^32 = 2^64 for fewer than 2^32 rows; and the signed sum of their high 32 bits (v >> 32), each in [-2^31,
 * 2^31), so of magnitude at most 2^31 * (2^32 - 1) < 2^63.  Neither can overflow, and sum = hi * 2^32 + lo exactly.  The same
 * bound keeps a workgroup's 32-bit bin counts from overflowing.
 * THE EMPTY CASES.  n_rows == 0, live == 0 and n_keys == 0 are legal: every key has zero counts and sums and the empty minima and
 * maxima; no kernel is launched with an empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_result; NULL d_indices, d_types or d_values with n_rows > 0; NULL d_stats with n_keys > 0;
 * n_keys > SJMI_DICT_MAX_ENTRIES; d_indices not 4-byte aligned; d_validity, d_values, d_row_count, d_stats or d_result not 8-byte
 * aligned; n_rows >= 2^32.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node: a kernel that
 * writes every word's accumulation identity and the record, ONE kernel over the rows, and a kernel per key that finishes the
 * words, which the stream orders.  The context keeps NO state for this call -- no scratch, nothing to grow: calls on one context
 * need no ordering among themselves beyond what their buffers ask.  All buffers are device memory.
 * KERNELS.  n_keys <= SJMI_GROUP_LDS_KEYS: a workgroup takes chunks of 1024 rows in a grid stride into bins of its own in LDS
 * (three 32-bit counts and seven 64-bit words per key, 68 bytes) with LDS atomics, and sends the words of the keys it touched to
 * d_stats once, with agent-scope relaxed atomics (64-bit add, double add, signed / unsigned minimum and maximum; the doubles'
 * minima and maxima as unsigned integers on an order-preserving key of the bits).  Larger n_keys: such atomics go straight to
 * d_stats, the rows of a wave that have the same key combined into one cell first.  Nothing spins or waits for another workgroup;
 * d_stats is read across the kernel boundary only.
 * KNOWN LIMIT.  Above SJMI_GROUP_LDS_KEYS equal keys are combined inside a wave only, as in the census.  Out of scope: several
 * value columns per call, mean / variance (the caller divides), a compensated or reproducible double sum. */
#define SJMI_GROUP_STATS_WORDS 10u
#define SJMI_GROUP_LDS_KEYS 512u           /* 68 bytes of bins per key = 34 KiB of LDS per workgroup */
typedef struct sjmi_group_result {
    uint64_t n_rows, n_grouped, n_out_of_range, n_nan;
    uint32_t flags, reserved;
} sjmi_group_result;
int sjmi_group_stats_device(sjmi_ctx* ctx, const void* d_indices, const void* d_validity, const void* d_types, const void* d_values,
                            uint64_t n_rows, const void* d_row_count, uint64_t n_keys, void* d_stats, void* d_result, void* stream);

/* ---- the top k rows of a column: ORDER BY a value, LIMIT k, on the device -------------------------------------------------
 * "The 100 statuses with the most retweets", "the 50 latest events by created_at": the k rows with the largest (or smallest)
 * value of ONE key column, in rank order, with the cells of any number of carried columns (csrc/toprows.hip, csrc/sj_toprows.h;
 * DESIGN.md 4.18).
 *
 * INPUTS.  The key column: d_key_values, uint64[n_rows], 8-byte aligned; d_key_types (uint8, any alignment) and d_key_validity
 * (LSB-first 64-bit words, 8-byte aligned), each of which may be NULL.  With types it is ONE (type, value) column: a row of sel_* or
 * exp_*, or of a filter's compacted pair.  Without types and with validity it is a finished Arrow array: a row of
 * sjmi_arrow_columns_device or sjmi_time_columns_device.  With both, both must pass; with neither, every live row is a number.
 * The live rows are min(n_rows, *d_row_count), read on the device, exactly as sjmi_key_census_device takes them; rows at or above
 * them are not read.  A row is read in the order validity word, type byte, value word, each only behind the test in front of it:
 * the value word behind a type byte that makes no candidate is never read.
 * MEANING.  Every live row is exactly one of: a CANDIDATE; NULL (its validity bit is clear, or its type byte is MISSING or 'n');
 * OTHER (any other type byte that is no number of the kind); a NaN.  SJMI_TOP_LONG: with types only 'l' cells are candidates and
 * 'd' cells are OTHER; without types every valid row is an int64.  SJMI_TOP_DOUBLE: 'd' cells are candidates, 'l' cells are
 * converted as sjmi_arrow_columns_device converts them for a FLOAT64 field (round to nearest even; those that rounded are counted in
 * n_inexact); without types every valid row is the bits of a double.  A NaN is counted in n_nan and nowhere else.  Doubles are
 * ordered by IEEE totalOrder on the non-NaN values, -0.0 < +0.0, as sjmi_group_stats_device orders them.  flags:
 * SJMI_TOP_SMALLEST takes the k smallest and ranks them smallest first.
 * OUTPUT.  n_out = min(k, n_candidates).  d_rows, uint64[k]: d_rows[j], j < n_out, are the row indices in RANK order: by value,
 * largest first (smallest first under the flag), equal values by ASCENDING ROW INDEX -- and which of the rows that tie at the cut
 * are taken follows the same rule: the lowest row indices.  d_out_types[col * k + j] / d_out_values[col * k + j] are the cell of
 * row d_rows[j] in carried column col (d_types / d_values, n_cols columns col_stride cells apart; n_cols may be 0): the layout of
 * a filter's compacted pair with capacity k.  Entries at or behind n_out are not written, and nothing before or behind the
 * buffers is touched.  The record, sjmi_top_result, nine uint64 words, always complete: n_rows = live, n_candidates, n_null,
 * n_other, n_nan, n_inexact, n_out, kth_bits = the value word of the last returned row as the chosen kind (an int64, or the bits
 * of a double; 0 when n_out == 0), flags = 0.  n_candidates + n_null + n_other + n_nan == n_rows.  THE WHOLE OUTPUT IS A FUNCTION
 * OF THE INPUT ALONE.
 * THE EMPTY CASES.  k == 0, n_rows == 0, live == 0 and a column without candidates are legal: n_out = 0 and nothing but the record
 * is written; no kernel is launched with an empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_result; an unknown kind; a flag other than SJMI_TOP_SMALLEST; k > SJMI_TOP_MAX_K;
 * n_rows >= 2^32; NULL d_key_values with n_rows > 0; NULL d_rows with k > 0; with n_cols > 0: col_stride < n_rows, or with k > 0 a
 * NULL d_types, d_values, d_out_types or d_out_values; d_key_validity, d_key_values, d_row_count, d_values, d_rows, d_out_values
 * or d_result not 8-byte aligned.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node.  The context owns a
 * scratch slot of its own for this call (48 KiB, a word per 1024 rows, 12 bytes per unit of k); when it has to grow, the device
 * is drained first.  Calls on one context that share it must be ordered by the caller, as for sjmi_filter_columns_device.  All
 * buffers are device memory.
 * KERNELS.  An exact radix select on a 64-bit order-preserving unsigned key (a long with its sign bit flipped, a double's
 * totalOrder key; complemented under SJMI_TOP_SMALLEST): a pass over the rows for the counts and the candidates' minimum and
 * maximum key -- the bits above the highest bit in which they differ are common to all candidates and are skipped --, then per
 * 11-bit digit below them (0 to 6 of them) a histogram pass (2048 32-bit LDS bins per workgroup, the non-zero ones added to the
 * pass's histogram with agent-scope relaxed atomics) and one workgroup that picks the digit's bin; then the filter's three-pass
 * scheme (counts per 1024 rows, their scan by one workgroup, the emit) takes the rows above the threshold and the first rows, in
 * row order, equal to it; one workgroup sorts the n_out (key, row) pairs in LDS with a bitonic network under (key descending, row
 * ascending) -- a strict total order -- and gathers the carried cells.  Nothing spins or waits for another workgroup; the scratch
 * is read across kernel boundaries only.
 * KNOWN LIMITS.  k <= SJMI_TOP_MAX_K: the final sort is one workgroup's.  n_rows < 2^32: a row index travels as 32 bits inside
 * the kernels, and a histogram bin is 32 bits.  Every digit pass reads the key column again.  A full sort, and an order by
 * several columns, is sjmi_sort_rows_device below.  Out of scope: an order across longs and doubles as real numbers, string keys,
 * top k per group. */
#define SJMI_TOP_LONG 1u
#define SJMI_TOP_DOUBLE 2u
#define SJMI_TOP_SMALLEST 1u               /* flags: the k smallest, smallest first */
#define SJMI_TOP_MAX_K 2048u
#define SJMI_TOP_RESULT_WORDS 9u
typedef struct sjmi_top_result {
    uint64_t n_rows, n_candidates, n_null, n_other, n_nan, n_inexact, n_out, kth_bits;
    uint32_t flags, reserved;
} sjmi_top_result;
int sjmi_top_rows_device(sjmi_ctx* ctx, const void* d_key_types, const void* d_key_validity, const void* d_key_values, uint64_t n_rows,
                         const void* d_row_count, uint32_t kind, uint32_t flags, uint64_t k, const void* d_types, const void* d_values,
                         uint64_t n_cols, uint64_t col_stride, void* d_rows, void* d_out_types, void* d_out_values, void* d_result,
                         void* stream);

/* ---- all rows ordered by a column: a stable sort, chainable over several keys, on the device ------------------------------
 * "The exploded statuses ordered by created_at", "by (lang, retweet_count descending)", "in key order for a merge": ALL live rows
 * ordered by the value of ONE key column, with the cells of any number of carried columns, where sjmi_top_rows_device stops at
 * k = 2048 (csrc/sortrows.hip, csrc/sj_sortrows.h).  The sort is STABLE: equal keys keep their input order, so an
 * order by several columns is a chain of these calls, last key first, each taking the d_rows of the one before as its d_rows_in;
 * a sort of a filter's selection is the same call with the selection vector as d_rows_in.
 *
 * INPUTS.  The key column, n_source_rows rows: d_key_values, d_key_types, d_key_validity as sjmi_top_rows_device takes them (types
 * or validity or both may be NULL).  The call orders POSITIONS [0, live), live = min(n_rows, *d_row_count), the count read on the
 * device exactly as sjmi_top_rows_device reads it (NULL: n_rows).  Position i stands for source row d_rows_in[i] (uint64[n_rows],
 * 8-byte aligned), or for row i when d_rows_in is NULL (then n_rows <= n_source_rows).  A position whose entry is at or above
 * n_source_rows is a BAD position: it is never dereferenced, it is counted in n_bad, and it is ordered with the NULLs.  Positions
 * at or above live are not read.  A row is read in the order validity word, type byte, value word, each only behind the test in
 * front of it: the value word behind a type byte that makes no candidate is never read.  d_rows must not alias d_rows_in.
 * MEANING.  The classes are those of sjmi_top_rows_device -- CANDIDATE, NaN, OTHER, NULL --, and SJMI_SORT_LONG / SJMI_SORT_DOUBLE
 * mean what SJMI_TOP_LONG / SJMI_TOP_DOUBLE mean, the conversion of 'l' cells under DOUBLE and n_inexact included.  Doubles are
 * ordered by IEEE totalOrder on the non-NaN values, -0.0 < +0.0.
 * OUTPUT.  All live positions come out: the candidates first, by ascending value (descending under SJMI_SORT_DESCENDING), then the
 * NaN positions, then OTHER, then NULL together with the BAD positions.  Inside every class, and among equal values, positions
 * are ASCENDING -- under SJMI_SORT_DESCENDING too: the key is complemented, the tie rule does not change.  d_rows, uint64[n_rows]:
 * d_rows[j], j < live, is the source row at output place j; a BAD position stores its entry unchanged.  d_out_types[c *
 * out_stride + j] / d_out_values[c * out_stride + j] are that row's cell in carried column c (d_types / d_values, n_cols columns
 * col_stride >= n_source_rows cells apart; n_cols may be 0), type byte 0 and value 0 for a BAD position.  Entries at or behind
 * live are not written, and nothing before or behind the buffers is touched.  The record, sjmi_sort_result, nine uint64 words,
 * always complete: n_rows = live, n_candidates, n_null (without the BAD positions), n_other, n_nan, n_inexact, n_bad, n_passes =
 * the digit passes that moved data, 0 to 8, flags = SJMI_SORT_BAD_ROW iff n_bad > 0.  n_candidates + n_null + n_other + n_nan +
 * n_bad == n_rows.  THE WHOLE OUTPUT IS A FUNCTION OF THE INPUT ALONE.
 * THE EMPTY CASES.  n_rows == 0, live == 0, a column without candidates and n_cols == 0 are legal; no kernel is launched with an
 * empty grid.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_result; an unknown kind; a flag other than SJMI_SORT_DESCENDING; n_source_rows or n_rows >=
 * 2^32; NULL d_rows_in with n_rows > n_source_rows; NULL d_key_values with n_source_rows > 0 and n_rows > 0; NULL d_rows with
 * n_rows > 0; with n_cols > 0: col_stride < n_source_rows, out_stride < n_rows, or with n_rows > 0 a NULL d_types, d_values,
 * d_out_types or d_out_values; d_key_validity, d_key_values, d_rows_in, d_row_count, d_values, d_rows, d_out_values or d_result
 * not 8-byte aligned.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node.  The context owns a
 * scratch slot of its own for this call (24 bytes per position for the two pair buffers, 2 KiB per 4096 positions, 16 bytes per
 * 1024 positions, 2 KiB); when it has to grow, the device is drained first.  Calls on one context that share it must be ordered
 * by the caller, as for sjmi_filter_columns_device.  The call leaves nothing else on the context and forgets nothing.  All
 * buffers are device memory.
 * KERNELS.  A stable least-significant-digit radix sort of (64-bit order-preserving key, 32-bit position) pairs: a pass over the
 * positions for the counts and the candidates' minimum and maximum key -- the bits above the highest bit in which they differ are
 * common to all candidates and are skipped: n_passes = ceil((that bit + 1) / 8) --; the filter's three-pass scheme with four
 * counts per 1024 positions puts the candidates into a pair buffer in position order and every other position at its final place
 * behind them; per 8-bit digit, lowest first, a count of the 256 digit values per tile of 4096 pairs, 256 workgroups that scan one
 * value's counts over the tiles each, and a scatter through LDS into the other buffer; then a gather, a lane per output place.  A pair's rank
 * inside its tile is a function of the data: eight ballots give a lane the lanes of its wave with its digit value, every wave
 * walks a run of consecutive pairs in order, and the waves' counts are scanned in wave order -- no atomic hands out a slot.
 * Nothing spins or waits for another workgroup; the scratch is read across kernel boundaries only.
 * KNOWN LIMITS.  n_source_rows and n_rows < 2^32: a position travels as 32 bits.  A tile's pairs are put in output order in LDS
 * before they are stored, so a value's run of a tile is stored side by side; with 256 values in use a run is 16 pairs.
 * Thirty-one launches per call whatever the size.  Out of scope: string keys, an order across
 * longs and doubles as real numbers, a segmented sort / top k per group, a Java handle. */
#define SJMI_SORT_LONG 1u
#define SJMI_SORT_DOUBLE 2u
#define SJMI_SORT_DESCENDING 1u            /* flags: the candidates by descending value (ties still by ascending position) */
#define SJMI_SORT_BAD_ROW 1u               /* result flags: an entry of d_rows_in at or above n_source_rows was met */
#define SJMI_SORT_RESULT_WORDS 9u
typedef struct sjmi_sort_result {
    uint64_t n_rows, n_candidates, n_null, n_other, n_nan, n_inexact, n_bad, n_passes;
    uint32_t flags, reserved;
} sjmi_sort_result;
int sjmi_sort_rows_device(sjmi_ctx* ctx, const void* d_key_types, const void* d_key_validity, const void* d_key_values,
                          uint64_t n_source_rows, const void* d_rows_in, uint64_t n_rows, const void* d_row_count, uint32_t kind,
                          uint32_t flags, const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride, void* d_rows,
                          void* d_out_types, void* d_out_values, uint64_t out_stride, void* d_result, void* stream);

/* ---- the document of every exploded row, and that document's cells on the row, on the device -------------------------------
 * "Commits per /actor/login", "the longest commit messages with their event's /type": sjmi_select_batch_device gives one cell per
 * (path, document), sjmi_explode_batch_device one row per element; this call says which document a row belongs to and copies
 * that document's cells onto the row -- pandas.json_normalize(record_path, meta), SQL's UNNEST with the outer row's columns
 * (csrc/parents.hip, csrc/sj_parents.h).  Every operator that takes a (types, values) column set then works
 * across the document / element boundary; string cells of both sides point into the same string buffer.
 *
 * ROWS.  d_row_offsets is uint64[n_docs + 1] as sjmi_explode_batch_device writes it, total = d_row_offsets[n_docs].  The live
 * rows are min(n_rows, *d_row_count), read on the device as sjmi_key_census_device and sjmi_top_rows_device read them (NULL:
 * n_rows).  Output slot i < live stands for row index x = i when d_rows is NULL -- the DENSE form: the rows of an explode, with
 * d_row_count typically d_row_offsets + n_docs -- and for x = d_rows[i] (uint64) otherwise -- the SPARSE form: a filter's
 * selection vector, or sjmi_top_rows_device's d_rows, which is in rank order and not ascending.  The sparse form assumes no order;
 * duplicates are legal.
 * PARENTS.  A row x < total has exactly one parent: the k with d_row_offsets[k] <= x < d_row_offsets[k + 1]; a document without
 * rows is never a parent.  A row x >= total is an ORPHAN: d_parents[i] is all ones, d_parent_types[i] is 0 (MISSING), and every
 * carried cell of it has type 0 and value 0.  Orphans occur in the dense form when n_rows exceeds total and in the sparse form
 * with any index at or above total; with n_docs == 0 every live row is one.
 * OUTPUT, each part optional (NULL).  d_parents, int64[n_rows]; d_parent_types, uint8[n_rows], 'l' for a row with a parent: the
 * pair IS a typed long column, for LONG_* filter terms and as a key of sjmi_top_rows_device.  d_out_types[c * out_stride + i] =
 * d_types[c * col_stride + k], and likewise d_out_values, for the n_cols DOCUMENT columns d_types / d_values (select's layout,
 * col_stride >= n_docs cells apart): the layout of a filter's compacted pair.  With out_stride = the explode's row_capacity the
 * out pointers may be the tail rows of a wider column set whose head rows the explode wrote.  Nothing at or behind `live` is
 * written, and nothing outside the buffers' extents.  Type pointers may have any alignment.  The record, sjmi_parent_result,
 * three uint64 words, always complete: n_rows = live, n_orphans, flags = 0.  n_rows == 0 and n_docs == 0 are legal.  THE WHOLE
 * OUTPUT IS A FUNCTION OF THE INPUT ALONE.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL d_row_offsets or d_result; n_cols > SJMI_PARENT_MAX_COLS; with n_cols > 0 a NULL d_types,
 * d_values, d_out_types or d_out_values, col_stride < n_docs or out_stride < n_rows; n_rows or n_docs >= 2^32; d_row_offsets,
 * d_rows, d_row_count, d_values, d_parents, d_out_values or d_result not 8-byte aligned.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node, no scratch: the
 * call leaves nothing on the context and forgets nothing.  All buffers are device memory.
 * KERNELS.  One lane writes the record.  DENSE: one workgroup of 256 lanes per 1024 rows.  Two waves find the parents of the
 * chunk's first and last live row with a 64-ary search over the offsets (64 pivots, one ballot, at most 6 rounds); the documents
 * of that span are walked 256 at a time, and a document with rows whose first row lies in the chunk marks LDS at that row -- one
 * document begins at any row, so no two lanes write one address; a running maximum over the marks, seeded with the first row's
 * parent, is the parent of every position; then the stores, and per carried column a load at the parent and a coalesced store.
 * SPARSE: a lane per slot and a binary search bounded by n_docs -- latency-bound by design, meant for the rows of a top k or of a
 * filter.  The orphans are counted with one agent-scope relaxed atomic per workgroup.  Nothing spins or waits for another
 * workgroup.
 * ROBUSTNESS.  The offsets are trusted to be what the explode wrote.  Every search is bounded by n_docs all the same, and a
 * parent is compared with n_docs before it becomes a load address: wild offset words may give wrong parents, never a load or
 * store outside a buffer or an unbounded loop.
 * KNOWN LIMITS.  The spans of all chunks sum to at most n_docs plus the number of chunks, but one chunk behind a long run of
 * documents without rows walks that run alone.  Out of scope: nested explodes, joins on anything but the row-to-document relation,
 * distinct-parent counts, several offset arrays per call. */
#define SJMI_PARENT_MAX_COLS 64u
#define SJMI_PARENT_RESULT_WORDS 3u
typedef struct sjmi_parent_result {
    uint64_t n_rows, n_orphans;
    uint32_t flags, reserved;
} sjmi_parent_result;
int sjmi_parent_columns_device(sjmi_ctx* ctx, const void* d_row_offsets, uint64_t n_docs, const void* d_rows, uint64_t n_rows,
                               const void* d_row_count, const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride,
                               void* d_parent_types, void* d_parents, void* d_out_types, void* d_out_values, uint64_t out_stride,
                               void* d_result, void* stream);

/* ---- two row sets joined on a long key: inner, left, semi, anti, on the device -----------------------------------------------
 * "Every event with the columns of its actor's row in the users file", "every status whose /retweeted_status/user/id is mentioned
 * somewhere in the batch, with the mention": an equi-join of a LEFT (probe) row set with a RIGHT (build) row set on one integer
 * key a side (csrc/joinrows.hip, csrc/sj_joinrows.h).
 *
 * A SIDE, sjmi_join_side, is read from HOST memory during the call (as the terms of sjmi_filter_plan_compile are); the pointers
 * in it are device memory: the key column of n_source_rows rows as sjmi_sort_rows_device takes it (d_key_types or d_key_validity
 * or both may be NULL), and n_cols carried columns d_types / d_values, col_stride >= n_source_rows cells apart (NULL with n_cols
 * == 0).
 * THE LEFT SIDE.  Positions [0, live_left), live_left = min(n_left, *d_left_count), the count read on the device (NULL: n_left).
 * Position i stands for source row d_left_rows_in[i] (uint64[n_left]), or for row i when d_left_rows_in is NULL (then n_left <=
 * n_source_rows).  A position is classified exactly as sjmi_sort_rows_device classifies it under SJMI_SORT_LONG -- CANDIDATE, NULL,
 * OTHER (a 'd' cell is OTHER), BAD (an entry at or above n_source_rows: never dereferenced) --, its cell read in the same order:
 * validity word, type byte, value word, each only behind the test in front of it.
 * THE RIGHT SIDE has been ordered by the caller with sjmi_sort_rows_device, kind SJMI_SORT_LONG, ascending: d_right_order is that
 * call's d_rows, d_right_sort_result its record IN DEVICE MEMORY, n_right its n_rows.  The join reads n_candidates from the
 * record on the device; the BUILD SET is the first n_build = min(n_right, n_candidates) entries of d_right_order, and nothing
 * behind them is read.  A right side is therefore sorted once and probed by many left batches, and may be a filter's selection or
 * stand behind a device row count, because the sort took both.  WILD INPUT: an entry of the build set at or above
 * right->n_source_rows is never dereferenced; such an entry, an entry whose cell is not a CANDIDATE (both counted in n_right_bad)
 * and an adjacent pair of build keys that descends each set SJMI_JOIN_BAD_ORDER.  The pairs are then unspecified; every load and
 * store still stays inside its buffer.
 * THE RELATION.  m(i) = the number of build places whose key equals the key of candidate position i, 0 for every other class.
 * Position i emits e(i) pairs: SJMI_JOIN_INNER m(i); SJMI_JOIN_LEFT max(m(i), 1); SJMI_JOIN_SEMI m(i) > 0; SJMI_JOIN_ANTI m(i) ==
 * 0.  For LEFT and ANTI that is every live position, NULL, OTHER and BAD ones included: SQL's rule for a null key.
 * OUTPUT.  Pairs come out by ascending left position, inside one position by ascending build place -- the sort is stable, so
 * among equal keys by ascending right position.  Pair j < min(n_pairs, pair_capacity): d_left_rows[j] = the source row of its left
 * position (a BAD entry unchanged); d_right_rows[j] = the matching right source row, SJMI_JOIN_NO_ROW for the unmatched pair of
 * LEFT and for every ANTI pair (d_right_rows may be NULL under SEMI and ANTI; under SEMI it is the first match); the carried cells
 * d_left_out_* / d_right_out_*[c * out_stride + j], type 0 and value 0 where the row is BAD or NO_ROW.  Nothing at or behind
 * min(n_pairs, pair_capacity) is written, and nothing outside the buffers.  d_pair_offsets, optional, uint64[n_left + 1]: off[i]
 * = the pairs in front of position i, i <= live_left, the TRUE count, not clipped by the capacity; entries behind live_left are
 * not written.  It has the layout of an explode's row_offsets: sjmi_parent_columns_device reads it as "left position = document,
 * pair = row".  The record, sjmi_join_result, nine uint64 words, always complete: n_left = live_left, n_build, n_pairs (the true
 * total: both sides are below 2^32, it cannot wrap), n_matched = the positions with m > 0, n_null, n_other, n_bad over the left,
 * n_right_bad, flags = SJMI_JOIN_OVERFLOW iff n_pairs > pair_capacity, SJMI_JOIN_BAD_ROW iff n_bad > 0, SJMI_JOIN_BAD_ORDER.  THE
 * WHOLE OUTPUT IS A FUNCTION OF THE INPUT ALONE: no atomic decides a place.
 * ARGUMENTS.  SJMI_ERR_ARG: NULL left, right or d_result; an unknown how; n_left, n_right or a side's n_source_rows >= 2^32;
 * pair_capacity >= SJMI_JOIN_MAX_PAIR_CAPACITY; NULL d_left_rows_in with n_left > left->n_source_rows; a NULL key values pointer
 * of a side with source rows and positions; NULL d_right_sort_result or d_right_order with n_right != 0; NULL d_left_rows with
 * pair_capacity != 0; NULL d_right_rows under INNER or LEFT with pair_capacity != 0; with carried columns on a side: col_stride
 * < n_source_rows, out_stride < pair_capacity, or with pair_capacity != 0 a NULL column or output pointer; right carried columns
 * under SEMI or ANTI; a uint64 pointer (key validity, key values, carried values, d_left_rows_in, d_left_count, d_right_order,
 * d_right_sort_result, d_left_rows, d_right_rows, both out values, d_pair_offsets, d_result) not 8-byte aligned.
 * STREAM AND STATE.  Asynchronous on `stream` (NULL = the context's), no host synchronisation, no memset node.  The context owns a
 * scratch slot of its own for this call (8 bytes per build place, 16 bytes per left position, 8 bytes per 1024 left positions);
 * when it has to grow, the device is drained first.  Calls on one context that share it must be ordered by the caller.  The call
 * leaves nothing else on the context and forgets nothing.
 * KERNELS.  The build keys are gathered once into a dense sorted array (and checked: bad places, descending neighbours); every
 * left position is classified and finds the lower bound of its key there through 1024 pivots that its workgroup keeps in LDS,
 * and the upper bound by galloping from the lower one (a unique key: three loads; at most 33 + 33 steps); the filter's
 * three-pass scheme turns e(i) into the pair offsets; the pairs are written by
 * one workgroup per 1024 OUTPUT pairs, which finds the owners of its pairs with the load-balanced search of
 * sjmi_parent_columns_device's dense form on the offsets -- so one position with a million matches is a thousand output chunks of
 * equal cost.  Nothing spins or waits for another workgroup; the scratch is read across kernel boundaries only; the atomics
 * (agent scope, relaxed, results unused) touch the record only.
 * KNOWN LIMITS.  The caller sizes pair_capacity; on SJMI_JOIN_OVERFLOW it reads n_pairs and calls again, as with
 * sjmi_filter_columns_device.  The emit's grid is sized by pair_capacity, not by n_pairs.  A probe is a chain of dependent loads
 * a position.  Out of scope: double, string and composite keys, right and full outer joins, a merge path for a sorted left side, a
 * hash-table build, paging through the pairs, a Java handle. */
#define SJMI_JOIN_INNER 0u
#define SJMI_JOIN_LEFT 1u
#define SJMI_JOIN_SEMI 2u
#define SJMI_JOIN_ANTI 3u
#define SJMI_JOIN_OVERFLOW 1u              /* result flags: n_pairs > pair_capacity */
#define SJMI_JOIN_BAD_ROW 2u               /* result flags: an entry of d_left_rows_in at or above the left source rows was met */
#define SJMI_JOIN_BAD_ORDER 4u             /* result flags: the build set is not what an ascending LONG sort of the right side wrote */
#define SJMI_JOIN_NO_ROW 0xFFFFFFFFFFFFFFFFull
#define SJMI_JOIN_RESULT_WORDS 9u
#define SJMI_JOIN_MAX_PAIR_CAPACITY (1ull << 40)
typedef struct sjmi_join_side {
    const void* d_key_types;     /* uint8, any alignment, or NULL (every valid row is a long) */
    const void* d_key_validity;  /* uint64 words or NULL */
    const void* d_key_values;    /* uint64 */
    uint64_t n_source_rows;      /* rows of the key column and of the carried columns */
    const void* d_types;         /* carried columns [n_cols * col_stride], or NULL with n_cols == 0 */
    const void* d_values;
    uint64_t n_cols, col_stride;
} sjmi_join_side;
typedef struct sjmi_join_result {
    uint64_t n_left, n_build, n_pairs, n_matched, n_null, n_other, n_bad, n_right_bad;
    uint32_t flags, reserved;
} sjmi_join_result;
int sjmi_join_rows_device(sjmi_ctx* ctx, const sjmi_join_side* left, const void* d_left_rows_in, uint64_t n_left, const void* d_left_count,
                          const sjmi_join_side* right, const void* d_right_order, uint64_t n_right, const void* d_right_sort_result,
                          uint32_t how, uint64_t pair_capacity, void* d_left_rows, void* d_right_rows, void* d_left_out_types,
                          void* d_left_out_values, void* d_right_out_types, void* d_right_out_values, uint64_t out_stride,
                          void* d_pair_offsets, void* d_result, void* stream);

/* Optional: page-lock caller-owned host memory that is passed to the host-buffer entry points again and again
 * (SimdJsonParser's padded input, index array and string buffer): H2D / D2H copies of pinned memory skip the
 * driver's staging copy (3-4x faster for the ~1 MB transfers of a single-document parse).  Purely a performance
 * hint: every entry point also works with pageable memory.  Unregister before freeing the memory.
 * ZERO-COPY OUTPUTS: when the output arrays of sjmi_stage1 (indexes), sjmi_stage1_unescape (indexes AND string_buffer) or
 * sjmi_parse_document (tape) are page-locked, device-visible and 16-byte aligned, the kernels write them directly over PCIe:
 * no download, one host synchronisation per call.  The results are the same bytes; as on the staged path, array elements
 * behind the returned counts (up to the capacities) may be overwritten.  A context remembers the device view of such a
 * buffer; sjmi_host_register / sjmi_host_unregister (on any context) make every context forget them, so memory that was
 * page-locked by other means (hipHostMalloc / hipHostRegister of the caller's own) must stay page-locked as long as it is
 * passed to a context, or be followed by one sjmi_host_unregister call (its failure for a foreign pointer is harmless).
 * SJMI_ZERO_COPY=0 in the environment switches the zero-copy paths off. */
int sjmi_host_register(sjmi_ctx* ctx, void* ptr, uint64_t bytes);
/* Optional: a page-locked staging buffer for the INPUT of the single-document host entry points (sjmi_stage1,
 * sjmi_stage1_unescape, sjmi_parse_document).  With one set (bytes >= the document's length), a document handed in from any
 * other address is copied through it -- the reference's padIfNeeded copy (SimdJsonParser.java:42-48), which a caller needs
 * anyway for its stage 2 -- and from 4 MiB on in chunks whose H2D copies run while the next chunk is being copied: the
 * memcpy and the PCIe transfer of a 64 MiB document overlap instead of adding up.  After the call staging[0, len) holds the
 * document.  pinned == NULL switches it off.  The buffer stays the caller's (register it with sjmi_host_register). */
int sjmi_set_input_staging(sjmi_ctx* ctx, void* pinned, uint64_t bytes);
int sjmi_host_unregister(sjmi_ctx* ctx, void* ptr);

/* Run the on-device self-test of the bit-plane transposition; *mismatches == 0 on success. */
int sjmi_selftest(sjmi_ctx* ctx, uint32_t* mismatches);

/* tuning knob for tests: force the chain granule = steps x 4 KiB per worker wave and iteration (1, 2 or 4;
 * 0 = automatic: 1 for documents up to 4 MiB, 2 up to 16 MiB, else 4) */
int sjmi_set_tile_steps(sjmi_ctx* ctx, int steps);

/* Liveness mode of the stage-1 kernel (results never depend on it): 0 (default) = FAST: persistent worker waves plus
 * one scanner workgroup that turns the workers' per-granule aggregates into prefixes; assumes that the whole grid
 * (sized with the occupancy API) is resident at the same time.  1 = SAFE: no scanner, granules by one atomic ticket,
 * every worker resolves its prefix by a decoupled look-back; no residency assumption at all, ~2.5x slower.
 * A FAST launch whose bounded spins trip reports SJMI_ST_INTERNAL: the host-buffer entry points then latch SAFE mode
 * and re-run the launch; the *_device entry points return the status bit to the caller.
 * Environment: SJMI_TILE_MODE=ticket selects SAFE mode at context creation. */
int sjmi_set_tile_mode(sjmi_ctx* ctx, int ticket);
/* Forward-progress assumption, stated once: a FAST launch spins (bounded: tens of milliseconds) on values only OTHER
 * workgroups of the same launch produce, so it needs its whole grid -- sized with the occupancy API to what fits the
 * device -- resident at the same time.  That holds when the kernel has the GPU to itself and, by giving up the static first
 * granule (done automatically while another context of this process still has a stage-1 launch running), when two such
 * kernels share it; it can fail when foreign kernels (another process, PyTorch on another stream) hold CUs for longer
 * than the spin bound.  Results never depend on it -- a launch either completes correctly or reports SJMI_ST_INTERNAL.
 * The host-buffer entry points then latch SAFE mode and re-run by themselves.  For the asynchronous *_device entry
 * point the caller chooses: read SJMI_ST_INTERNAL from its result record and call sjmi_set_tile_mode(ctx, 1), or opt in
 * here (on = 1): sjmi_stage1_device then synchronises its stream after every FAST launch, and on a tripped bound latches
 * SAFE mode and repeats the launch before returning (costs the asynchrony; SAFE mode itself has no residency assumption). */
int sjmi_set_auto_safe(sjmi_ctx* ctx, int on);

/* Measurement hooks for bench.py: when on, every sjmi_stage1_device launch is bracketed by HIP events
 * on the launch stream (kernel only); sjmi_kernel_time returns their summed duration and count. */
int sjmi_set_profiling(sjmi_ctx* ctx, int on);
/* performance-ablation switches for sjmi_stage1_device (1 = no index stores, 2 = no look-back): results are
 * INVALID while any is set (experiments only); test hooks with valid results: 16 = fast-mode launches report
 * SJMI_ST_INTERNAL, 32 = launch only 8 worker workgroups (as if most of the GPU were busy with other work), 0x800 = every
 * granule by ticket, the first one of a wave included (as if another context were launching: what a stage-1 launch does by
 * itself while another context of the process still has one running). */
int sjmi_debug_set_flags(sjmi_ctx* ctx, uint32_t flags);
/* Read-only test hook: out[0 .. 3] = stage-1 launches this context has queued; those of them that took every granule by
 * ticket (another context of the process was busy, or debug flag 0x800); repeats in SAFE mode after a tripped spin bound (the
 * host forms' own, and sjmi_set_auto_safe's); SAFE mode now, 0 or 1 (sjmi_set_tile_mode, or latched).  Plain fields of the
 * context: call it from the thread that uses the context. */
int sjmi_debug_counters(sjmi_ctx* ctx, uint64_t* out);
int sjmi_kernel_time(sjmi_ctx* ctx, double* sum_ms, uint32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* SJMI_H */
