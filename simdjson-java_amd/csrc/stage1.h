// stage1.h -- internal declarations shared by the HIP kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "../../include/sjmi.h"

namespace sjmi {

// written by the kernel into the workspace header; mirrors sjmi_stage1_result in include/sjmi.h
struct Stage1Result {
    unsigned long long count;  // number of structural indexes (BitIndexes.writeIdx)
    uint32_t status;           // SJMI_ST_* bits
    uint32_t reserved;
};
static_assert(sizeof(Stage1Result) == sizeof(sjmi_stage1_result), "ABI struct mismatch");

// device-side result of one unescape call; mirrors sjmi_unescape_result in include/sjmi.h
struct UnescapeResult {
    unsigned long long total_bytes;      // bytes of [be32 len][bytes] records
    unsigned long long first_error_inv;  // 0 = no error, else ~((byte position | structural position << 8) | SJMI_E_* code)
    uint32_t flags;                      // bit0: string buffer capacity exceeded; bits 2-3: engine fault
    uint32_t reserved;                   // strings.hip: number of string literals
};
static_assert(sizeof(UnescapeResult) == sizeof(sjmi_unescape_result), "ABI struct mismatch");

// sjmi_parse_document: the result records of the three stages in one place (one D2H), written by the walk's LAST launch
struct WalkResult;
struct SingleDocPack;
struct SingleDocTail {          // where that launch finds / leaves them; pack == nullptr: no such tail
    const Stage1Result* s1 = nullptr;
    const UnescapeResult* u = nullptr;
    SingleDocPack* pack = nullptr;
    bool optimistic = false;    // the chunk path ends in k_chunk_finish and nothing is queued behind it: a document it does not
                                // take (pack->fallback != 0) is the caller's to run again with no_chunks
    bool no_chunks = false;     // the single-wave sweep only
    uint64_t in_place_cap = 0;  // != 0: d_tape is the CALLER's tape (mapped host memory) with this many words: the walkers write
                                // it in place whatever the structural count's bound says, clamped to it
};

// device-side result of one batch walk; mirrors sjmi_walk_result in include/sjmi.h
struct WalkResult {
    unsigned long long tape_words, host_documents, failed_documents;
    uint32_t flags, reserved;
};
static_assert(sizeof(WalkResult) == sizeof(sjmi_walk_result), "ABI struct mismatch");
struct SingleDocPack {
    Stage1Result s1;
    UnescapeResult u;
    WalkResult w;
    unsigned long long to[2];
    int32_t err;
    uint32_t fallback;
};
static_assert(sizeof(SingleDocPack) <= 256, "d_single / h_single hold 256 bytes of results");

// ablation switches for performance experiments only (results are NOT valid with any of them set)
constexpr uint32_t DBG_NO_WRITE = 1, DBG_NO_LOOKBACK = 2;
// test hook: a fast-mode launch reports SJMI_ST_INTERNAL as if its look-back spin had tripped
constexpr uint32_t DBG_FAKE_TIMEOUT = 16;
// test hook: launch only 8 worker workgroups (as if the GPU were shared with other work)
constexpr uint32_t DBG_SMALL_GRID = 32;
// kernel flag (not an ablation): SAFE liveness mode -- no scanner workgroup, every worker looks back itself
constexpr uint32_t FLAG_SAFE = 0x100;
// shards of a longer document (sjmi_stage1_shard_device): the shard is entered inside a string; it is not the document's
// last shard (no tail block); bits 16..31 = readable 64-byte blocks in front of the buffer (left halo)
constexpr uint32_t FLAG_ENTRY_PARITY = 0x1000;
constexpr uint32_t FLAG_NO_TAIL = 0x4000;
// the shard's left halo begins at the document's first byte (a backslash run that fills it is complete)
constexpr uint32_t FLAG_HALO_FROM_START = 0x2000;
// kernel flag: FAST mode without static first granules (several contexts may be launching concurrently)
constexpr uint32_t FLAG_ALL_TICKETS = 0x800;

// workspace layout (zeroed by one hipMemsetAsync per launch)
constexpr size_t WS_RESULT_OFFSET = 0;        // Stage1Result (16 bytes)
constexpr uint32_t WS_SCANNER_CU_WORD = 8;    // u32 index from the workspace start: id of the scanner's CU
constexpr size_t WS_TICKET_OFFSET = 64;       // 8 u32 granule tickets, each alone in its 64-byte line
constexpr size_t WS_BATCH_FLAGS_OFFSET = 576;  // fused batch pipeline: u32 [0] = why the plain pass is rejected (0: it is not), [1] != 0:
                                               // accepted (written by k_batch_layout).  In the header of the plain pass's OWN workspace
                                               // half: zero when the launch starts, like the rest of it -- no memset of their own
constexpr size_t WS_TILE_STATE_OFFSET = 640;   // u64 aggregates[granules], then u64 prefixes[granules]

size_t stage1_workspace_bytes(uint64_t len, int steps);
struct Stage1Prefixes {
    const unsigned long long* pfx = nullptr;
    uint64_t ngran = 0;
    uint32_t granule_bytes = 0;
};
Stage1Prefixes stage1_prefixes(const void* d_ws, uint64_t len, int steps);
int stage1_pick_steps(uint64_t len);
size_t stage1_block_entries(uint64_t len);
// sjmi_parse_document: the delimiters of ONE document for the batch kernels behind stage 1 (doc / index / string offsets, status)
// and the two small records the walk wants zeroed -- written by the stage-1 scanner together with the result record
struct Stage1Single {
    unsigned long long* doc_offsets = nullptr;
    unsigned long long* index_offsets = nullptr;  // nullptr: nothing to do
    uint32_t* doc_status = nullptr;
    unsigned long long* doc_str_offsets = nullptr;
    uint32_t* walk_result = nullptr;   // sizeof(WalkResult) bytes
    uint32_t* slow_header = nullptr;   // 64 bytes
};
// optional work folded into the kernel (device-resident path): see zero_next_workspace / Stage1Chain::finish in stage1.hip
struct Stage1Extras {
    bool workspace_is_zero = false;  // skip the workspace memset (a previous launch zeroed this workspace)
    void* zero_next = nullptr;       // workspace the NEXT launch will use: zeroed by this one (16-byte aligned)
    size_t zero_bytes = 0;           //   ... this many bytes of it (multiple of 16)
    void* result_out = nullptr;      // device sjmi_stage1_result written by the scanner (FAST mode only)
    const uint32_t* skip = nullptr;  // device flag: != 0 -> the launch does nothing (fused batch pipeline)
    void* zero2 = nullptr;           // a second region zeroed by the workers on their way out (16-byte aligned, multiple of 16 bytes):
    size_t zero2_bytes = 0;          //   the string pass's workspace on the single-document latency path (one memset less)
    Stage1Single single;             // ... and what k_single_doc_setup would write, done by the scanner (FAST mode; one launch less)
    void* blkidx = nullptr;          // batch side outputs (both or neither): u32 per 64-byte block = index position of the block's
    void* blkw = nullptr;            //   first structural; u16 per block = its tape words for entry parity 0 | 1 << 8; stage1_block_entries(len) each
    void* blkpar = nullptr;          // side output for strings.hip: u64 per 4 KiB of input, bit l = block l is entered inside a
                                     // string (StructuralIndexer.java:233-234's prevInString, per block); len / 4096 + 4 words
};
// ev_start/ev_stop (optional) are attached to the kernel's dispatch (not the workspace memset)
hipError_t stage1_launch(const uint8_t* d_buf, uint64_t len, uint32_t* d_out, uint64_t out_cap, void* d_ws, int steps,
                         hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop, uint32_t dbg = 0,
                         const Stage1Extras& ex = Stage1Extras());
// strings.hip: the string buffer of a document in one streaming pass (from the bytes and stage 1's block parities)
size_t strings_workspace_bytes(uint64_t len);
size_t strings_parity_words(uint64_t len);
// the fused batch pipeline decides ON THE DEVICE whether the string pass runs over the batch itself (*d_sel != 0) or over its
// sanitized copy (d_buf / d_blkpar here)
struct StringsAlt {
    const uint32_t* d_sel = nullptr;
    const uint8_t* d_buf = nullptr;
    const unsigned long long* d_blkpar = nullptr;
};
hipError_t strings_launch(const uint8_t* d_buf, uint64_t len, const unsigned long long* d_blkpar, uint8_t* d_sb, uint64_t sb_cap,
                          uint32_t* d_soff, uint64_t soff_cap, uint32_t* d_blk_ord, void* d_ws, UnescapeResult* d_res,
                          hipStream_t stream, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                          const StringsAlt& alt = StringsAlt(), bool workspace_is_zero = false, const uint32_t* d_skip = nullptr);
// batches whose documents were indexed one by one: the copy the string pass runs on (failed documents blanked); d_skip != null
// and *d_skip != 0: nothing to do (the optimistic plain pass was accepted)
hipError_t strings_sanitize_launch(const uint8_t* d_buf, uint64_t total_len, const unsigned long long* d_doc_offsets,
                                   const unsigned long long* d_index_offsets, uint64_t n_docs, uint8_t* d_copy, const uint32_t* d_skip,
                                   hipStream_t stream, const uint32_t* d_doc_status = nullptr);
// (d_doc_status != nullptr: a document is blanked when its stage-1 verdict is not 0 -- the repair pass, which has no index offsets
//  yet; else when it has no structurals)
// per document: ordinal of its first string in the record table (and, optionally, that record's offset)
hipError_t strings_doc_ordinals_launch(const uint8_t* d_buf, const unsigned long long* d_blkpar, const StringsAlt& alt, uint64_t len,
                                       const unsigned long long* d_doc_offsets, uint64_t n_docs, const uint32_t* d_blk_ord,
                                       const uint32_t* d_soff, const UnescapeResult* d_res, unsigned long long* d_doc_ord,
                                       unsigned long long* d_doc_str_offsets, hipStream_t stream, const uint32_t* d_skip = nullptr);
size_t strings_parse_pack_bytes();
hipError_t strings_error_index_pack_launch(const uint32_t* d_idx, const Stage1Result* dev_count, const UnescapeResult* d_res, void* d_pack,
                                           hipStream_t stream);
UnescapeResult* strings_workspace_result(void* d_ws);
hipError_t strings_error_index_launch(const uint32_t* d_idx, uint64_t count, const Stage1Result* dev_count, const UnescapeResult* d_res,
                                      unsigned long long* d_out, hipStream_t stream);
// the string pass of a batch (sjmi_unescape_batch_device): document / index offsets on the device (n_docs + 1 entries each) and,
// optionally, where the string-buffer offset of every document's first record goes
struct UnescapeBatch {
    const unsigned long long* d_doc_offsets = nullptr;
    const unsigned long long* d_index_offsets = nullptr;
    uint64_t n_docs = 0;
    unsigned long long* d_doc_str_offsets = nullptr;
};
hipError_t split_docs_launch(const uint32_t* d_idx, const Stage1Result* d_res, const unsigned long long* d_doc_offsets,
                             uint64_t n_docs, unsigned long long* d_index_offsets, hipStream_t stream);
size_t batch_isolated_workspace_bytes(uint64_t n_docs);
// What the batch walker (coop_walk.hip k_tok_stream) reads per document, one 32-byte record instead of six arrays: n_docs + 1
// records, the last one carrying only `tape` (a document's room on the tape = the next record's `tape` - its own).
struct DocMeta {
    uint32_t from, to;            // its structurals: indexes[from, to)
    uint32_t dso;                 // ordinal of its first string in the string pass's record table
    uint32_t doc_start, doc_end;  // its bytes
    uint32_t st;                  // its stage-1 status (SJMI_ST_*)
    uint32_t tape_lo, tape_hi;    // where its tape goes (word offset)
};
static_assert(sizeof(DocMeta) == 32, "one s_load_dwordx8");
// The accepted plain pass of the fused batch pipeline, everything a document needs from it in ONE pass over the documents
// (batch.hip k_doc_prepare; replaces the binary search of k_split_docs_accept and k_doc_str_ordinals): index_offsets, doc_status
// = 0, the ordinal / record offset of its first string, its PREDICTED tape length (exact for a well-formed document) and the
// DocMeta record without `tape`; chunk_sums[j] = predicted words of documents [256 j, 256 j + 256).
struct DocPrepare {
    const uint8_t* buf = nullptr;
    const uint32_t* idx = nullptr;
    const unsigned long long* doc_offsets = nullptr;
    uint64_t n_docs = 0, total_len = 0;
    const uint32_t* blkidx = nullptr;
    const uint16_t* blkw = nullptr;
    const unsigned long long* blkpar = nullptr;
    const uint32_t* blk_ord = nullptr;
    const uint32_t* soff = nullptr;
    const UnescapeResult* strings = nullptr;
    const Stage1Result* stage1 = nullptr;
    uint32_t* flags = nullptr;        // [0]: reject bits -- this kernel adds "a separator is missing / the offsets do not cover the buffer"
    unsigned long long* index_offsets = nullptr;
    uint32_t* doc_status = nullptr;
    unsigned long long* doc_ord = nullptr;
    unsigned long long* doc_str_offsets = nullptr;
    uint32_t* lens = nullptr;
    unsigned long long* chunk_sums = nullptr;
    DocMeta* metas = nullptr;
    // the REPAIR pass (round 6, sjmi_api.hip parse_batch_pipeline stage B): the same kernel over the sanitized copy of a batch
    // whose plain pass was rejected -- the documents that failed stage 1 (status_in[k] != 0, from the verdict pass
    // k_doc_pass<false>) are blank there, so every surviving document begins and ends outside a string whatever separates them
    const uint32_t* gate = nullptr;       // device flag: != 0 -> nothing to do
    const uint32_t* status_in = nullptr;  // per-document stage-1 verdicts to keep (nullptr: every document passed)
    const uint8_t* boundary_buf = nullptr;  // the ORIGINAL batch: a surviving document that ends in a backslash there fails the boundary
                                          // rule (the sanitized copy has an odd trailing backslash run shortened by one)
    bool relaxed = false;                 // boundary rule: the last byte of a document must not be a non-quote scalar character
                                          // (instead of: must be a control-character separator)
};
constexpr int PREP_DOCS = 256;  // documents per workgroup of k_doc_prepare = per chunk of the tape-offset scan
hipError_t batch_prepare_launch(const DocPrepare& a, hipStream_t stream);
// walk.hip k_batch_layout, queued behind k_doc_prepare: DECIDES whether the plain pass is accepted (flags[0] == 0 and a clean
// stage-1 verdict) -> flags[1]; zeroes the walk's result record, the literal list's header and the exact walker's list; hands the
// string pass's record (inside its workspace) to the caller's -- or zeroes that for the per-document string pass to fill;
// accepted: the scan of the predicted tape lengths (chunk bases, tape_offsets[n_docs], walk.tape_words).  optimistic_only: a
// rejected batch gets SJMI_ST_REJECTED in the caller's stage-1 record (nothing else is queued for it).
struct BatchLayout {
    uint32_t* flags = nullptr;
    const Stage1Result* stage1 = nullptr;          // the plain pass's record as the kernel left it
    Stage1Result* stage1_out = nullptr;            // the caller's (optimistic_only: |= SJMI_ST_REJECTED)
    const UnescapeResult* strings_ws = nullptr;    // the string pass's own record
    UnescapeResult* strings_out = nullptr;         // the caller's
    WalkResult* walk = nullptr;
    void* slow_header = nullptr;                   // 64 bytes
    uint32_t* list = nullptr;
    unsigned long long* chunk_sums = nullptr;
    uint64_t n_docs = 0, tape_capacity = 0;
    unsigned long long* tape_offsets = nullptr;
    bool optimistic_only = false;
    // round 6: the pipeline's stage flags (sjmi_api.hip): pipe_flags[0] != 0 = the plain pass over the batch itself was accepted
    // (stage A), pipe_flags[1] != 0 = A or the repair pass over the sanitized copy (stage B) was -- the tapes are laid out
    uint32_t* pipe_flags = nullptr;
    int stage = 0;                         // 0: A (writes both flags), 1: B (writes [1])
    const uint32_t* gate = nullptr;        // device flag: != 0 -> nothing to do (stage B behind an accepted A)
    const uint32_t* status_or = nullptr;   // stage B: OR of the documents' verdicts, into the caller's stage-1 record
};
hipError_t batch_reject_launch(Stage1Result* d_stage1, hipStream_t stream);  // sjmi_parse_batch_device_optimistic on a batch it cannot even try
hipError_t batch_layout_launch(const BatchLayout& a, void* d_ws, uint64_t count, const uint32_t* lens, DocMeta* metas,
                               int32_t* d_doc_errors, hipStream_t stream);
// walk.hip: stage 2 of every document of a batch (the cooperative walker + packing of the tapes); d_doc_str_ordinals[k] =
// ordinal of document k's first string in the record table d_soff of the string pass (strings.hip)
size_t walk_workspace_bytes(uint64_t count, uint64_t n_docs);
struct WalkLaunch {
    const uint8_t* d_buf = nullptr;
    const unsigned long long* d_doc_offsets = nullptr;
    uint64_t n_docs = 0;
    const uint32_t* d_idx = nullptr;
    uint64_t count = 0;
    const unsigned long long* d_index_offsets = nullptr;
    const uint32_t* d_doc_status = nullptr;
    const uint8_t* d_sb = nullptr;
    const unsigned long long* d_doc_str_ordinals = nullptr;
    uint64_t string_base = 0;
    int max_depth = 0;
    unsigned long long* d_tape = nullptr;
    uint64_t tape_capacity = 0;
    unsigned long long* d_tape_offsets = nullptr;
    int32_t* d_doc_errors = nullptr;
    void* d_ws = nullptr;
    WalkResult* d_res = nullptr;
    const Stage1Result* dev_count = nullptr;
    const UnescapeResult* dev_strings = nullptr;
    const uint32_t* d_soff = nullptr;
    bool index_from_zero = false;
    bool results_zeroed = false;
    SingleDocTail tail;
    // d_prepared (the fused batch pipeline; nullptr: the separate calls): batch_layout_launch ran -- the result record and the list
    // headers are zeroed, nothing of that is queued again -- and left this device flag: != 0 = the tapes ARE laid out, from the
    // DocMeta / predicted tape lengths batch.hip k_doc_prepare left in the walk workspace (walk_prepared), and are written at their
    // final addresses -- there a document that fails keeps its (unused) slot: tape_offsets[k + 1] - tape_offsets[k] is its
    // PREDICTED length, the words are unspecified, doc_errors[k] says so.  optimistic_only: only the kernels of that path are queued.
    const uint32_t* d_prepared = nullptr;
    bool optimistic_only = false;
};
hipError_t walk_launch(const WalkLaunch& w, hipStream_t stream);
struct WalkPrepared {
    DocMeta* metas;
    uint32_t* lens;
    unsigned long long* chunk_sums;
};
WalkPrepared walk_prepared(void* d_ws, uint64_t count, uint64_t n_docs);
// coop_walk.hip: the batch walkers -- k_tok_stream over tokens, then k_coop_walk (list mode) for the documents it declined
struct TokLaunch {
    const uint8_t* d_buf;
    const uint32_t* d_idx;
    const DocMeta* d_metas;
    uint64_t n_docs;
    const unsigned long long* d_doc_offsets;
    const unsigned long long* d_index_offsets;
    const uint32_t* d_doc_status;
    const unsigned long long* d_doc_str_ordinals;
    const uint32_t* d_soff;
    const uint8_t* d_sb;
    uint64_t string_base;
    int max_depth;
    unsigned long long* d_tape;     // *d_sel != 0 (or d_sel == nullptr): where the DocMeta offsets point
    unsigned long long* d_scratch;  // otherwise
    const uint32_t* d_sel;
    uint32_t* d_tape_lens;
    int32_t* d_doc_errors;
    uint32_t* d_list;
    const Stage1Result* dev_count;
    const UnescapeResult* dev_strings;
    WalkResult* d_res;
    void* d_deep_ws;
    bool header_zeroed = false;     // the literal list's 64-byte header is zero already (k_batch_layout)
};
hipError_t tok_walk_launch(const TokLaunch& t, hipStream_t stream);
// coop_walk.hip: the cooperative walker (a wave per document); d_soff = offset of every string's record in d_sb, by ordinal
hipError_t coop_walk_launch(const uint8_t* d_buf, const unsigned long long* d_doc_offsets, uint64_t n_docs, const uint32_t* d_idx,
                            const unsigned long long* d_index_offsets, const uint32_t* d_doc_status, const uint32_t* d_soff,
                            const uint8_t* d_sb, const unsigned long long* d_doc_str_ordinals, uint64_t string_base,
                            int max_depth, unsigned long long* d_scratch_tape, uint32_t* d_tape_lens, int32_t* d_doc_errors,
                            const Stage1Result* dev_count, const UnescapeResult* dev_strings, WalkResult* d_res,
                            hipStream_t stream, void* d_chunk_ws = nullptr, uint64_t count_bound = 0, void* d_deep_ws = nullptr,
                            unsigned long long* d_single_tape_offsets = nullptr, uint64_t tape_capacity = 0, bool header_zeroed = false,
                            const SingleDocTail& tail = SingleDocTail());
// nesting levels 64 .. 1023 of the wave-per-document walker live in global memory: bytes for a batch of n_docs documents
size_t coop_deep_workspace_bytes(uint64_t n_docs);
// workspace of the chunk-parallel path for one large document (coop_walk.hip)
size_t coop_chunk_workspace_bytes(uint64_t count_bound);
hipError_t single_doc_setup_launch(const Stage1Result* d_res, uint64_t len, unsigned long long* d_doc_offsets,
                                   unsigned long long* d_index_offsets, uint32_t* d_doc_status, unsigned long long* d_doc_str_offsets,
                                   hipStream_t stream, WalkResult* d_walk_result = nullptr, void* d_slow_header = nullptr);
// the 64 bytes at the head of the walk workspace's literal list (count + the chunk path's flags): walk_launch zeroes them unless
// the caller did (results_zeroed: single_doc_setup_launch on the latency path, together with *d_res)
void* walk_slow_header(void* d_ws, uint64_t count, uint64_t n_docs);
hipError_t batch_isolated_launch(const uint8_t* d_buf, const unsigned long long* d_doc_offsets, uint64_t n_docs, uint32_t* d_out,
                                 uint64_t out_cap, unsigned long long* d_index_offsets, uint32_t* d_doc_status,
                                 uint32_t* d_counts, Stage1Result* d_res, hipStream_t stream, uint64_t total_len, const uint32_t* d_skip = nullptr);
// the same in two halves (round 6): the VERDICTS only (doc_status[k], counts[k], their OR in batch_status_or(d_counts, n_docs)) --
// all the repair pass needs -- and the rest (index offsets + the indexes of the passing documents)
hipError_t batch_verdicts_launch(const uint8_t* d_buf, const unsigned long long* d_doc_offsets, uint64_t n_docs, uint32_t* d_doc_status,
                                 uint32_t* d_counts, hipStream_t stream, uint64_t total_len, const uint32_t* d_skip, uint8_t* d_copy);
// (d_copy != nullptr: the sanitized copy for the repair pass made on the way -- the documents' own bytes, a failing document blank)
hipError_t batch_indexes_launch(const uint8_t* d_buf, const unsigned long long* d_doc_offsets, uint64_t n_docs, uint32_t* d_out,
                                uint64_t out_cap, unsigned long long* d_index_offsets, uint32_t* d_doc_status, uint32_t* d_counts,
                                Stage1Result* d_res, hipStream_t stream, uint64_t total_len, const uint32_t* d_skip);
const uint32_t* batch_status_or(const uint32_t* d_counts, uint64_t n_docs);
// the optimistic plain pass of the fused batch pipeline (batch.hip)
hipError_t batch_plain_check_launch(const uint8_t* d_buf, const unsigned long long* d_doc_offsets, uint64_t n_docs, uint64_t total_len,
                                    uint32_t* d_flags, hipStream_t stream);
hipError_t batch_plain_accept_launch(const uint32_t* d_idx, const Stage1Result* d_res, const unsigned long long* d_doc_offsets,
                                     uint64_t n_docs, unsigned long long* d_index_offsets, uint32_t* d_doc_status, uint32_t* d_flags,
                                     hipStream_t stream, const Stage1Prefixes& hint = Stage1Prefixes(), bool split = true);
// masks.hip: the reference's six per-block masks (6 x u64 per block, len / 64 + 1 blocks)
size_t masks_workspace_bytes(uint64_t len);
hipError_t masks_launch(const uint8_t* d_buf, uint64_t len, unsigned long long* d_masks, void* d_ws, hipStream_t stream);
hipError_t transpose_selftest_launch(const uint32_t* d_words, uint32_t nblocks, uint32_t* d_mismatches,
                                     hipStream_t stream);

// workgroups of 256 threads of KERNEL that are resident at the same time on the current device (the grid of a persistent
// launch), cached per device and per kernel (contexts on several host threads may get here together)
template <auto KERNEL>
inline hipError_t resident_workgroups(unsigned* out) {
    static std::atomic<unsigned> cached[16];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool cacheable = dev >= 0 && dev < 16;
    if (cacheable && (*out = cached[dev].load(std::memory_order_relaxed)) != 0) return hipSuccess;
    int per_cu = 0, cus = 0;
    if ((e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL, 256, 0)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    *out = (unsigned)(per_cu > 0 ? per_cu : 1) * (unsigned)(cus > 0 ? cus : 1);
    if (cacheable) cached[dev].store(*out, std::memory_order_relaxed);
    return hipSuccess;
}

// ---- the selector (select.hip) ----
// a compiled plan as the kernel reads it (host memory owned by the plan), its size, the plan's serial number and its paths
const void* select_plan_image(const sjmi_select_plan* plan, size_t* bytes, uint64_t* serial, uint32_t* n_paths);
// k_select over a parsed batch with the plan image at d_plan; columns types[p * n_docs + k] / values[p * n_docs + k]
hipError_t select_launch(const void* d_plan, size_t plan_bytes, const void* d_tape, const void* d_tape_offsets, const void* d_doc_errors,
                         const void* d_string_buffer, uint64_t n_docs, void* d_types, void* d_values, hipStream_t stream);

// ---- explode (explode.hip) ----
// a compiled plan as the kernels read it: [the base pointer as a plan of one path: base_bytes][the element plan], the plan's
// serial number, the columns of a row (the paths of the element plan, and a members plan's key) and whether it is a members plan
const void* explode_plan_image(const sjmi_explode_plan* plan, size_t* bytes, size_t* base_bytes, uint64_t* serial, uint32_t* n_cols,
                               bool* members);
// per-document scratch of one call: row counts, base tape indexes, the scan's chunk sums
size_t explode_workspace_bytes(uint64_t n_docs);
// k_explode_count, the scan into d_row_offsets[n_docs + 1], and (row_capacity != 0, n_cols != 0) k_explode_rows into the columns
// types[p * row_capacity + r] / values[p * row_capacity + r]; `members` picks the kernels' instantiation
hipError_t explode_launch(const void* d_plan, size_t plan_bytes, size_t base_bytes, uint32_t n_cols, bool members, const void* d_tape,
                          const void* d_tape_offsets, const void* d_doc_errors, const void* d_string_buffer, uint64_t n_docs, void* d_ws,
                          void* d_row_offsets, uint64_t row_capacity, void* d_types, void* d_values, hipStream_t stream);

// ---- NDJSON document offsets (ndjson.hip) ----
uint64_t ndjson_tile_bytes();
// per-tile scratch of one call over len bytes: a state and a count per tile
size_t ndjson_workspace_bytes(uint64_t len);
// k_ndjson_summary, k_ndjson_scan (the sjmi_ndjson_result at d_result, doc_offsets[0] and [n_docs]) and, with offset_capacity > 1,
// k_ndjson_emit (doc_offsets[1 ..] below the capacity); d_buf of any alignment
hipError_t ndjson_launch(const void* d_buf, uint64_t len, void* d_doc_offsets, uint64_t offset_capacity, void* d_result, void* d_ws,
                         hipStream_t stream);

// ---- a string column as Arrow offsets, validity and bytes (strcol.hip) ----
// scratch of one call over n_rows rows: three sums per chunk
size_t strcol_workspace_bytes(uint64_t n_rows);
// k_strcol_chunk_sums (d_validity, may be NULL), k_strcol_chunk_scan (d_offsets[n_rows], the sjmi_strcol_result at d_result),
// k_strcol_offsets and, with byte_capacity != 0, k_strcol_copy (the bytes below the capacity); d_types and d_bytes of any alignment
hipError_t strcol_launch(const void* d_types, const void* d_values, uint64_t n_rows, const void* d_string_buffer, void* d_offsets,
                         void* d_validity, void* d_bytes, uint64_t byte_capacity, void* d_result, void* d_ws, hipStream_t stream);

// ---- a row filter over typed columns (filter.hip) ----
// -1: a term looks at a column >= n_cols; else 1 when the plan has a STRING term, 0 when it has none
int filter_plan_columns(const sjmi_filter_plan* plan, uint64_t n_cols);
// scratch of one call over n_rows rows: a count per chunk and the keep words
size_t filter_workspace_bytes(uint64_t n_rows);
// k_filter_eval (the keep words into d_keep, or into the scratch without one), k_filter_scan (the sjmi_filter_result at d_result)
// and, with out_capacity != 0, k_filter_emit (d_rows and the compacted columns below the capacity); the plan goes by value
hipError_t filter_launch(const sjmi_filter_plan* plan, const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride,
                         uint64_t n_rows, const void* d_string_buffer, void* d_keep, void* d_rows, uint64_t out_capacity, void* d_out_types,
                         void* d_out_values, void* d_result, void* d_ws, hipStream_t stream);

// ---- fixed-width Arrow columns: int64 / float64 / bool (arrowcol.hip) and timestamps of RFC 3339 strings (timecol.hip) ----
// Two operators in one frame (sj_fieldcol.h, fieldcol_launch.h): <op> is arrowcol or timecol.
constexpr size_t FIELDCOL_PLAN_BYTES = 16 + 64 * 16;  // sizeof(FcPlan): the validated fields, a launch argument
struct FieldColArgs {  // the device pointers and strides of one call, as the entry points of include/sjmi.h name them
    const void *d_types, *d_values;
    uint64_t col_stride, n_rows;
    const void *d_row_count, *d_string_buffer;  // d_row_count may be NULL: the kernels read it; d_string_buffer: timecol only
    void* d_data;
    uint64_t data_stride;
    void* d_validity;
    uint64_t validity_stride;
    void* d_results;
};
// the fields (sjmi_arrow_field / sjmi_time_field) validated into plan_out (FIELDCOL_PLAN_BYTES, 8-byte aligned): 0, or -2 for a
// schema the call refuses
int arrowcol_plan(const void* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out);
int timecol_plan(const void* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out);
// scratch of one call: one packed count word per field and chunk of 1024 (arrowcol) or 256 (timecol) rows
size_t arrowcol_workspace_bytes(uint64_t n_fields, uint64_t n_rows);
size_t timecol_workspace_bytes(uint64_t n_fields, uint64_t n_rows);
// the operator's convert kernel (n_rows != 0: data, validity, the chunk words) and the finish kernel (the record per field); the
// plan goes by value
hipError_t arrowcol_launch(const void* plan, const FieldColArgs& a, void* d_ws, hipStream_t stream);
hipError_t timecol_launch(const void* plan, const FieldColArgs& a, void* d_ws, hipStream_t stream);

// ---- a string column as an Arrow dictionary array (dictcol.hip) ----
// scratch of one call: the hash table for dict_capacity entries, a slot per row, two counts per chunk of 1024 rows, the compacted
// dictionary column and the string gather's sums over it
size_t dictcol_workspace_bytes(uint64_t n_rows, uint64_t dict_capacity);
// k_dict_clear, k_dict_insert (d_validity, may be NULL), k_dict_count, k_dict_scan (the sjmi_dict_result at d_result), k_dict_emit
// (d_dict_rows, may be NULL), k_dict_index and the string gather's four kernels over the dictionary (the copy with
// dict_byte_capacity != 0); n_rows == 0: the two scans only.  d_row_count (may be NULL) is read by the kernels
hipError_t dictcol_launch(const void* d_types, const void* d_values, uint64_t n_rows, const void* d_row_count, const void* d_string_buffer,
                          void* d_indices, void* d_validity, uint64_t dict_capacity, void* d_dict_rows, void* d_dict_offsets, void* d_dict_bytes,
                          uint64_t dict_byte_capacity, void* d_result, void* d_ws, hipStream_t stream);

// ---- the key census: rows per dictionary entry and value type (census.hip) ----
// k_census_clear (the counts, the sjmi_census_result at d_result) and, with n_rows != 0, k_census_lds (n_keys <=
// SJMI_CENSUS_LDS_KEYS) or k_census_global; no scratch.  d_validity and d_row_count may be NULL; d_row_count is read by the kernels
hipError_t census_launch(const void* d_indices, const void* d_validity, const void* d_types, uint64_t n_rows, const void* d_row_count,
                         uint64_t n_keys, void* d_counts, void* d_result, hipStream_t stream);

// ---- group statistics per dictionary key: count, sum, min, max (groupstats.hip) ----
// k_group_clear (the stats, the sjmi_group_result at d_result), with n_rows != 0 k_group_lds (n_keys <= SJMI_GROUP_LDS_KEYS) or
// k_group_global, and with n_keys != 0 k_group_finish; no scratch.  d_validity and d_row_count may be NULL; d_row_count is read by
// the kernels
hipError_t groupstats_launch(const void* d_indices, const void* d_validity, const void* d_types, const void* d_values, uint64_t n_rows,
                             const void* d_row_count, uint64_t n_keys, void* d_stats, void* d_result, hipStream_t stream);

// ---- the top k rows of a key column: ORDER BY a value, LIMIT k (toprows.hip) ----
// scratch of one call: the select's state, six histograms of 2048 bins, a word per chunk of 1024 rows, k (key, row) pairs
size_t toprows_workspace_bytes(uint64_t n_rows, uint64_t k);
// k_top_clear, with n_rows != 0 k_top_range, k_top_plan (the sjmi_top_result at d_result but for kth_bits) and, with n_rows != 0 and
// k != 0, six times k_top_hist + k_top_pick, then k_top_mark, k_top_scan, k_top_emit and k_top_sort (d_rows, the carried cells,
// kth_bits).  d_key_types, d_key_validity and d_row_count may be NULL; d_row_count is read by the kernels
hipError_t toprows_launch(const void* d_key_types, const void* d_key_validity, const void* d_key_values, uint64_t n_rows, const void* d_row_count,
                          uint32_t kind, uint32_t flags, uint64_t k, const void* d_types, const void* d_values, uint64_t n_cols,
                          uint64_t col_stride, void* d_rows, void* d_out_types, void* d_out_values, void* d_result, void* d_ws, hipStream_t stream);

// ---- all rows ordered by a key column: a stable radix sort (sortrows.hip) ----
// scratch of one call: the state, two words per chunk of 1024 positions, 256 words per tile of 4096 pairs, 256 totals, two buffers
// of n_rows (key, 32-bit position) pairs
size_t sortrows_workspace_bytes(uint64_t n_rows);
// k_sort_clear, with n_rows != 0 k_sort_range, k_sort_plan (the sjmi_sort_result at d_result) and, with n_rows != 0, k_sort_count,
// k_sort_scan, k_sort_emit, eight times k_sort_hist + k_sort_digit_scan + k_sort_scatter, and k_sort_gather (d_rows, the carried
// cells).  d_key_types, d_key_validity, d_rows_in and d_row_count may be NULL; d_row_count is read by the kernels
hipError_t sortrows_launch(const void* d_key_types, const void* d_key_validity, const void* d_key_values, uint64_t n_source_rows,
                           const void* d_rows_in, uint64_t n_rows, const void* d_row_count, uint32_t kind, uint32_t flags, const void* d_types,
                           const void* d_values, uint64_t n_cols, uint64_t col_stride, void* d_rows, void* d_out_types, void* d_out_values,
                           uint64_t out_stride, void* d_result, void* d_ws, hipStream_t stream);

// ---- the document of every exploded row, and that document's cells on the row (parents.hip) ----
// k_parent_clear (the sjmi_parent_result at d_result) and, with n_rows != 0, k_parent_dense (d_rows NULL) or k_parent_sparse; no
// scratch.  d_row_count, d_parent_types, d_parents and, with n_cols == 0, the column pointers may be NULL; d_row_count is read by
// the kernels
hipError_t parents_launch(const void* d_row_offsets, uint64_t n_docs, const void* d_rows, uint64_t n_rows, const void* d_row_count,
                          const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride, void* d_parent_types, void* d_parents,
                          void* d_out_types, void* d_out_values, uint64_t out_stride, void* d_result, hipStream_t stream);

// ---- two row sets joined on a long key: inner, left, semi, anti (joinrows.hip) ----
// scratch of one call: n_right build keys, a word per chunk of 1024 left positions, n_left + 1 pair offsets, n_left 32-bit lower
// bounds and n_left 32-bit pair counts
size_t joinrows_workspace_bytes(uint64_t n_left, uint64_t n_right);
// k_join_clear (the sjmi_join_result at d_result), with n_right != 0 k_join_keys, with n_left != 0 k_join_count, k_join_scan and
// k_join_offsets, and with n_left != 0 and pair_capacity != 0 k_join_emit.  The sides are host structs; d_left_rows_in, d_left_count,
// d_right_rows (SEMI, ANTI) and d_pair_offsets may be NULL; d_left_count and the n_candidates of d_right_sort_result are read by
// the kernels
hipError_t joinrows_launch(const sjmi_join_side& left, const void* d_left_rows_in, uint64_t n_left, const void* d_left_count,
                           const sjmi_join_side& right, const void* d_right_order, uint64_t n_right, const void* d_right_sort_result,
                           uint32_t how, uint64_t pair_capacity, void* d_left_rows, void* d_right_rows, void* d_left_out_types,
                           void* d_left_out_values, void* d_right_out_types, void* d_right_out_values, uint64_t out_stride,
                           void* d_pair_offsets, void* d_result, void* d_ws, hipStream_t stream);

}  // namespace sjmi
