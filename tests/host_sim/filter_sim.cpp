// Host simulation of the row filter (simdjson-java_amd/csrc/filter.hip): sj_filter.h, the header the kernels compile verbatim,
// with the lane primitives in their sequential form (seq_group.h) -- ONE wave per chunk whose 64 lanes run one after the other (a ballot
// collects their answers, every scan is empty and every total the wave's own value).
// TEST ONLY: lets the CPU suite check the three passes against the reference of tests/filter_common.py without a GPU, at any
// chunk size.  The string buffer is placed so that it ENDS at a page that cannot be read: one use of a value word that is no
// string's as an offset, or one byte read behind a string that ends the buffer, is a SIGSEGV here and not a fault on a GPU.
// Built by tests/test_host_filter.py with g++.
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_filter.h"
#include "seq_group.h"

extern "C" {

uint32_t sim_filter_chunk_rows() { return FL_CHUNK_ROWS; }

// n_terms terms (sjmi_filter_term) with their constants in bytes[0, n_bytes); n_cols columns types (any alignment) / values
// strided by col_stride, n_rows rows of them; the string buffer sb[0, sb_len) (copied against a guard page); chunk_rows a
// multiple of 64.  keep: (n_rows + 63) / 64 words or NULL; rows / out_types / out_values: out_capacity entries (times n_cols),
// all three or none (NULL with 0: the sizing call) -- each with whatever canaries the caller put behind it.  result = {n_kept,
// flags}.  -> 0, -2 for a bad argument or a plan that does not compile, -3 without memory
int sim_filter(const void* terms, uint64_t n_terms, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* types, const uint64_t* values,
               uint64_t n_cols, uint64_t col_stride, uint64_t n_rows, const uint8_t* sb, uint64_t sb_len, uint32_t chunk_rows, uint64_t* keep,
               uint64_t* rows, uint64_t out_capacity, uint8_t* out_types, uint64_t* out_values, uint64_t* result) {
    if (!chunk_rows || chunk_rows % 64 || !result || col_stride < n_rows || (out_capacity && (!rows || !out_types || !out_values))) return -2;
    FlPlan plan;
    if (fl_plan_compile((const FlTerm*)terms, n_terms, bytes, n_bytes, &plan) != 0) return -2;
    for (uint32_t k = 0; k < plan.n_terms; ++k)
        if (plan.terms[k].column >= n_cols) return -2;
    Guarded gs;
    if (!gs.open(sb_len ? sb_len : 1)) return -3;
    const FlCols c = {types, (const sj_u64*)values, n_cols, col_stride, n_rows, gs.place(sb, sb_len), chunk_rows};
    const sj_u64 nchunks = fl_chunks(c);
    std::vector<sj_u64> ws(nchunks + fl_words(c) + 1, 0xA5A5A5A5A5A5A5A5ull);  // (the scratch is not zero on the device either)
    sj_u64* counts = ws.data();
    sj_u64* words = keep ? (sj_u64*)keep : counts + nchunks;
    const SeqGroup g;
    for (sj_u64 k = 0; k < nchunks; ++k) fl_eval_chunk(g, plan, c, k, words, counts);
    FlResult res;
    fl_chunk_scan(g, counts, nchunks, out_capacity, &res);
    if (nchunks && out_capacity) {
        const FlOut o = {(sj_u64*)rows, out_types, (sj_u64*)out_values, out_capacity};
        for (sj_u64 k = 0; k < nchunks; ++k) fl_emit_chunk(g, c, k, words, counts, o);
    }
    result[0] = res.n_kept;
    result[1] = ((uint64_t)res.reserved << 32) | res.flags;
    return 0;
}

}  // extern "C"
