// Host simulation of the top rows (simdjson-java_amd/csrc/toprows.hip): sj_toprows.h, the header the kernels compile verbatim,
// with the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the members the passes ask for -- on
// the device LDS atomics, agent-scope atomics, a barrier and a minimum / maximum over the workgroup; here plain operations on the
// word, nothing, and the lane's own value).  TEST ONLY: lets the CPU suite check every pass against the Python reference without
// a GPU.  The groups of the capped grids and the chunks run in the caller's order: 0 ascending, 1 descending, 2 the odd ones
// first -- nothing may depend on it.  The scratch, a group's bins and the sort's keys and rows are heap blocks of exactly their
// size, not cleared.  Built by tests/test_host_toprows.py with g++; tests/host_sim/toprows_asan_main.cpp includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_toprows.h"
#include "seq_group.h"

struct TrSeqOps {
    void add32(uint32_t* p, uint32_t n) const { *p += n; }
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
    void umin(sj_u64* p, sj_u64 v) const { if (v < *p) *p = v; }
    void umax(sj_u64* p, sj_u64 v) const { if (v > *p) *p = v; }
};

struct TrSeq : SeqGroup {
    TrSeqOps wg, agent;
    void sync() const {}
    sj_u64 all_umin(sj_u64 v) const { return v; }  // (one lane)
    sj_u64 all_umax(sj_u64 v) const { return v; }
};

static std::vector<sj_u64> tr_order(sj_u64 n, uint32_t order) {
    std::vector<sj_u64> o;
    if (order == 0)
        for (sj_u64 i = 0; i < n; ++i) o.push_back(i);
    else if (order == 1)
        for (sj_u64 i = n; i-- > 0;) o.push_back(i);
    else {
        for (sj_u64 i = 1; i < n; i += 2) o.push_back(i);
        for (sj_u64 i = 0; i < n; i += 2) o.push_back(i);
    }
    return o;
}

// toprows_launch's schedule.  grid_cap: 0 = tr_grid's own, else a smaller cap (more chunks per group).  digits_seen: where the
// plan's number of digits goes (may be NULL)
static void tr_sim_passes(const TrColumn& c, const TrCarry& in, const TrOut& o, uint32_t order, uint32_t grid_cap, TrResult* res,
                          uint32_t* digits_seen) {
    const TrSeq g;
    const sj_u64 words = tr_workspace_words(c.n_rows, c.k, c.chunk_rows);
    sj_u64* ws = (sj_u64*)malloc(words * 8);
    memset(ws, 0xA5, words * 8);
    for (sj_u64 i : tr_order(TR_STATE_WORDS + TR_HIST_WORDS, order)) tr_clear_word(c, i, ws, res);
    const sj_u64 nchunks = tr_chunks(c.n_rows, c.chunk_rows);
    uint32_t grid = tr_grid(c.n_rows, c.chunk_rows);
    if (grid_cap && grid > grid_cap) grid = grid_cap;
    if (nchunks)
        for (sj_u64 group : tr_order(grid, order)) tr_range(g, c, group, grid, ws, res);
    tr_plan(c, ws, res);
    if (digits_seen) *digits_seen = tr_state(ws)->n_digits;
    if (nchunks && c.k) {
        for (uint32_t d = 0; d < TR_MAX_DIGITS; ++d) {
            for (sj_u64 group : tr_order(grid, order)) {
                uint32_t* bins = (uint32_t*)malloc(TR_BINS * 4);
                memset(bins, 0xA5, TR_BINS * 4);
                tr_hist(g, c, d, group, grid, ws, bins);
                free(bins);
            }
            tr_pick(g, d, ws);
        }
        for (sj_u64 chunk : tr_order(nchunks, order)) tr_mark(g, c, chunk, ws);
        tr_scan(g, c, ws);
        for (sj_u64 chunk : tr_order(nchunks, order)) tr_emit(g, c, chunk, ws);
        sj_u64* s_key = (sj_u64*)malloc(TR_MAX_K * 8);
        uint32_t* s_row = (uint32_t*)malloc(TR_MAX_K * 4);
        memset(s_key, 0xA5, TR_MAX_K * 8);
        memset(s_row, 0xA5, TR_MAX_K * 4);
        tr_sort(g, c, in, ws, s_key, s_row, o, res);
        free(s_key);
        free(s_row);
    }
    free(ws);
}

extern "C" uint32_t sim_top_max_k(void) { return TR_MAX_K; }
extern "C" uint32_t sim_top_chunk_rows(void) { return TR_CHUNK_ROWS; }
extern "C" uint32_t sim_top_grid(uint64_t n_rows) { return tr_grid(n_rows, TR_CHUNK_ROWS); }
extern "C" uint64_t sim_top_workspace_words(uint64_t n_rows, uint64_t k) { return tr_workspace_words(n_rows, k, TR_CHUNK_ROWS); }

// the call as sjmi_top_rows_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows 0 = the
// kernels' 1024.  row_count: NULL or one uint64.  result: 9 x uint64 (flags in the low half of the ninth).
extern "C" int sim_top_rows(const uint8_t* key_types, const uint64_t* key_validity, const uint64_t* key_values, uint64_t n_rows,
                            const uint64_t* row_count, uint32_t kind, uint32_t flags, uint64_t k, const uint8_t* types, const uint64_t* values,
                            uint64_t n_cols, uint64_t col_stride, uint64_t* rows, uint8_t* out_types, uint64_t* out_values, uint64_t* result,
                            uint32_t chunk_rows, uint32_t order, uint32_t grid_cap, uint32_t* digits_seen) {
    if (!result || (n_rows && !key_values) || (k && !rows)) return -2;
    if ((kind != TR_LONG && kind != TR_DOUBLE) || (flags & ~TR_SMALLEST) || k > TR_MAX_K) return -2;
    if (n_rows >= (1ull << 32)) return -2;
    if (n_cols && (col_stride < n_rows || (k && (!types || !values || !out_types || !out_values)))) return -2;
    if (((uintptr_t)key_validity & 7) || ((uintptr_t)key_values & 7) || ((uintptr_t)row_count & 7) || ((uintptr_t)values & 7) ||
        ((uintptr_t)rows & 7) || ((uintptr_t)out_values & 7) || ((uintptr_t)result & 7))
        return -2;
    const TrColumn c = {key_types, (const sj_u64*)key_validity, (const sj_u64*)key_values, n_rows, (const sj_u64*)row_count, kind, flags, k,
                        chunk_rows ? chunk_rows : TR_CHUNK_ROWS};
    const TrCarry in = {types, (const sj_u64*)values, n_cols, col_stride};
    const TrOut o = {(sj_u64*)rows, out_types, (sj_u64*)out_values};
    tr_sim_passes(c, in, o, order, grid_cap, (TrResult*)result, digits_seen);
    return 0;
}
