// Host simulation of the sort (simdjson-java_amd/csrc/sortrows.hip): sj_sortrows.h, the header the kernels compile verbatim, with
// the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the members the passes ask for -- on the
// device agent-scope atomics, a barrier, a wave's fence and a minimum / maximum over the workgroup; here plain operations on the
// word, nothing, and the lane's own value -- and a ballot over a wave of ONE lane: the passes ask every lane for its own answer).
// TEST ONLY: lets the CPU suite check every pass against the Python reference without a GPU.  The groups of the capped grid, the
// chunks, the tiles and the 256 groups of a digit's scan run in the caller's order: 0 ascending, 1 descending, 2 the odd ones first
// -- nothing may depend on it.  The scratch and a tile's counts, bases, starts and staged pairs are heap blocks of exactly their size, filled with 0xA5.
// Built by tests/test_host_sortrows.py with g++; tests/host_sim/sortrows_asan_main.cpp includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_sortrows.h"
#include "seq_group.h"

struct SrSeqOps {
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
    void umin(sj_u64* p, sj_u64 v) const { if (v < *p) *p = v; }
    void umax(sj_u64* p, sj_u64 v) const { if (v > *p) *p = v; }
};

struct SrSeq : SeqGroup {
    SrSeqOps agent;
    void sync() const {}
    void wave_fence() const {}
    sj_u64 all_umin(sj_u64 v) const { return v; }  // (one lane)
    sj_u64 all_umax(sj_u64 v) const { return v; }
    template <class F>
    sj_u64 ballot(F f) const {  // (a wave of one lane)
        return f(0) ? 1ull : 0ull;
    }
};

static std::vector<sj_u64> sr_order(sj_u64 n, uint32_t order) {
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

template <class T>
static T* sr_block(sj_u64 n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset(p, 0xA5, n * sizeof(T));
    return p;
}

// sortrows_launch's schedule.  grid_cap: 0 = sr_grid's own, else a smaller cap (more chunks per group)
static void sr_sim_passes(const SrColumn& c, const SrCarry& in, const SrOut& o, uint32_t order, uint32_t grid_cap, SrResult* res) {
    const SrSeq g;
    const sj_u64 words = sr_workspace_words(c.n_rows, c.chunk_rows, c.tile_rows);
    sj_u64* ws = sr_block<sj_u64>(words);
    for (sj_u64 i : sr_order(64, order)) sr_clear_word(c, i, ws, res);
    const sj_u64 nchunks = sr_chunks(c), ntiles = sr_tiles(c, c.n_rows);
    uint32_t grid = sr_grid(c.n_rows, c.chunk_rows);
    if (grid_cap && grid > grid_cap) grid = grid_cap;
    if (nchunks)
        for (sj_u64 group : sr_order(grid, order)) sr_range(g, c, group, grid, ws, res);
    sr_plan(ws, res);
    if (nchunks) {
        for (sj_u64 chunk : sr_order(nchunks, order)) sr_count(g, c, chunk, ws);
        sr_scan(g, c, ws);
        for (sj_u64 chunk : sr_order(nchunks, order)) sr_emit(g, c, chunk, ws);
        for (uint32_t d = 0; d < SR_MAX_DIGITS; ++d) {
            for (sj_u64 tile : sr_order(ntiles, order)) {
                uint32_t* count = sr_block<uint32_t>(g.waves() * SR_VALUES);
                sr_hist(g, c, d, tile, ws, count);
                free(count);
            }
            for (sj_u64 value : sr_order(SR_VALUES, order)) sr_digit_scan(g, c, d, (uint32_t)value, ws);
            for (sj_u64 tile : sr_order(ntiles, order)) {
                uint32_t* count = sr_block<uint32_t>(g.waves() * SR_VALUES);
                sj_u64* base = sr_block<sj_u64>(SR_VALUES);
                uint32_t* start = sr_block<uint32_t>(SR_VALUES);
                sj_u64* staged_key = sr_block<sj_u64>(c.tile_rows);
                uint32_t* staged_pos = sr_block<uint32_t>(c.tile_rows);
                sr_scatter(g, c, d, tile, ws, base, start, count, staged_key, staged_pos);
                free(count), free(base), free(start), free(staged_key), free(staged_pos);
            }
        }
        for (sj_u64 j : sr_order(c.n_rows, order)) sr_gather(c, in, j, ws, o);
    }
    free(ws);
}

extern "C" uint32_t sim_sort_chunk_rows(void) { return SR_CHUNK_ROWS; }
extern "C" uint32_t sim_sort_tile_rows(void) { return SR_TILE_ROWS; }
extern "C" uint64_t sim_sort_workspace_words(uint64_t n_rows) { return sr_workspace_words(n_rows, SR_CHUNK_ROWS, SR_TILE_ROWS); }

// the call as sjmi_sort_rows_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows / tile_rows
// 0 = the kernels' own.  row_count: NULL or one uint64.  result: 9 x uint64 (flags in the low half of the ninth).
extern "C" int sim_sort_rows(const uint8_t* key_types, const uint64_t* key_validity, const uint64_t* key_values, uint64_t n_source_rows,
                             const uint64_t* rows_in, uint64_t n_rows, const uint64_t* row_count, uint32_t kind, uint32_t flags,
                             const uint8_t* types, const uint64_t* values, uint64_t n_cols, uint64_t col_stride, uint64_t* rows,
                             uint8_t* out_types, uint64_t* out_values, uint64_t out_stride, uint64_t* result, uint32_t chunk_rows,
                             uint32_t tile_rows, uint32_t order, uint32_t grid_cap) {
    if (!result || (n_source_rows && n_rows && !key_values) || (n_rows && !rows)) return -2;
    if ((kind != SR_LONG && kind != SR_DOUBLE) || (flags & ~SR_DESCENDING)) return -2;
    if (n_rows >= (1ull << 32) || n_source_rows >= (1ull << 32)) return -2;
    if (!rows_in && n_rows > n_source_rows) return -2;
    if (n_cols && (col_stride < n_source_rows || out_stride < n_rows || (n_rows && (!types || !values || !out_types || !out_values)))) return -2;
    if (((uintptr_t)key_validity & 7) || ((uintptr_t)key_values & 7) || ((uintptr_t)rows_in & 7) || ((uintptr_t)row_count & 7) ||
        ((uintptr_t)values & 7) || ((uintptr_t)rows & 7) || ((uintptr_t)out_values & 7) || ((uintptr_t)result & 7))
        return -2;
    const SrColumn c = {key_types, (const sj_u64*)key_validity, (const sj_u64*)key_values, n_source_rows, (const sj_u64*)rows_in, n_rows,
                        (const sj_u64*)row_count, kind, flags, chunk_rows ? chunk_rows : SR_CHUNK_ROWS, tile_rows ? tile_rows : SR_TILE_ROWS};
    const SrCarry in = {types, (const sj_u64*)values, n_cols, col_stride};
    const SrOut o = {(sj_u64*)rows, out_types, (sj_u64*)out_values, out_stride};
    sr_sim_passes(c, in, o, order, grid_cap, (SrResult*)result);
    return 0;
}
