// Host simulation of the group statistics (simdjson-java_amd/csrc/groupstats.hip): sj_groupstats.h, the header the kernels compile
// verbatim, with the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the members the passes ask
// for -- on the device LDS atomics, agent-scope atomics, a barrier and the combine of a wave's equal keys; here plain operations on
// the word, nothing, and a lane that adds for itself).  TEST ONLY: lets the CPU suite check the clear, the LDS path (every group of
// the capped grid with bins of its own), the global path and the finish against the Python reference without a GPU.  The groups
// (LDS path) or chunks (global path) run in the caller's order: 0 ascending, 1 descending, 2 the odd ones first -- only sum_double
// may depend on it, and not where every partial sum is exact.  Built by tests/test_host_groupstats.py with g++;
// tests/host_sim/groupstats_asan_main.cpp includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_groupstats.h"
#include "seq_group.h"

struct GsSeqOps {  // (a double is added through copies of the word's bytes: the word stays a uint64 for everybody else)
    void add32(uint32_t* p, uint32_t n) const { *p += n; }
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
    void addf(sj_u64* p, double x) const { *p = gs_bits(gs_double(*p) + x); }
    void smin(sj_u64* p, sj_i64 v) const { if (v < (sj_i64)*p) *p = (sj_u64)v; }
    void smax(sj_u64* p, sj_i64 v) const { if (v > (sj_i64)*p) *p = (sj_u64)v; }
    void umin(sj_u64* p, sj_u64 v) const { if (v < *p) *p = v; }
    void umax(sj_u64* p, sj_u64 v) const { if (v > *p) *p = v; }
};

struct GsSeq : SeqGroup {
    GsSeqOps wg, agent;
    void sync() const {}
    bool merge(uint32_t, bool active, GsCell*) const { return active; }  // (one lane: nobody to combine with)
};

static std::vector<sj_u64> gs_order(sj_u64 n, uint32_t order) {
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

// groupstats_launch's schedule.  grid_cap: 0 = gs_lds_grid's own, else a smaller cap (more chunks per group)
static void gs_sim_passes(const GsColumn& c, uint32_t order, uint32_t grid_cap, sj_u64* stats, GsResult* res) {
    const GsSeq g;
    const sj_u64 words = c.n_keys * GS_WORDS;
    for (sj_u64 i : gs_order(words ? words : 1, order)) gs_clear_word(c, i, stats, res);
    const sj_u64 nchunks = gs_chunks(c.n_rows, c.chunk_rows);
    if (nchunks && c.n_keys <= GS_LDS_KEYS) {
        uint32_t grid = gs_lds_grid(c.n_rows, c.n_keys, c.chunk_rows);
        if (grid_cap && grid > grid_cap) grid = grid_cap;
        for (sj_u64 group : gs_order(grid, order)) {
            // (a group's own bins, exactly their size, not cleared at first: the 64-bit words, the counts behind them)
            uint8_t* bins = (uint8_t*)malloc(c.n_keys ? c.n_keys * GS_BIN_BYTES : 1);
            memset(bins, 0xA5, c.n_keys * GS_BIN_BYTES);
            gs_lds_rows(g, c, group, grid, (sj_u64*)bins, (uint32_t*)(bins + c.n_keys * GS_BIN_WORDS * 8), stats, res);
            free(bins);
        }
    } else if (nchunks) {
        for (sj_u64 chunk : gs_order(nchunks, order)) gs_global_rows(g, c, chunk, stats, res);
    }
    for (sj_u64 k : gs_order(c.n_keys, order)) gs_finish_key(c, k, stats);
}

extern "C" uint32_t sim_group_lds_keys(void) { return GS_LDS_KEYS; }
extern "C" uint32_t sim_group_chunk_rows(void) { return GS_CHUNK_ROWS; }
extern "C" uint32_t sim_group_grid(uint64_t n_rows, uint64_t n_keys) { return gs_lds_grid(n_rows, n_keys, GS_CHUNK_ROWS); }
extern "C" uint64_t sim_group_okey(uint64_t bits) { return gs_okey(bits); }
extern "C" uint64_t sim_group_okey_bits(uint64_t key) { return gs_okey_bits(key); }

// the call as sjmi_group_stats_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows 0 = the
// kernels' 1024.  row_count: NULL or one uint64.  result: 5 x uint64 (flags in the low half of the fifth).
extern "C" int sim_group_stats(const int32_t* indices, const uint64_t* validity, const uint8_t* types, const uint64_t* values, uint64_t n_rows,
                               const uint64_t* row_count, uint64_t n_keys, uint32_t chunk_rows, uint32_t order, uint32_t grid_cap, uint64_t* stats,
                               uint64_t* result) {
    if (!result || (n_rows && (!indices || !types || !values)) || (n_keys && !stats)) return -2;
    if (n_keys > (1u << 20) || n_rows >= (1ull << 32)) return -2;
    if (((uintptr_t)indices & 3) || ((uintptr_t)validity & 7) || ((uintptr_t)values & 7) || ((uintptr_t)row_count & 7) || ((uintptr_t)stats & 7) ||
        ((uintptr_t)result & 7))
        return -2;
    const GsColumn c = {indices, (const sj_u64*)validity, types, (const sj_u64*)values, n_rows, (const sj_u64*)row_count, n_keys,
                        chunk_rows ? chunk_rows : GS_CHUNK_ROWS};
    gs_sim_passes(c, order, grid_cap, (sj_u64*)stats, (GsResult*)result);
    return 0;
}
