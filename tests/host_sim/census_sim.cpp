// Host simulation of the key census (simdjson-java_amd/csrc/census.hip): sj_census.h, the header the kernels compile verbatim, with
// the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the three members the passes ask for --
// on the device an LDS atomic, an agent-scope atomic add, a barrier and the merge of a wave's equal bins; here plain adds, nothing,
// and a lane that adds for itself).  TEST ONLY: lets the CPU
// suite check the clear, the LDS path (every group of the capped grid with bins of its own) and the global path against a Python
// Counter without a GPU.  The groups (LDS path) or chunks (global path) run in the caller's order: 0 ascending, 1 descending,
// 2 the odd ones first -- the sums do not depend on it.  Built by tests/test_host_census.py with g++;
// tests/host_sim/census_asan_main.cpp includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_census.h"
#include "seq_group.h"

struct CsSeq : SeqGroup {
    void bin_add(uint32_t* p) const { ++*p; }
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
    void sync() const {}
    uint32_t merge(uint32_t, bool active) const { return active ? 1u : 0u; }  // (one lane: nobody to merge with)
};

static std::vector<sj_u64> cs_order(sj_u64 n, uint32_t order) {
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

// census_launch's schedule.  grid_cap: 0 = cs_lds_grid's own, else a smaller cap (more chunks per group)
static void cs_sim_passes(const CsColumn& c, uint32_t order, uint32_t grid_cap, sj_u64* counts, CsResult* res) {
    const CsSeq g;
    const sj_u64 words = c.n_keys * CS_CLASSES;
    for (sj_u64 i : cs_order(words ? words : 1, order)) cs_clear_word(c, i, counts, res);
    const sj_u64 nchunks = cs_chunks(c.n_rows, c.chunk_rows);
    if (!nchunks) return;
    if (c.n_keys <= CS_LDS_KEYS) {
        uint32_t grid = cs_lds_grid(c.n_rows, c.n_keys, c.chunk_rows);
        if (grid_cap && grid > grid_cap) grid = grid_cap;
        for (sj_u64 group : cs_order(grid, order)) {
            uint32_t* bins = (uint32_t*)malloc(words ? words * 4 : 1);  // (a group's own, exactly its size, not zero at first)
            memset(bins, 0xA5, words * 4);
            cs_lds_rows(g, c, group, grid, bins, counts, res);
            free(bins);
        }
    } else {
        for (sj_u64 chunk : cs_order(nchunks, order)) cs_global_rows(g, c, chunk, counts, res);
    }
}

extern "C" uint32_t sim_census_lds_keys(void) { return CS_LDS_KEYS; }
extern "C" uint32_t sim_census_chunk_rows(void) { return CS_CHUNK_ROWS; }
extern "C" uint32_t sim_census_class(uint32_t type) { return cs_class((uint8_t)type); }
extern "C" uint32_t sim_census_grid(uint64_t n_rows, uint64_t n_keys) { return cs_lds_grid(n_rows, n_keys, CS_CHUNK_ROWS); }

// the call as sjmi_key_census_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows 0 = the
// kernels' 1024.  row_count: NULL or one uint64.  result: 4 x uint64 (flags in the low half of the fourth).
extern "C" int sim_census(const int32_t* indices, const uint64_t* validity, const uint8_t* types, uint64_t n_rows, const uint64_t* row_count,
                          uint64_t n_keys, uint32_t chunk_rows, uint32_t order, uint32_t grid_cap, uint64_t* counts, uint64_t* result) {
    if (!result || (n_rows && (!indices || !types)) || (n_keys && !counts)) return -2;
    if (n_keys > (1u << 20) || n_rows >= (1ull << 40)) return -2;
    if (((uintptr_t)indices & 3) || ((uintptr_t)validity & 7) || ((uintptr_t)row_count & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)result & 7)) return -2;
    const CsColumn c = {indices, (const sj_u64*)validity, types, n_rows, (const sj_u64*)row_count, n_keys, chunk_rows ? chunk_rows : CS_CHUNK_ROWS};
    cs_sim_passes(c, order, grid_cap, (sj_u64*)counts, (CsResult*)result);
    return 0;
}
