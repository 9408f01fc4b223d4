// Host simulation of the parent columns (simdjson-java_amd/csrc/parents.hip): sj_parents.h, the header the kernels compile
// verbatim, with the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the members the passes ask
// for -- on the device an agent-scope atomic, a barrier and a running maximum over the workgroup; here a plain add, nothing, and
// the lane's own value).  TEST ONLY: lets the CPU suite check both forms against the numpy reference without a GPU.  The chunks
// run in the caller's order: 0 ascending, 1 descending, 2 the odd ones first -- nothing may depend on it.  A chunk's marks and
// seeds are heap blocks of exactly their size, not cleared.  With guard != 0 the row offsets, the rows, the document columns and
// every output END at an unreadable page.  Built by tests/test_host_parents.py with g++; tests/host_sim/parents_asan_main.cpp
// includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_parents.h"
#include "seq_group.h"

struct PaSeqOps {
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
};

struct PaSeq : SeqGroup {
    PaSeqOps agent;
    void sync() const {}
    sj_u64 scan_max(sj_u64 v, sj_u64* total) const {  // (one lane)
        *total = v;
        return v;
    }
};

static std::vector<sj_u64> pa_order(sj_u64 n, uint32_t order) {
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

// parents_launch's schedule
static void pa_sim_passes(const PaArgs& a, uint32_t order, PaResult* res) {
    const PaSeq g;
    pa_clear(a, res);
    for (sj_u64 chunk : pa_order(pa_chunks(a), order)) {
        if (a.rows) {
            pa_sparse(g, a, chunk, res);
            continue;
        }
        sj_u64* marks = (sj_u64*)malloc((size_t)a.chunk_rows * 8);
        sj_u64* seeds = (sj_u64*)malloc(2 * 8);
        memset(marks, 0xA5, (size_t)a.chunk_rows * 8);
        memset(seeds, 0xA5, 2 * 8);
        pa_dense(g, a, chunk, marks, seeds, res);
        free(marks);
        free(seeds);
    }
}

extern "C" uint32_t sim_parent_chunk_rows(void) { return PA_CHUNK_ROWS; }
extern "C" uint32_t sim_parent_max_cols(void) { return PA_MAX_COLS; }
extern "C" uint64_t sim_parent_count_wave(const uint64_t* off, uint64_t n_docs, uint64_t x) {
    return pa_count_wave(PaSeq(), (const sj_u64*)off, n_docs, x);
}
extern "C" uint64_t sim_parent_count_lane(const uint64_t* off, uint64_t n_docs, uint64_t x) { return pa_count_lane((const sj_u64*)off, n_docs, x); }

// the extent of a column set that the call may touch: cells [0, used) of n_cols columns `stride` apart
static size_t pa_extent(uint64_t n_cols, uint64_t stride, uint64_t used) { return n_cols ? (size_t)((n_cols - 1) * stride + used) : 0; }

// the call as sjmi_parent_columns_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows 0 =
// the kernels' 1024.  row_count: NULL or one uint64.  result: 3 x uint64 (flags in the low half of the third).
extern "C" int sim_parent_columns(const uint64_t* row_offsets, uint64_t n_docs, const uint64_t* rows, uint64_t n_rows, const uint64_t* row_count,
                                  const uint8_t* types, const uint64_t* values, uint64_t n_cols, uint64_t col_stride, uint8_t* parent_types,
                                  uint64_t* parents, uint8_t* out_types, uint64_t* out_values, uint64_t out_stride, uint64_t* result,
                                  uint32_t chunk_rows, uint32_t order, uint32_t guard) {
    if (!row_offsets || !result || n_cols > PA_MAX_COLS) return -2;
    if (n_rows >= (1ull << 32) || n_docs >= (1ull << 32)) return -2;
    if (n_cols && (!types || !values || !out_types || !out_values || col_stride < n_docs || out_stride < n_rows)) return -2;
    if (((uintptr_t)row_offsets & 7) || ((uintptr_t)rows & 7) || ((uintptr_t)row_count & 7) || ((uintptr_t)values & 7) || ((uintptr_t)parents & 7) ||
        ((uintptr_t)out_values & 7) || ((uintptr_t)result & 7))
        return -2;
    PaArgs a = {(const sj_u64*)row_offsets, n_docs, (const sj_u64*)rows, n_rows, (const sj_u64*)row_count, types, (const sj_u64*)values, n_cols,
                col_stride, parent_types, (sj_u64*)parents, out_types, (sj_u64*)out_values, out_stride, chunk_rows ? chunk_rows : PA_CHUNK_ROWS};
    if (!guard) {
        pa_sim_passes(a, order, (PaResult*)result);
        return 0;
    }
    // every block ends at an unreadable page; the outputs keep what the caller put there and are copied back
    const size_t in_cells = pa_extent(n_cols, col_stride, n_docs), out_cells = pa_extent(n_cols, out_stride, n_rows);
    Guarded g_off, g_rows, g_t, g_v, g_pt, g_p, g_ot, g_ov;
    if (!g_off.open((n_docs + 1) * 8) || !g_rows.open(n_rows * 8) || !g_t.open(in_cells) || !g_v.open(in_cells * 8) || !g_pt.open(n_rows) ||
        !g_p.open(n_rows * 8) || !g_ot.open(out_cells) || !g_ov.open(out_cells * 8))
        return -1;
    a.row_offsets = (const sj_u64*)g_off.place(row_offsets, (n_docs + 1) * 8);
    if (rows) a.rows = (const sj_u64*)g_rows.place(rows, n_rows * 8);
    if (n_cols) {
        a.types = g_t.place(types, in_cells);
        a.values = (const sj_u64*)g_v.place(values, in_cells * 8);
        a.out_types = g_ot.place(out_types, out_cells);
        a.out_values = (sj_u64*)g_ov.place(out_values, out_cells * 8);
    }
    if (parent_types) a.parent_types = g_pt.place(parent_types, n_rows);
    if (parents) a.parents = (sj_u64*)g_p.place(parents, n_rows * 8);
    pa_sim_passes(a, order, (PaResult*)result);
    if (n_cols && out_cells) memcpy(out_types, a.out_types, out_cells), memcpy(out_values, a.out_values, out_cells * 8);
    if (parent_types && n_rows) memcpy(parent_types, a.parent_types, n_rows);
    if (parents && n_rows) memcpy(parents, a.parents, n_rows * 8);
    return 0;
}
