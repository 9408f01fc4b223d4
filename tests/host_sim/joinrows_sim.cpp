// Host simulation of the join (simdjson-java_amd/csrc/joinrows.hip): sj_joinrows.h, the header the kernels compile verbatim, with
// the workgroup in its sequential form (seq_group.h's SeqGroup, to which this file adds the members the passes ask for -- on the
// device agent-scope atomics, a barrier and a running maximum over the workgroup; here plain operations on the word, nothing, and
// the lane's own value).  TEST ONLY: lets the CPU suite check every pass against the Python reference without a GPU.  The chunks
// of build places, of left positions and of output pairs run in the caller's order: 0 ascending, 1 descending, 2 the odd ones
// first -- nothing may depend on it.  The scratch and a chunk's keys, flags, pivots, marks and seeds are heap blocks of exactly their
// size, filled with 0xA5.  Built by tests/test_host_joinrows.py with g++; tests/host_sim/joinrows_asan_main.cpp includes this file.
#include <stdlib.h>

#include <vector>
#include "../../simdjson-java_amd/csrc/sj_joinrows.h"
#include "seq_group.h"

struct JrSeqOps {
    void add64(sj_u64* p, sj_u64 v) const { *p += v; }
    void or32(uint32_t* p, uint32_t v) const { *p |= v; }
};

struct JrSeq : SeqGroup {
    JrSeqOps agent;
    void sync() const {}
    sj_u64 scan_max(sj_u64 v, sj_u64* total) const {  // (one lane)
        *total = v;
        return v;
    }
};

static std::vector<sj_u64> jr_order(sj_u64 n, uint32_t order) {
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
static T* jr_block(sj_u64 n) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    memset(p, 0xA5, n * sizeof(T));
    return p;
}

// joinrows_launch's schedule
static void jr_sim_passes(const JrArgs& a, uint32_t order, JrResult* res) {
    const JrSeq g;
    sj_u64* ws = jr_block<sj_u64>(jr_workspace_words(a.left.n_rows, a.right.n_rows, a.chunk_rows));
    const sj_u64 left_chunks = jr_chunks(a.left.n_rows, a.chunk_rows), build_chunks = jr_chunks(a.right.n_rows, a.chunk_rows),
                 pair_chunks = jr_chunks(a.pair_capacity, a.chunk_rows);
    jr_clear(a, ws, res);
    for (sj_u64 chunk : jr_order(build_chunks, order)) {
        sj_u64* key_of = jr_block<sj_u64>(a.chunk_rows);
        uint8_t* good = jr_block<uint8_t>(a.chunk_rows);
        jr_keys(g, a, chunk, ws, key_of, good, res);
        free(key_of), free(good);
    }
    if (left_chunks) {
        for (sj_u64 chunk : jr_order(left_chunks, order)) {
            sj_u64* pivots = jr_block<sj_u64>(a.chunk_rows);
            jr_count(g, a, chunk, ws, pivots, res);
            free(pivots);
        }
        jr_scan(g, a, ws, res);
        for (sj_u64 chunk : jr_order(left_chunks, order)) jr_offsets(g, a, chunk, ws);
        for (sj_u64 chunk : jr_order(pair_chunks, order)) {
            sj_u64* marks = jr_block<sj_u64>(a.chunk_rows);
            sj_u64* seeds = jr_block<sj_u64>(2);
            jr_emit(g, a, chunk, ws, marks, seeds, res);
            free(marks), free(seeds);
        }
    }
    free(ws);
}

extern "C" uint32_t sim_join_chunk_rows(void) { return JR_CHUNK_ROWS; }
extern "C" uint64_t sim_join_workspace_words(uint64_t n_left, uint64_t n_right) { return jr_workspace_words(n_left, n_right, JR_CHUNK_ROWS); }

struct SimJoinSide {  // sjmi_join_side
    const uint8_t* key_types;
    const uint64_t* key_validity;
    const uint64_t* key_values;
    uint64_t n_source_rows;
    const uint8_t* types;
    const uint64_t* values;
    uint64_t n_cols, col_stride;
};

static bool sim_side_ok(const SimJoinSide* s, uint64_t positions, bool rows_in, uint64_t pair_capacity, uint64_t out_stride, const void* out_types,
                        const void* out_values) {
    if (s->n_source_rows >= (1ull << 32) || positions >= (1ull << 32)) return false;
    if (s->n_source_rows && positions && !s->key_values) return false;
    if (!rows_in && positions > s->n_source_rows) return false;
    if (s->n_cols && (s->col_stride < s->n_source_rows || out_stride < pair_capacity ||
                      (pair_capacity && (!s->types || !s->values || !out_types || !out_values))))
        return false;
    return !(((uintptr_t)s->key_validity & 7) || ((uintptr_t)s->key_values & 7) || ((uintptr_t)s->values & 7) || ((uintptr_t)out_values & 7));
}

// the call as sjmi_join_rows_device makes it (the argument rules restated: -2 where it answers SJMI_ERR_ARG); chunk_rows 0 = the
// kernels' own.  left_count: NULL or one uint64.  right_sort_result: the sort's record, 9 x uint64.  result: 9 x uint64 (flags in
// the low half of the ninth).
extern "C" int sim_join_rows(const SimJoinSide* left, const uint64_t* left_rows_in, uint64_t n_left, const uint64_t* left_count,
                             const SimJoinSide* right, const uint64_t* right_order, uint64_t n_right, const uint64_t* right_sort_result,
                             uint32_t how, uint64_t pair_capacity, uint64_t* left_rows, uint64_t* right_rows, uint8_t* left_out_types,
                             uint64_t* left_out_values, uint8_t* right_out_types, uint64_t* right_out_values, uint64_t out_stride,
                             uint64_t* pair_offsets, uint64_t* result, uint32_t chunk_rows, uint32_t order) {
    if (!left || !right || !result || how > JR_ANTI || pair_capacity >= JR_MAX_PAIR_CAPACITY) return -2;
    const bool keeps_right = how == JR_INNER || how == JR_LEFT;
    if (!sim_side_ok(left, n_left, left_rows_in != nullptr, pair_capacity, out_stride, left_out_types, left_out_values) ||
        !sim_side_ok(right, n_right, true, pair_capacity, out_stride, right_out_types, right_out_values))
        return -2;
    if (n_right && (!right_order || !right_sort_result)) return -2;
    if (pair_capacity && (!left_rows || (keeps_right && !right_rows))) return -2;
    if (right->n_cols && !keeps_right) return -2;
    if (((uintptr_t)left_rows_in & 7) || ((uintptr_t)left_count & 7) || ((uintptr_t)right_order & 7) || ((uintptr_t)right_sort_result & 7) ||
        ((uintptr_t)left_rows & 7) || ((uintptr_t)right_rows & 7) || ((uintptr_t)pair_offsets & 7) || ((uintptr_t)result & 7))
        return -2;
    const uint32_t chunk = chunk_rows ? chunk_rows : JR_CHUNK_ROWS;
    const JrArgs a = {{left->key_types, (const sj_u64*)left->key_validity, (const sj_u64*)left->key_values, left->n_source_rows,
                       (const sj_u64*)left_rows_in, n_left, (const sj_u64*)left_count, SR_LONG, 0u, chunk, SR_TILE_ROWS},
                      {right->key_types, (const sj_u64*)right->key_validity, (const sj_u64*)right->key_values, right->n_source_rows,
                       (const sj_u64*)right_order, n_right, n_right ? (const sj_u64*)right_sort_result + 1 : nullptr, SR_LONG, 0u, chunk, SR_TILE_ROWS},
                      {left->types, (const sj_u64*)left->values, left->n_cols, left->col_stride},
                      {right->types, (const sj_u64*)right->values, right->n_cols, right->col_stride},
                      how,
                      chunk,
                      pair_capacity,
                      (sj_u64*)left_rows,
                      (sj_u64*)right_rows,
                      left_out_types,
                      (sj_u64*)left_out_values,
                      right_out_types,
                      (sj_u64*)right_out_values,
                      out_stride,
                      (sj_u64*)pair_offsets};
    jr_sim_passes(a, order, (JrResult*)result);
    return 0;
}
