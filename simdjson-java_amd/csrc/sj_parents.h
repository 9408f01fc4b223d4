// sj_parents.h -- which document does a row of an explode belong to, and what are that document's cells (include/sjmi.h,
// sjmi_parent_columns_device): pandas.json_normalize(record_path, meta), SQL's UNNEST with the outer row's columns.
//
// row_offsets is uint64[n_docs + 1] as sjmi_explode_batch_device writes it: document k owns the rows [off[k], off[k + 1]),
// total = off[n_docs].  Output slot i < live = min(n_rows, *row_count) stands for row x = i (DENSE, rows == NULL) or x = rows[i]
// (SPARSE, any order, duplicates legal).  THE COUNT c(x) = #{ j in [1, n_docs] : off[j] <= x } is the whole relation: for
// monotone offsets it is the one k with off[k] <= x < off[k + 1] when x < total -- a document without rows is never it --, and
// n_docs when x >= total: the row is an ORPHAN (parent all ones, parent type MISSING, every carried cell 0 / 0).  With n_docs == 0
// every row is one.  pa_emit is the only writer of a slot, and a parent becomes a load address only behind k < n_docs.
//
// THE PASSES, each a kernel of csrc/parents.hip (the stream orders them):
//   pa_clear    ONE lane: the record with n_rows = live, n_orphans = 0
//   pa_dense    per chunk of chunk_rows rows, a load-balanced search:
//                 1  one wave finds c(first row), another c(last live row) with pa_count_wave, a 64-ary search: 64 pivots, one
//                    ballot, the sub-range behind the pivots that passed -- 2^32 entries take 6 rounds;
//                 2  the documents of that span, a trip of the group's lanes at a time: document k with rows (off[k] < off[k + 1])
//                    whose first row lies in the chunk marks the group's own memory at off[k] - first with k + 1.  Index n_docs
//                    is walked as a document that begins at total and never ends: it marks the first orphan.  EXACTLY ONE SUCH
//                    DOCUMENT BEGINS AT ANY ROW: no two lanes write one address;
//                 3  a running maximum over the positions, seeded at position 0 with c(first row) + 1: position p holds
//                    c(first + p) + 1;
//                 4  pa_emit of every live slot; the orphans counted, one g.agent.add64 per group.
//   pa_sparse   per chunk of slots: a lane per slot, pa_count_lane (a binary search, at most 33 steps), pa_emit, the orphans.
// Nothing spins or waits for another group; every loop is bounded by n_docs, the chunk or the columns; the whole output is a
// function of the input alone.  WILD OFFSETS (not monotone, above the rows): both searches still end within their bounds and
// return at most n_docs, the walk covers at most the indices [0, n_docs], a mark is stored only behind the test of its position,
// and what the maximum yields is compared with n_docs before it addresses a document: wrong parents, never a load or store
// outside a buffer.
//
// The lanes come from the caller: a workgroup G (sj_group.h) with these members added:
//   g.agent.add64(p, v)     an agent-scope relaxed atomic on the record, result unused
//   g.sync()                a barrier of the group: what its lanes wrote to its own memory is visible to all of them
//   g.scan_max(v, &total)   called by every lane: the INCLUSIVE running maximum of v over the group's lanes, total = over all
// uses: lanes, lane, waves, wave, first, ballot, scan_add, agent, sync, scan_max.  csrc/parents.hip runs this file with the device
// form, tests/host_sim/parents_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"

constexpr uint32_t PA_CHUNK_ROWS = 1024;   // rows of a dense chunk: a multiple of its group's lanes, which take them a trip at a time
constexpr uint32_t PA_MAX_COLS = 64;       // SJMI_PARENT_MAX_COLS
constexpr uint32_t PA_RESULT_WORDS = 3;    // SJMI_PARENT_RESULT_WORDS
constexpr uint32_t PA_GATHER = 4;          // columns whose loads are issued before the first of their stores
constexpr sj_u64 PA_ORPHAN = ~0ull;        // d_parents of a row without a parent

struct PaResult {  // sjmi_parent_result
    sj_u64 n_rows, n_orphans;
    uint32_t flags, reserved;
};
static_assert(sizeof(PaResult) == PA_RESULT_WORDS * 8, "the record is whole words");

struct PaArgs {
    const sj_u64* row_offsets;  // [n_docs + 1]
    sj_u64 n_docs;
    const sj_u64* rows;         // NULL: the dense form
    sj_u64 n_rows;
    const sj_u64* row_count;    // NULL, or where the live rows are counted (on the device)
    const uint8_t* types;       // the document columns: any alignment
    const sj_u64* values;
    sj_u64 n_cols, col_stride;
    uint8_t* parent_types;      // [n_rows], may be NULL; any alignment
    sj_u64* parents;            // [n_rows], may be NULL
    uint8_t* out_types;         // [n_cols * out_stride], any alignment
    sj_u64* out_values;
    sj_u64 out_stride;
    uint32_t chunk_rows;
};

SJ_HD sj_u64 pa_live(const PaArgs& a) { return fc_live(a.n_rows, a.row_count); }
SJ_HD sj_u64 pa_chunks(const PaArgs& a) { return fc_chunks(a.n_rows, a.chunk_rows); }

SJ_HD void pa_clear(const PaArgs& a, PaResult* res) {
    res->n_rows = pa_live(a);
    res->n_orphans = 0;
    res->flags = 0;
    res->reserved = 0;
}

// c(x), by ALL lanes of one wave.  [lo, hi] holds the count; a round probes lo + step, lo + 2 * step, ... and keeps what lies
// behind the pivots that passed IN A ROW from the first, so span -> at most ceil(span / 64) - 1.
template <class G>
SJ_HD sj_u64 pa_count_wave(const G& g, const sj_u64* off, sj_u64 n_docs, sj_u64 x) {
    sj_u64 lo = 0, hi = n_docs;
    for (uint32_t round = 0; round < 7 && lo < hi; ++round) {  // (6 rounds for 2^32)
        const sj_u64 step = (hi - lo + 63) / 64;
        const sj_u64 passed = g.ballot([&](uint32_t t) {
            const sj_u64 p = lo + (sj_u64)(t + 1) * step;
            return p <= hi && off[p] <= x;
        });
        const sj_u64 n = ~passed ? (sj_u64)__builtin_ctzll(~passed) : 64;
        lo += n * step;
        if (n < 64 && lo + step - 1 < hi) hi = lo + step - 1;
    }
    return lo;
}

// c(x), by one lane
SJ_HD sj_u64 pa_count_lane(const sj_u64* off, sj_u64 n_docs, sj_u64 x) {
    sj_u64 lo = 0, hi = n_docs;
    for (uint32_t step = 0; step < 34 && lo < hi; ++step) {  // (33 steps for 2^32)
        const sj_u64 mid = lo + (hi - lo) / 2;
        if (off[mid + 1] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// slot i of a row whose count is k (k >= n_docs: an orphan); returns whether it is one
SJ_HD bool pa_emit(const PaArgs& a, sj_u64 i, sj_u64 k) {
    const bool orphan = k >= a.n_docs;
    if (a.parents) a.parents[i] = orphan ? PA_ORPHAN : k;
    if (a.parent_types) a.parent_types[i] = orphan ? 0 : (uint8_t)'l';
    for (sj_u64 c0 = 0; c0 < a.n_cols; c0 += PA_GATHER) {
        uint8_t t[PA_GATHER];
        sj_u64 v[PA_GATHER];
        for (uint32_t j = 0; j < PA_GATHER; ++j) {
            const bool there = c0 + j < a.n_cols && !orphan;
            t[j] = there ? a.types[(c0 + j) * a.col_stride + k] : 0;
            v[j] = there ? a.values[(c0 + j) * a.col_stride + k] : 0;
        }
        for (uint32_t j = 0; j < PA_GATHER && c0 + j < a.n_cols; ++j) {
            a.out_types[(c0 + j) * a.out_stride + i] = t[j];
            a.out_values[(c0 + j) * a.out_stride + i] = v[j];
        }
    }
    return orphan;
}

// the dense form: chunk `chunk`; marks = chunk_rows words and seeds = 2 words of the group's own memory
template <class G>
SJ_HD void pa_dense(const G& g, const PaArgs& a, sj_u64 chunk, sj_u64* marks, sj_u64* seeds, PaResult* res) {
    const sj_u64 live = pa_live(a), first = chunk * a.chunk_rows;
    if (first >= live) return;  // (the whole group, in front of every barrier)
    const sj_u64 last = (first + a.chunk_rows < live ? first + a.chunk_rows : live) - 1;
    if (g.wave() == 0) {
        const sj_u64 c = pa_count_wave(g, a.row_offsets, a.n_docs, first);
        if (g.first()) seeds[0] = c;
    }
    if (g.wave() == g.waves() - 1) {
        const sj_u64 c = pa_count_wave(g, a.row_offsets, a.n_docs, last);
        if (g.first()) seeds[1] = c;
    }
    for (uint32_t p = g.lane(); p < a.chunk_rows; p += g.lanes()) marks[p] = 0;
    g.sync();
    const sj_u64 k_first = seeds[0], k_last = seeds[1] < a.n_docs ? seeds[1] : a.n_docs;
    for (sj_u64 at = k_first; at <= k_last; at += g.lanes()) {
        const sj_u64 k = at + g.lane();
        if (k > k_last) continue;
        const sj_u64 begin = a.row_offsets[k];
        const bool has_rows = k == a.n_docs || a.row_offsets[k + 1] > begin;
        if (has_rows && begin >= first && begin - first < a.chunk_rows) marks[begin - first] = k + 1;
    }
    g.sync();
    sj_u64 run = 0, orphans = 0, total;
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        sj_u64 mine = marks[r - first];
        if (r == first && mine < k_first + 1) mine = k_first + 1;  // (the seed)
        sj_u64 highest;
        sj_u64 incl = g.scan_max(mine, &highest);
        if (incl < run) incl = run;
        if (highest > run) run = highest;
        if (r < live) orphans += pa_emit(a, r, incl - 1);
    }
    (void)g.scan_add(orphans, &total);
    if (g.lane() == 0 && total) g.agent.add64(&res->n_orphans, total);
}

// the sparse form: the slots of chunk `chunk`
template <class G>
SJ_HD void pa_sparse(const G& g, const PaArgs& a, sj_u64 chunk, PaResult* res) {
    const sj_u64 live = pa_live(a), first = chunk * a.chunk_rows;
    if (first >= live) return;  // (the whole group)
    sj_u64 orphans = 0, total;
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 i = at + g.lane();
        if (i < live) orphans += pa_emit(a, i, pa_count_lane(a.row_offsets, a.n_docs, a.rows[i]));
    }
    (void)g.scan_add(orphans, &total);
    if (g.lane() == 0 && total) g.agent.add64(&res->n_orphans, total);
}
