// sj_fieldcol.h -- the frame of the operators that export (type, value) columns as fixed-width Arrow arrays, one array per FIELD
// of a schema: sj_arrowcol.h (int64, float64, bool) and sj_timecol.h (timestamps; 4.14).  Everything here is
// the same for both; what an operator adds is its cell function, its chunk loop, and what a field's second word and flags mean.
//
// The cell of column c, row r is types[c * col_stride + r] / values[c * col_stride + r].  A FIELD is (column, what, flags): what
// one output array is made of.  The rows that count are [0, live), live = min(n_rows, *row_count) read on the device, where a row
// count is given: n_rows only sizes the grid.  Two passes: the operator's chunk pass per (chunk of rows, field) -- between
// fc_chunk_head and FcCounts::store: the data words, the validity words and the chunk's N counts packed into one scratch word --
// and fc_finish per field: the sum of its chunk words, the record of N + 1 words.  No atomics, and no group waits for another.
//
// The lanes come from the caller as a workgroup G (sj_group.h); used here: lanes, lane, scan_add.  Compiled verbatim by the
// kernels and by the host simulations (tests/host_sim/fieldcol_sim.h).
#pragma once
#include <stdint.h>

#include "sj_block.h"

constexpr uint32_t FC_MAX_FIELDS = 64;  // SJMI_ARROW_MAX_FIELDS, SJMI_TIME_MAX_FIELDS

struct FcField {  // sjmi_arrow_field, sjmi_time_field
    uint32_t column, what, flags, reserved;  // what: the operator's kind or unit
};

// a validated schema: what the kernels take BY VALUE as a launch argument (nothing of it lives in device memory)
struct FcPlan {
    uint32_t n_fields, pad[3];
    FcField fields[FC_MAX_FIELDS];
};

// The column set.  An operator derives its own from it, duck-typed as `Cols` below, and ends it with
//     uint32_t chunk_rows;  // a multiple of 64
// behind whatever else its cells need (sj_timecol.h: the string buffer, which the kernel then loads together with row_count)
struct FcCols {
    const uint8_t* types;  // any alignment: loaded as bytes
    const sj_u64* values;
    sj_u64 col_stride, n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
};
SJ_HD sj_u64 fc_chunks(sj_u64 rows, uint32_t chunk_rows) { return (rows + chunk_rows - 1) / chunk_rows; }
SJ_HD sj_u64 fc_live(sj_u64 n_rows, const sj_u64* row_count) {
    if (!row_count) return n_rows;
    const sj_u64 n = *row_count;
    return n < n_rows ? n : n_rows;
}

struct FcOut {
    sj_u64* data;  // NULL: the counting call
    sj_u64 data_stride;
    sj_u64* validity;  // NULL: not written
    sj_u64 validity_stride;
};

// Host only: fields -> a plan.  0, or -2 (SJMI_ERR_ARG): no field or more than 64, reserved != 0, a column >= n_cols, or a field
// whose `what` / `flags` the operator's test refuses.
template <class Valid>
inline int fc_plan_compile(const FcField* fields, sj_u64 n_fields, sj_u64 n_cols, FcPlan* out, Valid valid) {
    if (!fields || n_fields == 0 || n_fields > FC_MAX_FIELDS) return -2;
    out->n_fields = (uint32_t)n_fields;
    out->pad[0] = out->pad[1] = out->pad[2] = 0;
    for (uint32_t k = 0; k < FC_MAX_FIELDS; ++k) {
        const FcField zero = {0, 0, 0, 0};
        out->fields[k] = k < n_fields ? fields[k] : zero;
    }
    for (sj_u64 k = 0; k < n_fields; ++k)
        if (!valid(fields[k]) || fields[k].reserved != 0 || fields[k].column >= n_cols) return -2;
    return 0;
}

// A chunk's N counts in one word, BITS each: a count is at most the chunk's rows, ROWS in the kernels
template <uint32_t N, uint32_t BITS, uint32_t ROWS>
struct FcCounts {
    static_assert(ROWS < (1u << BITS) && N * BITS <= 64, "a chunk's counts fit one word");
    static constexpr uint32_t COUNTS = N;
    // what ONE row adds: count j iff is[j]
    static SJ_HD sj_u64 of(const bool (&is)[N]) {
        sj_u64 w = 0;
#pragma unroll
        for (uint32_t j = 0; j < N; ++j) w |= is[j] ? 1ull << (j * BITS) : 0ull;
        return w;
    }
    static SJ_HD sj_u64 get(sj_u64 w, uint32_t j) { return (w >> (j * BITS)) & ((1ull << BITS) - 1); }
    // the group's word of (field, chunk) into the scratch: counts[field * chunks + chunk]
    template <class G, class Cols>
    static SJ_HD void store(const G& g, const Cols& c, uint32_t field, sj_u64 chunk, sj_u64* counts, sj_u64 word) {
        if (g.lane() == 0) counts[(sj_u64)field * fc_chunks(c.n_rows, c.chunk_rows) + chunk] = word;
    }
};

// the head of a chunk pass, behind its test of the live rows -- a chunk that begins at or above `live` does nothing at all: the
// whole group leaves, in front of any scan --: the field, its column's first cell, its slices of the outputs, the chunk's first word
struct FcChunk {
    FcField f;
    sj_u64 col;
    sj_u64 *data, *validity;  // NULL as in FcOut
    sj_u64 first;
};
template <class Cols>
SJ_HD FcChunk fc_chunk_head(const FcPlan& p, const Cols& c, sj_u64 chunk, uint32_t field, const FcOut& o) {
    FcChunk h;
    h.f = p.fields[field];
    h.col = (sj_u64)h.f.column * c.col_stride;
    h.data = o.data ? o.data + field * o.data_stride : nullptr;
    h.validity = o.validity ? o.validity + field * o.validity_stride : nullptr;
    h.first = chunk * (c.chunk_rows / 64);
    return h;
}

// pass 2, one group per field: the chunk words of the live chunks summed, the record res[field * (N + 1) ..] = live, the N sums
template <class Counts, class G, class Cols>
SJ_HD void fc_finish(const G& g, const Cols& c, uint32_t field, const sj_u64* counts, sj_u64* res) {
    constexpr uint32_t N = Counts::COUNTS;
    const sj_u64 live = fc_live(c.n_rows, c.row_count);
    const sj_u64 nlive = fc_chunks(live, c.chunk_rows);
    const sj_u64* mine = counts + (sj_u64)field * fc_chunks(c.n_rows, c.chunk_rows);
    sj_u64 sum[N], total[N];
    for (uint32_t j = 0; j < N; ++j) sum[j] = 0;
    for (sj_u64 k = g.lane(); k < nlive; k += g.lanes()) {
        const sj_u64 w = mine[k];
        for (uint32_t j = 0; j < N; ++j) sum[j] += Counts::get(w, j);
    }
    for (uint32_t j = 0; j < N; ++j) (void)g.scan_add(sum[j], &total[j]);
    if (g.lane() == 0) {
        res[(sj_u64)field * (N + 1)] = live;
        for (uint32_t j = 0; j < N; ++j) res[(sj_u64)field * (N + 1) + 1 + j] = total[j];
    }
}
