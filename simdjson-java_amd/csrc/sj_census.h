// sj_census.h -- the key census: how many rows every dictionary entry has of every value type (include/sjmi.h,
// sjmi_key_census_device).  A count by (index, type class) over two finished columns with the same rows: the
// int32 indices (and the validity bitmap) of sjmi_dictionary_column_device, and ONE column of type bytes -- normally the ""
// element pointer of a members explode.  Sums, minima and maxima are not here: sj_groupstats.h (sjmi_group_stats_device) has them.
//
// The rows that count are [0, live), live = min(n_rows, *row_count) read HERE, on the device, where a row count is given.  A live
// row r whose validity bit is set (every row without a bitmap) and whose index lies in [0, n_keys) adds 1 to counts[index *
// CS_CLASSES + cs_class(types[r])]; a valid live row with any other index (negatives, INT32_MIN, INT32_MAX: the unspecified
// indices of an overflowed dictionary) is counted in n_out_of_range and touches nothing else.  cs_row is the only reader of a
// row: the validity word, then the index, then the type byte, each only behind the test in front of it.
//
// THE PASSES, each a kernel of csrc/census.hip (the stream orders them; the counts are read across the kernel boundary only):
//   cs_clear_word    word i of the counts to zero; word 0's lane writes the record with n_rows = live and the sums zero
//   cs_lds_rows      n_keys <= CS_LDS_KEYS, one group of a GRID of groups: clears its n_keys * 8 32-bit bins, takes the chunks
//                    group, group + grid, ... of the live rows, one add per row into a bin (g.bin_add: on the device an LDS
//                    atomic), then adds every NON-ZERO bin to counts once (g.add64) and its two sums to the record
//   cs_global_rows   larger n_keys, one group per chunk: the rows of a wave that fall into the same bin are merged first
//                    (g.merge: the lowest lane of up to CS_MERGE_ROUNDS sets of equal bins adds their number, a row outside these
//                    sets adds its own 1), then g.add64 straight into counts; the sums to the record.  Without the merge a column
//                    whose rows all fall into one bin queues 8 Mi adds on one address: 80.5 ms for 8 Mi rows, measured (4.16)
// g.add64 is, on the device, an agent-scope relaxed 64-bit atomic add: it is performed at the L2 / memory that all XCDs share,
// its result is not used, and nobody reads a count before the kernel ends.  The sums are exact integers, so the outputs are a
// function of the input alone, whatever the order of the groups.  Nothing spins or waits for another group; every loop is
// bounded by the rows or the bins.
// A BIN CANNOT OVERFLOW: a group of cs_lds_rows takes at most ceil(chunks / grid) chunks; cs_lds_grid gives grid = CS_MAX_GRID
// whenever there are more than CS_MAX_GRID * cs_min_chunks(n_keys) chunks, and n_rows < 2^40 means fewer than 2^30 chunks: at most
// 2^30 / 512 = 2^21 chunks = 2^31 rows per group (a smaller grid: at most cs_min_chunks <= 32 chunks), below 2^32.
//
// The lanes come from the caller: a workgroup G (sj_group.h; a chunk is a multiple of its lanes) with four members added:
// bin_add(p), add64(p, v), sync() (a barrier of the group: what its lanes wrote to the bins is visible to all of them) and
// merge(bin, active) -- called by every lane of a wave: the number a lane is to add for its bin, 0 where another lane of the wave
// adds for it, the sum over the wave's lanes being the number of active ones; the sequential form is one lane: active ? 1 : 0 --;
// uses: lanes, lane, scan_add, bin_add, add64, sync, merge.  csrc/census.hip runs this file with the device form,
// tests/host_sim/census_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"

constexpr uint32_t CS_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t CS_CLASSES = 8;        // SJMI_CENSUS_CLASSES
constexpr uint32_t CS_LDS_KEYS = 1024;    // SJMI_CENSUS_LDS_KEYS: 8192 bins of 32 bits = 32 KiB
constexpr uint32_t CS_MAX_GRID = 512;     // groups of cs_lds_rows: two workgroups of 1024 lanes on each of 256 CUs
constexpr uint32_t CS_BINS_PER_CHUNK = 256;  // a group of cs_lds_rows takes at least four rows per bin it may have to flush
constexpr uint32_t CS_MERGE_ROUNDS = 8;      // sets of equal bins that a wave of cs_global_rows merges before it adds

struct CsResult {  // sjmi_census_result
    sj_u64 n_rows, n_counted, n_out_of_range;
    uint32_t flags, reserved;
};

struct CsColumn {
    const int32_t* indices;
    const sj_u64* validity;  // NULL: every live row counts
    const uint8_t* types;    // any alignment: loaded as bytes
    sj_u64 n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
    sj_u64 n_keys;
    uint32_t chunk_rows;
};
SJ_HD sj_u64 cs_live(const CsColumn& c) { return fc_live(c.n_rows, c.row_count); }
SJ_HD sj_u64 cs_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }

SJ_HD uint32_t cs_class(uint8_t t) {
    switch (t) {
        case 'l': return 0;
        case 'd': return 1;
        case '"': return 2;
        case 't':
        case 'f': return 3;
        case 'n': return 4;
        case '[': return 5;
        case '{': return 6;
        default: return 7;
    }
}

// the chunks a group of cs_lds_rows takes at least, and the grid for n_rows rows (>= 1)
SJ_HD sj_u64 cs_min_chunks(sj_u64 n_keys) {
    const sj_u64 m = n_keys * CS_CLASSES / CS_BINS_PER_CHUNK;
    return m ? m : 1;
}
SJ_HD uint32_t cs_lds_grid(sj_u64 n_rows, sj_u64 n_keys, uint32_t chunk_rows) {
    const sj_u64 per = cs_min_chunks(n_keys);
    const sj_u64 want = (cs_chunks(n_rows, chunk_rows) + per - 1) / per;
    return want > CS_MAX_GRID ? CS_MAX_GRID : (uint32_t)want;
}

// clearing: word i of the counts; the lane of word 0 writes the record (a grid of at least one group)
SJ_HD void cs_clear_word(const CsColumn& c, sj_u64 i, sj_u64* counts, CsResult* res) {
    if (i < c.n_keys * CS_CLASSES) counts[i] = 0;
    if (i == 0) {
        res->n_rows = cs_live(c);
        res->n_counted = 0;
        res->n_out_of_range = 0;
        res->flags = 0;
        res->reserved = 0;
    }
}

// the live row r -> its bin, CS_OUT_OF_RANGE, or CS_NOT_VALID
constexpr sj_u64 CS_OUT_OF_RANGE = ~0ull, CS_NOT_VALID = ~0ull - 1;
SJ_HD sj_u64 cs_row(const CsColumn& c, sj_u64 r) {
    if (c.validity && !((c.validity[r >> 6] >> (r & 63)) & 1)) return CS_NOT_VALID;
    const int32_t ix = c.indices[r];
    if (ix < 0 || (sj_u64)ix >= c.n_keys) return CS_OUT_OF_RANGE;
    return (sj_u64)ix * CS_CLASSES + cs_class(c.types[r]);
}

// a group's two sums into the record: every lane comes here (scan_add is a barrier)
template <class G>
SJ_HD void cs_record(const G& g, sj_u64 counted, sj_u64 outside, CsResult* res) {
    sj_u64 n_counted, n_outside;
    (void)g.scan_add(counted, &n_counted);
    (void)g.scan_add(outside, &n_outside);
    if (g.lane() == 0) {
        if (n_counted) g.add64(&res->n_counted, n_counted);
        if (n_outside) g.add64(&res->n_out_of_range, n_outside);
    }
}

// n_keys <= CS_LDS_KEYS: group `group` of `grid` with its bins (n_keys * CS_CLASSES words of the group's own)
template <class G>
SJ_HD void cs_lds_rows(const G& g, const CsColumn& c, sj_u64 group, sj_u64 grid, uint32_t* bins, sj_u64* counts, CsResult* res) {
    const sj_u64 live = cs_live(c);
    const uint32_t n_bins = (uint32_t)(c.n_keys * CS_CLASSES);
    for (uint32_t b = g.lane(); b < n_bins; b += g.lanes()) bins[b] = 0;
    g.sync();
    sj_u64 counted = 0, outside = 0;
    for (sj_u64 first = group * c.chunk_rows; first < live; first += grid * c.chunk_rows)
        for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
            const sj_u64 r = at + g.lane();
            if (r >= live) continue;
            const sj_u64 bin = cs_row(c, r);
            if (bin == CS_NOT_VALID) continue;
            if (bin == CS_OUT_OF_RANGE) {
                ++outside;
                continue;
            }
            g.bin_add(bins + bin);
            ++counted;
        }
    g.sync();
    for (uint32_t b = g.lane(); b < n_bins; b += g.lanes()) {
        const uint32_t n = bins[b];
        if (n) g.add64(counts + b, n);
    }
    cs_record(g, counted, outside, res);
}

// larger n_keys, per chunk.  A chunk that begins at or above `live` does nothing at all: the whole group leaves in front of the
// scans.
template <class G>
SJ_HD void cs_global_rows(const G& g, const CsColumn& c, sj_u64 chunk, sj_u64* counts, CsResult* res) {
    const sj_u64 live = cs_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64 counted = 0, outside = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        const sj_u64 bin = r < live ? cs_row(c, r) : CS_NOT_VALID;
        const bool inside = bin != CS_NOT_VALID && bin != CS_OUT_OF_RANGE;
        outside += bin == CS_OUT_OF_RANGE;
        counted += inside;
        const uint32_t n = g.merge((uint32_t)bin, inside);  // (every lane of the wave comes here; a bin is below 2^23)
        if (n) g.add64(counts + bin, n);
    }
    cs_record(g, counted, outside, res);
}
