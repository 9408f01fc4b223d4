// sj_groupstats.h -- group statistics per dictionary key: count, sum, minimum and maximum of ONE (type, value) column, grouped by
// the int32 indices (and the validity bitmap) of sjmi_dictionary_column_device (include/sjmi.h, sjmi_group_stats_device; DESIGN.md
// 4.17).  The aggregate that the key census (sj_census.h) leaves out, over the same rows and with the same two paths.
//
// The rows that count are [0, live), live = min(n_rows, *row_count) read HERE, on the device, where a row count is given.  A live
// row r whose validity bit is set (every row without a bitmap) and whose index lies in [0, n_keys) belongs to that key; a valid
// live row with any other index is counted in n_out_of_range and touches nothing else.  gs_row is the only reader of a row: the
// validity word, then the index, then the type byte, then -- only for 'l' and 'd' -- the value word, each only behind the test in
// front of it.  A 'd' cell that is a NaN is counted in n_nan and nowhere else.  Longs and doubles are never mixed.
//
// A key's GS_WORDS = 10 words of the stats (key-major; GsWord names them).  Between the clear and the finish they hold the
// ACCUMULATION FORM, every word with an identity that an atomic can start from:
//   n_long, n_double, n_other   0, added to
//   sum_long_lo                 0: the UNSIGNED sum of the cells' low 32 bits            | below 2^32 rows neither can overflow:
//   sum_long_hi                 0: the SIGNED sum of the cells' high 32 bits (v >> 32)   | < 2^32 * 2^32 and <= 2^31 * (2^32 - 1)
//   sum_double                  +0.0, the double's bits, added to in whatever order the groups arrive
//   min_long / max_long         INT64_MAX / INT64_MIN under a signed minimum / maximum
//   min_double / max_double     ~0 / 0 under an UNSIGNED minimum / maximum of gs_okey(bits), the order-preserving key: IEEE
//                               totalOrder on the non-NaN doubles, -inf < ... < -0.0 < +0.0 < ... < +inf
// and gs_finish_key turns them into the words of the contract: the 128-bit two's-complement sum (hi * 2^32 + lo, exact), the
// keys back into double bits, +inf / -inf for a key without doubles (a key without longs keeps INT64_MAX / INT64_MIN).
//
// THE PASSES, each a kernel of csrc/groupstats.hip (the stream orders them; the stats are read across the kernel boundary only):
//   gs_clear_word     word i of the stats to its identity; word 0's lane writes the record with n_rows = live and the sums zero
//   gs_lds_rows       n_keys <= GS_LDS_KEYS, one group of a GRID of groups with bins of its own (GS_BIN_WORDS 64-bit words and
//                     three 32-bit counts per key, 68 bytes): identities, the chunks group, group + grid, ... of the live rows
//                     into the bins (g.wg: on the device LDS atomics at workgroup scope), then every word of every key THE
//                     GROUP TOUCHED (a non-zero count of its class) to the stats once (g.agent), its three sums to the record
//   gs_global_rows    larger n_keys, one group per chunk: the rows of a wave that have the same key are combined first (g.merge:
//                     the lowest lane of up to GS_MERGE_ROUNDS sets of equal keys takes the set's counts, sums, minima and
//                     maxima; a row outside these sets keeps its own), then g.agent straight into the stats
//   gs_finish_key     per key, see above
// g.agent's members are, on the device, agent-scope relaxed atomics whose results are not used: they are performed at the memory
// that all XCDs share, and nobody reads a word of the stats before the kernel ends.  Every word but sum_double is a sum of
// integers, a minimum or a maximum: a function of the input alone, whatever the order of the groups.  sum_double is a
// floating-point sum in the order of arrival and may differ between two runs in its last bits; any order of n additions stays
// within gamma(n - 1) * sum|x| of the exact sum (Higham, Accuracy and Stability, 4.2), partial sums per group included, because
// adding an exact zero is exact.  Nothing spins or waits for another group; every loop is bounded by the rows or the keys.
// A 32-BIT BIN COUNT CANNOT OVERFLOW: n_rows < 2^32 (the call refuses more), so no group of gs_lds_rows takes 2^32 rows.
//
// The lanes come from the caller: a workgroup G (sj_group.h; a chunk is a multiple of its lanes) with these members added:
//   g.wg, g.agent       two sets of the same seven operations on a word -- add32(p, n), add64(p, v), addf(p, x) (p: the bits of
//                       a double), smin / smax (signed 64-bit), umin / umax (unsigned 64-bit) --, g.wg on the group's own bins,
//                       g.agent on the stats and the record
//   g.sync()            a barrier of the group: what its lanes wrote to the bins is visible to all of them
//   g.merge(key, active, cell)   called by every lane of a wave: true in the lanes that are to add `cell`, which then holds the
//                       combined cell of the lane's set; the cells of the lanes that return true add up to those of the active
//                       ones.  The sequential form is one lane: active, the cell untouched
// uses: lanes, lane, scan_add, wg, agent, sync, merge.  csrc/groupstats.hip runs this file with the device form,
// tests/host_sim/groupstats_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"
#include "sj_okey.h"

constexpr uint32_t GS_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t GS_WORDS = 10;         // SJMI_GROUP_STATS_WORDS
constexpr uint32_t GS_BIN_WORDS = 7;      // the 64-bit words of a key's bins: GS_WORDS less the three counts
// SJMI_GROUP_LDS_KEYS: 512 keys * (7 * 8 + 3 * 4 = 68 bytes) = 34 KiB of bins.  Two workgroups of 1024 lanes per CU then hold 68 of
// its 160 KiB, and one workgroup stays below the 64 KiB a workgroup may ask for
constexpr uint32_t GS_LDS_KEYS = 512;
constexpr uint32_t GS_BIN_BYTES = GS_BIN_WORDS * 8 + 3 * 4;
constexpr uint32_t GS_MAX_GRID = 512;         // groups of gs_lds_rows: two workgroups of 1024 lanes on each of 256 CUs
constexpr uint32_t GS_WORDS_PER_CHUNK = 256;  // a group of gs_lds_rows takes at least four rows per word it may have to flush
constexpr uint32_t GS_MERGE_ROUNDS = 8;       // sets of equal keys that a wave of gs_global_rows combines before it adds
static_assert(GS_LDS_KEYS * GS_BIN_BYTES == 34 * 1024 && GS_LDS_KEYS * GS_BIN_BYTES + 1024 <= 64 * 1024, "the bins fit a workgroup's LDS");

typedef long long sj_i64;
constexpr sj_i64 GS_I64_MAX = 0x7FFFFFFFFFFFFFFFll, GS_I64_MIN = -GS_I64_MAX - 1;

enum GsWord : uint32_t { GS_N_LONG, GS_N_DOUBLE, GS_N_OTHER, GS_SUM_LO, GS_SUM_HI, GS_SUM_DOUBLE, GS_MIN_LONG, GS_MAX_LONG, GS_MIN_DOUBLE, GS_MAX_DOUBLE };

struct GsResult {  // sjmi_group_result
    sj_u64 n_rows, n_grouped, n_out_of_range, n_nan;
    uint32_t flags, reserved;
};

struct GsColumn {
    const int32_t* indices;
    const sj_u64* validity;  // NULL: every live row counts
    const uint8_t* types;    // any alignment: loaded as bytes
    const sj_u64* values;    // loaded only behind type == 'l' or 'd'
    sj_u64 n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
    sj_u64 n_keys;
    uint32_t chunk_rows;
};
SJ_HD sj_u64 gs_live(const GsColumn& c) { return fc_live(c.n_rows, c.row_count); }
SJ_HD sj_u64 gs_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }

// (gs_okey, gs_okey_bits and gs_is_nan -- the order-preserving key of a double's bits -- are sj_okey.h's)
// a double <-> its bits (a copy of the bytes: no lvalue of the other type)
SJ_HD double gs_double(sj_u64 bits) {
    double x;
    __builtin_memcpy(&x, &bits, 8);
    return x;
}
SJ_HD sj_u64 gs_bits(double x) {
    sj_u64 bits;
    __builtin_memcpy(&bits, &x, 8);
    return bits;
}

// word w (GS_SUM_LO ...) of a key among its GS_BIN_WORDS words of a group's bins
SJ_HD uint32_t gs_bin(uint32_t w) { return w - GS_SUM_LO; }

// the identity of word w of a key in the accumulation form
SJ_HD sj_u64 gs_identity(uint32_t w) {
    switch (w) {
        case GS_MIN_LONG: return (sj_u64)GS_I64_MAX;
        case GS_MAX_LONG: return (sj_u64)GS_I64_MIN;
        case GS_MIN_DOUBLE: return ~0ull;
        default: return 0;  // the counts, the sums (+0.0 is all zero bits), the maximum's key
    }
}

// What one row, or the rows of a wave with one key, add to a key.  The identities where a class has no row.
struct GsCell {
    uint32_t n_long, n_double, n_other;
    sj_u64 lo;    // sum of the longs' low halves
    sj_i64 hi;    // sum of the longs' high halves, signed
    double dsum;  // sum of the doubles
    sj_i64 min_long, max_long;
    sj_u64 min_key, max_key;  // gs_okey of the doubles
};
SJ_HD GsCell gs_empty_cell() { return {0, 0, 0, 0, 0, 0.0, GS_I64_MAX, GS_I64_MIN, ~0ull, 0}; }

// the chunks a group of gs_lds_rows takes at least, and the grid for n_rows rows (>= 1)
SJ_HD sj_u64 gs_min_chunks(sj_u64 n_keys) {
    const sj_u64 m = n_keys * GS_WORDS / GS_WORDS_PER_CHUNK;
    return m ? m : 1;
}
SJ_HD uint32_t gs_lds_grid(sj_u64 n_rows, sj_u64 n_keys, uint32_t chunk_rows) {
    const sj_u64 per = gs_min_chunks(n_keys);
    const sj_u64 want = (gs_chunks(n_rows, chunk_rows) + per - 1) / per;
    return want > GS_MAX_GRID ? GS_MAX_GRID : (uint32_t)want;
}

// clearing: word i of the stats; the lane of word 0 writes the record (a grid of at least one group)
SJ_HD void gs_clear_word(const GsColumn& c, sj_u64 i, sj_u64* stats, GsResult* res) {
    if (i < c.n_keys * GS_WORDS) stats[i] = gs_identity((uint32_t)(i % GS_WORDS));
    if (i == 0) {
        res->n_rows = gs_live(c);
        res->n_grouped = 0;
        res->n_out_of_range = 0;
        res->n_nan = 0;
        res->flags = 0;
        res->reserved = 0;
    }
}

// the live row r -> its key, GS_OUT_OF_RANGE, GS_NOT_VALID or GS_NAN; with a key, what the row adds to it
constexpr sj_u64 GS_OUT_OF_RANGE = ~0ull, GS_NOT_VALID = ~0ull - 1, GS_NAN = ~0ull - 2;
SJ_HD sj_u64 gs_row(const GsColumn& c, sj_u64 r, GsCell* cell) {
    if (c.validity && !((c.validity[r >> 6] >> (r & 63)) & 1)) return GS_NOT_VALID;
    const int32_t ix = c.indices[r];
    if (ix < 0 || (sj_u64)ix >= c.n_keys) return GS_OUT_OF_RANGE;
    const uint8_t t = c.types[r];
    if (t == 'l') {
        const sj_u64 v = c.values[r];
        cell->n_long = 1;
        cell->lo = v & 0xFFFFFFFFull;
        cell->hi = (sj_i64)v >> 32;
        cell->min_long = cell->max_long = (sj_i64)v;
    } else if (t == 'd') {
        const sj_u64 v = c.values[r];
        if (gs_is_nan(v)) return GS_NAN;
        cell->n_double = 1;
        cell->dsum = gs_double(v);
        cell->min_key = cell->max_key = gs_okey(v);
    } else {
        cell->n_other = 1;
    }
    return (sj_u64)ix;
}

// a cell into a key's words of the stats: only the words of the classes it has
template <class G>
SJ_HD void gs_add_cell(const G& g, sj_u64* key_words, const GsCell& cell) {
    if (cell.n_long) {
        g.agent.add64(key_words + GS_N_LONG, cell.n_long);
        g.agent.add64(key_words + GS_SUM_LO, cell.lo);
        g.agent.add64(key_words + GS_SUM_HI, (sj_u64)cell.hi);
        g.agent.smin(key_words + GS_MIN_LONG, cell.min_long);
        g.agent.smax(key_words + GS_MAX_LONG, cell.max_long);
    }
    if (cell.n_double) {
        g.agent.add64(key_words + GS_N_DOUBLE, cell.n_double);
        g.agent.addf(key_words + GS_SUM_DOUBLE, cell.dsum);
        g.agent.umin(key_words + GS_MIN_DOUBLE, cell.min_key);
        g.agent.umax(key_words + GS_MAX_DOUBLE, cell.max_key);
    }
    if (cell.n_other) g.agent.add64(key_words + GS_N_OTHER, cell.n_other);
}

// a group's three sums into the record: every lane comes here (scan_add is a barrier)
template <class G>
SJ_HD void gs_record(const G& g, sj_u64 grouped, sj_u64 outside, sj_u64 nan, GsResult* res) {
    sj_u64 n_grouped, n_outside, n_nan;
    (void)g.scan_add(grouped, &n_grouped);
    (void)g.scan_add(outside, &n_outside);
    (void)g.scan_add(nan, &n_nan);
    if (g.lane() == 0) {
        if (n_grouped) g.agent.add64(&res->n_grouped, n_grouped);
        if (n_outside) g.agent.add64(&res->n_out_of_range, n_outside);
        if (n_nan) g.agent.add64(&res->n_nan, n_nan);
    }
}

// n_keys <= GS_LDS_KEYS: group `group` of `grid` with its bins: words[n_keys * GS_BIN_WORDS] (a key's words GS_SUM_LO ... in
// their order) and counts[n_keys * 3], the group's own
template <class G>
SJ_HD void gs_lds_rows(const G& g, const GsColumn& c, sj_u64 group, sj_u64 grid, sj_u64* words, uint32_t* counts, sj_u64* stats, GsResult* res) {
    const sj_u64 live = gs_live(c);
    const uint32_t n_keys = (uint32_t)c.n_keys;
    for (uint32_t b = g.lane(); b < n_keys * GS_BIN_WORDS; b += g.lanes()) words[b] = gs_identity(GS_SUM_LO + b % GS_BIN_WORDS);
    for (uint32_t b = g.lane(); b < n_keys * 3; b += g.lanes()) counts[b] = 0;
    g.sync();
    sj_u64 grouped = 0, outside = 0, nan = 0;
    for (sj_u64 first = group * c.chunk_rows; first < live; first += grid * c.chunk_rows)
        for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
            const sj_u64 r = at + g.lane();
            if (r >= live) continue;
            GsCell cell = gs_empty_cell();
            const sj_u64 key = gs_row(c, r, &cell);
            if (key == GS_NOT_VALID) continue;
            if (key == GS_OUT_OF_RANGE || key == GS_NAN) {
                outside += key == GS_OUT_OF_RANGE;
                nan += key == GS_NAN;
                continue;
            }
            ++grouped;
            sj_u64* w = words + key * GS_BIN_WORDS;
            uint32_t* n = counts + key * 3;
            if (cell.n_long) {
                g.wg.add32(n + GS_N_LONG, 1);
                g.wg.add64(w + gs_bin(GS_SUM_LO), cell.lo);
                g.wg.add64(w + gs_bin(GS_SUM_HI), (sj_u64)cell.hi);
                g.wg.smin(w + gs_bin(GS_MIN_LONG), cell.min_long);
                g.wg.smax(w + gs_bin(GS_MAX_LONG), cell.max_long);
            } else if (cell.n_double) {
                g.wg.add32(n + GS_N_DOUBLE, 1);
                g.wg.addf(w + gs_bin(GS_SUM_DOUBLE), cell.dsum);
                g.wg.umin(w + gs_bin(GS_MIN_DOUBLE), cell.min_key);
                g.wg.umax(w + gs_bin(GS_MAX_DOUBLE), cell.max_key);
            } else {
                g.wg.add32(n + GS_N_OTHER, 1);
            }
        }
    g.sync();
    // the flush: one lane per word of the stats; a word goes out only where the group has a row of its class
    for (uint32_t b = g.lane(); b < n_keys * GS_WORDS; b += g.lanes()) {
        const uint32_t key = b / GS_WORDS, w = b % GS_WORDS;
        const uint32_t* n = counts + key * 3;
        sj_u64* out = stats + b;
        const sj_u64 v = w < 3 ? n[w] : words[key * GS_BIN_WORDS + gs_bin(w)];
        if (w < 3) {
            if (v) g.agent.add64(out, v);
        } else if (w == GS_SUM_LO || w == GS_SUM_HI) {
            if (n[GS_N_LONG]) g.agent.add64(out, v);
        } else if (w == GS_MIN_LONG) {
            if (n[GS_N_LONG]) g.agent.smin(out, (sj_i64)v);
        } else if (w == GS_MAX_LONG) {
            if (n[GS_N_LONG]) g.agent.smax(out, (sj_i64)v);
        } else if (w == GS_SUM_DOUBLE) {
            if (n[GS_N_DOUBLE]) g.agent.addf(out, gs_double(v));
        } else if (w == GS_MIN_DOUBLE) {
            if (n[GS_N_DOUBLE]) g.agent.umin(out, v);
        } else {
            if (n[GS_N_DOUBLE]) g.agent.umax(out, v);
        }
    }
    gs_record(g, grouped, outside, nan, res);
}

// larger n_keys, per chunk.  A chunk that begins at or above `live` does nothing at all: the whole group leaves in front of the
// scans.
template <class G>
SJ_HD void gs_global_rows(const G& g, const GsColumn& c, sj_u64 chunk, sj_u64* stats, GsResult* res) {
    const sj_u64 live = gs_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64 grouped = 0, outside = 0, nan = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        GsCell cell = gs_empty_cell();
        const sj_u64 key = r < live ? gs_row(c, r, &cell) : GS_NOT_VALID;
        const bool inside = key < GS_NAN;
        outside += key == GS_OUT_OF_RANGE;
        nan += key == GS_NAN;
        grouped += inside;
        if (g.merge((uint32_t)key, inside, &cell)) gs_add_cell(g, stats + key * GS_WORDS, cell);  // (every lane of the wave comes here)
    }
    gs_record(g, grouped, outside, nan, res);
}

// finishing: key k's words from the accumulation form to the contract's
SJ_HD void gs_finish_key(const GsColumn& c, sj_u64 k, sj_u64* stats) {
    if (k >= c.n_keys) return;
    sj_u64* w = stats + k * GS_WORDS;
    const sj_u64 lo = w[GS_SUM_LO];
    const sj_i64 hi = (sj_i64)w[GS_SUM_HI];
    const sj_u64 low = ((sj_u64)hi << 32) + lo;  // hi * 2^32 + lo in 128 bits
    w[GS_SUM_LO] = low;
    w[GS_SUM_HI] = (sj_u64)(hi >> 32) + (low < lo ? 1 : 0);
    const bool none = w[GS_N_DOUBLE] == 0;
    w[GS_MIN_DOUBLE] = none ? GS_INF_BITS : gs_okey_bits(w[GS_MIN_DOUBLE]);
    w[GS_MAX_DOUBLE] = none ? GS_INF_BITS | GS_SIGN : gs_okey_bits(w[GS_MAX_DOUBLE]);
}
