// sj_sortrows.h -- ALL rows ordered by ONE key column: a stable sort (include/sjmi.h, sjmi_sort_rows_device).  A
// least-significant-digit radix sort of (64-bit order-preserving key, 32-bit position) pairs on 8-bit digits, then a gather of
// the rows and of the carried cells.  Equal keys keep their input order, so a sort by several columns is a chain of these calls,
// last key first, and a sort of a filter's selection is the same call with the selection as d_rows_in.
//
// POSITIONS AND ROWS.  The positions that count are [0, live), live = min(n_rows, *row_count) read HERE, on the device.  Position
// i stands for the source row rows_in[i], or i without rows_in.  sr_pos is the only reader of a position: the entry of rows_in,
// and -- only where that is below n_source_rows -- tr_row of sj_toprows.h on that row, with its classes (CANDIDATE, NULL, OTHER,
// NaN), its read order (validity word, type byte, value word, each behind the test in front of it) and its key; a position whose
// entry is at or above n_source_rows is BAD, is never dereferenced, and is ordered with the NULLs.  Under SR_DESCENDING the key
// is complemented (tr_row's TR_SMALLEST); the tie rule -- ascending position -- does not change.
//
// THE PASSES, each a kernel of csrc/sortrows.hip (the stream orders them; the scratch is read across kernel boundaries only):
//   sr_clear_word   the state to its identities; word 0's lane writes the record with n_rows = live
//   sr_range        a GRID of groups, group, group + grid, ... of the chunks: every live position classified, the counts to the
//                   record, the minimum and the maximum key of the group's candidates to the state (one g.agent.umin / umax each)
//   sr_plan         ONE lane: n_digits = ceil((msb(min ^ max) + 1) / 8), 0 .. 8 (min == max: nothing moves); where the classes
//                   behind the candidates begin; n_passes and the flags of the record
//   sr_count        per chunk: its candidates and NaNs in one word, its OTHER and NULL + BAD positions in a second one (all four
//                   below 2^32)
//   sr_scan         ONE group: the exclusive scans of the two words (no carry leaves a low half: n_rows < 2^32)
//   sr_emit         per chunk: a candidate as (key, position) into buffer A at its rank among the candidates, in position order; a
//                   NaN, OTHER, NULL or BAD position straight to its FINAL place behind the candidates, in the position list that
//                   the last digit pass writes (A's with an even number of digits, B's with an odd one) -- final, because the
//                   sort is stable and these positions take part in no digit pass
//   per digit d, lowest first, from buffer d & 1 into the other; a pass at or above n_digits reads the plan and leaves:
//   sr_hist(d)      per tile: how many pairs of the tile have each of the 256 digit values, to table[value][tile]
//   sr_digit_scan(d) group `value` of 256: the exclusive scan of table[value][0, tiles), its total to totals[value]
//   sr_scatter(d)   per tile: totals[] scanned, so value v's pairs begin at base[v] + table[v][tile]; every pair to its place in the
//                   tile's order in the group's own memory, and from there, neighbours side by side, to its place in the output
//   sr_gather       a lane per output place j < live: rows[j] = the source row of the position there (a BAD entry unchanged),
//                   and that row's cell in every carried column (type byte 0 and value 0 for a BAD position)
//
// THE RANK OF A PAIR INSIDE ITS TILE IS A FUNCTION OF THE DATA.  A tile is cut into one run of consecutive pairs per wave, in
// wave order, and a wave walks its run in position order, `width` pairs a step.  sr_match gives every lane the mask of the lanes
// of its wave that hold a pair with its digit value (eight ballots): popcount(mask below the lane) is the pair's rank in the
// step, and the lowest lane of the mask -- one lane per value, so no two lanes write one address -- adds popcount(mask) to
// count[wave][value] in the group's own memory.  First walk (sr_hist, and again in sr_scatter): the counts of every wave.  They
// are then scanned over the values in order and per value over the waves IN WAVE ORDER, which turns count[wave][value] into the
// place, in the tile's output order, of the wave's next pair with that value; the second walk reads it, adds the rank in the
// step, stages the pair there, and the value's lowest lane moves it on.  Behind a barrier lane s stores staged pair s at
// base[value] + (s - start[value]).  No atomic hands out a slot anywhere: no order depends on which wave runs first.
// Nothing spins or waits for another group; every loop is bounded by the rows, the 256 values, the waves or the tiles.  A 32-BIT
// COUNT CANNOT OVERFLOW: n_rows < 2^32.  Every count is a sum of integers and every place a function of keys and positions: the
// whole output is a function of the input alone, whatever the order of the groups.
//
// The lanes come from the caller: a workgroup G (sj_group.h; a chunk is a multiple of its lanes, a tile a multiple of its lanes
// too, and it has at most SR_VALUES lanes a wave) with these members added:
//   g.agent.add64 / umin / umax   on the state and the record (agent-scope relaxed atomics, results unused)
//   g.sync()                      a barrier of the group: what its lanes wrote to its own memory is visible to all of them
//   g.wave_fence()                orders the accesses of ONE wave to the group's own memory (no barrier: called inside a wave's walk)
//   g.all_umin(v) / g.all_umax(v) called by every lane: the minimum / maximum of v over the group's lanes, in every lane
// and g.ballot(f) called with an f that ignores its argument and answers for the calling lane: bit t of the result is lane t's
// answer, over the lanes of the calling lane's wave (the sequential form's wave is ONE lane).  BARRIERS: sync, all_umin,
// all_umax, scan_add and scan_in_place must be reached by every lane of the group; ballot and wave_fence by whole waves -- the
// walks' loop bounds are wave-uniform.  uses: lanes, lane, waves, wave, ballot, scan_add, scan_in_place, agent, sync, wave_fence,
// all_umin, all_umax.  csrc/sortrows.hip runs this file with the device form, tests/host_sim/sortrows_sim.cpp with the
// sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_filter.h"
#include "sj_toprows.h"

constexpr uint32_t SR_CHUNK_ROWS = 1024;  // positions of a chunk = threads of its workgroup
constexpr uint32_t SR_TILE_ROWS = 4096;   // pairs of a tile of a digit pass: a run of 256 consecutive pairs per wave of 1024 threads
constexpr uint32_t SR_DIGIT_BITS = 8, SR_VALUES = 1u << SR_DIGIT_BITS, SR_MAX_DIGITS = 8;
constexpr uint32_t SR_MAX_GRID = 512;     // groups of sr_range: two workgroups of 1024 lanes on each of 256 CUs
enum : uint32_t { SR_LONG = 1, SR_DOUBLE = 2 };  // SJMI_SORT_<KIND> (= TR_<KIND>: tr_row reads the column)
constexpr uint32_t SR_DESCENDING = 1u;           // SJMI_SORT_DESCENDING
constexpr uint32_t SR_BAD_ROW = 1u;              // SJMI_SORT_BAD_ROW
constexpr uint32_t SR_RESULT_WORDS = 9;          // SJMI_SORT_RESULT_WORDS
static_assert((uint32_t)SR_LONG == (uint32_t)TR_LONG && (uint32_t)SR_DOUBLE == (uint32_t)TR_DOUBLE, "the kinds are tr_row's");

struct SrResult {  // sjmi_sort_result
    sj_u64 n_rows, n_candidates, n_null, n_other, n_nan, n_inexact, n_bad, n_passes;
    uint32_t flags, reserved;
};

struct SrColumn {
    const uint8_t* types;    // NULL: every valid row is a number of the kind.  Any alignment: loaded as bytes
    const sj_u64* validity;  // NULL: every source row is valid
    const sj_u64* values;    // loaded only behind the tests in front of it
    sj_u64 n_source_rows;    // rows of the key column and of the carried columns
    const sj_u64* rows_in;   // NULL: position i IS row i
    sj_u64 n_rows;           // positions
    const sj_u64* row_count;  // NULL, or where the live positions are counted (on the device)
    uint32_t kind, flags;
    uint32_t chunk_rows, tile_rows;
};
struct SrCarry {
    const uint8_t* types;  // any alignment
    const sj_u64* values;
    sj_u64 n_cols, col_stride;
};
struct SrOut {
    sj_u64* rows;    // [n_rows]
    uint8_t* types;  // n_cols rows `stride` cells apart, any alignment
    sj_u64* values;
    sj_u64 stride;
};

// THE SCRATCH, in 64-bit words: the state | two words per chunk (all chunks' first words, then their second ones) | the table,
// SR_VALUES rows of a word per tile | SR_VALUES totals | buffer A: n_rows keys, n_rows 32-bit positions | buffer B likewise
struct SrState {
    sj_u64 min_key, max_key;  // of the candidates; ~0 / 0 where there is none
    sj_u64 n_cand;            // the pairs of the digit passes; the NaN positions begin here
    sj_u64 other_base, null_base;  // where the OTHER and the NULL + BAD positions begin
    uint32_t n_digits, reserved;
};
constexpr sj_u64 SR_STATE_WORDS = sizeof(SrState) / 8;
static_assert(sizeof(SrState) == 48 && sizeof(SrResult) == SR_RESULT_WORDS * 8, "the state and the record are whole words");
SJ_HD sj_u64 sr_live(const SrColumn& c) { return fc_live(c.n_rows, c.row_count); }
SJ_HD sj_u64 sr_chunks(const SrColumn& c) { return fc_chunks(c.n_rows, c.chunk_rows); }
SJ_HD sj_u64 sr_tiles(const SrColumn& c, sj_u64 pairs) { return fc_chunks(pairs, c.tile_rows); }
SJ_HD SrState* sr_state(sj_u64* ws) { return (SrState*)ws; }
SJ_HD sj_u64* sr_counts(sj_u64* ws) { return ws + SR_STATE_WORDS; }
SJ_HD sj_u64* sr_table(const SrColumn& c, sj_u64* ws) { return sr_counts(ws) + 2 * sr_chunks(c); }
SJ_HD sj_u64* sr_totals(const SrColumn& c, sj_u64* ws) { return sr_table(c, ws) + (sj_u64)SR_VALUES * sr_tiles(c, c.n_rows); }
SJ_HD sj_u64 sr_buffer_words(const SrColumn& c) { return c.n_rows + (c.n_rows + 1) / 2; }
SJ_HD sj_u64* sr_keys(const SrColumn& c, sj_u64* ws, uint32_t which) { return sr_totals(c, ws) + SR_VALUES + which * sr_buffer_words(c); }
SJ_HD uint32_t* sr_positions(const SrColumn& c, sj_u64* ws, uint32_t which) { return (uint32_t*)(sr_keys(c, ws, which) + c.n_rows); }
SJ_HD sj_u64 sr_workspace_words(sj_u64 n_rows, uint32_t chunk_rows, uint32_t tile_rows) {
    return SR_STATE_WORDS + 2 * fc_chunks(n_rows, chunk_rows) + (sj_u64)SR_VALUES * fc_chunks(n_rows, tile_rows) + SR_VALUES +
           2 * (n_rows + (n_rows + 1) / 2);
}
// the groups of sr_range for n_rows positions (>= 1)
SJ_HD uint32_t sr_grid(sj_u64 n_rows, uint32_t chunk_rows) {
    const sj_u64 want = fc_chunks(n_rows, chunk_rows);
    return want > SR_MAX_GRID ? SR_MAX_GRID : (uint32_t)want;
}

// the live position i -> its source row and its class; a candidate's key, and whether a long had to be rounded to become a double
constexpr uint32_t SR_BAD = 4;  // behind TR_CANDIDATE, TR_NULL, TR_OTHER, TR_NAN
SJ_HD uint32_t sr_pos(const SrColumn& c, sj_u64 i, sj_u64* row, sj_u64* key, bool* inexact) {
    const sj_u64 r = c.rows_in ? c.rows_in[i] : i;
    *row = r;
    if (r >= c.n_source_rows) return SR_BAD;
    const TrColumn col = {c.types, c.validity, c.values, c.n_source_rows, nullptr, c.kind, (c.flags & SR_DESCENDING) ? TR_SMALLEST : 0u, 0, c.chunk_rows};
    return tr_row(col, r, key, inexact);
}

// clearing: word i of the state; the lane of word 0 writes the record
SJ_HD void sr_clear_word(const SrColumn& c, sj_u64 i, sj_u64* ws, SrResult* res) {
    if (i < SR_STATE_WORDS) ws[i] = i == 0 ? ~0ull : 0;  // (word 0 is min_key)
    if (i == 0) {
        res->n_rows = sr_live(c);
        res->n_candidates = res->n_null = res->n_other = res->n_nan = res->n_inexact = res->n_bad = 0;
        res->n_passes = 0;
        res->flags = 0;
        res->reserved = 0;
    }
}

// pass 1: group `group` of `grid`
template <class G>
SJ_HD void sr_range(const G& g, const SrColumn& c, sj_u64 group, sj_u64 grid, sj_u64* ws, SrResult* res) {
    const sj_u64 live = sr_live(c);
    sj_u64 lo = ~0ull, hi = 0, n[5] = {0, 0, 0, 0, 0}, rounded = 0;
    for (sj_u64 first = group * c.chunk_rows; first < live; first += grid * c.chunk_rows)
        for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
            const sj_u64 i = at + g.lane();
            if (i >= live) continue;
            sj_u64 row, key = 0;
            bool inexact = false;
            const uint32_t cls = sr_pos(c, i, &row, &key, &inexact);
            for (uint32_t k = 0; k < 5; ++k) n[k] += cls == k;
            if (cls != TR_CANDIDATE) continue;
            rounded += inexact;
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
    lo = g.all_umin(lo);
    hi = g.all_umax(hi);
    sj_u64 total[5], n_rounded;
    for (uint32_t cls = 0; cls < 5; ++cls) (void)g.scan_add(n[cls], &total[cls]);
    (void)g.scan_add(rounded, &n_rounded);
    if (g.lane() == 0) {
        SrState* st = sr_state(ws);
        if (total[TR_CANDIDATE]) {
            g.agent.umin(&st->min_key, lo);
            g.agent.umax(&st->max_key, hi);
            g.agent.add64(&res->n_candidates, total[TR_CANDIDATE]);
        }
        if (total[TR_NULL]) g.agent.add64(&res->n_null, total[TR_NULL]);
        if (total[TR_OTHER]) g.agent.add64(&res->n_other, total[TR_OTHER]);
        if (total[TR_NAN]) g.agent.add64(&res->n_nan, total[TR_NAN]);
        if (total[SR_BAD]) g.agent.add64(&res->n_bad, total[SR_BAD]);
        if (n_rounded) g.agent.add64(&res->n_inexact, n_rounded);
    }
}

// pass 2, ONE lane: which bits the digit passes have to look at, and where the classes behind the candidates begin
SJ_HD void sr_plan(sj_u64* ws, SrResult* res) {
    SrState* st = sr_state(ws);
    st->n_cand = res->n_candidates;
    st->other_base = st->n_cand + res->n_nan;
    st->null_base = st->other_base + res->n_other;
    const sj_u64 differ = st->n_cand ? st->min_key ^ st->max_key : 0;
    const uint32_t bits = differ ? 64u - (uint32_t)__builtin_clzll(differ) : 0u;  // msb + 1
    st->n_digits = (bits + SR_DIGIT_BITS - 1) / SR_DIGIT_BITS;
    st->reserved = 0;
    res->n_passes = st->n_digits;
    res->flags = res->n_bad ? SR_BAD_ROW : 0u;
}

// what position i adds to its chunk's two words: word 0 = candidates | NaNs << 32, word 1 = OTHER | NULL + BAD << 32
SJ_HD uint32_t sr_mark_pos(const SrColumn& c, sj_u64 i, sj_u64 live, sj_u64* key, sj_u64* w0, sj_u64* w1) {
    *w0 = *w1 = 0;
    if (i >= live) return SR_BAD + 1;  // (no position)
    sj_u64 row;
    bool inexact = false;
    const uint32_t cls = sr_pos(c, i, &row, key, &inexact);
    if (cls == TR_CANDIDATE) *w0 = 1;
    else if (cls == TR_NAN) *w0 = 1ull << 32;
    else if (cls == TR_OTHER) *w1 = 1;
    else *w1 = 1ull << 32;
    return cls;
}

// pass 3a, per chunk
template <class G>
SJ_HD void sr_count(const G& g, const SrColumn& c, sj_u64 chunk, sj_u64* ws) {
    const sj_u64 live = sr_live(c), first = chunk * c.chunk_rows;
    sj_u64 mine0 = 0, mine1 = 0, total0, total1;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        sj_u64 key = 0, w0, w1;
        (void)sr_mark_pos(c, at + g.lane(), live, &key, &w0, &w1);
        mine0 += w0;
        mine1 += w1;
    }
    (void)g.scan_add(mine0, &total0);
    (void)g.scan_add(mine1, &total1);
    if (g.lane() == 0) {
        sr_counts(ws)[chunk] = total0;
        sr_counts(ws)[sr_chunks(c) + chunk] = total1;
    }
}

// pass 3b, ONE group
template <class G>
SJ_HD void sr_scan(const G& g, const SrColumn& c, sj_u64* ws) {
    (void)g.scan_in_place(sr_counts(ws), sr_chunks(c));
    (void)g.scan_in_place(sr_counts(ws) + sr_chunks(c), sr_chunks(c));
}

// pass 3c, per chunk.  A chunk that begins at or above `live` does nothing at all: the whole group leaves in front of the scans.
// Every place is below `live` (the four classes' counts sum to it), and is compared with n_rows all the same before the store
template <class G>
SJ_HD void sr_emit(const G& g, const SrColumn& c, sj_u64 chunk, sj_u64* ws) {
    const SrState* st = sr_state(ws);
    const sj_u64 live = sr_live(c), first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64* keys = sr_keys(c, ws, 0);
    uint32_t* pos = sr_positions(c, ws, 0);
    uint32_t* last = sr_positions(c, ws, st->n_digits & 1u);  // the list that sr_gather reads
    sj_u64 run0 = sr_counts(ws)[chunk], run1 = sr_counts(ws)[sr_chunks(c) + chunk];  // in front of this chunk, then of this trip
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 i = at + g.lane();
        sj_u64 key = 0, w0, w1, total0, total1;
        const uint32_t cls = sr_mark_pos(c, i, live, &key, &w0, &w1);
        const sj_u64 before0 = run0 + g.scan_add(w0, &total0), before1 = run1 + g.scan_add(w1, &total1);
        if (cls == TR_CANDIDATE) {
            const sj_u64 j = before0 & 0xFFFFFFFFull;
            if (j < c.n_rows) {
                keys[j] = key;
                pos[j] = (uint32_t)i;
            }
        } else if (cls <= SR_BAD) {
            const sj_u64 j = cls == TR_NAN ? st->n_cand + (before0 >> 32) : cls == TR_OTHER ? st->other_base + (before1 & 0xFFFFFFFFull)
                                                                                           : st->null_base + (before1 >> 32);
            if (j < c.n_rows) last[j] = (uint32_t)i;
        }
        run0 += total0;
        run1 += total1;
    }
}

// the lanes of the calling lane's wave that hold a pair (`valid`) with the same digit value as the calling lane: eight ballots
template <class G>
SJ_HD sj_u64 sr_match(const G& g, uint32_t value, bool valid) {
    sj_u64 mask = g.ballot([&](uint32_t) { return valid; });
    for (uint32_t b = 0; b < SR_DIGIT_BITS; ++b) {
        const bool bit = (value >> b) & 1u;
        const sj_u64 have = g.ballot([&](uint32_t) { return bit; });
        mask &= bit ? have : ~have;
    }
    return mask;
}
SJ_HD uint32_t sr_lowest(sj_u64 mask) { return (uint32_t)__builtin_ctzll(mask); }

// a tile's first walk: count[wave * SR_VALUES + value] = the pairs with that value in the wave's run.  Ends with a barrier.
template <class G>
SJ_HD void sr_wave_counts(const G& g, const SrColumn& c, uint32_t shift, sj_u64 tile, const sj_u64* keys, sj_u64 n, uint32_t* count) {
    const uint32_t width = g.lanes() / g.waves(), me = g.lane() - g.wave() * width, run = c.tile_rows / g.waves();
    for (uint32_t b = g.lane(); b < g.waves() * SR_VALUES; b += g.lanes()) count[b] = 0;
    g.sync();
    const sj_u64 first = tile * c.tile_rows + (sj_u64)g.wave() * run;
    for (sj_u64 at = first; at < first + run && at < n; at += width) {
        const sj_u64 i = at + me;
        const bool valid = i < n;
        const uint32_t value = valid ? (uint32_t)(keys[i] >> shift) & (SR_VALUES - 1) : 0u;
        const sj_u64 mask = sr_match(g, value, valid);
        if (valid && sr_lowest(mask) == me) count[g.wave() * SR_VALUES + value] += fl_popcount(mask);
        g.wave_fence();
    }
    g.sync();
}

// pass 4a, digit d, per tile with waves * SR_VALUES counts of its own
template <class G>
SJ_HD void sr_hist(const G& g, const SrColumn& c, uint32_t d, sj_u64 tile, sj_u64* ws, uint32_t* count) {
    const SrState* st = sr_state(ws);
    const sj_u64 n = st->n_cand, tiles = sr_tiles(c, n);
    if (d >= st->n_digits || tile >= tiles) return;  // (the whole group)
    sr_wave_counts(g, c, d * SR_DIGIT_BITS, tile, sr_keys(c, ws, d & 1u), n, count);
    sj_u64* table = sr_table(c, ws);
    for (uint32_t v = g.lane(); v < SR_VALUES; v += g.lanes()) {
        sj_u64 sum = 0;
        for (uint32_t w = 0; w < g.waves(); ++w) sum += count[w * SR_VALUES + v];
        table[(sj_u64)v * sr_tiles(c, c.n_rows) + tile] = sum;
    }
}

// pass 4b, digit d, group `value` of SR_VALUES: the pairs with this value in front of every tile
template <class G>
SJ_HD void sr_digit_scan(const G& g, const SrColumn& c, uint32_t d, uint32_t value, sj_u64* ws) {
    const SrState* st = sr_state(ws);
    if (d >= st->n_digits) return;
    const sj_u64 total = g.scan_in_place(sr_table(c, ws) + (sj_u64)value * sr_tiles(c, c.n_rows), sr_tiles(c, st->n_cand));
    if (g.lane() == 0) sr_totals(c, ws)[value] = total;
}

// pass 4c, digit d, per tile with SR_VALUES bases and starts, waves * SR_VALUES counts and tile_rows staged pairs of its own.  The
// pairs go to the group's own memory first, in the order of the output (by value, then by position), and from there to the
// output: neighbouring lanes then store neighbouring pairs of one value's run, whole lines where the run is long enough
template <class G>
SJ_HD void sr_scatter(const G& g, const SrColumn& c, uint32_t d, sj_u64 tile, sj_u64* ws, sj_u64* base, uint32_t* start, uint32_t* count,
                      sj_u64* staged_key, uint32_t* staged_pos) {
    const SrState* st = sr_state(ws);
    const sj_u64 n = st->n_cand, tiles = sr_tiles(c, n);
    if (d >= st->n_digits || tile >= tiles) return;  // (the whole group)
    const uint32_t shift = d * SR_DIGIT_BITS, from = d & 1u;
    const sj_u64* keys = sr_keys(c, ws, from);
    const uint32_t* pos = sr_positions(c, ws, from);
    sj_u64* keys_out = sr_keys(c, ws, from ^ 1u);
    uint32_t* pos_out = sr_positions(c, ws, from ^ 1u);
    // where the tile's pairs with value v begin in the output: the pairs with a smaller value, and those with v in the tiles in front
    const sj_u64* totals = sr_totals(c, ws);
    const sj_u64* table = sr_table(c, ws);
    sj_u64 below = 0;
    for (uint32_t at = 0; at < SR_VALUES; at += g.lanes()) {
        const uint32_t v = at + g.lane();
        sj_u64 total;
        const sj_u64 before = below + g.scan_add(v < SR_VALUES ? totals[v] : 0ull, &total);
        if (v < SR_VALUES) base[v] = before + table[(sj_u64)v * sr_tiles(c, c.n_rows) + tile];
        below += total;
    }
    sr_wave_counts(g, c, shift, tile, keys, n, count);
    // where they begin INSIDE the tile, and count[wave][value] -> the staged place of the wave's next pair with that value: the
    // values in order, the waves in wave order
    sj_u64 inside = 0;
    for (uint32_t at = 0; at < SR_VALUES; at += g.lanes()) {
        const uint32_t v = at + g.lane();
        sj_u64 mine = 0, total;
        if (v < SR_VALUES)
            for (uint32_t w = 0; w < g.waves(); ++w) mine += count[w * SR_VALUES + v];
        uint32_t next = (uint32_t)(inside + g.scan_add(mine, &total));
        if (v < SR_VALUES) {
            start[v] = next;
            for (uint32_t w = 0; w < g.waves(); ++w) {
                const uint32_t has = count[w * SR_VALUES + v];
                count[w * SR_VALUES + v] = next;
                next += has;
            }
        }
        inside += total;
    }
    g.sync();
    const uint32_t width = g.lanes() / g.waves(), me = g.lane() - g.wave() * width, run = c.tile_rows / g.waves();
    const sj_u64 tile_first = tile * c.tile_rows, first = tile_first + (sj_u64)g.wave() * run;
    for (sj_u64 at = first; at < first + run && at < n; at += width) {
        const sj_u64 i = at + me;
        const bool valid = i < n;
        const sj_u64 key = valid ? keys[i] : 0;
        const uint32_t value = (uint32_t)(key >> shift) & (SR_VALUES - 1);
        const sj_u64 mask = sr_match(g, value, valid);
        uint32_t* next = count + g.wave() * SR_VALUES + value;
        const uint32_t j = *next + fl_popcount(mask & ((1ull << me) - 1));
        g.wave_fence();  // (every lane has read the place before the value's lowest lane moves it on)
        if (valid && sr_lowest(mask) == me) *next += fl_popcount(mask);
        g.wave_fence();
        if (valid && j < c.tile_rows) {  // (always: j < the tile's pairs)
            staged_key[j] = key;
            staged_pos[j] = pos[i];
        }
    }
    g.sync();
    const sj_u64 left = n - tile_first;
    const uint32_t pairs = left < c.tile_rows ? (uint32_t)left : c.tile_rows;
    for (uint32_t s = g.lane(); s < pairs; s += g.lanes()) {
        const sj_u64 key = staged_key[s];
        const uint32_t value = (uint32_t)(key >> shift) & (SR_VALUES - 1);
        const sj_u64 j = base[value] + (s - start[value]);
        if (j < c.n_rows) {  // (always: j < n_cand)
            keys_out[j] = key;
            pos_out[j] = staged_pos[s];
        }
    }
}

// pass 5: output place j
SJ_HD void sr_gather(const SrColumn& c, const SrCarry& in, sj_u64 j, sj_u64* ws, const SrOut& o) {
    if (j >= sr_live(c)) return;
    const sj_u64 i = sr_positions(c, ws, sr_state(ws)->n_digits & 1u)[j];
    if (i >= c.n_rows) return;  // (never: every place holds a live position)
    const sj_u64 r = c.rows_in ? c.rows_in[i] : i;
    o.rows[j] = r;
    const bool bad = r >= c.n_source_rows;
    for (sj_u64 col = 0; col < in.n_cols; ++col) {
        o.types[col * o.stride + j] = bad ? (uint8_t)0 : in.types[col * in.col_stride + r];
        o.values[col * o.stride + j] = bad ? 0ull : in.values[col * in.col_stride + r];
    }
}
