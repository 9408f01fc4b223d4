// sj_joinrows.h -- two row sets joined on a long key: INNER, LEFT, SEMI, ANTI (include/sjmi.h, sjmi_join_rows_device; DESIGN.md
// 4.21).  A sort-merge join in which only the BUILD side is sorted: the caller has ordered the right side with
// sjmi_sort_rows_device (kind LONG, ascending, stable); every left position finds the run of build places with its key by two
// binary searches, the runs' lengths are scanned into pair offsets, and the pairs are written by OUTPUT chunk, each pair finding
// the left position that owns it with the load-balanced search of sj_parents.h.
//
// THE LEFT (PROBE) SIDE is an SrColumn of sj_sortrows.h: positions [0, live), live = min(n_left, *left_count) read HERE, on the
// device; sr_pos is the only reader of a position, with its classes (CANDIDATE, NULL, OTHER, BAD), its read order and its key.
// THE RIGHT (BUILD) SIDE is an SrColumn too: rows_in = the sort's d_rows, n_rows = the sort's n_rows, row_count = the
// n_candidates word of the sort's record.  Its live positions are the BUILD PLACES [0, n_build), n_build = min(n_right,
// n_candidates): the candidates of the right side by ascending key, equal keys by ascending right position.  Nothing behind them
// is read.  A place whose entry is at or above the source rows (never dereferenced) or whose cell is no candidate is counted in
// n_right_bad; such a place, and a key below the key of the place in front of it, set JR_BAD_ORDER: the pairs are then
// unspecified, and every load and store still stays inside its buffer -- a search ends inside [0, n_build], a build place is
// compared with n_build and a source row with the source rows before either addresses anything.
//
// m(i) = the build places whose key equals the key of candidate position i, 0 for every other class.  Position i emits e(i)
// pairs: INNER m, LEFT max(m, 1), SEMI m > 0, ANTI m == 0 -- so LEFT and ANTI keep every live position, NULL, OTHER and BAD ones
// included.  Pairs come out by ascending left position, inside one position by ascending build place.
//
// THE PASSES, each a kernel of csrc/joinrows.hip (the stream orders them; the scratch is read across kernel boundaries only):
//   jr_clear    ONE lane: the record with n_left = live and n_build, everything else 0; off[0] = 0
//   jr_keys     per chunk of build places: the key of every place into the dense sorted array of the scratch (0 for a bad place),
//               the bad places counted; every place's key against the key in front of it -- from the group's own memory where
//               that place is the chunk's, by a second gather at the chunk's first place
//   jr_count    per chunk of left positions: every step-th build key (step = ceil(n_build / chunk_rows)) into the group's own memory as
//               pivots; per position the class, a lower bound of the key -- among the pivots, then among the at most `step` places
//               between two of them -- and an upper bound that gallops from there (a unique key: three loads); lo[i] (JR_NO_MATCH
//               with m == 0) and e(i) as 32-bit words, the chunk's sum of e as a 64-bit word; n_null, n_other, n_bad and n_matched
//               by scan_add and one g.agent.add64 each
//   jr_scan     ONE group: the chunk sums scanned in place; n_pairs and the flags JR_OVERFLOW, JR_BAD_ROW
//   jr_offsets  per chunk of left positions: off[i + 1] = the chunk's base + the inclusive scan of e inside the chunk, into the
//               scratch and into pair_offsets where given -- explode's row_offsets with "left position = document, pair = row"
//   jr_emit     per chunk of OUTPUT pairs below n = min(n_pairs, pair_capacity): pa_dense's scheme on off[] -- pa_count_wave on the
//               chunk's first and last pair, the positions WITH pairs whose first pair lies in the chunk mark the group's own
//               memory (exactly one such position begins at any pair: no two lanes write one address), a running maximum; then
//               t = j - off[p], the build place lo[p] + t, the rows and the carried cells of both sides, every store behind j < n
// A HOT KEY IS NO HAZARD: one position with a million matches is a thousand output chunks, none of which begins a position; each
// finds its owner by the two searches.  Nothing spins or waits for another group; every loop is bounded by the positions, 33
// search steps, the chunk or the columns.  No atomic decides a place: the whole output is a function of the input alone.
//
// The lanes come from the caller: a workgroup G (sj_group.h; a chunk is a multiple of its lanes) with these members added:
//   g.agent.add64(p, v) / or32(p, v)   on the record (agent-scope relaxed atomics, results unused)
//   g.sync()                           a barrier of the group: what its lanes wrote to its own memory is visible to all of them
//   g.scan_max(v, &total)              called by every lane: the INCLUSIVE running maximum of v over the group's lanes
// uses: lanes, lane, waves, wave, first, ballot, scan_add, scan_in_place, agent, sync, scan_max.  csrc/joinrows.hip runs this
// file with the device form, tests/host_sim/joinrows_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_parents.h"
#include "sj_sortrows.h"

constexpr uint32_t JR_CHUNK_ROWS = 1024;  // left positions, build places and output pairs of a chunk
enum : uint32_t { JR_INNER = 0, JR_LEFT = 1, JR_SEMI = 2, JR_ANTI = 3 };  // SJMI_JOIN_<HOW>
constexpr uint32_t JR_OVERFLOW = 1u, JR_BAD_ROW = 2u, JR_BAD_ORDER = 4u;   // SJMI_JOIN_<FLAG>
constexpr uint32_t JR_RESULT_WORDS = 9;                                   // SJMI_JOIN_RESULT_WORDS
constexpr sj_u64 JR_NO_ROW = ~0ull;                                       // SJMI_JOIN_NO_ROW
constexpr uint32_t JR_NO_MATCH = 0xFFFFFFFFu;  // lo[i] of a position with m == 0 (with m > 0 the bound is below n_build < 2^32)
constexpr sj_u64 JR_MAX_PAIR_CAPACITY = 1ull << 40;  // one group per 1024 pairs
constexpr uint32_t JR_GATHER = 4;                    // carried columns whose loads are issued before the first of their stores

struct JrResult {  // sjmi_join_result
    sj_u64 n_left, n_build, n_pairs, n_matched, n_null, n_other, n_bad, n_right_bad;
    uint32_t flags, reserved;
};
static_assert(sizeof(JrResult) == JR_RESULT_WORDS * 8, "the record is whole words");

struct JrArgs {
    SrColumn left, right;  // (right: rows_in = the build order, row_count = the sort record's n_candidates)
    SrCarry left_carry, right_carry;
    uint32_t how, chunk_rows;
    sj_u64 pair_capacity;
    sj_u64* left_rows;    // [pair_capacity]
    sj_u64* right_rows;   // [pair_capacity]; may be NULL under SEMI and ANTI
    uint8_t* left_types;  // the carried cells, n_cols rows `out_stride` cells apart, any alignment
    sj_u64* left_values;
    uint8_t* right_types;
    sj_u64* right_values;
    sj_u64 out_stride;
    sj_u64* pair_offsets;  // [n_left + 1], may be NULL
};

// THE SCRATCH, in 64-bit words: n_right build keys | a sum per left chunk | n_left + 1 offsets | n_left 32-bit lower bounds | n_left
// 32-bit pair counts
SJ_HD sj_u64 jr_chunks(sj_u64 n, uint32_t chunk_rows) { return fc_chunks(n, chunk_rows); }
SJ_HD sj_u64* jr_keys_at(sj_u64* ws) { return ws; }
SJ_HD sj_u64* jr_sums(const JrArgs& a, sj_u64* ws) { return ws + a.right.n_rows; }
SJ_HD sj_u64* jr_off(const JrArgs& a, sj_u64* ws) { return jr_sums(a, ws) + jr_chunks(a.left.n_rows, a.chunk_rows); }
SJ_HD uint32_t* jr_lo(const JrArgs& a, sj_u64* ws) { return (uint32_t*)(jr_off(a, ws) + a.left.n_rows + 1); }
SJ_HD uint32_t* jr_e(const JrArgs& a, sj_u64* ws) { return jr_lo(a, ws) + a.left.n_rows + (a.left.n_rows & 1); }
SJ_HD sj_u64 jr_workspace_words(sj_u64 n_left, sj_u64 n_right, uint32_t chunk_rows) {
    return n_right + jr_chunks(n_left, chunk_rows) + n_left + 1 + 2 * ((n_left + 1) / 2);
}
SJ_HD sj_u64 jr_live(const JrArgs& a) { return sr_live(a.left); }
SJ_HD sj_u64 jr_build(const JrArgs& a) { return sr_live(a.right); }
SJ_HD sj_u64 jr_written(const JrArgs& a, const JrResult* res) { return res->n_pairs < a.pair_capacity ? res->n_pairs : a.pair_capacity; }

// pass 0, ONE lane
SJ_HD void jr_clear(const JrArgs& a, sj_u64* ws, JrResult* res) {
    res->n_left = jr_live(a);
    res->n_build = jr_build(a);
    res->n_pairs = res->n_matched = res->n_null = res->n_other = res->n_bad = res->n_right_bad = 0;
    res->flags = 0;
    res->reserved = 0;
    jr_off(a, ws)[0] = 0;
    if (a.pair_offsets) a.pair_offsets[0] = 0;
}

// build place p < n_build -> its key, and whether it is a candidate of a source row
SJ_HD bool jr_place(const JrArgs& a, sj_u64 p, sj_u64* key) {
    sj_u64 row;
    bool inexact = false;
    *key = 0;
    return sr_pos(a.right, p, &row, key, &inexact) == TR_CANDIDATE;
}

// pass 1, per chunk of build places; key_of = chunk_rows words and good = chunk_rows bytes of the group's own memory
template <class G>
SJ_HD void jr_keys(const G& g, const JrArgs& a, sj_u64 chunk, sj_u64* ws, sj_u64* key_of, uint8_t* good, JrResult* res) {
    const sj_u64 n_build = jr_build(a), first = chunk * a.chunk_rows;
    if (first >= n_build) return;  // (the whole group, in front of every barrier)
    sj_u64* keys = jr_keys_at(ws);
    sj_u64 bad = 0, descents = 0, n_bad, n_descents;
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 p = at + g.lane();
        if (p >= n_build) continue;
        sj_u64 key;
        const bool ok = jr_place(a, p, &key);
        if (!ok) key = 0;
        keys[p] = key;
        key_of[p - first] = key;
        good[p - first] = ok;
        bad += !ok;
    }
    g.sync();
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 p = at + g.lane();
        if (p >= n_build || p == 0 || !good[p - first]) continue;
        sj_u64 before;
        bool ok;
        if (p > first) {
            before = key_of[p - first - 1];
            ok = good[p - first - 1];
        } else {  // (the chunk's first place: the neighbour is another group's)
            ok = jr_place(a, p - 1, &before);
        }
        descents += ok && before > key_of[p - first];
    }
    (void)g.scan_add(bad, &n_bad);
    (void)g.scan_add(descents, &n_descents);
    if (g.lane() == 0) {
        if (n_bad) g.agent.add64(&res->n_right_bad, n_bad);
        if (n_bad || n_descents) g.agent.or32(&res->flags, JR_BAD_ORDER);
    }
}

// the first place in [lo, n) whose key is not below `key` (upper == false) or is above it (upper == true); n < 2^32: 33 steps
SJ_HD sj_u64 jr_bound(const sj_u64* keys, sj_u64 lo, sj_u64 n, sj_u64 key, bool upper) {
    sj_u64 hi = n;
    for (uint32_t step = 0; step < 34 && lo < hi; ++step) {
        const sj_u64 mid = lo + (hi - lo) / 2, k = keys[mid];
        if (upper ? k <= key : k < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the first place in [lo, n) whose key is above `key`, GALLOPING from lo: places lo, lo + 1, lo + 3, lo + 7, ... until one is above,
// then the search between the last two.  A key without a match costs one load, a unique one three; 33 + 33 steps at most
SJ_HD sj_u64 jr_upper(const sj_u64* keys, sj_u64 lo, sj_u64 n, sj_u64 key) {
    sj_u64 width = 1;
    for (uint32_t step = 0; step < 34; ++step) {
        const sj_u64 p = lo + width - 1;
        if (p >= n) break;
        if (keys[p] > key) {
            n = p;
            break;
        }
        lo = p + 1;
        width <<= 1;
    }
    return jr_bound(keys, lo, n, key, true);
}

// the lower bound of `key` in keys[0, n_build), through the chunk's pivots: pivots[k] = keys[k * step], k < n_pivots.  The first
// pivot that is not below the key bounds the places that the search has to look at: at most `step` of them
SJ_HD sj_u64 jr_lower(const sj_u64* keys, const sj_u64* pivots, sj_u64 n_pivots, sj_u64 step, sj_u64 n_build, sj_u64 key) {
    const sj_u64 k = jr_bound(pivots, 0, n_pivots, key, false);
    return jr_bound(keys, k ? (k - 1) * step + 1 : 0, k < n_pivots ? k * step : n_build, key, false);
}

// pass 2, per chunk of left positions; pivots = chunk_rows words of the group's own memory
template <class G>
SJ_HD void jr_count(const G& g, const JrArgs& a, sj_u64 chunk, sj_u64* ws, sj_u64* pivots, JrResult* res) {
    const sj_u64 live = jr_live(a), n_build = jr_build(a), first = chunk * a.chunk_rows;
    const sj_u64* keys = jr_keys_at(ws);
    uint32_t* lo_of = jr_lo(a, ws);
    uint32_t* e_of = jr_e(a, ws);
    // every step-th build key into the group's own memory: the first ten steps of a lower bound stay there
    const sj_u64 step = (n_build + a.chunk_rows - 1) / a.chunk_rows, n_pivots = step && first < live ? (n_build + step - 1) / step : 0;
    for (sj_u64 s = g.lane(); s < n_pivots; s += g.lanes()) pivots[s] = keys[s * step];
    g.sync();
    sj_u64 pairs = 0, w0 = 0, w1 = 0;  // w0 = NULL | OTHER << 32, w1 = BAD | matched << 32 (each at most the chunk)
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 i = at + g.lane();
        if (i >= live) continue;
        sj_u64 row, key = 0, m = 0, lo = 0;
        bool inexact = false;
        const uint32_t cls = sr_pos(a.left, i, &row, &key, &inexact);
        if (cls == TR_CANDIDATE) {
            lo = jr_lower(keys, pivots, n_pivots, step, n_build, key);
            m = jr_upper(keys, lo, n_build, key) - lo;
        } else if (cls == TR_NULL) {
            w0 += 1;
        } else if (cls == SR_BAD) {
            w1 += 1;
        } else {
            w0 += 1ull << 32;
        }
        const sj_u64 e = a.how == JR_INNER ? m : a.how == JR_LEFT ? (m ? m : 1) : a.how == JR_SEMI ? (sj_u64)(m > 0) : (sj_u64)(m == 0);
        if (m) w1 += 1ull << 32;
        lo_of[i] = m ? (uint32_t)lo : JR_NO_MATCH;
        e_of[i] = (uint32_t)e;  // (e <= max(n_build, 1) < 2^32)
        pairs += e;
    }
    sj_u64 n_pairs, t0, t1;
    (void)g.scan_add(pairs, &n_pairs);
    (void)g.scan_add(w0, &t0);
    (void)g.scan_add(w1, &t1);
    if (g.lane() == 0) {
        jr_sums(a, ws)[chunk] = n_pairs;
        if (t0 & 0xFFFFFFFFull) g.agent.add64(&res->n_null, t0 & 0xFFFFFFFFull);
        if (t0 >> 32) g.agent.add64(&res->n_other, t0 >> 32);
        if (t1 & 0xFFFFFFFFull) g.agent.add64(&res->n_bad, t1 & 0xFFFFFFFFull);
        if (t1 >> 32) g.agent.add64(&res->n_matched, t1 >> 32);
    }
}

// pass 3, ONE group
template <class G>
SJ_HD void jr_scan(const G& g, const JrArgs& a, sj_u64* ws, JrResult* res) {
    const sj_u64 total = g.scan_in_place(jr_sums(a, ws), jr_chunks(a.left.n_rows, a.chunk_rows));
    if (g.lane() == 0) {
        res->n_pairs = total;
        res->flags |= (total > a.pair_capacity ? JR_OVERFLOW : 0u) | (res->n_bad ? JR_BAD_ROW : 0u);
    }
}

// pass 4, per chunk of left positions
template <class G>
SJ_HD void jr_offsets(const G& g, const JrArgs& a, sj_u64 chunk, sj_u64* ws) {
    const sj_u64 live = jr_live(a), first = chunk * a.chunk_rows;
    if (first >= live) return;  // (the whole group, in front of every barrier)
    const uint32_t* e_of = jr_e(a, ws);
    sj_u64* off = jr_off(a, ws);
    sj_u64 run = jr_sums(a, ws)[chunk];
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 i = at + g.lane(), e = i < live ? e_of[i] : 0;
        sj_u64 total;
        const sj_u64 behind = run + g.scan_add(e, &total) + e;
        if (i < live) {
            off[i + 1] = behind;
            if (a.pair_offsets) a.pair_offsets[i + 1] = behind;
        }
        run += total;
    }
}

// the cells of source row r (none: type 0 and value 0) in every carried column, to pair j: the loads of JR_GATHER columns are
// issued before the first of their stores
SJ_HD void jr_cells(const SrCarry& in, sj_u64 r, bool none, uint8_t* types, sj_u64* values, sj_u64 stride, sj_u64 j) {
    for (sj_u64 c0 = 0; c0 < in.n_cols; c0 += JR_GATHER) {
        uint8_t t[JR_GATHER];
        sj_u64 v[JR_GATHER];
        for (uint32_t k = 0; k < JR_GATHER; ++k) {
            const bool there = c0 + k < in.n_cols && !none;
            t[k] = there ? in.types[(c0 + k) * in.col_stride + r] : 0;
            v[k] = there ? in.values[(c0 + k) * in.col_stride + r] : 0;
        }
        for (uint32_t k = 0; k < JR_GATHER && c0 + k < in.n_cols; ++k) {
            types[(c0 + k) * stride + j] = t[k];
            values[(c0 + k) * stride + j] = v[k];
        }
    }
}

// pair j of left position p
SJ_HD void jr_pair(const JrArgs& a, const sj_u64* ws_off, const uint32_t* lo_of, sj_u64 n_build, sj_u64 j, sj_u64 p) {
    const sj_u64 l = a.left.rows_in ? a.left.rows_in[p] : p;
    const uint32_t lo = lo_of[p];
    const sj_u64 place = (sj_u64)lo + (j - ws_off[p]);
    sj_u64 r = JR_NO_ROW;
    if (a.how != JR_ANTI && lo != JR_NO_MATCH && place < n_build) r = a.right.rows_in[place];
    a.left_rows[j] = l;
    if (a.right_rows) a.right_rows[j] = r;
    jr_cells(a.left_carry, l, l >= a.left.n_source_rows, a.left_types, a.left_values, a.out_stride, j);
    jr_cells(a.right_carry, r, r >= a.right.n_source_rows, a.right_types, a.right_values, a.out_stride, j);  // (NO_ROW is none)
}

// pass 5, per chunk of output pairs; marks = chunk_rows words and seeds = 2 words of the group's own memory
template <class G>
SJ_HD void jr_emit(const G& g, const JrArgs& a, sj_u64 chunk, sj_u64* ws, sj_u64* marks, sj_u64* seeds, const JrResult* res) {
    const sj_u64 n = jr_written(a, res), first = chunk * a.chunk_rows;
    if (first >= n) return;  // (the whole group, in front of every barrier)
    const sj_u64 live = jr_live(a), n_build = jr_build(a);
    const sj_u64 last = (first + a.chunk_rows < n ? first + a.chunk_rows : n) - 1;
    const sj_u64* off = jr_off(a, ws);
    const uint32_t* lo_of = jr_lo(a, ws);
    // (off[live] = n_pairs > last: both counts are below `live`)
    if (g.wave() == 0) {
        const sj_u64 c = pa_count_wave(g, off, live, first);
        if (g.first()) seeds[0] = c;
    }
    if (g.wave() == g.waves() - 1) {
        const sj_u64 c = pa_count_wave(g, off, live, last);
        if (g.first()) seeds[1] = c;
    }
    for (uint32_t s = g.lane(); s < a.chunk_rows; s += g.lanes()) marks[s] = 0;
    g.sync();
    const sj_u64 p_first = seeds[0], p_last = seeds[1] < live ? seeds[1] : live - 1;  // (live >= 1: there is a pair)
    for (sj_u64 at = p_first; at <= p_last; at += g.lanes()) {
        const sj_u64 p = at + g.lane();
        if (p > p_last) continue;
        const sj_u64 begin = off[p];
        if (off[p + 1] > begin && begin >= first && begin - first < a.chunk_rows) marks[begin - first] = p + 1;
    }
    g.sync();
    sj_u64 run = 0;
    for (sj_u64 at = first; at < first + a.chunk_rows; at += g.lanes()) {
        const sj_u64 j = at + g.lane();
        sj_u64 mine = marks[j - first];
        if (j == first && mine < p_first + 1) mine = p_first + 1;  // (the seed)
        sj_u64 highest;
        sj_u64 incl = g.scan_max(mine, &highest);
        if (incl < run) incl = run;
        if (highest > run) run = highest;
        if (j < n && incl - 1 < live) jr_pair(a, off, lo_of, n_build, j, incl - 1);
    }
}
