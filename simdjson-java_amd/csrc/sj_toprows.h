// sj_toprows.h -- the top k rows of ONE key column: ORDER BY a value, LIMIT k (include/sjmi.h, sjmi_top_rows_device; DESIGN.md
// 4.18).  An exact radix select on a 64-bit order-preserving unsigned key, then a sort of the k rows it took.
//
// The rows that count are [0, live), live = min(n_rows, *row_count) read HERE, on the device, where a row count is given.  tr_row
// is the only reader of a row: the validity word, then the type byte, then -- only behind a type byte that makes the cell a
// candidate -- the value word, each only behind the test in front of it.  A row is a CANDIDATE (its value takes part in the
// order), NULL (its validity bit is clear, or its type byte is MISSING or 'n'), OTHER (any other type byte that is no number of
// the chosen kind) or, under TR_DOUBLE, a NaN; every live row is exactly one of the four.  A candidate's KEY: a long with its sign
// bit flipped, a double through gs_okey (sj_okey.h; a long under TR_DOUBLE converted first, as sj_arrowcol.h converts it for a
// FLOAT64 field), and all bits complemented under TR_SMALLEST -- so every pass selects the LARGEST keys, and a key is a function
// of the cell alone.
//
// THE PASSES, each a kernel of csrc/toprows.hip (the stream orders them; the scratch is read across kernel boundaries only):
//   tr_clear_word   the state and the six histograms to their identities; word 0's lane writes the record with n_rows = live
//   tr_range        a GRID of groups, group, group + grid, ... of the chunks: every live row classified, the counts to the record,
//                   the minimum and the maximum key of the group's candidates to the state (one g.agent.umin / umax per group)
//   tr_plan         ONE lane: n_out = min(k, candidates); the bits above msb(min ^ max) are common to all candidates and go into
//                   the prefix as they are, the TR_DIGIT_BITS-bit digits below them are n_digits = ceil((msb + 1) / 11), 0 .. 6
//                   (min == max: no digit, every candidate ties)
//   tr_hist(d)      d < n_digits: the same grid; the digit d (from the top) of every candidate whose higher bits equal the prefix
//                   into TR_BINS bins of the group (g.wg), the non-zero bins to the pass's histogram in the scratch (g.agent)
//   tr_pick(d)      ONE group: the bins from the top until the count reaches what remains of k: the digit joins the prefix, the
//                   rows above it leave the remainder.  Behind the last pass prefix = T, the key of the last row taken,
//                   n_above = the candidates above T, rem = need_equal = n_out - n_above >= 1
//   tr_mark         per chunk: its candidates above T and equal to T, packed in one word (both below 2^32)
//   tr_scan         ONE group: the exclusive scan of these words (no carry leaves the low half: n_rows < 2^32)
//   tr_emit         per chunk: a row above T is taken; a row equal to T is taken iff fewer than need_equal rows equal to T lie in
//                   front of it IN ROW ORDER; the taken rows as (key, 32-bit row) into n_out slots of the scratch
//   tr_sort         ONE group: the slots into the group's own memory, a bitonic network under (key descending, row ascending) --
//                   a strict total order, so the result is the sorted sequence whatever the network --, then the rows, the
//                   carried cells and kth_bits
// With k == 0 only the first three run.  Every count is a sum of integers and every choice a function of keys and row indices:
// the whole output is a function of the input alone, whatever the order of the groups.  Nothing spins or waits for another
// group; every loop is bounded by the rows, the bins or the network's stages.  A 32-BIT BIN CANNOT OVERFLOW: n_rows < 2^32.
//
// The lanes come from the caller: a workgroup G (sj_group.h; a chunk is a multiple of its lanes, and TR_BINS of them) with
// these members added:
//   g.wg.add32(p, n)                    on the group's own bins (on the device an LDS atomic at workgroup scope)
//   g.agent.add32 / add64 / umin / umax on the scratch and the record (agent-scope relaxed atomics, results unused)
//   g.sync()                            a barrier of the group: what its lanes wrote to its own memory is visible to all of them
//   g.all_umin(v) / g.all_umax(v)       called by every lane: the minimum / maximum of v over the group's lanes, in every lane
// uses: lanes, lane, scan_add, scan_in_place, wg, agent, sync, all_umin, all_umax.  csrc/toprows.hip runs this file with the
// device form, tests/host_sim/toprows_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_arrowcol.h"
#include "sj_okey.h"

constexpr uint32_t TR_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t TR_MAX_K = 2048;       // SJMI_TOP_MAX_K: the final sort is one workgroup's, in LDS
constexpr uint32_t TR_DIGIT_BITS = 11, TR_BINS = 1u << TR_DIGIT_BITS;  // 2048 32-bit bins = 8 KiB of LDS
constexpr uint32_t TR_MAX_DIGITS = 6;     // ceil(64 / 11)
constexpr uint32_t TR_MAX_GRID = 512;     // groups of tr_range and tr_hist: two workgroups of 1024 lanes on each of 256 CUs
enum : uint32_t { TR_LONG = 1, TR_DOUBLE = 2 };  // SJMI_TOP_<KIND>
constexpr uint32_t TR_SMALLEST = 1u;             // SJMI_TOP_SMALLEST
constexpr uint32_t TR_RESULT_WORDS = 9;          // SJMI_TOP_RESULT_WORDS

struct TrResult {  // sjmi_top_result
    sj_u64 n_rows, n_candidates, n_null, n_other, n_nan, n_inexact, n_out, kth_bits;
    uint32_t flags, reserved;
};

struct TrColumn {
    const uint8_t* types;    // NULL: every valid row is a number of the kind.  Any alignment: loaded as bytes
    const sj_u64* validity;  // NULL: every live row is valid
    const sj_u64* values;    // loaded only behind the tests in front of it
    sj_u64 n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
    uint32_t kind, flags;
    sj_u64 k;
    uint32_t chunk_rows;
};
// the columns that travel with the rows, and where everything goes
struct TrCarry {
    const uint8_t* types;  // any alignment
    const sj_u64* values;
    sj_u64 n_cols, col_stride;
};
struct TrOut {
    sj_u64* rows;    // [k]
    uint8_t* types;  // [n_cols * k], any alignment
    sj_u64* values;  // [n_cols * k]
};

// THE SCRATCH, in 64-bit words: the state | TR_MAX_DIGITS histograms of TR_BINS 32-bit bins | a word per chunk | k keys | k 32-bit
// rows
struct TrState {
    sj_u64 min_key, max_key;  // of the candidates; ~0 / 0 where there is none
    sj_u64 prefix;            // the bits of T found so far, the others 0
    sj_u64 rem;               // what remains of n_out below the prefix; in the end need_equal
    sj_u64 n_above;           // candidates above every key with this prefix
    uint32_t n_digits, reserved;
};
constexpr sj_u64 TR_STATE_WORDS = sizeof(TrState) / 8, TR_HIST_WORDS = (sj_u64)TR_MAX_DIGITS * TR_BINS / 2;
static_assert(sizeof(TrState) == 48 && sizeof(TrResult) == TR_RESULT_WORDS * 8, "the state and the record are whole words");
SJ_HD sj_u64 tr_live(const TrColumn& c) { return fc_live(c.n_rows, c.row_count); }
SJ_HD sj_u64 tr_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }
SJ_HD TrState* tr_state(sj_u64* ws) { return (TrState*)ws; }
SJ_HD uint32_t* tr_hists(sj_u64* ws) { return (uint32_t*)(ws + TR_STATE_WORDS); }
SJ_HD sj_u64* tr_counts(sj_u64* ws) { return ws + TR_STATE_WORDS + TR_HIST_WORDS; }
SJ_HD sj_u64* tr_cand_keys(const TrColumn& c, sj_u64* ws) { return tr_counts(ws) + tr_chunks(c.n_rows, c.chunk_rows); }
SJ_HD uint32_t* tr_cand_rows(const TrColumn& c, sj_u64* ws) { return (uint32_t*)(tr_cand_keys(c, ws) + c.k); }
SJ_HD sj_u64 tr_workspace_words(sj_u64 n_rows, sj_u64 k, uint32_t chunk_rows) {
    return TR_STATE_WORDS + TR_HIST_WORDS + tr_chunks(n_rows, chunk_rows) + k + (k + 1) / 2;
}
// the groups of tr_range and tr_hist for n_rows rows (>= 1)
SJ_HD uint32_t tr_grid(sj_u64 n_rows, uint32_t chunk_rows) {
    const sj_u64 want = tr_chunks(n_rows, chunk_rows);
    return want > TR_MAX_GRID ? TR_MAX_GRID : (uint32_t)want;
}

// the live row r -> its class; a candidate's key, and whether a long had to be rounded to become a double
enum : uint32_t { TR_CANDIDATE = 0, TR_NULL = 1, TR_OTHER = 2, TR_NAN = 3 };
SJ_HD uint32_t tr_row(const TrColumn& c, sj_u64 r, sj_u64* key, bool* inexact) {
    if (c.validity && !((c.validity[r >> 6] >> (r & 63)) & 1)) return TR_NULL;
    sj_u64 bits;
    if (c.types) {
        const uint8_t t = c.types[r];
        if (t == 'l') {
            const sj_u64 v = c.values[r];
            if (c.kind == TR_LONG) {
                bits = v;
            } else {  // (as ac_cell converts an 'l' cell of a FLOAT64 field)
                bits = ac_double_bits((double)(int64_t)v);
                *inexact = !ac_exact_as_double(v);
            }
        } else if (t == 'd' && c.kind == TR_DOUBLE) {
            bits = c.values[r];
        } else {
            return t == 0 || t == 'n' ? TR_NULL : TR_OTHER;
        }
    } else {
        bits = c.values[r];
    }
    if (c.kind == TR_DOUBLE && gs_is_nan(bits)) return TR_NAN;
    const sj_u64 k = c.kind == TR_LONG ? bits ^ GS_SIGN : gs_okey(bits);
    *key = (c.flags & TR_SMALLEST) ? ~k : k;
    return TR_CANDIDATE;
}
// a key back into the value word of the chosen kind
SJ_HD sj_u64 tr_value(const TrColumn& c, sj_u64 key) {
    const sj_u64 k = (c.flags & TR_SMALLEST) ? ~key : key;
    return c.kind == TR_LONG ? k ^ GS_SIGN : gs_okey_bits(k);
}
// key >> s, for s up to 66
SJ_HD sj_u64 tr_high(sj_u64 key, uint32_t s) { return s >= 64 ? 0 : key >> s; }

// clearing: word i of the state and the histograms; the lane of word 0 writes the record
SJ_HD void tr_clear_word(const TrColumn& c, sj_u64 i, sj_u64* ws, TrResult* res) {
    if (i < TR_STATE_WORDS + TR_HIST_WORDS) ws[i] = i == 0 ? ~0ull : 0;  // (word 0 is min_key)
    if (i == 0) {
        res->n_rows = tr_live(c);
        res->n_candidates = res->n_null = res->n_other = res->n_nan = res->n_inexact = 0;
        res->n_out = 0;
        res->kth_bits = 0;
        res->flags = 0;
        res->reserved = 0;
    }
}

// pass 1: group `group` of `grid`
template <class G>
SJ_HD void tr_range(const G& g, const TrColumn& c, sj_u64 group, sj_u64 grid, sj_u64* ws, TrResult* res) {
    const sj_u64 live = tr_live(c);
    sj_u64 lo = ~0ull, hi = 0, n_cand = 0, n_null = 0, n_other = 0, n_nan = 0, rounded = 0;
    for (sj_u64 first = group * c.chunk_rows; first < live; first += grid * c.chunk_rows)
        for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
            const sj_u64 r = at + g.lane();
            if (r >= live) continue;
            sj_u64 key = 0;
            bool inexact = false;
            const uint32_t cls = tr_row(c, r, &key, &inexact);
            n_null += cls == TR_NULL;
            n_other += cls == TR_OTHER;
            n_nan += cls == TR_NAN;
            if (cls != TR_CANDIDATE) continue;
            ++n_cand;
            rounded += inexact;
            lo = key < lo ? key : lo;
            hi = key > hi ? key : hi;
        }
    lo = g.all_umin(lo);
    hi = g.all_umax(hi);
    sj_u64 total[4], n_rounded;
    (void)g.scan_add(n_cand, &total[TR_CANDIDATE]);
    (void)g.scan_add(n_null, &total[TR_NULL]);
    (void)g.scan_add(n_other, &total[TR_OTHER]);
    (void)g.scan_add(n_nan, &total[TR_NAN]);
    (void)g.scan_add(rounded, &n_rounded);
    if (g.lane() == 0) {
        TrState* st = tr_state(ws);
        if (total[TR_CANDIDATE]) {
            g.agent.umin(&st->min_key, lo);
            g.agent.umax(&st->max_key, hi);
            g.agent.add64(&res->n_candidates, total[TR_CANDIDATE]);
        }
        if (total[TR_NULL]) g.agent.add64(&res->n_null, total[TR_NULL]);
        if (total[TR_OTHER]) g.agent.add64(&res->n_other, total[TR_OTHER]);
        if (total[TR_NAN]) g.agent.add64(&res->n_nan, total[TR_NAN]);
        if (n_rounded) g.agent.add64(&res->n_inexact, n_rounded);
    }
}

// pass 2, ONE lane: how many rows go out, and which bits the digit passes have to look at
SJ_HD void tr_plan(const TrColumn& c, sj_u64* ws, TrResult* res) {
    TrState* st = tr_state(ws);
    const sj_u64 n_out = c.k < res->n_candidates ? c.k : res->n_candidates;
    res->n_out = n_out;
    st->rem = n_out;
    st->n_above = 0;
    st->reserved = 0;
    const sj_u64 differ = n_out ? st->min_key ^ st->max_key : 0;
    const uint32_t bits = differ ? 64u - (uint32_t)__builtin_clzll(differ) : 0u;  // msb + 1
    st->n_digits = (bits + TR_DIGIT_BITS - 1) / TR_DIGIT_BITS;
    const uint32_t low = st->n_digits * TR_DIGIT_BITS;
    st->prefix = n_out && low < 64 ? (st->max_key >> low) << low : 0;
}

// pass 3a, digit d from the top: group `group` of `grid` with its TR_BINS bins
template <class G>
SJ_HD void tr_hist(const G& g, const TrColumn& c, uint32_t d, sj_u64 group, sj_u64 grid, sj_u64* ws, uint32_t* bins) {
    const TrState* st = tr_state(ws);
    if (d >= st->n_digits) return;  // (the whole group)
    const uint32_t shift = (st->n_digits - 1 - d) * TR_DIGIT_BITS, known = shift + TR_DIGIT_BITS;
    const sj_u64 above = tr_high(st->prefix, known), live = tr_live(c);
    for (uint32_t b = g.lane(); b < TR_BINS; b += g.lanes()) bins[b] = 0;
    g.sync();
    for (sj_u64 first = group * c.chunk_rows; first < live; first += grid * c.chunk_rows)
        for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
            const sj_u64 r = at + g.lane();
            if (r >= live) continue;
            sj_u64 key = 0;
            bool inexact = false;
            if (tr_row(c, r, &key, &inexact) != TR_CANDIDATE || tr_high(key, known) != above) continue;
            g.wg.add32(bins + ((key >> shift) & (TR_BINS - 1)), 1);
        }
    g.sync();
    uint32_t* hist = tr_hists(ws) + (sj_u64)d * TR_BINS;
    for (uint32_t b = g.lane(); b < TR_BINS; b += g.lanes())
        if (bins[b]) g.agent.add32(hist + b, bins[b]);
}

// pass 3b, ONE group: the bin in which the count from the top reaches the remainder.  Exactly one lane finds it: 1 <= rem <= the
// candidates under the prefix, which are the sum of the bins
template <class G>
SJ_HD void tr_pick(const G& g, uint32_t d, sj_u64* ws) {
    TrState* st = tr_state(ws);
    if (d >= st->n_digits) return;
    const uint32_t shift = (st->n_digits - 1 - d) * TR_DIGIT_BITS;
    const sj_u64 rem = st->rem;
    const uint32_t* hist = tr_hists(ws) + (sj_u64)d * TR_BINS;
    sj_u64 run = 0;
    for (uint32_t at = 0; at < TR_BINS; at += g.lanes()) {
        const uint32_t i = at + g.lane();
        const sj_u64 count = i < TR_BINS ? hist[TR_BINS - 1 - i] : 0;
        sj_u64 total;
        const sj_u64 before = run + g.scan_add(count, &total);  // (a barrier: every lane has read rem)
        if (before < rem && rem <= before + count) {
            st->prefix |= (sj_u64)(TR_BINS - 1 - i) << shift;
            st->rem = rem - before;
            st->n_above += before;
        }
        run += total;
    }
}

// what row r adds to its chunk's word: 1 above T, 2^32 equal to T
SJ_HD sj_u64 tr_mark_row(const TrColumn& c, sj_u64 r, sj_u64 live, sj_u64 T, sj_u64* key) {
    bool inexact = false;
    if (r >= live || tr_row(c, r, key, &inexact) != TR_CANDIDATE) return 0;
    return *key > T ? 1ull : *key == T ? 1ull << 32 : 0ull;
}

// pass 4a, per chunk (k > 0)
template <class G>
SJ_HD void tr_mark(const G& g, const TrColumn& c, sj_u64 chunk, sj_u64* ws) {
    const sj_u64 live = tr_live(c), T = tr_state(ws)->prefix, first = chunk * c.chunk_rows;
    sj_u64 mine = 0, total;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        sj_u64 key = 0;
        mine += tr_mark_row(c, at + g.lane(), live, T, &key);
    }
    (void)g.scan_add(mine, &total);
    if (g.lane() == 0) tr_counts(ws)[chunk] = total;
}

// pass 4b, ONE group
template <class G>
SJ_HD void tr_scan(const G& g, const TrColumn& c, sj_u64* ws) {
    (void)g.scan_in_place(tr_counts(ws), tr_chunks(c.n_rows, c.chunk_rows));
}

// pass 4c, per chunk.  A chunk that begins at or above `live` does nothing at all: the whole group leaves in front of the scans.
template <class G>
SJ_HD void tr_emit(const G& g, const TrColumn& c, sj_u64 chunk, sj_u64* ws) {
    const TrState* st = tr_state(ws);
    const sj_u64 live = tr_live(c), T = st->prefix, need = st->rem, first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64* keys = tr_cand_keys(c, ws);
    uint32_t* rows = tr_cand_rows(c, ws);
    sj_u64 run = tr_counts(ws)[chunk];  // above | equal << 32, in front of this chunk, then in front of this trip
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        sj_u64 key = 0, total;
        const sj_u64 mine = tr_mark_row(c, r, live, T, &key);
        const sj_u64 before = run + g.scan_add(mine, &total);
        const sj_u64 above = before & 0xFFFFFFFFull, equal = before >> 32;
        if ((mine & 1) || (mine && equal < need)) {
            const sj_u64 j = above + (equal < need ? equal : need);
            if (j < c.k) {  // (always: j < n_above + need_equal = n_out <= k)
                keys[j] = key;
                rows[j] = (uint32_t)r;
            }
        }
        run += total;
    }
}

// does (key a, row ra) come before (key b, row rb)?
SJ_HD bool tr_before(sj_u64 a, uint32_t ra, sj_u64 b, uint32_t rb) { return a > b || (a == b && ra < rb); }

// pass 5, ONE group with TR_MAX_K keys and rows of its own
template <class G>
SJ_HD void tr_sort(const G& g, const TrColumn& c, const TrCarry& in, sj_u64* ws, sj_u64* s_key, uint32_t* s_row, const TrOut& o, TrResult* res) {
    const TrState* st = tr_state(ws);
    sj_u64 n_out = st->n_above + st->rem;
    if (n_out > c.k) n_out = c.k;  // (never)
    if (!n_out) return;
    uint32_t n2 = 2;
    while (n2 < n_out) n2 <<= 1;
    const sj_u64* keys = tr_cand_keys(c, ws);
    const uint32_t* rows = tr_cand_rows(c, ws);
    // (the padding sorts behind every row: no row is 2^32 - 1)
    for (uint32_t i = g.lane(); i < n2; i += g.lanes()) {
        s_key[i] = i < n_out ? keys[i] : 0;
        s_row[i] = i < n_out ? rows[i] : 0xFFFFFFFFu;
    }
    g.sync();
    for (uint32_t size = 2; size <= n2; size <<= 1)
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
            for (uint32_t p = g.lane(); p < n2 / 2; p += g.lanes()) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const bool forward = (i & size) == 0;  // (the last size: everywhere)
                const sj_u64 a = s_key[i], b = s_key[l];
                const uint32_t ra = s_row[i], rb = s_row[l];
                if (forward ? tr_before(b, rb, a, ra) : tr_before(a, ra, b, rb)) {
                    s_key[i] = b, s_key[l] = a;
                    s_row[i] = rb, s_row[l] = ra;
                }
            }
            g.sync();
        }
    for (uint32_t j = g.lane(); j < n_out; j += g.lanes()) {
        const sj_u64 r = s_row[j];
        o.rows[j] = r;
        if (r >= c.n_rows) continue;  // (never: every slot holds a live row)
        for (sj_u64 col = 0; col < in.n_cols; ++col) {
            o.types[col * c.k + j] = in.types[col * in.col_stride + r];
            o.values[col * c.k + j] = in.values[col * in.col_stride + r];
        }
    }
    if (g.lane() == 0) res->kth_bits = tr_value(c, s_key[n_out - 1]);
}
