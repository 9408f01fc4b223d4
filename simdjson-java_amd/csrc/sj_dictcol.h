// sj_dictcol.h -- dictionary-encoding ONE string column of the selector's (type, value) encoding into Arrow's dictionary shape:
// an int32 index per row, an LSB-first validity bitmap, and the dictionary -- one entry per distinct value IN THE ORDER OF FIRST
// OCCURRENCE -- as the row of every entry's first occurrence, int64 offsets and the bytes (include/sjmi.h,
// sjmi_dictionary_column_device).
//
// Row r is VALID iff types[r] == '"'; its length is values[r] >> 32 and its bytes lie at sb + (values[r] & 0xFFFFFFFF).  Two
// VALID rows are EQUAL iff they have the same length and the same bytes.  The rows that count are [0, live), live = min(n_rows,
// *row_count) read HERE, on the device, where a row count is given.  dc_type is the only reader of a type byte, dc_insert_chunk
// the only reader of a value word of the input, behind the type test; a string's bytes are read as the naturally aligned 8-byte
// words that hold at least one of them (dc_word) -- such a word lies in the page, and so in the allocation, of that byte.
//
// THE TABLE.  slots = the smallest power of two >= 2 * dict_capacity (and >= 2), two words per slot.  OWNER = a 24-bit tag (the
// hash's top bits) above the 40-bit row that claimed the slot, DC_EMPTY (all ones) while nobody has; FIRST = the smallest row
// seen with the slot's value, all ones at first.  OWNER is written ONCE, FIRST only shrinks.  The table's words are touched
// through three members of the group only -- load, cas, fetch_min -- which on the device are agent-scope relaxed atomics: a
// load is a hint (it may be stale: "empty" where a row sits, a FIRST that has shrunk since), the cas / fetch_min behind it
// decides.  The tag never decides equality: behind a matching tag the length and the bytes of the owner row's string -- input
// data, which nobody writes -- are compared.  A probe is linear, bounded by `slots`; a row that finds no place is counted
// (then more than `slots` > dict_capacity values are distinct: the call overflows).  Nothing spins or waits for another group.
//
// THE PASSES, each a kernel of csrc/dictcol.hip (the stream orders them; the table is read across kernel boundaries only):
//   dc_insert_chunk  per chunk: the validity words, slot_of_row[r], the chunk's counts (VALID, other-typed, placeless) packed
//   dc_count_chunk   per chunk: how many of its rows are FIRST rows (FIRST[slot(r)] == r)
//   dc_scan          ONE group: the first rows in front of every chunk (in place), the record, the dictionary's row count
//   dc_emit_chunk    per chunk: a first row's rank into its slot's OWNER word (the tag and row have served), its row into
//                    dict_rows, its cell into the compacted scratch column
//   dc_index_chunk   per chunk: indices[r] = the rank in slot(r)
//   then sj_strcol.h's passes over the compacted column, whose row count is read on the device (sc_chunk_sums, dc_dict_scan in
//   place of sc_chunk_scan -- the same scan, another record --, sc_offsets, sc_copy_wave): the dictionary is gathered by the
//   string gather's code.
// The output is a function of the input alone: which row owns a slot depends on the schedule, but a value's FIRST, and so the
// ranks, the indices and the dictionary, do not.
//
// The lanes come from the caller: a workgroup G (sj_group.h; the chunk is a multiple of 64 rows, one row per lane) with the
// three table members added; uses: lanes, lane, scan_add, scan_in_place, validity_bit, load, cas, fetch_min.  csrc/dictcol.hip
// runs this file with the device form, tests/host_sim/dictcol_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"
#include "sj_strcol.h"

constexpr uint32_t DC_CHUNK_ROWS = 1024;       // rows of a chunk = threads of its workgroup
constexpr uint32_t DC_MAX_ENTRIES = 1u << 20;  // SJMI_DICT_MAX_ENTRIES
constexpr uint32_t DC_OVERFLOW = 1u;           // SJMI_DICT_OVERFLOW
constexpr uint32_t DC_BYTES_OVERFLOW = 2u;     // SJMI_DICT_BYTES_OVERFLOW
constexpr sj_u64 DC_EMPTY = ~0ull;             // an OWNER nobody has claimed, a FIRST nobody has shrunk
constexpr uint32_t DC_ROW_BITS = 40;           // n_rows < 2^40: a row never reaches the all-ones of DC_EMPTY
constexpr sj_u64 DC_ROW_MASK = (1ull << DC_ROW_BITS) - 1;
constexpr uint32_t DC_NO_SLOT = 0xFFFFFFFFu;   // slot_of_row of a NULL row, and of a VALID row that found no place

struct DcResult {  // sjmi_dict_result
    sj_u64 n_rows, n_valid, n_other, n_distinct, dict_bytes;
    uint32_t flags, reserved;
};

struct DcColumn {
    const uint8_t* types;  // any alignment: loaded as bytes
    const sj_u64* values;
    sj_u64 n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
    const uint8_t* sb;
    uint32_t chunk_rows;  // a multiple of 64
};
// the frame's chunks and live rows (sj_fieldcol.h) on this operator's column
SJ_HD sj_u64 dc_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }
SJ_HD sj_u64 dc_live(const DcColumn& c) { return fc_live(c.n_rows, c.row_count); }
SJ_HD sj_u64 dc_slots(sj_u64 dict_capacity) {
    sj_u64 s = 2;
    while (s < 2 * dict_capacity) s <<= 1;
    return s;
}

struct DcTable {
    sj_u64* words;  // OWNER of slot s at [2 s], FIRST at [2 s + 1]: a slot is 16 bytes of one line
    sj_u64 slots;   // a power of two
};

// The context's scratch of one call, in 8-byte words: [the dictionary's row count: 8 words][the table][a count and a first-row
// count per chunk][the compacted column: values, then types][the strcol sums over it][slot_of_row: 4 bytes a row]
struct DcScratch {
    sj_u64* dict_n;  // rows of the compacted column = entries of the dictionary (0 under DC_OVERFLOW)
    DcTable table;
    sj_u64 *counts, *firsts;
    sj_u64* cvalues;
    uint8_t* ctypes;
    sj_u64* sums;  // sc_sums() over dc_chunks(dict_capacity) chunks
    uint32_t* slot_of_row;
};
SJ_HD sj_u64 dc_scratch_words(sj_u64 n_rows, sj_u64 dict_capacity, uint32_t chunk_rows) {
    const sj_u64 nchunks = dc_chunks(n_rows, chunk_rows);
    return 8 + 2 * dc_slots(dict_capacity) + 2 * nchunks + dict_capacity + (dict_capacity + 7) / 8 + 3 * dc_chunks(dict_capacity, SC_CHUNK_ROWS) + 1 +
           (n_rows + 1) / 2;
}
SJ_HD DcScratch dc_scratch(void* ws, sj_u64 n_rows, sj_u64 dict_capacity, uint32_t chunk_rows) {
    const sj_u64 nchunks = dc_chunks(n_rows, chunk_rows);
    sj_u64* p = (sj_u64*)ws;
    DcScratch s;
    s.dict_n = p, p += 8;
    s.table.words = p, s.table.slots = dc_slots(dict_capacity), p += 2 * s.table.slots;
    s.counts = p, p += nchunks;
    s.firsts = p, p += nchunks;
    s.cvalues = p, p += dict_capacity;
    s.ctypes = (uint8_t*)p, p += (dict_capacity + 7) / 8;
    s.sums = p, p += 3 * dc_chunks(dict_capacity, SC_CHUNK_ROWS) + 1;
    s.slot_of_row = (uint32_t*)p;
    return s;
}

// ---- the hash ------------------------------------------------------------------------------------------------------------
// Word k of a string is its bytes [8 k, 8 k + 8) as a little-endian number, bytes at or behind `len` being 0.  dc_hash is a
// FIXED function of (the bytes, the length), with no seed:
//     h = DC_SEED ^ len * DC_LEN_MUL;  for every word w, in order: h = (h ^ w) * DC_MUL, h ^= h >> 29;  at last h = dc_mix(h)
// dc_mix(x): x ^= x >> 32, x *= DC_MIX_MUL, x ^= x >> 32, x *= DC_MIX_MUL, x ^= x >> 32 -- all modulo 2^64.  The probe begins at
// h & (slots - 1), the tag is h >> 40.  tests/dictcol_common.py restates it in Python to build colliding strings.
constexpr sj_u64 DC_SEED = 0x9E3779B97F4A7C15ull, DC_LEN_MUL = 0xC2B2AE3D27D4EB4Full, DC_MUL = 0x9FB21C651E98DF25ull,
                 DC_MIX_MUL = 0xD6E8FEB86659FD93ull;
SJ_HD sj_u64 dc_mix(sj_u64 x) {
    x ^= x >> 32;
    x *= DC_MIX_MUL;
    x ^= x >> 32;
    x *= DC_MIX_MUL;
    x ^= x >> 32;
    return x;
}
// word k of the string [at, at + len), 8 k < len: from the one or two aligned words that hold its bytes.  The second is loaded
// only where it holds a byte of the string.
SJ_HD sj_u64 dc_word(const uint8_t* at, sj_u64 len, sj_u64 k) {
    const uint8_t* p = at + 8 * k;
    const sj_u64 rem = len - 8 * k;  // >= 1
    const uint32_t skip = (uint32_t)((uintptr_t)p & 7);
    const sj_u64* base = (const sj_u64*)(p - skip);
    sj_u64 w = base[0] >> (8 * skip);
    if (skip && rem > 8 - skip) w |= base[1] << (64 - 8 * skip);
    if (rem < 8) w &= (1ull << (8 * rem)) - 1;
    return w;
}
SJ_HD sj_u64 dc_hash(const uint8_t* at, sj_u64 len) {
    sj_u64 h = DC_SEED ^ (len * DC_LEN_MUL);
    for (sj_u64 k = 0; 8 * k < len; ++k) {
        h = (h ^ dc_word(at, len, k)) * DC_MUL;
        h ^= h >> 29;
    }
    return dc_mix(h);
}
SJ_HD bool dc_equal(const uint8_t* a, const uint8_t* b, sj_u64 len) {
    if (a == b) return true;
    for (sj_u64 k = 0; 8 * k < len; ++k)
        if (dc_word(a, len, k) != dc_word(b, len, k)) return false;
    return true;
}

SJ_HD uint8_t dc_type(const DcColumn& c, sj_u64 r) { return c.types[r]; }

// clearing: word i of the table
SJ_HD void dc_clear_word(const DcTable& t, sj_u64 i) {
    if (i < 2 * t.slots) t.words[i] = DC_EMPTY;
}

// The VALID row r with the value word v into the table -> its slot, or DC_NO_SLOT.  Every slot the probe passes is taken for
// good (OWNER is written once), so two rows of one value walk the same slots and end in the same one: a value has ONE slot.
template <class G>
SJ_HD uint32_t dc_insert_row(const G& g, const DcColumn& c, const DcTable& t, sj_u64 r, sj_u64 v) {
    const sj_u64 len = v >> 32;
    const uint8_t* at = c.sb + (uint32_t)v;
    const sj_u64 h = dc_hash(at, len);
    const sj_u64 mine = ((h >> DC_ROW_BITS) << DC_ROW_BITS) | r;
    sj_u64 s = h & (t.slots - 1);
    for (sj_u64 trip = 0; trip < t.slots; ++trip, s = (s + 1) & (t.slots - 1)) {
        sj_u64* owner = t.words + 2 * s;
        sj_u64 o = g.load(owner);  // a hint: "empty" may be stale, an owner never is
        if (o == DC_EMPTY) {
            o = g.cas(owner, DC_EMPTY, mine);  // -> what was there: the truth
            if (o == DC_EMPTY) o = mine;
        }
        if ((o ^ mine) >> DC_ROW_BITS) continue;  // another tag: another value
        const sj_u64 orow = o & DC_ROW_MASK;
        if (orow != r) {  // the same tag decides nothing: the owner row's string does
            const sj_u64 ov = c.values[orow];
            if ((ov >> 32) != len || !dc_equal(c.sb + (uint32_t)ov, at, len)) continue;
        }
        if (g.load(owner + 1) > r) (void)g.fetch_min(owner + 1, r);  // (a stale FIRST: one fetch_min that changes nothing)
        return (uint32_t)s;
    }
    return DC_NO_SLOT;
}

// a chunk's counts in one word: each is at most the chunk's rows, and a chunk has at most 2^20 - 1
constexpr uint32_t DC_COUNT_BITS = 20;
constexpr sj_u64 DC_COUNT_MASK = (1ull << DC_COUNT_BITS) - 1;

// pass 1, per chunk: its live rows into the table; validity (may be NULL), slot_of_row, counts[chunk].  A chunk that begins at
// or above `live` does nothing at all -- the whole group leaves in front of the scan, which every lane reaches otherwise.
template <class G>
SJ_HD void dc_insert_chunk(const G& g, const DcColumn& c, const DcTable& t, sj_u64 chunk, sj_u64* validity, uint32_t* slot_of_row, sj_u64* counts) {
    const sj_u64 live = dc_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64 sum = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        bool valid = false, other = false, lost = false;
        if (r < live) {
            const uint8_t ty = dc_type(c, r);
            uint32_t slot = DC_NO_SLOT;
            if (ty == '"') {
                valid = true;
                slot = dc_insert_row(g, c, t, r, c.values[r]);  // (the only load of a row's own value word)
                lost = slot == DC_NO_SLOT;
            } else {
                other = ty != 0 && ty != 'n';
            }
            slot_of_row[r] = slot;
        }
        if (validity) g.validity_bit(validity, r, r < live, valid);
        sj_u64 total;
        (void)g.scan_add((valid ? 1ull : 0ull) | (other ? 1ull << DC_COUNT_BITS : 0ull) | (lost ? 1ull << (2 * DC_COUNT_BITS) : 0ull), &total);
        sum += total;
    }
    if (g.lane() == 0) counts[chunk] = sum;
}

// is the live row r the first of its value (behind the insert kernel: FIRST is final)
SJ_HD bool dc_is_first(const DcTable& t, const uint32_t* slot_of_row, sj_u64 r, uint32_t* slot) {
    *slot = slot_of_row[r];
    return *slot != DC_NO_SLOT && t.words[2 * (sj_u64)*slot + 1] == r;
}

// pass 2, per live chunk: firsts[chunk] = its first rows
template <class G>
SJ_HD void dc_count_chunk(const G& g, const DcColumn& c, const DcTable& t, sj_u64 chunk, const uint32_t* slot_of_row, sj_u64* firsts) {
    const sj_u64 live = dc_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64 sum = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        uint32_t slot;
        sj_u64 total;
        (void)g.scan_add(r < live && dc_is_first(t, slot_of_row, r, &slot) ? 1ull : 0ull, &total);
        sum += total;
    }
    if (g.lane() == 0) firsts[chunk] = sum;
}

// pass 3, ONE group: the first rows in front of every live chunk (in place), the record but for dict_bytes, *dict_n
template <class G>
SJ_HD void dc_scan(const G& g, const DcColumn& c, const sj_u64* counts, sj_u64* firsts, sj_u64 dict_capacity, sj_u64* dict_n, DcResult* res) {
    const sj_u64 live = dc_live(c);
    const sj_u64 nlive = dc_chunks(live, c.chunk_rows);
    sj_u64 valid = 0, other = 0, lost = 0;
    for (sj_u64 k = g.lane(); k < nlive; k += g.lanes()) {
        const sj_u64 w = counts[k];
        valid += w & DC_COUNT_MASK;
        other += (w >> DC_COUNT_BITS) & DC_COUNT_MASK;
        lost += w >> (2 * DC_COUNT_BITS);
    }
    sj_u64 n_valid, n_other, n_lost;
    (void)g.scan_add(valid, &n_valid);
    (void)g.scan_add(other, &n_other);
    (void)g.scan_add(lost, &n_lost);
    const sj_u64 n_distinct = g.scan_in_place(firsts, nlive);
    if (g.lane() == 0) {
        // (a placeless row has seen every slot taken: slots > dict_capacity values are distinct, and n_distinct says so itself)
        const bool overflow = n_distinct > dict_capacity || n_lost != 0;
        res->n_rows = live;
        res->n_valid = n_valid;
        res->n_other = n_other;
        res->n_distinct = n_distinct;
        res->dict_bytes = 0;
        res->flags = overflow ? DC_OVERFLOW : 0u;
        res->reserved = 0;
        *dict_n = overflow ? 0 : n_distinct;
    }
}

// pass 4, per live chunk: every first row's rank -> its slot's OWNER word, dict_rows (may be NULL), the compacted column.  Ranks
// at or above the capacity (DC_OVERFLOW) are written nowhere.
template <class G>
SJ_HD void dc_emit_chunk(const G& g, const DcColumn& c, const DcTable& t, sj_u64 chunk, const uint32_t* slot_of_row, const sj_u64* firsts,
                         sj_u64 dict_capacity, sj_u64* dict_rows, uint8_t* ctypes, sj_u64* cvalues) {
    const sj_u64 live = dc_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    if (first >= live) return;
    sj_u64 run = firsts[chunk];
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        uint32_t slot = DC_NO_SLOT;
        const bool is_first = r < live && dc_is_first(t, slot_of_row, r, &slot);
        sj_u64 total;
        const sj_u64 rank = run + g.scan_add(is_first ? 1ull : 0ull, &total);
        run += total;
        if (is_first && rank < dict_capacity) {
            t.words[2 * (sj_u64)slot] = rank;
            if (dict_rows) dict_rows[rank] = r;
            ctypes[rank] = '"';
            cvalues[rank] = c.values[r];
        }
    }
}

// pass 5, per live chunk: indices[r] of its live rows (a NULL row's, and a placeless row's under DC_OVERFLOW, is 0)
template <class G>
SJ_HD void dc_index_chunk(const G& g, const DcColumn& c, const DcTable& t, sj_u64 chunk, const uint32_t* slot_of_row, int32_t* indices) {
    const sj_u64 live = dc_live(c);
    const sj_u64 first = chunk * c.chunk_rows;
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        if (r >= live) continue;
        const uint32_t slot = slot_of_row[r];
        indices[r] = slot == DC_NO_SLOT ? 0 : (int32_t)(uint32_t)t.words[2 * (sj_u64)slot];
    }
}

// the compacted column as the string gather takes it: its rows are counted on the device
SJ_HD ScColumn dc_dict_column(const uint8_t* ctypes, const sj_u64* cvalues, const sj_u64* dict_n) {
    const ScColumn c = {ctypes, cvalues, *dict_n, SC_CHUNK_ROWS};
    return c;
}

// sc_chunk_scan for the dictionary, ONE group: the bytes in front of every chunk of the compacted column, dict_offsets[n], and
// what the record still lacks
template <class G>
SJ_HD void dc_dict_scan(const G& g, const ScSums& sums, sj_u64 nchunks, sj_u64 n, sj_u64* dict_offsets, sj_u64 byte_capacity, DcResult* res) {
    const sj_u64 total = g.scan_in_place(sums.bytes, nchunks);
    if (g.lane() == 0) {
        dict_offsets[n] = total;  // (n == 0: dict_offsets[0] = 0)
        res->dict_bytes = total;
        if (total > byte_capacity) res->flags |= DC_BYTES_OVERFLOW;
    }
}
