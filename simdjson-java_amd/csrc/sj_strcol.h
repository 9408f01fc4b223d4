// sj_strcol.h -- gathering ONE string column of the selector's (type, value) encoding into Arrow's large_utf8 shape: int64
// offsets, an LSB-first validity bitmap and the bytes, back to back (include/sjmi.h, sjmi_string_column_device).
//
// Row r is VALID iff types[r] == '"'; its length is values[r] >> 32 and its bytes lie at sb + (values[r] & 0xFFFFFFFF).  Every
// other row is NULL with length 0, and its value word is never looked at (sc_row is the only reader of a value word, and
// reads it behind the type test).  The offsets are the exclusive scan of the lengths, by the chunk-sum scheme of walk.hip's
// tape offsets and explode.hip's row offsets: sums per chunk (pass 1), their scan by one workgroup (pass 2), the offsets (pass
// 3).  Pass 4 copies: a wave owns 64 consecutive rows, whose bytes are ONE span of the output, [offsets[r0], offsets[r0 + 64]).
// It parks the 64 row offsets and source offsets in LDS and walks the span 64 bytes per trip; lane t of trip q owns output
// byte offsets[r0] + 64 q + t, finds the row that byte belongs to by a six-step search among the parked offsets, and copies
// one byte.  Short strings share a trip, empty and NULL rows cost nothing, consecutive waves write consecutive bytes.
// KNOWN LIMIT: one very long string is copied by one wave, 64 bytes per trip.
//
// The lanes come from the caller.  Passes 1 to 3 take a workgroup G (sj_group.h; the chunk is a multiple of 64 rows, one row per
// lane); uses: lanes, lane, scan_add, scan_in_place, validity_bit.  Pass 4 takes a wave W (sj_group.h) and its ScWave in LDS;
// uses: each, fence.  csrc/strcol.hip runs this file with the device forms, tests/host_sim/strcol_sim.cpp with the sequential
// ones (tests/host_sim/seq_group.h): it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_block.h"

constexpr uint32_t SC_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t SC_OVERFLOW = 1u;      // SJMI_STRCOL_OVERFLOW

struct ScResult {  // sjmi_strcol_result
    sj_u64 total_bytes, n_valid, n_other;
    uint32_t flags, reserved;
};

struct ScColumn {
    const uint8_t* types;  // any alignment: loaded as bytes
    const sj_u64* values;
    sj_u64 n_rows;
    uint32_t chunk_rows;   // a multiple of 64
};
SJ_HD sj_u64 sc_chunks(const ScColumn& c) { return (c.n_rows + c.chunk_rows - 1) / c.chunk_rows; }

// the chunk sums: three arrays of nchunks entries.  Behind pass 2 bytes[k] = the bytes in front of chunk k
struct ScSums {
    sj_u64 *bytes, *valid, *other;
};
SJ_HD ScSums sc_sums(void* ws, sj_u64 nchunks) {
    sj_u64* p = (sj_u64*)ws;
    ScSums s = {p, p + nchunks, p + 2 * nchunks};
    return s;
}

struct ScRow {
    sj_u64 len;         // 0 unless VALID
    uint32_t src;       // VALID: where its bytes begin in the string buffer
    bool valid, other;  // other: neither VALID nor MISSING nor 'n'
};
// row r (r >= n_rows: a NULL row that is not there)
SJ_HD ScRow sc_row(const ScColumn& c, sj_u64 r) {
    ScRow row = {0, 0, false, false};
    if (r >= c.n_rows) return row;
    const uint8_t t = c.types[r];
    if (t == '"') {
        const sj_u64 v = c.values[r];  // (the only load of a value word: a NULL row's is never read)
        row.len = v >> 32;
        row.src = (uint32_t)v;
        row.valid = true;
    } else {
        row.other = t != 0 && t != 'n';
    }
    return row;
}

// pass 1, per chunk: the chunk's sums and its validity words (validity may be NULL)
template <class G>
SJ_HD void sc_chunk_sums(const G& g, const ScColumn& c, sj_u64 chunk, sj_u64* validity, const ScSums& sums) {
    const sj_u64 first = chunk * c.chunk_rows;
    sj_u64 bytes = 0, counts = 0;  // counts: the VALID rows in the low half, the other-typed in the high one
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        const ScRow row = sc_row(c, r);
        if (validity) g.validity_bit(validity, r, r < c.n_rows, row.valid);
        sj_u64 total;
        (void)g.scan_add(row.len, &total);
        bytes += total;
        (void)g.scan_add((row.valid ? 1ull : 0ull) | (row.other ? 1ull << 32 : 0ull), &total);
        counts += total;
    }
    if (g.lane() == 0) {
        sums.bytes[chunk] = bytes;
        sums.valid[chunk] = counts & 0xFFFFFFFFull;
        sums.other[chunk] = counts >> 32;
    }
}

// pass 2, ONE group: the bytes in front of every chunk, offsets[n_rows] and the result record
template <class G>
SJ_HD void sc_chunk_scan(const G& g, const ScSums& sums, sj_u64 nchunks, sj_u64 n_rows, sj_u64* offsets, sj_u64 byte_capacity,
                         ScResult* res) {
    const sj_u64 total = g.scan_in_place(sums.bytes, nchunks);
    const sj_u64 valid = g.scan_in_place(sums.valid, nchunks);
    const sj_u64 other = g.scan_in_place(sums.other, nchunks);
    if (g.lane() == 0) {
        offsets[n_rows] = total;  // (n_rows == 0: offsets[0] = 0)
        res->total_bytes = total;
        res->n_valid = valid;
        res->n_other = other;
        res->flags = total > byte_capacity ? SC_OVERFLOW : 0u;
        res->reserved = 0;
    }
}

// pass 3, per chunk: offsets[r] of its rows
template <class G>
SJ_HD void sc_offsets(const G& g, const ScColumn& c, sj_u64 chunk, const ScSums& sums, sj_u64* offsets) {
    const sj_u64 first = chunk * c.chunk_rows;
    sj_u64 run = sums.bytes[chunk];
    for (sj_u64 at = first; at < first + c.chunk_rows; at += g.lanes()) {
        const sj_u64 r = at + g.lane();
        const ScRow row = sc_row(c, r);
        sj_u64 total;
        const sj_u64 off = run + g.scan_add(row.len, &total);
        if (r < c.n_rows) offsets[r] = off;
        run += total;
    }
}

// what a wave parks of its 64 rows: off[t] = offsets[r0 + t] (rows that are not there: offsets[n_rows]), off[64] = where the
// span ends, src[t] = the row's bytes in the string buffer (used for VALID rows only: no other row owns a byte)
struct ScWave {
    sj_u64 off[65];
    uint32_t src[64];
};

// pass 4, per wave: the bytes of rows [64 * wave, 64 * wave + 64) below byte_capacity
template <class W>
SJ_HD void sc_copy_wave(const W& w, const ScColumn& c, sj_u64 wave, const sj_u64* offsets, const uint8_t* sb, uint8_t* bytes,
                        sj_u64 byte_capacity, ScWave& s) {
    const sj_u64 r0 = wave * 64;
    w.each([&](uint32_t t) {
        const sj_u64 r = r0 + t;
        s.off[t] = offsets[r < c.n_rows ? r : c.n_rows];
        s.src[t] = sc_row(c, r).src;
        if (t == 63) s.off[64] = offsets[r + 1 < c.n_rows ? r + 1 : c.n_rows];
    });
    w.fence();
    const sj_u64 begin = s.off[0];
    const sj_u64 end = s.off[64] < byte_capacity ? s.off[64] : byte_capacity;
    for (sj_u64 pos = begin; pos < end; pos += 64) {  // (a span that begins at or behind the capacity: no trip)
        w.each([&](uint32_t t) {
            const sj_u64 i = pos + t;
            if (i >= end) return;
            // the last row whose offset is <= i: off[0] <= i < off[64], so the row behind it begins behind i and the row owns
            // byte i (rows without bytes in front of it share its offset and are passed over)
            uint32_t j = 0;
            for (uint32_t step = 32; step; step >>= 1)
                if (s.off[j + step] <= i) j += step;
            bytes[i] = sb[(sj_u64)s.src[j] + (i - s.off[j])];
        });
    }
}
