// sj_timecol.h -- the RFC 3339 strings of (type, value) columns as Arrow timestamp arrays: an int64 word per row at the unit of
// the field (seconds, milli-, micro- or nanoseconds since 1970-01-01T00:00:00Z), an LSB-first validity bitmap and a record of
// counts per field (include/sjmi.h, sjmi_time_columns_device).
//
// The cell of column c, row r is types[c * col_stride + r] / values[c * col_stride + r]; a FIELD is (column, unit, flags).  A
// row's chain is three dependent loads: the type byte, the value word -- only behind '"' -- and the string's bytes at
// c.strings + (value & 0xFFFFFFFF) -- only behind the test of the length value >> 32, which must be 20..35 (19 with NAIVE_UTC).
// tc_load_* / tc_string bring those bytes into five register words (byte i of the string = byte i & 7 of word i >> 3, zeros from the
// length on), in one of two forms:
//   tc_load_bytes    one byte-wide load per byte of the string
//   tc_load_words    the naturally aligned 8-byte words that hold at least one byte of the string -- such a word lies in the
//                    page, and so in the allocation, of that byte --, realigned by the address's low three bits
// and whatever else an aligned word carried is masked off before tc_parse sees it.  tc_parse decides the grammar on the words:
// digit ranges and separators of the fixed 19 bytes as SWAR tests, the fraction and the zone on the 16 bytes behind them.
// Everything is integer arithmetic without a signed overflow: only NANO can leave int64, and that is decided on the seconds.
//
// One of the two operators in the frame of sj_fieldcol.h -- the field, the plan, the column set, the live rows, the packed chunk
// counts and the finish pass are written there.  A field's `what` is its UNIT.  The chunk pass is tc_parse_chunk: the data
// words, the validity words and the chunk's five counts.
//
// The lanes come from the caller: takes a workgroup G (sj_group.h; a wave is 64 consecutive rows) and uses lanes, lane, waves,
// wave, first, scan_add, and group_ballots (sj_group_ballots.h): a lane can work on ROWS rows of as many waves' worth of rows
// AT ONCE -- all type bytes, then all value words, then all strings requested before the first is parsed.  The pass is bound
// by the latency of that chain, and what hides it on the MI355X is resident waves, not rows per lane: at 256 threads a
// workgroup, 1 and 2 rows per lane took the same time, 4 and 8 longer (tools/ubench/timecol_ab.hip, profiles/r16), so the
// kernel runs ROWS = 1 and the host simulation the others too.  csrc/timecol.hip runs this file with the device form,
// tests/host_sim/timecol_sim.cpp with the sequential one: it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"

constexpr uint32_t TC_CHUNK_ROWS = 256;  // rows of a chunk: TC_LANE_ROWS per thread of its workgroup
constexpr uint32_t TC_LANE_ROWS = 1;     // rows whose loads one lane has in flight (1, 2, 4, 8 were measured: profiles/r16)
enum : uint32_t { TC_SECOND = 0, TC_MILLI = 1, TC_MICRO = 2, TC_NANO = 3 };  // SJMI_TIME_<UNIT>
constexpr uint32_t TC_F_NAIVE_UTC = 1u;                                     // SJMI_TIME_F_NAIVE_UTC
constexpr uint32_t TC_MIN_LEN = 20, TC_MAX_LEN = 35;  // "YYYY-MM-DDThh:mm:ssZ" .. with 9 digits of fraction and "+hh:mm"

struct TcResult {  // sjmi_time_field_result
    sj_u64 n_rows, n_valid, n_other, n_malformed, n_range, n_inexact;
};
using TcCounts = FcCounts<5, 12, TC_CHUNK_ROWS>;  // VALID, other, malformed, range, inexact: the five behind n_rows
// the frame under this operator's names, as its kernel, its simulation and its callers spell them
using TcField = FcField;  // what = the UNIT
using TcPlan = FcPlan;
using TcOut = FcOut;
SJ_HD sj_u64 tc_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }

struct TcCols : FcCols {
    const uint8_t* strings;  // the string buffer the '"' cells point into
    uint32_t chunk_rows;     // a multiple of 64
};

// Host only: fields -> a plan.  0, or -2 (SJMI_ERR_ARG): what fc_plan_compile refuses, a unit above NANO, a flag other than
// NAIVE_UTC.
inline int tc_plan_compile(const TcField* fields, sj_u64 n_fields, sj_u64 n_cols, TcPlan* out) {
    return fc_plan_compile(fields, n_fields, n_cols, out, [](const FcField& f) { return f.what <= TC_NANO && !(f.flags & ~TC_F_NAIVE_UTC); });
}

// ---- the fetch: a string of 19..35 bytes as five words, zeros from byte `len` on ----
// In two steps, so that a lane can ask for the bytes of all its rows before it waits for the first: tc_load_* only loads, and
// is called behind the tests; tc_string only computes, on whatever the registers hold.
struct TcRaw {
    sj_u64 a[6];
};
struct TcString {
    sj_u64 w[5];
};
constexpr sj_u64 TC_ONES = 0x0101010101010101ull;
// the low n bytes of a word, n in 0..8
SJ_HD sj_u64 tc_low_bytes(uint32_t n) { return n >= 8 ? ~0ull : (1ull << (8 * n)) - 1; }

// form 1: byte-wide loads inside [at, at + len), put together as they come: a[0 .. 4] is the string already
SJ_HD TcRaw tc_load_bytes(const uint8_t* at, uint32_t len) {
    TcRaw raw = {{0, 0, 0, 0, 0, 0}};
#pragma unroll
    for (uint32_t i = 0; i < TC_MAX_LEN; ++i)
        if (i < len) raw.a[i >> 3] |= (sj_u64)at[i] << (8 * (i & 7));
    return raw;
}

// form 2: the aligned words that hold a byte of [at, at + len) -- six at most: 35 bytes behind up to 7 of another's.  Where the
// string ends in an earlier word that LAST word is loaded again in place of the ones behind it (a load more of an address already
// asked for, and no branch); what it brings lies at or above `len` and is masked off with the rest.
SJ_HD TcRaw tc_load_words(const uint8_t* at, uint32_t len) {
    const uint32_t skip = (uint32_t)((uintptr_t)at & 7);  // bytes of the first word in front of the string
    const sj_u64* base = (const sj_u64*)(at - skip);
    const uint32_t last = (skip + len - 1) >> 3;  // len >= 19: 2 at least
    TcRaw raw;
#pragma unroll
    for (uint32_t j = 0; j < 6; ++j) raw.a[j] = base[j < last ? j : last];
    return raw;
}

// what was loaded for the string at `at` -> the string.  Form 2: realigned by the address's low bits and cut at len
template <bool WORDS>
SJ_HD TcString tc_string(const TcRaw& raw, const uint8_t* at, uint32_t len) {
    TcString s;
    const uint32_t skip = WORDS ? (uint32_t)((uintptr_t)at & 7) : 0u;
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) {
        const sj_u64 lo = raw.a[i] >> (8 * skip);
        const sj_u64 hi = skip ? raw.a[i + 1] << (64 - 8 * skip) : 0;
        s.w[i] = WORDS ? (lo | hi) & tc_low_bytes(len > 8 * i ? len - 8 * i : 0) : raw.a[i];
    }
    return s;
}

// ---- the grammar, on the words ----
// 0x80 in every byte of x that is not an ASCII digit
SJ_HD sj_u64 tc_not_digit(sj_u64 x) {
    const sj_u64 d = x ^ (0x30 * TC_ONES);  // a digit: 0..9
    return (((d & (0x7F * TC_ONES)) + (0x76 * TC_ONES)) | d) & (0x80 * TC_ONES);
}
// byte i of the string
SJ_HD uint32_t tc_byte(const TcString& s, uint32_t i) { return (uint32_t)(s.w[i >> 3] >> (8 * (i & 7))) & 0xFFu; }
// the two digits at i, i + 1 as a number (they were tested to be digits)
SJ_HD uint32_t tc_two(const TcString& s, uint32_t i) { return (tc_byte(s, i) - '0') * 10 + (tc_byte(s, i + 1) - '0'); }

// days since 1970-01-01 of a proleptic Gregorian date, y in 0..9999 (H. Hinnant, "chrono-Compatible Low-Level Date
// Algorithms", days_from_civil; the year is shifted by one era of 400 years so that nothing is negative on the way)
SJ_HD int64_t tc_days_from_civil(uint32_t y, uint32_t m, uint32_t d) {
    y += 400 - (m <= 2 ? 1u : 0u);
    const uint32_t era = y / 400, yoe = y - era * 400;
    const uint32_t doy = (153 * (m > 2 ? m - 3 : m + 9) + 2) / 5 + d - 1;
    const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return (int64_t)(era * 146097u + doe) - 146097 - 719468;
}

struct TcCell {
    sj_u64 data;  // 0 unless VALID
    bool valid, other, malformed, range, inexact;
};

// a string of `len` bytes (19..35, the flag allowing 19 tested by the caller) under `unit` / `flags`.  Written without a branch
// that depends on the bytes: every lane of a wave takes the same way through it, whatever its string holds.  What is wrong is
// gathered in `bad`; a range test a <= b is the sign bit of b - a (every number here is far below 2^31, whatever the bytes are).
SJ_HD TcCell tc_parse(const TcString& s, uint32_t len, uint32_t unit, uint32_t flags) {
    // the fixed part: digits everywhere but at 4, 7 ('-'), 10 (T, t or a space), 13, 16 (':'); bytes 19 .. belong to the tail
    const sj_u64 M0 = 0xFF0000FF00000000ull, M1 = 0x0000FF0000FF0000ull, M2 = 0x00000000000000FFull, FIX2 = 0x0000000000FFFFFFull;
    const sj_u64 not_digits = (tc_not_digit(s.w[0]) & ~M0) | (tc_not_digit(s.w[1]) & ~M1) | (tc_not_digit(s.w[2]) & FIX2 & ~M2);
    const sj_u64 not_marks = ((s.w[0] & M0) ^ 0x2D00002D00000000ull) | ((s.w[1] & 0x0000FF0000000000ull) ^ 0x00003A0000000000ull) | ((s.w[2] & M2) ^ 0x3A);
    const uint32_t sep = tc_byte(s, 10);
    sj_u64 bad = not_digits | not_marks;
    bad |= ((sep | 0x20) ^ 't') * (sep ^ ' ');  // (a product of two bytes: 0 iff one of them is)
    const uint32_t year = tc_two(s, 0) * 100 + tc_two(s, 2), month = tc_two(s, 5), day = tc_two(s, 8);
    const uint32_t hour = tc_two(s, 11), minute = tc_two(s, 14), second = tc_two(s, 17);
    const bool leap = (year % 4 == 0) & ((year % 100 != 0) | (year % 400 == 0));
    const uint32_t days_in_month = month == 2 ? (leap ? 29u : 28u) : 30u + ((month + (month >> 3)) & 1u);
    uint32_t below = (month - 1) | (12 - month) | (day - 1) | (days_in_month - day) | (23 - hour) | (59 - minute) | (59 - second);

    // the tail: bytes 19 .. 34 as t0 (19 .. 26) and t1 (27 .. 34): ['.' 1 to 9 digits] zone
    const sj_u64 t0 = (s.w[2] >> 24) | (s.w[3] << 40), t1 = (s.w[3] >> 24) | (s.w[4] << 40);
    const uint32_t tail = len - 19;
    const bool dot = (t0 & 0xFF) == '.';
    const sj_u64 f8 = (t0 >> 8) | (t1 << 56);  // tail bytes 1 .. 8; the ninth digit is tail byte 9
    const uint32_t ninth = (uint32_t)(t1 >> 8) & 0xFFu;
    const sj_u64 stop = tc_not_digit(f8);
    uint32_t digits = stop ? (uint32_t)__builtin_ctzll(stop) >> 3 : 8u;
    digits += ((digits == 8) & (ninth - '0' <= 9u)) ? 1u : 0u;  // (a tenth digit stands where the zone must: malformed below)
    digits = dot ? digits : 0u;
    below |= dot ? digits - 1 : 0u;  // '.' and no digit
    uint32_t frac = 0;  // the fraction as nanoseconds
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) {
        const uint32_t ch = i < 8 ? (uint32_t)(f8 >> (8 * i)) & 0xFFu : ninth;
        frac = frac * 10 + (i < digits ? ch - '0' : 0u);
    }
    // the zone: tail bytes [zone_at, tail), zone_at <= 10: nothing (NAIVE_UTC only), Z / z, or +hh:mm / -hh:mm
    const uint32_t zone_at = dot ? 1 + digits : 0u;
    const uint32_t sh = 8 * (zone_at & 7);
    const sj_u64 z = zone_at < 8 ? (t0 >> sh) | ((t1 << 8) << (56 - sh)) : t1 >> sh;
    const uint32_t zone_len = tail - zone_at;  // (the digits counted lie below len: what follows len is zeros)
    const uint32_t sign = (uint32_t)z & 0xFFu;
    const sj_u64 ZM = 0x0000FFFF00FFFF00ull;  // the digits of sHH:MM
    const uint32_t zh = ((uint32_t)(z >> 8) & 0xFFu) * 10 + ((uint32_t)(z >> 16) & 0xFFu) - 11 * '0';
    const uint32_t zm = ((uint32_t)(z >> 32) & 0xFFu) * 10 + ((uint32_t)(z >> 40) & 0xFFu) - 11 * '0';
    const sj_u64 bad_numeric = (tc_not_digit(z) & ZM) | (((z >> 24) & 0xFF) ^ ':') | ((sign ^ '+') * (sign ^ '-')) | (((23 - zh) | (59 - zm)) >> 31);
    const sj_u64 bad_zone = zone_len == 0 ? (flags & TC_F_NAIVE_UTC) ^ TC_F_NAIVE_UTC : zone_len == 1 ? (sign | 0x20u) ^ 'z' : zone_len == 6 ? bad_numeric : 1u;
    const bool ok = (bad | bad_zone | (below >> 31)) == 0;
    const int32_t magnitude = zone_len == 6 ? (int32_t)(zh * 3600 + zm * 60) : 0;
    const int32_t offset = sign == '-' ? -magnitude : magnitude;

    const int64_t secs = tc_days_from_civil(year, month, day) * 86400 + (int64_t)(hour * 3600 + minute * 60 + second) - offset;
    // the fraction at the unit: its surplus digits dropped -- a floor, the fraction being positive
    const uint32_t per = unit == TC_SECOND ? 1000000000u : unit == TC_MILLI ? 1000000u : unit == TC_MICRO ? 1000u : 1u;
    const uint32_t kept = unit == TC_SECOND ? 0u : unit == TC_MILLI ? frac / 1000000u : unit == TC_MICRO ? frac / 1000u : frac;
    const sj_u64 scale = 1000000000u / per;
    // only NANO can leave int64: INT64_MAX = 9223372036 s + 854775807 ns, INT64_MIN = -9223372037 s + 145224192 ns -- decided
    // on the seconds, before anything is multiplied
    const int64_t top = 9223372036ll, bottom = -9223372037ll;
    const bool out = (unit == TC_NANO) & ((secs > top) | (secs < bottom) | ((secs == top) & (frac > 854775807u)) | ((secs == bottom) & (frac < 145224192u)));
    TcCell cell;
    cell.valid = ok & !out;
    cell.data = cell.valid ? (sj_u64)secs * scale + kept : 0;  // (unsigned: an in-range product wraps to its two's complement)
    cell.other = false;
    cell.malformed = !ok;
    cell.range = ok & out;
    cell.inexact = cell.valid & (kept * per != frac);
    return cell;
}

// does the cell (ty, val) have a string to parse: a '"' whose length the grammar can have.  The length decides before a byte
SJ_HD bool tc_wants_string(uint32_t flags, uint8_t ty, sj_u64 val) {
    const uint32_t len = (uint32_t)(val >> 32);
    return ty == '"' && len >= TC_MIN_LEN - ((flags & TC_F_NAIVE_UTC) ? 1u : 0u) && len <= TC_MAX_LEN;
}
// the cell of type ty under a field; wanted: its string of len bytes is s (else s is not looked at, whatever it holds).  The
// parse runs in every lane, wanted or not -- there is no branch for a wave to diverge on -- and its verdict is selected
SJ_HD TcCell tc_cell(uint32_t unit, uint32_t flags, uint8_t ty, bool wanted, uint32_t len, const TcString& s) {
    const TcCell parsed = tc_parse(s, wanted ? len : 19u, unit, flags);
    TcCell cell;
    cell.valid = wanted & parsed.valid;
    cell.data = cell.valid ? parsed.data : 0;
    cell.other = (ty != '"') & (ty != 0) & (ty != 'n');
    cell.malformed = (ty == '"') & !cell.valid & !(wanted & parsed.range);  // (a string of another length: no byte of it was read)
    cell.range = wanted & parsed.range;
    cell.inexact = wanted & parsed.inexact;
    return cell;
}

// pass 1, per chunk and field: the data words and the validity words of the chunk's live rows, and counts[field * nchunks +
// chunk].  The chunk IS what the group takes in one go, without a loop: c.chunk_rows = 64 * g.waves() * ROWS, lane t of wave w
// working on rows 64 * (w + k * waves) + t of the chunk, k < ROWS.  (A loop over more, with its invariants kept in registers
// across it, cost the kernel a third of its occupancy and spilled scalar registers.)  A chunk that begins at or above `live`
// does nothing at all -- the whole group leaves in front of the scan, which every lane reaches otherwise.  WORDS:
// tc_load_words, else tc_load_bytes; ROWS: the rows a lane has in flight.
template <bool WORDS, uint32_t ROWS, class G>
SJ_HD void tc_parse_chunk(const G& g, const TcPlan& p, const TcCols& c, sj_u64 chunk, uint32_t field, const TcOut& o, sj_u64* counts) {
    const sj_u64 live = fc_live(c.n_rows, c.row_count);
    if (chunk * c.chunk_rows >= live) return;
    const FcChunk h = fc_chunk_head(p, c, chunk, field, o);
    const sj_u64 end = h.first + c.chunk_rows / 64;
    sj_u64 mine = 0;  // (what the lanes of this wave count: one lane's on the device)
    sj_u64 valid[ROWS];
    group_ballots(g, [&](uint32_t t, bool (&vote)[ROWS]) {
        sj_u64 r[ROWS], val[ROWS];
        uint8_t ty[ROWS];
        bool on[ROWS], wanted[ROWS];
        TcRaw raw[ROWS];
#pragma unroll
        for (uint32_t k = 0; k < ROWS; ++k) {
            const sj_u64 word = h.first + (sj_u64)k * g.waves() + g.wave();
            r[k] = word * 64 + t;
            on[k] = word < end && r[k] < live;
            ty[k] = on[k] ? c.types[h.col + r[k]] : (uint8_t)0;
        }
#pragma unroll
        for (uint32_t k = 0; k < ROWS; ++k) val[k] = ty[k] == '"' ? c.values[h.col + r[k]] : 0;
#pragma unroll
        for (uint32_t k = 0; k < ROWS; ++k) {
            const TcRaw none = {{0, 0, 0, 0, 0, 0}};
            const uint8_t* bytes = c.strings + (uint32_t)val[k];
            const uint32_t len = (uint32_t)(val[k] >> 32);
            wanted[k] = tc_wants_string(h.f.flags, ty[k], val[k]);
            raw[k] = !wanted[k] ? none : WORDS ? tc_load_words(bytes, len) : tc_load_bytes(bytes, len);
        }
#pragma unroll
        for (uint32_t k = 0; k < ROWS; ++k) {
            const uint32_t len = (uint32_t)(val[k] >> 32);
            const TcCell cell = tc_cell(h.f.what, h.f.flags, ty[k], wanted[k], len, tc_string<WORDS>(raw[k], c.strings + (uint32_t)val[k], len));
            vote[k] = on[k] && cell.valid;
            if (!on[k]) continue;
            if (h.data) h.data[r[k]] = cell.data;
            mine += TcCounts::of({cell.valid, cell.other, cell.malformed, cell.range, cell.inexact});
        }
    }, valid);
#pragma unroll
    for (uint32_t k = 0; k < ROWS; ++k) {
        const sj_u64 word = h.first + (sj_u64)k * g.waves() + g.wave();
        if (h.validity && word < end && word * 64 < live && g.first()) h.validity[word] = valid[k];
    }
    sj_u64 total;
    (void)g.scan_add(mine, &total);
    TcCounts::store(g, c, field, chunk, counts, total);
}

// pass 2, one group per field: the frame's, with this operator's counts and record
template <class G>
SJ_HD void tc_finish(const G& g, const TcCols& c, uint32_t field, const sj_u64* counts, TcResult* res) {
    fc_finish<TcCounts>(g, c, field, counts, (sj_u64*)res);
}
