// sj_arrowcol.h -- the (type, value) columns of a select, an explode or a filter as Arrow int64, float64 and bool arrays: a data
// word per row (BOOL: a bit per row), an LSB-first validity bitmap and a record of counts per field (include/sjmi.h,
// sjmi_arrow_columns_device).
//
// The cell of column c, row r is types[c * col_stride + r] / values[c * col_stride + r].  A FIELD is (column, kind, flags): what
// one output array is made of.  ac_cell is the only reader of a cell: it loads the type byte, and the value word only behind
// 'l' / 'd' -- a boolean's type byte says it all, and whatever the value word of any other cell holds never shows.  The rows
// that count are [0, live), live = min(n_rows, *row_count) read HERE, on the device, where a row count is given: n_rows only
// sizes the grid.  Two passes: ac_convert_chunk per (chunk of rows, field) -- the data words, the validity words and the
// chunk's three counts packed into one scratch word -- and ac_finish per field: the sum of its chunk words, the record.  No
// atomics, and no group waits for another.
//
// The lanes come from the caller: takes a workgroup G (sj_group.h; the chunk is a multiple of 64 rows, and a wave is 64
// consecutive rows: its ballot of VALID is one validity word -- what G::validity_bit stores --, its ballot of 't' one data word
// of a BOOL field); uses: lanes, lane, waves, wave, ballot, first, scan_add.  Code outside the functions handed to ballot is
// wave-uniform.  csrc/arrowcol.hip runs this file with the device form, tests/host_sim/arrowcol_sim.cpp with the sequential one
// (tests/host_sim/seq_group.h): it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_block.h"

constexpr uint32_t AC_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t AC_MAX_FIELDS = 64;    // SJMI_ARROW_MAX_FIELDS
enum : uint32_t { AC_INT64 = 1, AC_FLOAT64 = 2, AC_BOOL = 3 };  // SJMI_ARROW_<KIND>
constexpr uint32_t AC_F_INTEGRAL_DOUBLES = 1u;                  // SJMI_ARROW_F_INTEGRAL_DOUBLES

struct AcField {  // sjmi_arrow_field
    uint32_t column, kind, flags, reserved;
};

// a validated schema: what the kernels take BY VALUE as a launch argument (nothing of it lives in device memory)
struct AcPlan {
    uint32_t n_fields, pad[3];
    AcField fields[AC_MAX_FIELDS];
};

struct AcResult {  // sjmi_arrow_field_result
    sj_u64 n_rows, n_valid, n_other, n_inexact;
};

struct AcCols {
    const uint8_t* types;  // any alignment: loaded as bytes
    const sj_u64* values;
    sj_u64 col_stride, n_rows;
    const sj_u64* row_count;  // NULL, or where the live rows are counted (on the device)
    uint32_t chunk_rows;      // a multiple of 64
};
SJ_HD sj_u64 ac_chunks(sj_u64 rows, uint32_t chunk_rows) { return (rows + chunk_rows - 1) / chunk_rows; }
SJ_HD sj_u64 ac_live(const AcCols& c) {
    if (!c.row_count) return c.n_rows;
    const sj_u64 n = *c.row_count;
    return n < c.n_rows ? n : c.n_rows;
}

struct AcOut {
    sj_u64* data;  // NULL: the counting call
    sj_u64 data_stride;
    sj_u64* validity;  // NULL: not written
    sj_u64 validity_stride;
};

// Host only: fields -> a plan.  0, or -2 (SJMI_ERR_ARG): no field or more than 64, an unknown kind, a flag that its kind does not
// define, reserved != 0, a column >= n_cols.
inline int ac_plan_compile(const AcField* fields, sj_u64 n_fields, sj_u64 n_cols, AcPlan* out) {
    if (!fields || n_fields == 0 || n_fields > AC_MAX_FIELDS) return -2;
    out->n_fields = (uint32_t)n_fields;
    out->pad[0] = out->pad[1] = out->pad[2] = 0;
    for (uint32_t k = 0; k < AC_MAX_FIELDS; ++k) {
        const AcField zero = {0, 0, 0, 0};
        out->fields[k] = k < n_fields ? fields[k] : zero;
    }
    for (sj_u64 k = 0; k < n_fields; ++k) {
        const AcField& f = fields[k];
        if (f.kind != AC_INT64 && f.kind != AC_FLOAT64 && f.kind != AC_BOOL) return -2;
        if (f.flags & ~(f.kind == AC_INT64 ? AC_F_INTEGRAL_DOUBLES : 0u)) return -2;
        if (f.reserved != 0 || f.column >= n_cols) return -2;
    }
    return 0;
}

// Is (double)v exact?  In integers, on the bit positions of |v|: a double holds 53 significant bits, so the highest and the
// lowest set bit are at most 52 apart.  (INT64_MIN: 0 - v wraps to 2^63, its magnitude.  Nothing is cast back from a double.)
SJ_HD bool ac_exact_as_double(sj_u64 v) {
    const sj_u64 mag = (v >> 63) ? 0ull - v : v;
    if (!mag) return true;
    return (63 - __builtin_clzll(mag)) - __builtin_ctzll(mag) <= 52;
}
SJ_HD sj_u64 ac_double_bits(double d) {
    sj_u64 bits;
    __builtin_memcpy(&bits, &d, sizeof bits);
    return bits;
}

// The double with these IEEE bits as an int64, when it is finite, has no fraction and lies in [-2^63, 2^63).  On the bits alone:
// no conversion that is undefined at 2^63 is made.
SJ_HD bool ac_integral_double(sj_u64 bits, sj_u64* out) {
    const uint32_t exp = (uint32_t)(bits >> 52) & 0x7FFu;
    const sj_u64 mant = bits & 0xFFFFFFFFFFFFFull;
    const bool neg = (bits >> 63) != 0;
    if (exp == 0) {  // +-0.0, or a subnormal
        *out = 0;
        return mant == 0;
    }
    if (exp < 1023 || exp > 1023 + 63) return false;  // below 1 in magnitude; at or above 2^64, an infinity or a NaN
    const uint32_t e = exp - 1023;                   // the value is sig * 2^(e - 52)
    const sj_u64 sig = mant | (1ull << 52);
    sj_u64 mag;
    if (e == 63) {  // 2^63 in magnitude at least: only -2^63 itself is an int64
        if (!neg || mant) return false;
        mag = 1ull << 63;
    } else if (e >= 52) {
        mag = sig << (e - 52);
    } else {
        if (sig & ((1ull << (52 - e)) - 1)) return false;  // a fraction
        mag = sig >> (52 - e);
    }
    *out = neg ? 0ull - mag : mag;
    return true;
}

struct AcCell {
    sj_u64 data;  // 0 unless VALID (BOOL: 1 iff 't')
    bool valid, other, inexact;  // other: NULL and neither MISSING nor 'n'; inexact: an 'l' that (double) rounded
};
// the cell `at` under a field of `kind` / `flags`
SJ_HD AcCell ac_cell(uint32_t kind, uint32_t flags, const AcCols& c, sj_u64 at) {
    AcCell cell = {0, false, false, false};
    const uint8_t ty = c.types[at];
    if (kind == AC_BOOL) {
        cell.valid = ty == 't' || ty == 'f';
        cell.data = ty == 't';
    } else if (ty == 'l') {
        const sj_u64 v = c.values[at];
        cell.valid = true;
        if (kind == AC_INT64) {
            cell.data = v;
        } else {  // (round to nearest, ties to even: the default mode on the device and on the host)
            cell.data = ac_double_bits((double)(int64_t)v);
            cell.inexact = !ac_exact_as_double(v);
        }
    } else if (ty == 'd') {
        if (kind == AC_FLOAT64) {
            cell.data = c.values[at];  // NaN and the infinities as they are
            cell.valid = true;
        } else if (flags & AC_F_INTEGRAL_DOUBLES) {
            cell.valid = ac_integral_double(c.values[at], &cell.data);
            if (!cell.valid) cell.data = 0;
        }
    }
    cell.other = !cell.valid && ty != 0 && ty != 'n';
    return cell;
}

// a chunk's counts in one word: each is at most the chunk's rows, and a chunk has at most 2^20 - 1
constexpr uint32_t AC_COUNT_BITS = 20;
constexpr sj_u64 AC_COUNT_MASK = (1ull << AC_COUNT_BITS) - 1;

// pass 1, per chunk and field: the data words (BOOL: the bit words) and the validity words of the chunk's live rows, and
// counts[field * nchunks + chunk].  A chunk that begins at or above `live` does nothing at all -- the whole group leaves in
// front of the scan, which every lane reaches otherwise, lanes at or above `live` with a 0 vote and without a store.
template <class G>
SJ_HD void ac_convert_chunk(const G& g, const AcPlan& p, const AcCols& c, sj_u64 chunk, uint32_t field, const AcOut& o, sj_u64* counts) {
    const sj_u64 live = ac_live(c);
    if (chunk * c.chunk_rows >= live) return;
    const AcField f = p.fields[field];
    const sj_u64 col = (sj_u64)f.column * c.col_stride;
    sj_u64* data = o.data ? o.data + field * o.data_stride : nullptr;
    sj_u64* validity = o.validity ? o.validity + field * o.validity_stride : nullptr;
    const sj_u64 first = chunk * (c.chunk_rows / 64);
    sj_u64 sum = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows / 64; at += g.waves()) {
        const sj_u64 word = at + g.wave(), r0 = word * 64;
        sj_u64 mine = 0;  // (what the lanes of this wave count: one lane's on the device)
        const sj_u64 valid = g.ballot([&](uint32_t t) {
            const sj_u64 r = r0 + t;
            if (r >= live) return false;
            const AcCell cell = ac_cell(f.kind, f.flags, c, col + r);
            if (data && f.kind != AC_BOOL) data[r] = cell.data;
            mine += (cell.valid ? 1ull : 0ull) | (cell.other ? 1ull << AC_COUNT_BITS : 0ull) | (cell.inexact ? 1ull << (2 * AC_COUNT_BITS) : 0ull);
            return cell.valid;
        });
        if (f.kind == AC_BOOL && data) {
            const sj_u64 bits = g.ballot([&](uint32_t t) { return r0 + t < live && c.types[col + r0 + t] == 't'; });
            if (r0 < live && g.first()) data[word] = bits;
        }
        if (validity && r0 < live && g.first()) validity[word] = valid;
        sj_u64 total;
        (void)g.scan_add(mine, &total);
        sum += total;
    }
    if (g.lane() == 0) counts[(sj_u64)field * ac_chunks(c.n_rows, c.chunk_rows) + chunk] = sum;
}

// pass 2, one group per field: the chunk words of the live chunks summed, the record
template <class G>
SJ_HD void ac_finish(const G& g, const AcCols& c, uint32_t field, const sj_u64* counts, AcResult* res) {
    const sj_u64 live = ac_live(c);
    const sj_u64 nlive = ac_chunks(live, c.chunk_rows);
    const sj_u64* mine = counts + (sj_u64)field * ac_chunks(c.n_rows, c.chunk_rows);
    sj_u64 valid = 0, other = 0, inexact = 0;
    for (sj_u64 k = g.lane(); k < nlive; k += g.lanes()) {
        const sj_u64 w = mine[k];
        valid += w & AC_COUNT_MASK;
        other += (w >> AC_COUNT_BITS) & AC_COUNT_MASK;
        inexact += w >> (2 * AC_COUNT_BITS);
    }
    sj_u64 n_valid, n_other, n_inexact;
    (void)g.scan_add(valid, &n_valid);
    (void)g.scan_add(other, &n_other);
    (void)g.scan_add(inexact, &n_inexact);
    if (g.lane() == 0) {
        res[field].n_rows = live;
        res[field].n_valid = n_valid;
        res[field].n_other = n_other;
        res[field].n_inexact = n_inexact;
    }
}
