// sj_arrowcol.h -- the (type, value) columns of a select, an explode or a filter as Arrow int64, float64 and bool arrays: a data
// word per row (BOOL: a bit per row), an LSB-first validity bitmap and a record of counts per field (include/sjmi.h,
// sjmi_arrow_columns_device).
//
// One of the two operators in the frame of sj_fieldcol.h -- the field, the plan, the column set, the live rows, the packed chunk
// counts and the finish pass are written there.  A field's `what` is its KIND.  ac_cell is the only reader of a cell: it loads
// the type byte, and the value word only behind 'l' / 'd' -- a boolean's type byte says it all, and whatever the value word of
// any other cell holds never shows.  The chunk pass is ac_convert_chunk: the data words, the validity words and the chunk's
// three counts.
//
// The lanes come from the caller: takes a workgroup G (sj_group.h; the chunk is a multiple of 64 rows, and a wave is 64
// consecutive rows: its ballot of VALID is one validity word -- what G::validity_bit stores --, its ballot of 't' one data word
// of a BOOL field); uses: lane, waves, wave, ballot, first, scan_add.  Code outside the functions handed to ballot is
// wave-uniform.  csrc/arrowcol.hip runs this file with the device form, tests/host_sim/arrowcol_sim.cpp with the sequential one
// (tests/host_sim/seq_group.h): it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_fieldcol.h"

constexpr uint32_t AC_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
enum : uint32_t { AC_INT64 = 1, AC_FLOAT64 = 2, AC_BOOL = 3 };  // SJMI_ARROW_<KIND>
constexpr uint32_t AC_F_INTEGRAL_DOUBLES = 1u;                  // SJMI_ARROW_F_INTEGRAL_DOUBLES

struct AcResult {  // sjmi_arrow_field_result
    sj_u64 n_rows, n_valid, n_other, n_inexact;
};
struct AcCols : FcCols {
    uint32_t chunk_rows;  // a multiple of 64
};
using AcCounts = FcCounts<3, 20, AC_CHUNK_ROWS>;  // VALID, other, inexact: the three behind n_rows
// the frame under this operator's names, as its kernel, its simulation and its callers spell them
using AcField = FcField;  // what = the KIND
using AcPlan = FcPlan;
using AcOut = FcOut;
SJ_HD sj_u64 ac_chunks(sj_u64 rows, uint32_t chunk_rows) { return fc_chunks(rows, chunk_rows); }

// Host only: fields -> a plan.  0, or -2 (SJMI_ERR_ARG): what fc_plan_compile refuses, an unknown kind, a flag that its kind
// does not define.
inline int ac_plan_compile(const AcField* fields, sj_u64 n_fields, sj_u64 n_cols, AcPlan* out) {
    return fc_plan_compile(fields, n_fields, n_cols, out, [](const FcField& f) {
        return (f.what == AC_INT64 || f.what == AC_FLOAT64 || f.what == AC_BOOL) && !(f.flags & ~(f.what == AC_INT64 ? AC_F_INTEGRAL_DOUBLES : 0u));
    });
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

// pass 1, per chunk and field: the data words (BOOL: the bit words) and the validity words of the chunk's live rows, and the
// chunk's word of counts.  Every lane of a live chunk reaches the scan, lanes at or above `live` with a 0 vote and without a store.
template <class G>
SJ_HD void ac_convert_chunk(const G& g, const AcPlan& p, const AcCols& c, sj_u64 chunk, uint32_t field, const AcOut& o, sj_u64* counts) {
    const sj_u64 live = fc_live(c.n_rows, c.row_count);
    if (chunk * c.chunk_rows >= live) return;
    const FcChunk h = fc_chunk_head(p, c, chunk, field, o);
    const uint32_t kind = h.f.what;
    sj_u64 sum = 0;
    for (sj_u64 at = h.first; at < h.first + c.chunk_rows / 64; at += g.waves()) {
        const sj_u64 word = at + g.wave(), r0 = word * 64;
        sj_u64 mine = 0;  // (what the lanes of this wave count: one lane's on the device)
        const sj_u64 valid = g.ballot([&](uint32_t t) {
            const sj_u64 r = r0 + t;
            if (r >= live) return false;
            const AcCell cell = ac_cell(kind, h.f.flags, c, h.col + r);
            if (h.data && kind != AC_BOOL) h.data[r] = cell.data;
            mine += AcCounts::of({cell.valid, cell.other, cell.inexact});
            return cell.valid;
        });
        if (kind == AC_BOOL && h.data) {
            const sj_u64 bits = g.ballot([&](uint32_t t) { return r0 + t < live && c.types[h.col + r0 + t] == 't'; });
            if (r0 < live && g.first()) h.data[word] = bits;
        }
        if (h.validity && r0 < live && g.first()) h.validity[word] = valid;
        sj_u64 total;
        (void)g.scan_add(mine, &total);
        sum += total;
    }
    AcCounts::store(g, c, field, chunk, counts, sum);
}

// pass 2, one group per field: the frame's, with this operator's counts and record
template <class G>
SJ_HD void ac_finish(const G& g, const AcCols& c, uint32_t field, const sj_u64* counts, AcResult* res) {
    fc_finish<AcCounts>(g, c, field, counts, (sj_u64*)res);
}
