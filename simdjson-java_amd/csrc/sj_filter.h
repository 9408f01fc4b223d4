// sj_filter.h -- filtering the rows of a set of (type, value) columns of a select or an explode by a conjunction of terms, and
// compacting the kept rows (include/sjmi.h, sjmi_filter_columns_device).
//
// The cell of column c, row r is types[c * col_stride + r] / values[c * col_stride + r].  A term looks at one column and is TRUE
// only on a cell of the type it can compare with: fl_term loads the type byte, and the value word only behind the type test -- as
// a number behind 'l' / 'd', as (length << 32) | offset behind '"', where the length decides before a byte is touched and only
// bytes inside [offset, offset + length) are read.  A row is KEPT iff every term is TRUE.  Three passes, the chunk-sum scheme of
// sj_strcol.h: the keep words and the kept rows per chunk (pass 1), the scan of the chunk counts by one workgroup (pass 2), the
// selection vector and the compacted columns (pass 3: rank = chunk base + kept rows of the chunk's earlier words + the kept
// rows below this one in its own word).
//
// The lanes come from the caller: takes a workgroup G (sj_group.h; the chunk is a multiple of 64 rows, and a wave is 64
// consecutive rows: its ballot IS one keep word); uses: waves, wave, ballot, each, first, scan_add, scan_in_place, lane.  Code
// outside the functions handed to ballot / each is wave-uniform.  csrc/filter.hip runs this file with the device form,
// tests/host_sim/filter_sim.cpp with the sequential one (tests/host_sim/seq_group.h): it is compiled verbatim by both.
#pragma once
#include <stdint.h>

#include "sj_block.h"

constexpr uint32_t FL_CHUNK_ROWS = 1024;  // rows of a chunk = threads of its workgroup
constexpr uint32_t FL_OVERFLOW = 1u;      // SJMI_FILTER_OVERFLOW
constexpr uint32_t FL_MAX_TERMS = 16, FL_MAX_CONST_BYTES = 1024, FL_MAX_STRING = 256;  // SJMI_FILTER_MAX_*

// op = kind << 4 | comparison (SJMI_F_<KIND>_<CMP>)
enum : uint32_t { FL_TYPE = 0, FL_LONG = 1, FL_DOUBLE = 2, FL_STRING = 3 };
enum : uint32_t { FL_EQ = 0, FL_NE = 1, FL_LT = 2, FL_LE = 3, FL_GT = 4, FL_GE = 5, FL_PREFIX = 6 };

struct FlTerm {  // sjmi_filter_term
    uint32_t column, op;
    sj_u64 operand;
};

// a compiled plan: what the kernels take BY VALUE as a launch argument (nothing of it lives in device memory)
struct FlPlan {
    uint32_t n_terms, n_bytes;
    FlTerm terms[FL_MAX_TERMS];
    uint8_t bytes[FL_MAX_CONST_BYTES];  // the string constants, where the caller's offsets point
};

struct FlResult {  // sjmi_filter_result
    sj_u64 n_kept;
    uint32_t flags, reserved;
};

struct FlCols {
    const uint8_t* types;  // any alignment: loaded as bytes
    const sj_u64* values;
    sj_u64 n_cols, col_stride, n_rows;
    const uint8_t* sb;     // the string buffer (read only for '"' cells under a STRING term)
    uint32_t chunk_rows;   // a multiple of 64
};
SJ_HD sj_u64 fl_chunks(const FlCols& c) { return (c.n_rows + c.chunk_rows - 1) / c.chunk_rows; }
SJ_HD sj_u64 fl_words(const FlCols& c) { return (c.n_rows + 63) / 64; }

SJ_HD double fl_double(sj_u64 bits) {
    double d;
    __builtin_memcpy(&d, &bits, sizeof d);
    return d;
}

// Host only: terms + constants -> a plan.  0, or -2 (SJMI_ERR_ARG): more than 16 terms, an unknown op, a type operand above 255,
// a NaN, a string constant outside bytes[0, n_bytes) or longer than 256 bytes, more than 1024 bytes of constants.
inline int fl_plan_compile(const FlTerm* terms, sj_u64 n_terms, const uint8_t* bytes, sj_u64 n_bytes, FlPlan* out) {
    if (n_terms > FL_MAX_TERMS || n_bytes > FL_MAX_CONST_BYTES || (n_terms && !terms) || (n_bytes && !bytes)) return -2;
    out->n_terms = (uint32_t)n_terms;
    out->n_bytes = (uint32_t)n_bytes;
    for (uint32_t k = 0; k < FL_MAX_TERMS; ++k) {
        const FlTerm zero = {0, 0, 0};
        out->terms[k] = k < n_terms ? terms[k] : zero;
    }
    for (uint32_t i = 0; i < FL_MAX_CONST_BYTES; ++i) out->bytes[i] = i < n_bytes ? bytes[i] : 0;
    for (sj_u64 k = 0; k < n_terms; ++k) {
        const FlTerm& t = terms[k];
        const uint32_t kind = t.op >> 4, cmp = t.op & 15u;
        if (kind == FL_TYPE) {
            if (cmp > FL_NE || t.operand > 255) return -2;
        } else if (kind == FL_LONG) {
            if (cmp > FL_GE) return -2;
        } else if (kind == FL_DOUBLE) {
            const double d = fl_double(t.operand);
            if (cmp > FL_GE || d != d) return -2;
        } else if (kind == FL_STRING) {
            const sj_u64 len = t.operand >> 32, off = t.operand & 0xFFFFFFFFull;
            if ((cmp > FL_NE && cmp != FL_PREFIX) || len > FL_MAX_STRING || off > n_bytes || len > n_bytes - off) return -2;
        } else {
            return -2;
        }
    }
    return 0;
}
inline bool fl_plan_has_string(const FlPlan& p) {
    for (uint32_t k = 0; k < p.n_terms; ++k)
        if ((p.terms[k].op >> 4) == FL_STRING) return true;
    return false;
}

// The order of two numbers AS REAL NUMBERS: -1, 0, 1, or 2 when one of them is a NaN (no comparison holds then; NaN cells are
// outside the contract and NaN constants do not compile).
SJ_HD int fl_cmp_ll(int64_t a, int64_t b) { return a < b ? -1 : a > b ? 1 : 0; }
SJ_HD int fl_cmp_dd(double a, double b) { return a < b ? -1 : a > b ? 1 : a == b ? 0 : 2; }
// int64 against double without rounding either side: a double at or above 2^63 is above every int64, one below -2^63 below every
// int64; otherwise its truncation is an int64, and where that ties the sign of the fraction decides (a double with a fraction is
// below 2^53 in magnitude, so the truncation converts back exactly and the subtraction is exact)
SJ_HD int fl_cmp_ld(int64_t a, double d) {
    if (d != d) return 2;
    if (d >= 9223372036854775808.0) return -1;
    if (d < -9223372036854775808.0) return 1;
    const int64_t t = (int64_t)d;
    if (a != t) return a < t ? -1 : 1;
    const double frac = d - (double)t;
    return frac > 0 ? -1 : frac < 0 ? 1 : 0;
}
SJ_HD bool fl_holds(uint32_t cmp, int order) {
    if (order == 2) return false;
    switch (cmp) {
        case FL_EQ: return order == 0;
        case FL_NE: return order != 0;
        case FL_LT: return order < 0;
        case FL_LE: return order <= 0;
        case FL_GT: return order > 0;
        default: return order >= 0;  // FL_GE
    }
}

// one term on row r
SJ_HD bool fl_term(const FlTerm& t, const uint8_t* consts, const FlCols& c, sj_u64 r) {
    const sj_u64 at = (sj_u64)t.column * c.col_stride + r;
    const uint8_t ty = c.types[at];
    const uint32_t kind = t.op >> 4, cmp = t.op & 15u;
    if (kind == FL_TYPE) return (ty == (uint8_t)t.operand) == (cmp == FL_EQ);
    if (kind == FL_STRING) {
        if (ty != '"') return false;
        const sj_u64 v = c.values[at];
        const uint32_t len = (uint32_t)(v >> 32), clen = (uint32_t)(t.operand >> 32);
        // the length decides first: most rows of an equality filter end here, without a byte read
        if (cmp == FL_PREFIX ? len < clen : len != clen) return cmp == FL_NE;
        const uint8_t* src = c.sb + (v & 0xFFFFFFFFull);
        const uint8_t* k = consts + (uint32_t)t.operand;
        for (uint32_t i = 0; i < clen; ++i)  // (clen <= len: inside the cell's bytes)
            if (src[i] != k[i]) return cmp == FL_NE;
        return cmp != FL_NE;
    }
    if (ty != 'l' && ty != 'd') return false;
    const sj_u64 v = c.values[at];
    int order;
    if (kind == FL_LONG)
        order = ty == 'l' ? fl_cmp_ll((int64_t)v, (int64_t)t.operand) : -fl_cmp_ld((int64_t)t.operand, fl_double(v));
    else
        order = ty == 'l' ? fl_cmp_ld((int64_t)v, fl_double(t.operand)) : fl_cmp_dd(fl_double(v), fl_double(t.operand));
    return fl_holds(cmp, order == -2 ? 2 : order);
}

SJ_HD uint32_t fl_popcount(sj_u64 w) {
    w = w - ((w >> 1) & 0x5555555555555555ull);
    w = (w & 0x3333333333333333ull) + ((w >> 2) & 0x3333333333333333ull);
    return (uint32_t)((((w + (w >> 4)) & 0x0F0F0F0F0F0F0F0Full) * 0x0101010101010101ull) >> 56);
}

// pass 1, per chunk: keep[word] of its words (bits at or above n_rows are 0) and counts[chunk] = its kept rows.  The terms in
// plan order; a wave whose word is empty skips the rest of them.
template <class G>
SJ_HD void fl_eval_chunk(const G& g, const FlPlan& p, const FlCols& c, sj_u64 chunk, sj_u64* keep, sj_u64* counts) {
    const sj_u64 first = chunk * (c.chunk_rows / 64), nwords = fl_words(c);
    sj_u64 kept = 0;
    for (sj_u64 at = first; at < first + c.chunk_rows / 64; at += g.waves()) {
        const sj_u64 word = at + g.wave(), r0 = word * 64;
        sj_u64 w = g.ballot([&](uint32_t t) { return r0 + t < c.n_rows; });
        for (uint32_t k = 0; k < p.n_terms && w; ++k)
            w = g.ballot([&](uint32_t t) { return ((w >> t) & 1) && fl_term(p.terms[k], p.bytes, c, r0 + t); });
        if (word < nwords && g.first()) keep[word] = w;
        sj_u64 total;
        (void)g.scan_add(g.first() ? (sj_u64)fl_popcount(w) : 0ull, &total);
        kept += total;
    }
    if (g.lane() == 0) counts[chunk] = kept;
}

// pass 2, ONE group: the kept rows in front of every chunk and the result record
template <class G>
SJ_HD void fl_chunk_scan(const G& g, sj_u64* counts, sj_u64 nchunks, sj_u64 out_capacity, FlResult* res) {
    const sj_u64 total = g.scan_in_place(counts, nchunks);
    if (g.lane() == 0) {
        res->n_kept = total;
        res->flags = total > out_capacity ? FL_OVERFLOW : 0u;
        res->reserved = 0;
    }
}

struct FlOut {
    sj_u64* rows;
    uint8_t* types;  // any alignment
    sj_u64* values;
    sj_u64 capacity;
};

// pass 3, per chunk: the kept rows whose rank is below the capacity -- the row index, then its cell of every column
template <class G>
SJ_HD void fl_emit_chunk(const G& g, const FlCols& c, sj_u64 chunk, const sj_u64* keep, const sj_u64* counts, const FlOut& o) {
    const sj_u64 base = counts[chunk];
    if (base >= o.capacity) return;  // (ranks only grow: nothing of this chunk is stored)
    const sj_u64 first = chunk * (c.chunk_rows / 64), nwords = fl_words(c);
    for (sj_u64 at = first; at < first + c.chunk_rows / 64; at += g.waves()) {
        const sj_u64 word = at + g.wave();
        if (word >= nwords) break;
        sj_u64 rank0 = base;
        for (sj_u64 e = first; e < word; ++e) rank0 += fl_popcount(keep[e]);
        const sj_u64 w = keep[word];
        g.each([&](uint32_t t) {
            if (!((w >> t) & 1)) return;
            const sj_u64 j = rank0 + fl_popcount(w & ((1ull << t) - 1)), r = word * 64 + t;
            if (j >= o.capacity) return;
            o.rows[j] = r;
            for (sj_u64 col = 0; col < c.n_cols; ++col) {
                o.types[col * o.capacity + j] = c.types[col * c.col_stride + r];
                o.values[col * o.capacity + j] = c.values[col * c.col_stride + r];
            }
        });
    }
}
