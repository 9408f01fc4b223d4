// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o sortrows_asan tests/host_sim/sortrows_asan_main.cpp && ./sortrows_asan [cases]
// Random adversarial key columns through sj_sortrows.h with the sequential group: position counts around the wave, chunk and tile
// edges, both kinds and both directions, every type byte, longs over the whole range or from a handful of values (ties everywhere)
// or equal but for one bit or all equal (no digit pass), doubles with both zeros, both infinities, denormals and NaNs, longs above
// 2^53 under the DOUBLE kind, poison behind every type byte that makes no candidate, with and without types, a validity bitmap, a
// device row count, carried columns, and rows_in: none, a permutation, a subset with BAD entries (n_source_rows, 2^32 - 1, 2^63);
// the groups / chunks / tiles in three orders, small chunks and tiles, a small grid cap.
// Every block is a heap allocation of EXACTLY its size -- the source columns end behind row n_source_rows - 1, rows_in behind the
// last LIVE position, rows behind entry n_rows, the carried outputs behind cell n_cols * n_rows; the scratch and a tile's counts
// and bases are such blocks inside sortrows_sim.cpp -- so one byte too far is a report.  Every run is compared with
// std::stable_sort of the positions.  TEST ONLY.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "sortrows_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}
static uint64_t rnd64() { return ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 11) ^ rnd(1u << 31); }
static double as_double(uint64_t bits) {
    double x;
    memcpy(&x, &bits, 8);
    return x;
}
static uint64_t as_bits(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return b;
}
template <class T>
static T* exact(const std::vector<T>& v, uint64_t n) {  // a heap block of exactly n entries
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, v.data(), n * sizeof(T));
    return p;
}

struct Pos {
    uint64_t pos, row, bits;  // the value word as the kind
    uint32_t cls;             // 0 candidate, 1 NaN, 2 other, 3 null or bad
};

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    static const uint64_t counts[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193};
    static const uint64_t nan_bits[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, ~0ull};
    static const double specials[] = {0.0, -0.0, INFINITY, -INFINITY, 5e-324, -5e-324, 1.5, -1.5, 1e300, -1e-300};
    static const uint64_t bad_entries[] = {0, 0xFFFFFFFFull, 1ull << 63};  // (entry 0 stands for n_source_rows)
    unsigned long long runs = 0, seen = 0, nan_seen = 0, inexact_seen = 0, bad_seen = 0, still = 0, ties = 0;
    for (int i = 0; i < cases; ++i) {
        const uint64_t n_source = i < 12 ? counts[i] : rnd(4) ? rnd(2600) : counts[rnd(12)];
        const uint32_t kind = i % 2 ? SR_DOUBLE : SR_LONG, flags = (i / 2) % 2 ? SR_DESCENDING : 0;
        const bool with_types = i % 5 != 0, with_validity = i % 3 != 0;
        const uint32_t shape = rnd(5);  // 0: the whole range, 1: a handful of values, 2: equal but for one bit, 3: counters, 4: all equal
        const uint32_t form = i % 3;    // rows_in: none, a permutation, a subset with BAD entries
        const uint64_t base = rnd64(), bit = 1ull << rnd(64);
        const uint64_t n_cols = i % 4 == 3 ? 0 : 1 + i % 3, stride = n_source + rnd(3);
        std::vector<uint8_t> types(n_source), ctypes(n_cols * stride);
        std::vector<sj_u64> values(n_source), validity((n_source + 63) / 64), cvalues(n_cols * stride);
        for (uint64_t r = 0; r < n_source; ++r) {
            types[r] = rnd(4) ? (uint8_t)"ldldldll\0n\"t"[rnd(12)] : (uint8_t)rnd(256);
            if (rnd(5)) validity[r >> 6] |= 1ull << (r & 63);
            const bool number = !with_types || types[r] == 'l' || (types[r] == 'd' && kind == SR_DOUBLE);
            const bool as_long = with_types ? types[r] == 'l' : kind == SR_LONG;
            if (!number)
                values[r] = rnd(2) ? ~0ull : 0x7FF8DEADBEEF0001ull;  // (poison: never read)
            else if (as_long)
                values[r] = shape == 0 ? (rnd(8) ? rnd64() : rnd(2) ? (sj_u64)INT64_MAX : (sj_u64)INT64_MIN)
                            : shape == 1 ? (sj_u64)((1ll << 53) + (int64_t)rnd(7) - 3) * (rnd(2) ? 1 : -1)
                            : shape == 2 ? (rnd(2) ? base | bit : base & ~bit)
                            : shape == 3 ? (sj_u64)rnd(10001)
                                         : 77;
            else
                values[r] = rnd(12) == 0 ? nan_bits[rnd(4)] : shape == 1 ? as_bits(specials[rnd(10)]) : shape == 2 ? as_bits(rnd(2) ? 0.0 : -0.0)
                            : shape == 3 ? as_bits((double)rnd(50))
                            : shape == 4 ? as_bits(2.5)
                                         : (rnd64() & ~(0x7FFull << 52)) | ((uint64_t)rnd(2047) << 52);  // (any finite double)
        }
        for (uint64_t j = 0; j < n_cols * stride; ++j) ctypes[j] = (uint8_t)rnd(256), cvalues[j] = rnd64();
        std::vector<sj_u64> rows_in;
        if (form == 1) {
            for (uint64_t r = 0; r < n_source; ++r) rows_in.push_back(r);
            for (uint64_t r = n_source; r > 1; --r) std::swap(rows_in[r - 1], rows_in[rnd((uint32_t)r)]);
        } else if (form == 2) {
            for (uint64_t r = 0; r < n_source + 3; ++r)
                if (rnd(3)) {
                    const uint64_t bad = bad_entries[rnd(3)];
                    rows_in.push_back(rnd(9) && r < n_source ? r : bad ? bad : n_source);
                }
        }
        const uint64_t n_rows = form ? rows_in.size() : n_source;
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = i % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        // the reference: the positions in order, a stable sort by (class, value)
        std::vector<Pos> ref;
        uint64_t n_cand = 0, n_null = 0, n_other = 0, n_nan = 0, n_inexact = 0, n_bad = 0, lo = ~0ull, hi = 0;
        for (uint64_t p = 0; p < live; ++p) {
            const uint64_t r = form ? rows_in[p] : p;
            if (r >= n_source) {
                ++n_bad;
                ref.push_back({p, r, 0, 3});
                continue;
            }
            const uint8_t t = types[r];
            if ((with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) || (with_types && (t == 0 || t == 'n'))) {
                ++n_null;
                ref.push_back({p, r, 0, 3});
            } else if (with_types && !(t == 'l' || (t == 'd' && kind == SR_DOUBLE))) {
                ++n_other;
                ref.push_back({p, r, 0, 2});
            } else {
                uint64_t bits = values[r];
                if (kind == SR_DOUBLE) {
                    double x = as_double(bits);
                    if (with_types && t == 'l') {
                        const int64_t v = (int64_t)bits;
                        x = (double)v;
                        n_inexact += (__int128)x != (__int128)v;
                    }
                    if (x != x) {
                        ++n_nan;
                        ref.push_back({p, r, 0, 1});
                        continue;
                    }
                    bits = as_bits(x);
                }
                ++n_cand;
                const uint64_t key = kind == SR_LONG ? bits ^ (1ull << 63) : (bits >> 63) ? ~bits : bits ^ (1ull << 63);
                lo = key < lo ? key : lo, hi = key > hi ? key : hi;
                ref.push_back({p, r, bits, 0});
            }
        }
        const bool descending = flags != 0;
        std::stable_sort(ref.begin(), ref.end(), [&](const Pos& a, const Pos& b) {
            if (a.cls != b.cls) return a.cls < b.cls;
            if (a.cls) return false;
            if (kind == SR_LONG) return descending ? (int64_t)a.bits > (int64_t)b.bits : (int64_t)a.bits < (int64_t)b.bits;
            const double x = as_double(a.bits), y = as_double(b.bits);
            const bool less = x < y || (x == y && std::signbit(x) && !std::signbit(y)), more = y < x || (x == y && std::signbit(y) && !std::signbit(x));
            return descending ? more : less;
        });
        const uint64_t differ = n_cand ? lo ^ hi : 0;
        const uint64_t passes = differ ? (64 - (uint64_t)__builtin_clzll(differ) + 7) / 8 : 0;
        for (uint64_t j = 1; j < n_cand; ++j) ties += ref[j].bits == ref[j - 1].bits;
        for (uint32_t shape_of : {0u, 1u, 2u})  // chunk / tile: 64 / 64, 256 / 1024, the kernels' own
            for (uint32_t order = 0; order < 3; ++order)
                for (uint32_t cap : {0u, 3u}) {
                    const uint32_t chunk = shape_of == 0 ? 64 : shape_of == 1 ? 256 : SR_CHUNK_ROWS, tile = shape_of == 0 ? 64 : shape_of == 1 ? 1024 : SR_TILE_ROWS;
                    uint8_t* t = with_types ? exact(types, n_source) : nullptr;
                    sj_u64* val = exact(values, n_source);
                    sj_u64* v = with_validity ? exact(validity, (n_source + 63) / 64) : nullptr;
                    sj_u64* ri = form ? exact(rows_in, live) : nullptr;
                    uint8_t* ct = exact(ctypes, n_cols * stride);
                    sj_u64* cv = exact(cvalues, n_cols * stride);
                    sj_u64* rows = (sj_u64*)malloc(n_rows ? n_rows * 8 : 1);
                    uint8_t* ot = (uint8_t*)malloc(n_cols * n_rows ? n_cols * n_rows : 1);
                    sj_u64* ov = (sj_u64*)malloc(n_cols * n_rows ? n_cols * n_rows * 8 : 1);
                    SrResult* res = (SrResult*)malloc(sizeof(SrResult));
                    memset(rows, 0xEE, n_rows * 8), memset(ot, 0xEE, n_cols * n_rows), memset(ov, 0xEE, n_cols * n_rows * 8), memset(res, 0xEE, sizeof *res);
                    const SrColumn c = {t, v, val, n_source, ri, n_rows, row_count, kind, flags, chunk, tile};
                    const SrCarry in = {ct, cv, n_cols, stride};
                    const SrOut o = {rows, ot, ov, n_rows};
                    sr_sim_passes(c, in, o, order, cap, res);
                    ++runs;
                    bool ok = res->n_rows == live && res->n_candidates == n_cand && res->n_null == n_null && res->n_other == n_other &&
                              res->n_nan == n_nan && res->n_inexact == n_inexact && res->n_bad == n_bad && res->n_passes == passes &&
                              res->flags == (n_bad ? SR_BAD_ROW : 0u) && res->reserved == 0;
                    for (uint64_t j = 0; ok && j < n_rows; ++j) {
                        ok = rows[j] == (j < live ? ref[j].row : 0xEEEEEEEEEEEEEEEEull);
                        for (uint64_t col = 0; ok && col < n_cols; ++col) {
                            const bool bad = j < live && ref[j].row >= n_source;
                            ok = j >= live ? ot[col * n_rows + j] == 0xEE && ov[col * n_rows + j] == 0xEEEEEEEEEEEEEEEEull
                                 : bad     ? ot[col * n_rows + j] == 0 && ov[col * n_rows + j] == 0
                                           : ot[col * n_rows + j] == ctypes[col * stride + ref[j].row] && ov[col * n_rows + j] == cvalues[col * stride + ref[j].row];
                        }
                    }
                    free(t), free(val), free(v), free(ri), free(ct), free(cv), free(rows), free(ot), free(ov), free(res);
                    if (!ok) return fprintf(stderr, "case %d: chunk %u, tile %u, order %u, cap %u differs from the reference\n", i, chunk, tile, order, cap), 1;
                }
        seen += live, nan_seen += n_nan, inexact_seen += n_inexact, bad_seen += n_bad, still += n_cand > 1 && !passes;
    }
    printf("%d cases, %llu runs: %llu live positions, %llu NaN, %llu inexact, %llu bad entries, %llu ties, %llu columns that moved nothing; all runs agree with the reference\n",
           cases, runs, seen, nan_seen, inexact_seen, bad_seen, ties, still);
    return seen && nan_seen && inexact_seen && bad_seen && ties && still ? 0 : 1;
}
