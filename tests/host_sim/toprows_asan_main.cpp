// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o toprows_asan tests/host_sim/toprows_asan_main.cpp && ./toprows_asan [cases]
// Random adversarial key columns through sj_toprows.h with the sequential group: row counts around the wave and chunk edges, k
// around 64 and at SJMI_TOP_MAX_K and above the candidates, both kinds and both directions, every type byte, longs over the whole
// range or from a handful of values (ties everywhere) or equal but for one bit, doubles with both zeros, both infinities, denormals
// and NaNs, longs above 2^53 under the DOUBLE kind, poison behind every type byte that makes no candidate, with and without types,
// a validity bitmap, a device row count and carried columns, the groups / chunks in three orders and under a small grid cap.
// Every block is a heap allocation of EXACTLY its size -- the types and values end behind the last LIVE row, the bitmap behind
// the last live row's word, rows behind entry k, the carried outputs behind cell n_cols * k; the scratch, a group's bins and the
// sort's pairs are such blocks inside toprows_sim.cpp -- so one byte too far is a report.  Every run is compared with
// std::stable_sort of the candidates in row order.  TEST ONLY.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "toprows_sim.cpp"

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

struct Cand {
    uint64_t row, bits;  // the value word as the kind
};

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    static const uint64_t row_counts[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 64 * 1024 + 1};
    static const uint64_t ks[] = {0, 1, 2, 63, 64, 65, 700, 2047, 2048};
    static const uint64_t nan_bits[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, ~0ull};
    static const double specials[] = {0.0, -0.0, INFINITY, -INFINITY, 5e-324, -5e-324, 1.5, -1.5, 1e300, -1e-300};
    unsigned long long runs = 0, rows_seen = 0, out_seen = 0, nan_seen = 0, inexact_seen = 0, tie_cuts = 0;
    for (int i = 0; i < cases; ++i) {
        const uint64_t n_rows = i < 10 ? row_counts[i] : rnd(4) ? rnd(2600) : row_counts[rnd(10)];
        const uint64_t k = ks[(i / 3) % 9];
        const uint32_t kind = i % 2 ? TR_DOUBLE : TR_LONG, flags = (i / 2) % 2 ? TR_SMALLEST : 0;
        const bool with_types = i % 5 != 0, with_validity = i % 3 != 0;
        const uint32_t shape = rnd(4);  // 0: the whole range, 1: a handful of values, 2: equal but for one bit, 3: counters
        const uint64_t base = rnd64(), bit = 1ull << rnd(64);
        const uint64_t n_cols = i % 4 == 3 ? 0 : 1 + i % 3, stride = n_rows + rnd(3);
        std::vector<uint8_t> types(n_rows), ctypes(n_cols * stride);
        std::vector<sj_u64> values(n_rows), validity((n_rows + 63) / 64), cvalues(n_cols * stride);
        for (uint64_t r = 0; r < n_rows; ++r) {
            types[r] = rnd(4) ? (uint8_t)"ldldldll\0n\"t"[rnd(12)] : (uint8_t)rnd(256);
            if (rnd(5)) validity[r >> 6] |= 1ull << (r & 63);
            const bool number = !with_types || types[r] == 'l' || (types[r] == 'd' && kind == TR_DOUBLE);
            const bool as_long = with_types ? types[r] == 'l' : kind == TR_LONG;
            if (!number)
                values[r] = rnd(2) ? ~0ull : 0x7FF8DEADBEEF0001ull;  // (poison: never read)
            else if (as_long)
                values[r] = shape == 0 ? (rnd(8) ? rnd64() : rnd(2) ? (sj_u64)INT64_MAX : (sj_u64)INT64_MIN)
                            : shape == 1 ? (sj_u64)((1ll << 53) + (int64_t)rnd(7) - 3) * (rnd(2) ? 1 : -1)
                            : shape == 2 ? (rnd(2) ? base | bit : base & ~bit)
                                         : (sj_u64)rnd(10001);
            else
                values[r] = rnd(12) == 0 ? nan_bits[rnd(4)] : shape == 1 ? as_bits(specials[rnd(10)]) : shape == 2 ? as_bits(rnd(2) ? 0.0 : -0.0)
                            : shape == 3 ? as_bits((double)rnd(50))
                                         : (rnd64() & ~(0x7FFull << 52)) | ((uint64_t)rnd(2047) << 52);  // (any finite double)
        }
        for (uint64_t j = 0; j < n_cols * stride; ++j) ctypes[j] = (uint8_t)rnd(256), cvalues[j] = rnd64();
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = i % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        // the reference: the candidates in row order, a stable sort by value
        std::vector<Cand> cand;
        uint64_t n_null = 0, n_other = 0, n_nan = 0, n_inexact = 0;
        for (uint64_t r = 0; r < live; ++r) {
            const uint8_t t = types[r];
            if (with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) {
                ++n_null;
            } else if (with_types && (t == 0 || t == 'n')) {
                ++n_null;
            } else if (with_types && !(t == 'l' || (t == 'd' && kind == TR_DOUBLE))) {
                ++n_other;
            } else if (kind == TR_LONG) {
                cand.push_back({r, values[r]});
            } else {
                double x = as_double(values[r]);
                if (with_types && t == 'l') {
                    const int64_t v = (int64_t)values[r];
                    x = (double)v;
                    n_inexact += (__int128)x != (__int128)v;
                }
                if (x != x)
                    ++n_nan;
                else
                    cand.push_back({r, as_bits(x)});
            }
        }
        const bool smallest = flags != 0;
        std::stable_sort(cand.begin(), cand.end(), [&](const Cand& a, const Cand& b) {
            if (kind == TR_LONG) return smallest ? (int64_t)a.bits < (int64_t)b.bits : (int64_t)a.bits > (int64_t)b.bits;
            const double x = as_double(a.bits), y = as_double(b.bits);
            const bool less = x < y || (x == y && std::signbit(x) && !std::signbit(y)), more = y < x || (x == y && std::signbit(y) && !std::signbit(x));
            return smallest ? less : more;
        });
        const uint64_t n_out = k < cand.size() ? k : cand.size();
        tie_cuts += n_out && n_out < cand.size() && cand[n_out].bits == cand[n_out - 1].bits;
        for (uint32_t chunk : {64u, 1024u})
            for (uint32_t order = 0; order < 3; ++order)
                for (uint32_t cap : {0u, 3u}) {
                    uint8_t* t = with_types ? (uint8_t*)malloc(live ? live : 1) : nullptr;
                    sj_u64* val = (sj_u64*)malloc(live ? live * 8 : 1);
                    const uint64_t words_live = (live + 63) / 64;
                    sj_u64* v = with_validity ? (sj_u64*)malloc(words_live ? words_live * 8 : 1) : nullptr;
                    if (t && live) memcpy(t, types.data(), live);
                    if (live) memcpy(val, values.data(), live * 8);
                    if (v && words_live) memcpy(v, validity.data(), words_live * 8);
                    uint8_t* ct = (uint8_t*)malloc(n_cols * stride ? n_cols * stride : 1);
                    sj_u64* cv = (sj_u64*)malloc(n_cols * stride ? n_cols * stride * 8 : 1);
                    if (n_cols * stride) memcpy(ct, ctypes.data(), n_cols * stride), memcpy(cv, cvalues.data(), n_cols * stride * 8);
                    sj_u64* rows = (sj_u64*)malloc(k ? k * 8 : 1);
                    uint8_t* ot = (uint8_t*)malloc(n_cols * k ? n_cols * k : 1);
                    sj_u64* ov = (sj_u64*)malloc(n_cols * k ? n_cols * k * 8 : 1);
                    TrResult* res = (TrResult*)malloc(sizeof(TrResult));
                    memset(rows, 0xEE, k * 8), memset(ot, 0xEE, n_cols * k), memset(ov, 0xEE, n_cols * k * 8), memset(res, 0xEE, sizeof *res);
                    const TrColumn c = {t, v, val, n_rows, row_count, kind, flags, k, chunk};
                    const TrCarry in = {ct, cv, n_cols, stride};
                    const TrOut o = {rows, ot, ov};
                    tr_sim_passes(c, in, o, order, cap, res, nullptr);
                    ++runs;
                    bool ok = res->n_rows == live && res->n_candidates == cand.size() && res->n_null == n_null && res->n_other == n_other &&
                              res->n_nan == n_nan && res->n_inexact == n_inexact && res->n_out == n_out &&
                              res->kth_bits == (n_out ? cand[n_out - 1].bits : 0) && res->flags == 0 && res->reserved == 0;
                    for (uint64_t j = 0; ok && j < k; ++j) {
                        ok = rows[j] == (j < n_out ? cand[j].row : 0xEEEEEEEEEEEEEEEEull);
                        for (uint64_t col = 0; ok && col < n_cols; ++col)
                            ok = j < n_out ? ot[col * k + j] == ctypes[col * stride + cand[j].row] && ov[col * k + j] == cvalues[col * stride + cand[j].row]
                                           : ot[col * k + j] == 0xEE && ov[col * k + j] == 0xEEEEEEEEEEEEEEEEull;
                    }
                    free(t), free(val), free(v), free(ct), free(cv), free(rows), free(ot), free(ov), free(res);
                    if (!ok) return fprintf(stderr, "case %d: chunk %u, order %u, cap %u differs from the reference\n", i, chunk, order, cap), 1;
                }
        rows_seen += live, out_seen += n_out, nan_seen += n_nan, inexact_seen += n_inexact;
    }
    printf("%d cases, %llu runs: %llu live rows, %llu rows returned, %llu NaN, %llu inexact, %llu cuts inside a tie; all runs agree with the reference\n",
           cases, runs, rows_seen, out_seen, nan_seen, inexact_seen, tie_cuts);
    return rows_seen && out_seen && nan_seen && inexact_seen && tie_cuts ? 0 : 1;
}
