// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o groupstats_asan tests/host_sim/groupstats_asan_main.cpp && ./groupstats_asan [cases]
// Random adversarial columns through sj_groupstats.h with the sequential group: row counts around the wave and chunk edges, key
// counts on both sides of GS_LDS_KEYS, wild indices (negatives, n_keys, INT32_MIN, INT32_MAX), every type byte, longs over the whole
// range with INT64_MIN and INT64_MAX among them, doubles that are integers below 2^20 (every partial sum exact: the sum is
// compared for equality in every schedule) with both zeros and NaNs among them, poison behind every other type byte, with and
// without a validity bitmap and a device row count, the groups / chunks in three orders and under a small grid cap.  The first
// cases are the 128-bit sum's: 1025 x INT64_MAX, 1025 x INT64_MIN, and a mix that cancels.  Every block is a heap allocation of
// EXACTLY its size -- the indices, types and values end behind the last LIVE row, the bitmap behind the last live row's word, the
// stats behind word n_keys * 10, a group's bins behind its last count -- so one byte too far is a report.  Every run is compared
// with a plain loop that sums in __int128.  TEST ONLY.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "groupstats_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}
static uint64_t rnd64() { return ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 11) ^ rnd(1u << 31); }

struct Want {
    uint64_t n_long = 0, n_double = 0, n_other = 0;
    __int128 sum = 0;
    double dsum = 0.0;
    int64_t min_long = INT64_MAX, max_long = INT64_MIN;
    double min_double = 0, max_double = 0;  // (with n_double)
};
// totalOrder on non-NaN doubles
static bool before(double a, double b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); }

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    static const uint64_t row_counts[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 64 * 1024 + 1};
    static const uint64_t key_counts[] = {0, 1, 5, 300, GS_LDS_KEYS, GS_LDS_KEYS + 1, 2000};
    static const uint64_t nan_bits[] = {0x7FF8000000000000ull, 0xFFF8000000000000ull, 0x7FF0000000000001ull, ~0ull};
    unsigned long long runs = 0, rows_seen = 0, outside_seen = 0, nan_seen = 0, lds_runs = 0, global_runs = 0;
    for (int k = 0; k < cases; ++k) {
        const int special = k < 6 ? k / 2 + 1 : 0;  // 1: INT64_MAX, 2: INT64_MIN, 3: a mix that cancels
        const uint64_t n_rows = special ? 1025 : k < 16 ? row_counts[k - 6] : rnd(4) ? rnd(2100) : row_counts[rnd(10)];
        const uint64_t n_keys = special ? (k % 2 ? GS_LDS_KEYS + 1 : 3) : key_counts[(k / 2) % 7];
        const bool one_bin = special || k % 5 == 0;
        std::vector<int32_t> indices(n_rows);
        std::vector<uint8_t> types(n_rows);
        std::vector<sj_u64> values(n_rows), validity((n_rows + 63) / 64);
        for (uint64_t r = 0; r < n_rows; ++r) {
            const uint32_t wild = rnd(12);
            indices[r] = one_bin ? (int32_t)(n_keys / 2) : wild == 0 ? -1 : wild == 1 ? (int32_t)n_keys : wild == 2 ? INT32_MIN : wild == 3 ? INT32_MAX
                                                                                                             : (int32_t)rnd((uint32_t)n_keys + 1);
            types[r] = special ? 'l' : rnd(3) ? (uint8_t)"\0nldtf[{\"ldld"[rnd(13)] : (uint8_t)rnd(256);
            if (special || rnd(4)) validity[r >> 6] |= 1ull << (r & 63);
            if (special)
                values[r] = special == 1 ? (sj_u64)INT64_MAX : special == 2 ? (sj_u64)INT64_MIN : r == 0 ? 0 : (r & 1) ? (sj_u64)INT64_MAX : (sj_u64)INT64_MIN + 1;
            else if (types[r] == 'l')
                values[r] = rnd(8) == 0 ? (sj_u64)INT64_MAX : rnd(8) == 0 ? (sj_u64)INT64_MIN : rnd(2) ? rnd64() : (sj_u64)(int64_t)((int)rnd(2001) - 1000);
            else if (types[r] == 'd')
                values[r] = rnd(10) == 0 ? nan_bits[rnd(4)] : rnd(10) == 0 ? (rnd(2) ? GS_SIGN : 0) : gs_bits((double)((int)rnd((1u << 21) - 1) - ((1 << 20) - 1)));
            else
                values[r] = rnd(2) ? ~0ull : 0x7FF8DEADBEEF0001ull;  // (poison: never read)
        }
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = !special && k % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        const bool with_validity = k % 3 != 0;
        // the reference
        std::vector<Want> want(n_keys);
        sj_u64 grouped = 0, outside = 0, nan = 0;
        for (uint64_t r = 0; r < live; ++r) {
            if (with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) continue;
            if (indices[r] < 0 || (uint64_t)indices[r] >= n_keys) {
                ++outside;
                continue;
            }
            Want& w = want[indices[r]];
            if (types[r] == 'l') {
                const int64_t v = (int64_t)values[r];
                ++w.n_long, w.sum += v;
                if (v < w.min_long) w.min_long = v;
                if (v > w.max_long) w.max_long = v;
            } else if (types[r] == 'd') {
                const double x = gs_double(values[r]);
                if (x != x) {
                    ++nan;
                    continue;
                }
                if (!w.n_double || before(x, w.min_double)) w.min_double = x;
                if (!w.n_double || before(w.max_double, x)) w.max_double = x;
                ++w.n_double, w.dsum += x;
            } else {
                ++w.n_other;
            }
            ++grouped;
        }
        if (special == 3 && (want[n_keys / 2].sum != 0 || want[n_keys / 2].n_long != 1025)) return fprintf(stderr, "the cancelling mix does not cancel\n"), 1;
        for (uint32_t chunk : {64u, 1024u})
            for (uint32_t order = 0; order < 3; ++order)
                for (uint32_t cap : {0u, 3u}) {
                    int32_t* ix = (int32_t*)malloc(live ? live * 4 : 1);
                    uint8_t* t = (uint8_t*)malloc(live ? live : 1);
                    sj_u64* val = (sj_u64*)malloc(live ? live * 8 : 1);
                    const uint64_t words_live = (live + 63) / 64;
                    sj_u64* v = with_validity ? (sj_u64*)malloc(words_live ? words_live * 8 : 1) : nullptr;
                    if (live) memcpy(ix, indices.data(), live * 4), memcpy(t, types.data(), live), memcpy(val, values.data(), live * 8);
                    if (v && words_live) memcpy(v, validity.data(), words_live * 8);
                    sj_u64* stats = (sj_u64*)malloc(n_keys ? n_keys * GS_WORDS * 8 : 1);
                    memset(stats, 0xEE, n_keys * GS_WORDS * 8);
                    GsResult* res = (GsResult*)malloc(sizeof(GsResult));
                    memset(res, 0xEE, sizeof *res);
                    const GsColumn c = {ix, v, t, val, n_rows, row_count, n_keys, chunk};
                    gs_sim_passes(c, order, cap, n_keys ? stats : nullptr, res);
                    ++runs;
                    (n_keys <= GS_LDS_KEYS ? lds_runs : global_runs) += n_rows != 0;
                    bool ok = res->n_rows == live && res->n_grouped == grouped && res->n_out_of_range == outside && res->n_nan == nan && res->flags == 0 &&
                              res->reserved == 0;
                    for (uint64_t key = 0; ok && key < n_keys; ++key) {
                        const sj_u64* s = stats + key * GS_WORDS;
                        const Want& w = want[key];
                        const __int128 sum = (__int128)(((unsigned __int128)s[GS_SUM_HI] << 64) | s[GS_SUM_LO]);
                        ok = s[GS_N_LONG] == w.n_long && s[GS_N_DOUBLE] == w.n_double && s[GS_N_OTHER] == w.n_other && sum == w.sum &&
                             (int64_t)s[GS_MIN_LONG] == w.min_long && (int64_t)s[GS_MAX_LONG] == w.max_long && gs_double(s[GS_SUM_DOUBLE]) == w.dsum &&
                             s[GS_MIN_DOUBLE] == (w.n_double ? gs_bits(w.min_double) : GS_INF_BITS) &&
                             s[GS_MAX_DOUBLE] == (w.n_double ? gs_bits(w.max_double) : GS_INF_BITS | GS_SIGN);
                    }
                    free(ix), free(t), free(val), free(v), free(stats), free(res);
                    if (!ok) return fprintf(stderr, "case %d: chunk %u, order %u, cap %u differs from the reference\n", k, chunk, order, cap), 1;
                }
        rows_seen += live, outside_seen += outside, nan_seen += nan;
    }
    printf("%d cases, %llu runs (%llu on the LDS path, %llu on the global path): %llu live rows, %llu out of range, %llu NaN; all runs agree with the reference\n",
           cases, runs, lds_runs, global_runs, rows_seen, outside_seen, nan_seen);
    return rows_seen && outside_seen && nan_seen && lds_runs && global_runs ? 0 : 1;
}
