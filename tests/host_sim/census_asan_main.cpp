// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o census_asan tests/host_sim/census_asan_main.cpp && ./census_asan [cases]
// Random adversarial columns through sj_census.h with the sequential group: row counts around the wave and chunk edges, key counts
// on both sides of CS_LDS_KEYS, wild indices (negatives, n_keys, INT32_MIN, INT32_MAX), every type byte, with and without a
// validity bitmap and a device row count, the groups / chunks in three orders and under a small grid cap.  Every block is a heap
// allocation of EXACTLY its size -- the indices and types end behind the last LIVE row, the bitmap behind the last live row's
// word, the counts behind word n_keys * 8, a group's bins behind its last bin -- so one byte too far is a report.  Every run is
// compared with a plain loop.  TEST ONLY.
#include <cstdio>
#include <cstdlib>

#include "census_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    static const uint64_t row_counts[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 3000, 64 * 1024 + 1};
    static const uint64_t key_counts[] = {0, 1, 5, 300, CS_LDS_KEYS, CS_LDS_KEYS + 1, 5000};
    unsigned long long runs = 0, rows_seen = 0, outside_seen = 0, lds_runs = 0, global_runs = 0;
    for (int k = 0; k < cases; ++k) {
        const uint64_t n_rows = k < 10 ? row_counts[k] : rnd(4) ? rnd(2100) : row_counts[rnd(10)];
        const uint64_t n_keys = key_counts[(k / 2) % 7];
        const bool one_bin = k % 5 == 0;
        std::vector<int32_t> indices(n_rows);
        std::vector<uint8_t> types(n_rows);
        std::vector<sj_u64> validity((n_rows + 63) / 64);
        for (uint64_t r = 0; r < n_rows; ++r) {
            const uint32_t wild = rnd(12);
            indices[r] = one_bin ? (int32_t)(n_keys / 2) : wild == 0 ? -1 : wild == 1 ? (int32_t)n_keys : wild == 2 ? INT32_MIN : wild == 3 ? INT32_MAX
                                                                                                             : (int32_t)rnd((uint32_t)n_keys + 1);
            types[r] = one_bin ? 'l' : rnd(3) ? (uint8_t)"\0nldtf[{\""[rnd(9)] : (uint8_t)rnd(256);
            if (rnd(4)) validity[r >> 6] |= 1ull << (r & 63);
        }
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = k % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        const bool with_validity = k % 3 != 0;
        // the reference
        std::vector<sj_u64> want(n_keys * CS_CLASSES + 1, 0);
        sj_u64 counted = 0, outside = 0;
        for (uint64_t r = 0; r < live; ++r) {
            if (with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) continue;
            if (indices[r] < 0 || (uint64_t)indices[r] >= n_keys) {
                ++outside;
                continue;
            }
            static const char order_of[] = "ld\"tn[{";
            uint32_t cl = 7;
            for (uint32_t j = 0; j < 7; ++j)
                if (types[r] == (uint8_t)order_of[j]) cl = j;
            if (types[r] == 'f') cl = 3;
            ++want[(uint64_t)indices[r] * CS_CLASSES + cl];
            ++counted;
        }
        for (uint32_t chunk : {64u, 1024u})
            for (uint32_t order = 0; order < 3; ++order)
                for (uint32_t cap : {0u, 3u}) {
                    int32_t* ix = (int32_t*)malloc(live ? live * 4 : 1);
                    uint8_t* t = (uint8_t*)malloc(live ? live : 1);
                    const uint64_t words_live = (live + 63) / 64;
                    sj_u64* v = with_validity ? (sj_u64*)malloc(words_live ? words_live * 8 : 1) : nullptr;
                    if (live) memcpy(ix, indices.data(), live * 4), memcpy(t, types.data(), live);
                    if (v && words_live) memcpy(v, validity.data(), words_live * 8);
                    sj_u64* counts = (sj_u64*)malloc(n_keys ? n_keys * CS_CLASSES * 8 : 1);
                    memset(counts, 0xEE, n_keys * CS_CLASSES * 8);
                    CsResult* res = (CsResult*)malloc(sizeof(CsResult));
                    memset(res, 0xEE, sizeof *res);
                    const CsColumn c = {ix, v, t, n_rows, row_count, n_keys, chunk};
                    cs_sim_passes(c, order, cap, n_keys ? counts : nullptr, res);
                    ++runs;
                    (n_keys <= CS_LDS_KEYS ? lds_runs : global_runs) += n_rows != 0;
                    bool ok = res->n_rows == live && res->n_counted == counted && res->n_out_of_range == outside && res->flags == 0 && res->reserved == 0;
                    ok = ok && (!n_keys || memcmp(counts, want.data(), n_keys * CS_CLASSES * 8) == 0);
                    free(ix), free(t), free(v), free(counts), free(res);
                    if (!ok) return fprintf(stderr, "case %d: chunk %u, order %u, cap %u differs from the reference\n", k, chunk, order, cap), 1;
                }
        rows_seen += live, outside_seen += outside;
    }
    printf("%d cases, %llu runs (%llu on the LDS path, %llu on the global path): %llu live rows, %llu out of range; all runs agree with the reference\n",
           cases, runs, lds_runs, global_runs, rows_seen, outside_seen);
    return rows_seen && outside_seen && lds_runs && global_runs ? 0 : 1;
}
