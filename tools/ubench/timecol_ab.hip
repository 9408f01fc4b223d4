// timecol_ab.hip -- the A/B of the timestamp parse pass (simdjson-java_amd/csrc/sj_timecol.h, compiled verbatim): both forms of
// the byte fetch (byte-wide loads; aligned 8-byte words realigned in registers) at 1, 2, 4 and 8 rows per lane, every variant a
// workgroup of 256 threads, all in ONE process and interleaved, so that drift of the box hits every variant alike.  The product
// ships one of them (csrc/timecol.hip: TC_FETCH_WORDS, TC_LANE_ROWS); an experiment's switch does not stay in the product, so the
// comparison lives here.  The input is made here: two columns of RFC 3339 strings in a string buffer with 4-byte headers and
// other strings between them -- "YYYY-MM-DDThh:mm:ssZ" and "YYYY-MM-DDThh:mm:ss.ffffff+hh:mm" --, about 1 % malformed and 1 %
// MISSING.  Every variant's data words, validity words and records must equal the first variant's, and its counts what the
// generator made.  Prints one JSON line; with a path, writes it there too.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench/timecol_ab tools/ubench/timecol_ab.hip
//   tools/ubench/timecol_ab [rows] [rounds] [out.json]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_group_ballots.h"
#include "../../simdjson-java_amd/csrc/sj_timecol.h"

#define CHECK(x)                                                                       \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(2);                                                                   \
        }                                                                              \
    } while (0)

constexpr uint32_t AB_THREADS = 256;

template <bool WORDS, uint32_t ROWS>
__global__ __launch_bounds__(AB_THREADS) void k_ab_parse(const TcPlan p, TcCols c, TcOut o, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[AB_THREADS / 64];
    const sjmi::WgGroup g = {s_wave};
    tc_parse_chunk<WORDS, ROWS>(g, p, c, blockIdx.x, blockIdx.y, o, counts);
}
__global__ __launch_bounds__(AB_THREADS) void k_ab_finish(TcCols c, const sj_u64* __restrict__ counts, TcResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[AB_THREADS / 64];
    const sjmi::WgGroup g = {s_wave};
    tc_finish(g, c, blockIdx.x, counts, res);
}

struct Variant {
    const char* name;
    uint32_t rows;
    void (*kernel)(const TcPlan, TcCols, TcOut, sj_u64*);
};
static const Variant VARIANTS[] = {
    {"bytes_x1", 1, k_ab_parse<false, 1>}, {"words_x1", 1, k_ab_parse<true, 1>}, {"bytes_x2", 2, k_ab_parse<false, 2>}, {"words_x2", 2, k_ab_parse<true, 2>},
    {"bytes_x4", 4, k_ab_parse<false, 4>}, {"words_x4", 4, k_ab_parse<true, 4>}, {"bytes_x8", 8, k_ab_parse<false, 8>}, {"words_x8", 8, k_ab_parse<true, 8>},
};
constexpr int NV = sizeof(VARIANTS) / sizeof(VARIANTS[0]);

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1000000;
    const int rounds = argc > 2 ? atoi(argv[2]) : 30;
    const char* out_path = argc > 3 ? argv[3] : nullptr;
    // ---- the input
    std::vector<uint8_t> types(2 * n), sb;
    std::vector<sj_u64> values(2 * n);
    uint64_t want_valid[2] = {0, 0}, want_malformed[2] = {0, 0}, string_bytes = 0;
    sb.reserve(n * 90);
    for (uint64_t r = 0; r < n; ++r)
        for (int col = 0; col < 2; ++col) {
            char text[64];
            int len;
            const int y = 1990 + (int)rnd(50), mo = 1 + (int)rnd(12), d = 1 + (int)rnd(28), h = (int)rnd(24), mi = (int)rnd(60), s = (int)rnd(60);
            if (col == 0)
                len = snprintf(text, sizeof text, "%04d-%02d-%02dT%02d:%02d:%02dZ", y, mo, d, h, mi, s);
            else
                len = snprintf(text, sizeof text, "%04d-%02d-%02dT%02d:%02d:%02d.%06u%c%02u:%02u", y, mo, d, h, mi, s, rnd(1000000), rnd(2) ? '+' : '-', rnd(14), 15 * rnd(4));
            const uint32_t kind = rnd(100);
            if (kind == 0) text[rnd((uint32_t)len)] = '/';  // malformed: '/' is nowhere in the grammar
            sb.insert(sb.end(), 4, 0);                      // (a record header)
            const uint64_t at = sb.size();
            sb.insert(sb.end(), text, text + len);
            for (uint32_t k = rnd(25); k > 0; --k) sb.push_back((uint8_t)('a' + rnd(26)));  // (another string of the document)
            const uint64_t cell = col * n + r;
            if (kind == 1) {
                types[cell] = 0, values[cell] = ~0ull;
            } else {
                types[cell] = '"', values[cell] = ((sj_u64)len << 32) | at;
                string_bytes += (uint64_t)len;
                (kind == 0 ? want_malformed : want_valid)[col]++;
            }
        }
    if (sb.size() >= (1ull << 32)) return fprintf(stderr, "the string buffer does not fit 32-bit offsets\n"), 2;
    // ---- the device
    const TcField fields[2] = {{0, TC_MICRO, 0, 0}, {1, TC_MICRO, 0, 0}};
    TcPlan plan;
    if (tc_plan_compile(fields, 2, 2, &plan) != 0) return 2;
    const uint64_t words = (n + 63) / 64;
    uint8_t *d_types, *d_sb;
    sj_u64 *d_values, *d_data, *d_validity, *d_ws;
    TcResult* d_res;
    CHECK(hipMalloc(&d_types, 2 * n));
    CHECK(hipMalloc(&d_sb, sb.size()));
    CHECK(hipMalloc(&d_values, 2 * n * 8));
    CHECK(hipMalloc(&d_data, 2 * n * 8));
    CHECK(hipMalloc(&d_validity, 2 * words * 8));
    CHECK(hipMalloc(&d_ws, (2 * tc_chunks(n, 256) + 1) * 8));
    CHECK(hipMalloc(&d_res, 2 * sizeof(TcResult)));
    CHECK(hipMemcpy(d_types, types.data(), 2 * n, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_sb, sb.data(), sb.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_values, values.data(), 2 * n * 8, hipMemcpyHostToDevice));
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    auto launch = [&](const Variant& v) {
        const TcCols c = {d_types, d_values, n, n, nullptr, d_sb, AB_THREADS * v.rows};
        const TcOut o = {d_data, n, d_validity, words};
        hipLaunchKernelGGL(v.kernel, dim3((unsigned)tc_chunks(n, c.chunk_rows), 2), dim3(AB_THREADS), 0, st, plan, c, o, d_ws);
        hipLaunchKernelGGL(k_ab_finish, dim3(2), dim3(AB_THREADS), 0, st, c, (const sj_u64*)d_ws, d_res);
    };
    // ---- every variant gives the same, and the counts the generator made
    std::vector<sj_u64> first_data(2 * n), data(2 * n), first_validity(2 * words), validity(2 * words);
    TcResult first_res[2], res[2];
    for (int v = 0; v < NV; ++v) {
        CHECK(hipMemsetAsync(d_data, 0xEE, 2 * n * 8, st));
        CHECK(hipMemsetAsync(d_validity, 0xEE, 2 * words * 8, st));
        launch(VARIANTS[v]);
        CHECK(hipGetLastError());
        CHECK(hipStreamSynchronize(st));
        CHECK(hipMemcpy(data.data(), d_data, 2 * n * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(validity.data(), d_validity, 2 * words * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(res, d_res, sizeof res, hipMemcpyDeviceToHost));
        for (int f = 0; f < 2; ++f)
            if (res[f].n_rows != n || res[f].n_valid != want_valid[f] || res[f].n_malformed != want_malformed[f] || res[f].n_other || res[f].n_range || res[f].n_inexact)
                return fprintf(stderr, "%s: the record of field %d is not what the generator made\n", VARIANTS[v].name, f), 1;
        if (v == 0) {
            first_data = data, first_validity = validity;
            memcpy(first_res, res, sizeof res);
        } else if (data != first_data || validity != first_validity || memcmp(res, first_res, sizeof res) != 0) {
            return fprintf(stderr, "%s differs from %s\n", VARIANTS[v].name, VARIANTS[0].name), 1;
        }
    }
    // ---- interleaved single calls between events
    std::vector<std::vector<float>> ms(NV);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    for (int round = -3; round < rounds; ++round)
        for (int v = 0; v < NV; ++v) {
            CHECK(hipEventRecord(e0, st));
            launch(VARIANTS[v]);
            CHECK(hipEventRecord(e1, st));
            CHECK(hipEventSynchronize(e1));
            float t;
            CHECK(hipEventElapsedTime(&t, e0, e1));
            if (round >= 0) ms[v].push_back(t);
        }
    const double least = 2.0 * n * 9 + (double)string_bytes + 2.0 * n * 8.125;  // bytes the call must move
    std::string json = "{\"rows\": " + std::to_string(n) + ", \"fields\": 2, \"unit\": \"us\", \"rounds\": " + std::to_string(rounds) +
                       ", \"string_buffer_bytes\": " + std::to_string(sb.size()) + ", \"least_bytes_moved\": " + std::to_string((uint64_t)least) +
                       ", \"verified\": \"every variant's data, validity and records equal the first's; counts equal the generator's\", \"variants\": {";
    for (int v = 0; v < NV; ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        char buf[256];
        snprintf(buf, sizeof buf, "%s\"%s\": {\"median_ms\": %.5f, \"min_ms\": %.5f, \"p25_ms\": %.5f, \"p75_ms\": %.5f, \"max_ms\": %.5f}", v ? ", " : "", VARIANTS[v].name,
                 ms[v][ms[v].size() / 2], ms[v].front(), ms[v][ms[v].size() / 4], ms[v][ms[v].size() * 3 / 4], ms[v].back());
        json += buf;
    }
    json += "}}";
    puts(json.c_str());
    if (out_path) {
        FILE* f = fopen(out_path, "w");
        if (!f) return fprintf(stderr, "cannot write %s\n", out_path), 2;
        fprintf(f, "%s\n", json.c_str());
        fclose(f);
    }
    return 0;
}
