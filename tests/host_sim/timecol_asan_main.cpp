// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o timecol_asan tests/host_sim/timecol_asan_main.cpp && ./timecol_asan [cases]
// Random column sets and schemas through sj_timecol.h with the sequential group, at every chunk size the simulation has and with
// both fetch forms.  Every block is a heap allocation of EXACTLY its size -- the type and value blocks end behind the last
// column's last live row, the outputs behind the last field's slice, the scratch behind its last word -- so one byte too far is
// a report.  The string buffer is exact for the byte-wide fetch; for the aligned-word fetch it begins 8-byte aligned and is
// rounded up to whole words, which is what that form asks of its memory (a word never leaves the page of the byte it is read for;
// a heap block is not a page).  All runs of a case must agree word for word.  TEST ONLY.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "timecol_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}

static std::string stamp() {
    static const int years[] = {0, 1, 1677, 1678, 1900, 1969, 1970, 2000, 2024, 2262, 2263, 9999};
    char text[80];
    const int y = rnd(3) ? years[rnd(12)] : (int)rnd(10000);
    int len = snprintf(text, sizeof text, "%04d-%02d-%02d%c%02d:%02d:%02d", y, 1 + (int)rnd(12), 1 + (int)rnd(rnd(4) ? 28 : 31), "TTt "[rnd(4)], (int)rnd(rnd(8) ? 24 : 25),
                       (int)rnd(60), (int)rnd(60));
    const int digits = (int)rnd(11);
    if (digits) {
        text[len++] = '.';
        for (int i = 0; i < digits; ++i) text[len++] = (char)('0' + rnd(10));
    }
    static const char* zones[] = {"Z", "z", "+00:00", "-00:00", "+05:30", "-23:59", "+23:59", "+24:00", "", "+00:60"};
    len += snprintf(text + len, sizeof text - len, "%s", zones[rnd(10)]);
    std::string s(text, len);
    if (rnd(5) == 0 && !s.empty()) s[rnd((uint32_t)s.size())] = "/:09TZ+-. \xb0"[rnd(11)];
    if (rnd(9) == 0) s.resize(rnd((uint32_t)s.size() + 1));
    return s;
}

template <bool WORDS>
static bool run(uint32_t chunk, const TcPlan& plan, uint64_t n_fields, const std::vector<uint8_t>& types, const std::vector<sj_u64>& values, uint64_t n_cols,
                uint64_t stride, uint64_t n_rows, const sj_u64* row_count, uint64_t live, const std::vector<uint8_t>& sb, bool with_data, bool with_validity,
                std::vector<sj_u64>& data_out, std::vector<sj_u64>& validity_out, std::vector<TcResult>& results_out) {
    const uint64_t readable = (n_cols - 1) * stride + live, words = (live + 63) / 64;
    uint8_t* t = (uint8_t*)malloc(readable ? readable : 1);
    sj_u64* v = (sj_u64*)malloc(readable ? readable * 8 : 1);
    if (readable) memcpy(t, types.data(), readable), memcpy(v, values.data(), readable * 8);
    const size_t sb_bytes = WORDS ? (sb.size() + 7) / 8 * 8 : sb.size();
    uint8_t* s = (uint8_t*)(WORDS ? aligned_alloc(8, sb_bytes ? sb_bytes : 8) : malloc(sb_bytes ? sb_bytes : 1));
    if (!sb.empty()) memcpy(s, sb.data(), sb.size());
    // (the strides are the least the arguments allow: n_rows -- but the last field's slice ends behind its last LIVE word)
    const uint64_t data_stride = n_rows, validity_stride = (n_rows + 63) / 64;
    const size_t data_words = with_data && live ? (n_fields - 1) * data_stride + live : 0, validity_words = with_validity && live ? (n_fields - 1) * validity_stride + words : 0;
    sj_u64* d = with_data ? (sj_u64*)malloc(data_words ? data_words * 8 : 1) : nullptr;
    sj_u64* b = with_validity ? (sj_u64*)malloc(validity_words ? validity_words * 8 : 1) : nullptr;
    TcResult* res = (TcResult*)malloc(n_fields * sizeof(TcResult));
    const uint64_t nchunks = tc_chunks(n_rows, chunk);
    sj_u64* ws = (sj_u64*)malloc((n_fields * nchunks + 1) * 8);
    const TcCols c = {t, v, stride, n_rows, row_count, s, chunk};
    const TcOut o = {d, with_data ? data_stride : 0, b, validity_stride};
    const bool ok = tc_sim_rows<WORDS>(chunk, plan, c, o, ws, res);
    data_out.assign(n_fields * live, 0);
    validity_out.assign(n_fields * words, 0);
    for (uint64_t f = 0; f < n_fields; ++f) {
        if (with_data && live) memcpy(data_out.data() + f * live, d + f * data_stride, live * 8);
        if (with_validity && live) memcpy(validity_out.data() + f * words, b + f * validity_stride, words * 8);
    }
    results_out.assign(res, res + n_fields);
    free(t), free(v), free(s), free(d), free(b), free(res), free(ws);
    return ok;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 300;
    uint64_t rows_seen = 0, valid_seen = 0, malformed_seen = 0, range_seen = 0;
    for (int k = 0; k < cases; ++k) {
        const uint64_t n_cols = 1 + rnd(4), n_rows = rnd(8) ? rnd(400) : 1000 + rnd(1200), stride = n_rows + rnd(9), n_fields = 1 + rnd(6);
        std::vector<uint8_t> types(n_cols * stride), sb;
        std::vector<sj_u64> values(n_cols * stride);
        for (uint64_t i = 0; i < n_cols * stride; ++i) {
            const uint32_t kind = rnd(10);
            values[i] = ((sj_u64)rnd(1u << 31) << 33) ^ ((sj_u64)rnd(1u << 31) << 2) ^ rnd(4);  // wild
            if (kind < 6) {
                const std::string s = stamp();
                for (uint32_t gap = rnd(10); gap > 0; --gap) sb.push_back((uint8_t)"0123456789:-TZ"[rnd(14)]);
                types[i] = '"', values[i] = ((sj_u64)s.size() << 32) | sb.size();
                sb.insert(sb.end(), s.begin(), s.end());
            } else if (kind == 6) {
                types[i] = '"', values[i] = ((sj_u64)(rnd(2) ? 36 + rnd(1000) : rnd(19)) << 32) | (values[i] & 0xFFFFFFFFull);  // a length the grammar cannot have: not followed
            } else {
                types[i] = (uint8_t)"\0nldtf[{"[rnd(8)];
            }
        }
        TcField fields[6];
        for (uint64_t f = 0; f < n_fields; ++f) fields[f] = {rnd((uint32_t)n_cols), rnd(4), rnd(2), 0};
        TcPlan plan;
        if (tc_plan_compile(fields, n_fields, n_cols, &plan) != 0) return fprintf(stderr, "case %d: the plan does not compile\n", k), 1;
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = k % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        const bool with_data = k % 5 != 0, with_validity = k % 7 != 0;
        std::vector<sj_u64> d0, b0, d, b;
        std::vector<TcResult> r0, r;
        bool first = true;
        for (uint32_t chunk : {64u, 128u, 256u, 1024u})
            for (int words = 0; words < 2; ++words) {
                const bool ok = words ? run<true>(chunk, plan, n_fields, types, values, n_cols, stride, n_rows, row_count, live, sb, with_data, with_validity, d, b, r)
                                      : run<false>(chunk, plan, n_fields, types, values, n_cols, stride, n_rows, row_count, live, sb, with_data, with_validity, d, b, r);
                if (!ok) return fprintf(stderr, "case %d: chunk %u is not one of the simulation's\n", k, chunk), 1;
                if (first) {
                    d0 = d, b0 = b, r0 = r, first = false;
                } else if (d != d0 || b != b0 || memcmp(r.data(), r0.data(), n_fields * sizeof(TcResult)) != 0) {
                    return fprintf(stderr, "case %d: chunk %u, words %d differs from the first run\n", k, chunk, words), 1;
                }
            }
        for (uint64_t f = 0; f < n_fields; ++f) rows_seen += r0[f].n_rows, valid_seen += r0[f].n_valid, malformed_seen += r0[f].n_malformed, range_seen += r0[f].n_range;
    }
    printf("%d cases, 8 runs each: %llu field rows, %llu VALID, %llu malformed, %llu out of range; all runs agree\n", cases, (unsigned long long)rows_seen,
           (unsigned long long)valid_seen, (unsigned long long)malformed_seen, (unsigned long long)range_seen);
    return valid_seen && malformed_seen && range_seen ? 0 : 1;
}
