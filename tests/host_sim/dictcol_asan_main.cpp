// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o dictcol_asan tests/host_sim/dictcol_asan_main.cpp && ./dictcol_asan [cases]
// Random adversarial columns through sj_dictcol.h / sj_strcol.h with the sequential group, at chunks of 64, 128 and 1024 rows, the
// chunks in three orders, with and without stale table loads.  Every block is a heap allocation of EXACTLY its size -- the type
// and value blocks end behind the last LIVE row, the indices behind the last live row, the dictionary's arrays behind entry
// n_distinct, the bytes behind the capacity, the scratch behind its last word -- so one byte too far is a report.  The string
// buffer begins 8-byte aligned and is rounded up to whole words, which is what the aligned-word fetch asks of its memory (a
// word never leaves the page of the byte it is read for; a heap block is not a page).  Every run of a case is compared with a
// std::map reference: first-occurrence order, indices, offsets, bytes, the record.  TEST ONLY.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

#include "dictcol_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}

struct Want {
    std::vector<int32_t> indices;
    std::vector<sj_u64> rows, offsets;
    std::string bytes;
    sj_u64 n_valid = 0, n_other = 0;
};

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 300;
    unsigned long long rows_seen = 0, distinct_seen = 0, overflows = 0, runs = 0;
    for (int k = 0; k < cases; ++k) {
        const uint64_t n_rows = rnd(8) ? rnd(300) : 1000 + rnd(1500);
        const uint32_t vocabulary = 1 + rnd(rnd(3) ? 6 : 200), max_len = rnd(4) ? 1 + rnd(12) : 40;
        std::vector<std::string> words(vocabulary);
        for (auto& w : words) {
            w.resize(rnd(max_len + 1));
            for (auto& ch : w) ch = (char)('a' + rnd(3));  // (few letters: many values share long prefixes, some are prefixes of others)
        }
        std::vector<uint8_t> types(n_rows), sb;
        std::vector<sj_u64> values(n_rows);
        for (uint64_t r = 0; r < n_rows; ++r) {
            values[r] = ((sj_u64)rnd(1u << 31) << 33) ^ ((sj_u64)rnd(1u << 31) << 2) ^ rnd(4);  // wild
            if (rnd(10) < 7) {
                const std::string& w = words[rnd(vocabulary)];
                for (uint32_t gap = rnd(6); gap > 0; --gap) sb.push_back((uint8_t)('a' + rnd(3)));
                types[r] = '"', values[r] = ((sj_u64)w.size() << 32) | sb.size();
                sb.insert(sb.end(), w.begin(), w.end());
            } else {
                types[r] = (uint8_t)"\0nldtf[{"[rnd(8)];
            }
        }
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = k % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        static const uint64_t capacities[] = {0, 1, 2, 5, 32, 300};
        const uint64_t dict_capacity = capacities[rnd(6)];
        // the reference
        Want want;
        std::map<std::string, int32_t> seen;
        want.indices.assign(live, 0);
        want.offsets.push_back(0);
        for (uint64_t r = 0; r < live; ++r) {
            if (types[r] != '"') {
                want.n_other += types[r] != 0 && types[r] != 'n';
                continue;
            }
            ++want.n_valid;
            const std::string s((const char*)sb.data() + (uint32_t)values[r], values[r] >> 32);
            auto it = seen.find(s);
            if (it == seen.end()) {
                it = seen.emplace(s, (int32_t)seen.size()).first;
                want.rows.push_back(r);
                want.bytes += s;
                want.offsets.push_back(want.bytes.size());
            }
            want.indices[r] = it->second;
        }
        const uint64_t nd = seen.size();
        const bool overflow = nd > dict_capacity;
        const uint64_t byte_capacity = rnd(3) == 0 ? 0 : rnd(2) ? want.bytes.size() : rnd((uint32_t)want.bytes.size() + 9);
        const bool with_validity = k % 7 != 0, with_rows = k % 5 != 0;
        for (uint32_t chunk : {64u, 128u, 1024u})
            for (uint32_t order = 0; order < 3; ++order)
                for (int stale = 0; stale < 2; ++stale) {
                    uint8_t* t = (uint8_t*)malloc(live ? live : 1);
                    sj_u64* v = (sj_u64*)malloc(live ? live * 8 : 1);
                    if (live) memcpy(t, types.data(), live), memcpy(v, values.data(), live * 8);
                    const size_t sb_bytes = (sb.size() + 7) / 8 * 8;
                    uint8_t* s = (uint8_t*)aligned_alloc(8, sb_bytes ? sb_bytes : 8);
                    if (!sb.empty()) memcpy(s, sb.data(), sb.size());
                    const uint64_t words_live = (live + 63) / 64;
                    // (under OVERFLOW the dictionary's arrays are unspecified inside their stated extents)
                    const uint64_t dict_entries = overflow ? dict_capacity : nd;
                    int32_t* indices = (int32_t*)malloc(live ? live * 4 : 1);
                    sj_u64* validity = with_validity ? (sj_u64*)malloc(words_live ? words_live * 8 : 1) : nullptr;
                    sj_u64* dict_rows = with_rows ? (sj_u64*)malloc(dict_entries ? dict_entries * 8 : 1) : nullptr;
                    sj_u64* dict_offsets = (sj_u64*)malloc(((overflow ? 0 : nd) + 1) * 8);
                    uint8_t* dict_bytes = byte_capacity ? (uint8_t*)malloc(byte_capacity) : nullptr;
                    sj_u64* ws = (sj_u64*)malloc(dc_scratch_words(n_rows, dict_capacity, chunk) * 8);
                    DcResult res;
                    const DcColumn c = {t, v, n_rows, row_count, s, chunk};
                    dc_sim_passes(c, order, stale != 0, indices, validity, dict_capacity, dict_rows, dict_offsets, dict_bytes, byte_capacity, &res, ws);
                    ++runs;
                    bool ok = res.n_rows == live && res.n_valid == want.n_valid && res.n_other == want.n_other && ((res.flags & DC_OVERFLOW) != 0) == overflow;
                    if (ok && overflow) ok = res.n_distinct > dict_capacity;
                    if (ok && !overflow) {
                        const uint64_t below = want.bytes.size() < byte_capacity ? want.bytes.size() : byte_capacity;
                        ok = res.n_distinct == nd && res.dict_bytes == want.bytes.size() &&
                             ((res.flags & DC_BYTES_OVERFLOW) != 0) == (want.bytes.size() > byte_capacity) &&
                             (!live || memcmp(indices, want.indices.data(), live * 4) == 0) && memcmp(dict_offsets, want.offsets.data(), (nd + 1) * 8) == 0 &&
                             (!with_rows || !nd || memcmp(dict_rows, want.rows.data(), nd * 8) == 0) && (!below || memcmp(dict_bytes, want.bytes.data(), below) == 0);
                    }
                    if (ok && with_validity)
                        for (uint64_t r = 0; r < live && ok; ++r) ok = ((validity[r >> 6] >> (r & 63)) & 1) == (types[r] == '"');
                    free(t), free(v), free(s), free(indices), free(validity), free(dict_rows), free(dict_offsets), free(dict_bytes), free(ws);
                    if (!ok) return fprintf(stderr, "case %d: chunk %u, order %u, stale %d differs from the reference\n", k, chunk, order, stale), 1;
                }
        rows_seen += live, distinct_seen += nd, overflows += overflow;
    }
    printf("%d cases, %llu runs: %llu live rows, %llu distinct values, %llu overflowing cases; all runs agree with the reference\n", cases, runs, rows_seen,
           distinct_seen, overflows);
    return distinct_seen && overflows ? 0 : 1;
}
