// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o parents_asan tests/host_sim/parents_asan_main.cpp && ./parents_asan [cases]
// Random shapes through sj_parents.h with the sequential group: document counts around the search's fan-out of 64, rows per
// document from none to several chunks, runs of documents without rows, row counts around the wave and chunk edges and above the
// total (dense orphans), a device row count, the sparse form in any order with duplicates and indices at and far above the total,
// 0 to 64 carried columns with strides wider than they must be, each output left out in turn, the chunks in three orders.  Every
// block is a heap allocation of EXACTLY its size -- the offsets end behind entry n_docs, a column set behind the last cell of its
// last column that a document (a live slot) can address, the parents behind the last LIVE slot; the marks and seeds are such
// blocks inside parents_sim.cpp -- so one byte too far is a report.  Every run is compared with a plain loop over the documents.
// TEST ONLY.
#include <cstdio>
#include <cstdlib>

#include "parents_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}
static uint64_t rnd64() { return ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 11) ^ rnd(1u << 31); }

template <class T>
static T* exact(const std::vector<T>& v, size_t n) {  // a block of exactly n entries with v's first n
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, v.data(), n * sizeof(T));
    return p;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    static const uint64_t doc_counts[] = {0, 1, 2, 63, 64, 65, 200, 4095, 4097, 9000};
    static const uint64_t extra_rows[] = {0, 0, 1, 63, 64, 65, 1025};
    unsigned long long runs = 0, slots_seen = 0, orphans_seen = 0, cells_seen = 0, empty_seen = 0;
    for (int i = 0; i < cases; ++i) {
        const uint64_t n_docs = doc_counts[i % 10];
        const uint32_t shape = rnd(4);  // 0: small documents, 1: mostly none, 2: one huge, 3: runs without rows
        std::vector<sj_u64> off(n_docs + 1, 0);
        for (uint64_t k = 0; k < n_docs; ++k) {
            uint64_t c = shape == 0 ? rnd(6) : shape == 1 ? (rnd(10) ? 0 : 1 + rnd(40)) : shape == 2 ? (k == n_docs / 2 ? 2500 + rnd(900) : rnd(3))
                                                                                                 : ((k / 700) % 2 ? 0 : rnd(4));
            empty_seen += c == 0;
            off[k + 1] = off[k] + c;
        }
        const uint64_t total = off[n_docs];
        const bool sparse = i % 3 == 2;
        const uint64_t n_rows = sparse ? rnd(2600) : total + extra_rows[i % 7] - (i % 5 == 4 && total > 70 ? 70 : 0);
        std::vector<sj_u64> rows(n_rows);
        for (uint64_t j = 0; j < n_rows; ++j)
            rows[j] = rnd(8) == 0 ? total + (rnd(2) ? 0 : rnd(3) ? rnd(1000) : 1ull << 40) : total ? rnd64() % total : rnd(5);
        sj_u64 rc = rnd((uint32_t)n_rows + 5);
        const sj_u64* row_count = i % 2 ? &rc : nullptr;
        const uint64_t live = row_count && rc < n_rows ? rc : n_rows;
        const uint64_t n_cols = i % 4 == 3 ? 0 : i % 11 == 5 ? 64 : 1 + i % 6, col_stride = n_docs + rnd(3), out_stride = n_rows + rnd(3);
        const bool with_parents = i % 7 != 6, with_types = i % 5 != 3;
        std::vector<uint8_t> types(n_cols * col_stride);
        std::vector<sj_u64> values(n_cols * col_stride);
        for (size_t j = 0; j < types.size(); ++j) types[j] = (uint8_t)(1 + rnd(255)), values[j] = rnd64() | 1;
        // the reference: a plain loop over the documents' rows gives every row below the total its owner
        std::vector<sj_u64> owner(total), want(live);
        for (uint64_t k = 0; k < n_docs; ++k)
            for (uint64_t x = off[k]; x < off[k + 1]; ++x) owner[x] = k;
        uint64_t n_orphans = 0;
        for (uint64_t s = 0; s < live; ++s) {
            const uint64_t x = sparse ? rows[s] : s;
            want[s] = x < total ? owner[x] : PA_ORPHAN;
            n_orphans += want[s] == PA_ORPHAN;
        }
        const size_t in_cells = pa_extent(n_cols, col_stride, n_docs), out_cells = pa_extent(n_cols, out_stride, live);
        for (uint32_t chunk : {64u, 128u, 1024u})
            for (uint32_t order = 0; order < 3; ++order) {
                sj_u64* o = exact(off, n_docs + 1);
                sj_u64* r = sparse ? exact(rows, live) : nullptr;
                uint8_t* t = exact(types, in_cells);
                sj_u64* v = exact(values, in_cells);
                uint8_t* pt = with_types ? (uint8_t*)malloc(live ? live : 1) : nullptr;
                sj_u64* pp = with_parents ? (sj_u64*)malloc(live ? live * 8 : 1) : nullptr;
                uint8_t* ot = (uint8_t*)malloc(out_cells ? out_cells : 1);
                sj_u64* ov = (sj_u64*)malloc(out_cells ? out_cells * 8 : 1);
                memset(ot, 0xEE, out_cells), memset(ov, 0xEE, out_cells * 8);
                PaResult* res = (PaResult*)malloc(sizeof(PaResult));
                memset(res, 0xEE, sizeof *res);
                const PaArgs a = {o, n_docs, r, n_rows, row_count, t, v, n_cols, col_stride, pt, pp, ot, ov, out_stride, chunk};
                pa_sim_passes(a, order, res);
                ++runs;
                bool ok = res->n_rows == live && res->n_orphans == n_orphans && res->flags == 0 && res->reserved == 0;
                for (uint64_t s = 0; ok && s < live; ++s) {
                    const bool orphan = want[s] == PA_ORPHAN;
                    ok = (!pp || pp[s] == want[s]) && (!pt || pt[s] == (orphan ? 0 : 'l'));
                    for (uint64_t c = 0; ok && c < n_cols; ++c)
                        ok = ot[c * out_stride + s] == (orphan ? 0 : types[c * col_stride + want[s]]) &&
                             ov[c * out_stride + s] == (orphan ? 0 : values[c * col_stride + want[s]]);
                }
                // (between the columns, behind the live slots: untouched)
                for (uint64_t c = 0; ok && c + 1 < n_cols; ++c)
                    for (uint64_t s = live; ok && s < out_stride; ++s) ok = ot[c * out_stride + s] == 0xEE && ov[c * out_stride + s] == 0xEEEEEEEEEEEEEEEEull;
                free(o), free(r), free(t), free(v), free(pt), free(pp), free(ot), free(ov), free(res);
                if (!ok) return fprintf(stderr, "case %d: chunk %u, order %u differs from the reference\n", i, chunk, order), 1;
            }
        slots_seen += live, orphans_seen += n_orphans, cells_seen += live * n_cols;
    }
    printf("%d cases, %llu runs: %llu live slots, %llu orphans, %llu carried cells, %llu documents without rows; all runs agree with the reference\n",
           cases, runs, slots_seen, orphans_seen, cells_seen, empty_seen);
    return slots_seen && orphans_seen && cells_seen && empty_seen ? 0 : 1;
}
