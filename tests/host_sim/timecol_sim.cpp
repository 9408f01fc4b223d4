// Host simulation of the timestamp column export (simdjson-java_amd/csrc/timecol.hip): sj_timecol.h, the header the kernels compile
// verbatim, with the lane primitives in their sequential form (seq_group.h, seq_ballots.h) -- ONE wave per chunk whose 64 lanes
// run one after the other, each on chunk_rows / 64 rows at once.
// TEST ONLY: lets the CPU suite check the two passes against the reference of tests/timecol_common.py without a GPU, with both
// forms of the byte fetch.  The type block, the value block, the string buffer and both output blocks each END at a page that
// cannot be touched, the type and value blocks right behind the last column's last LIVE row: a read of a row at or above the live
// rows, of a byte behind the buffer's last string, or a write past the last field's slice, is a SIGSEGV here and not a fault on a
// GPU.  The passes run a SECOND time with the string buffer BEGINNING on a page boundary behind a page that cannot be touched
// (its first string is at offset 0), and both runs must give the same.  Built by tests/test_host_timecol.py with g++; the
// stand-alone sanitizer run of tests/host_sim/timecol_asan_main.cpp includes this file.
#include "../../simdjson-java_amd/csrc/sj_timecol.h"
#include "fieldcol_sim.h"
#include "seq_ballots.h"

// the other edge: memory that BEGINS where a PROT_NONE page ends
struct GuardedFront {
    uint8_t* map = nullptr;
    size_t bytes = 0, page = 0;
    bool open(size_t need) {
        page = (size_t)sysconf(_SC_PAGESIZE);
        bytes = (need + page - 1) / page * page + page;
        void* m = mmap(nullptr, bytes + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return false;
        map = (uint8_t*)m;
        return mprotect(map, page, PROT_NONE) == 0;
    }
    uint8_t* place(const void* src, size_t n) {  // -> the copy, beginning behind the guard page
        memset(map + page, 0xA5, bytes);
        if (n) memcpy(map + page, src, n);
        return map + page;
    }
    ~GuardedFront() {
        if (map) munmap(map, bytes + page);
    }
};

template <bool WORDS, uint32_t ROWS>
static void tc_sim_run(const TcPlan& plan, const TcCols& c, const TcOut& o, sj_u64* ws, TcResult* results) {
    fc_sim_run(plan, c, o, ws, results, tc_parse_chunk<WORDS, ROWS, SeqGroup>, tc_finish<SeqGroup>);
}
template <bool WORDS>
static bool tc_sim_rows(uint32_t chunk_rows, const TcPlan& plan, const TcCols& c, const TcOut& o, sj_u64* ws, TcResult* results) {
    switch (chunk_rows) {  // (a chunk is what the group takes in one go: 64 rows per row of a lane)
        case 64: tc_sim_run<WORDS, 1>(plan, c, o, ws, results); return true;
        case 128: tc_sim_run<WORDS, 2>(plan, c, o, ws, results); return true;
        case 256: tc_sim_run<WORDS, 4>(plan, c, o, ws, results); return true;
        case 1024: tc_sim_run<WORDS, 16>(plan, c, o, ws, results); return true;
    }
    return false;
}
static_assert(TC_CHUNK_ROWS == 64 || TC_CHUNK_ROWS == 128 || TC_CHUNK_ROWS == 256 || TC_CHUNK_ROWS == 1024, "the kernels' chunk is one this simulation has");

extern "C" {

uint32_t sim_timecol_chunk_rows() { return TC_CHUNK_ROWS; }

// n_fields fields (sjmi_time_field); n_cols columns types (any alignment) / values strided by col_stride, of which
// cells_readable = (n_cols - 1) * col_stride + live cells are copied in front of a guard page; row_count: NULL, or where the live
// rows are counted; sb: the string buffer of sb_bytes; chunk_rows: 64, 128, 256 or 1024 (the kernels' own is one of them); words != 0: the aligned-word
// fetch, else the byte-wide one.  data: data_words words or NULL (with data_stride 0: the counting call), validity:
// validity_words words or NULL -- what the caller gives is copied against a guard page and copied back, so whatever canaries it
// holds are the caller's.  results: 6 * n_fields words.  -> 0, -2 for a bad argument, -3 without memory, -4 when a byte in front
// of an output block was written, -5 when the run with the string buffer at the other edge gave something else
int sim_timecol(const void* fields, uint64_t n_fields, const uint8_t* types, const uint64_t* values, uint64_t n_cols, uint64_t col_stride,
                uint64_t n_rows, uint64_t cells_readable, const uint64_t* row_count, const uint8_t* sb, uint64_t sb_bytes, uint32_t chunk_rows,
                int words, uint64_t* data, uint64_t data_stride, uint64_t data_words, uint64_t* validity, uint64_t validity_stride,
                uint64_t validity_words, uint64_t* results) {
    if (!fc_sim_args(types, values, n_cols, col_stride, n_rows, cells_readable, chunk_rows, data, data_stride, validity, validity_stride, results)) return -2;
    if (n_rows && !sb) return -2;
    TcPlan plan;
    if (tc_plan_compile((const TcField*)fields, n_fields, n_cols, &plan) != 0) return -2;
    FcSimCols in;
    FcSimOut out, out2;
    Guarded gs;
    GuardedFront gs2;
    if (!in.open(cells_readable) || !gs.open(sb_bytes + 1) || !gs2.open(sb_bytes + 1) || !out.open(data_words, validity_words) || !out2.open(data_words, validity_words))
        return -3;
    TcCols c = {in.place(types, values, cells_readable, col_stride, n_rows, row_count), gs.place(sb, sb_bytes), chunk_rows};
    out.place(data, data_stride, validity, validity_stride);
    out2.place(data, data_stride, validity, validity_stride);
    std::vector<sj_u64> ws(n_fields * tc_chunks(n_rows, chunk_rows) + 1, 0xA5A5A5A5A5A5A5A5ull);  // (the scratch is not zero on the device either)
    std::vector<TcResult> again(n_fields);
    if (!(words ? tc_sim_rows<true>(chunk_rows, plan, c, out.o, ws.data(), (TcResult*)results) : tc_sim_rows<false>(chunk_rows, plan, c, out.o, ws.data(), (TcResult*)results)))
        return -2;
    c.strings = gs2.place(sb, sb_bytes);
    ws.assign(ws.size(), 0x5A5A5A5A5A5A5A5Aull);
    (void)(words ? tc_sim_rows<true>(chunk_rows, plan, c, out2.o, ws.data(), again.data()) : tc_sim_rows<false>(chunk_rows, plan, c, out2.o, ws.data(), again.data()));
    if (memcmp(again.data(), results, n_fields * sizeof(TcResult)) != 0) return -5;
    if ((data && memcmp(out.o.data, out2.o.data, data_words * 8) != 0) || (validity && memcmp(out.o.validity, out2.o.validity, validity_words * 8) != 0)) return -5;
    return out.copy_back(data, validity) ? 0 : -4;
}

}  // extern "C"
