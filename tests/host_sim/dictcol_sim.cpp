// Host simulation of the dictionary encoder (simdjson-java_amd/csrc/dictcol.hip): sj_dictcol.h and, for the dictionary's offsets
// and bytes, sj_strcol.h -- the headers the kernels compile verbatim -- with the lane primitives in their sequential form
// (seq_group.h) and the three table operations added to that group HERE, as dictcol.hip adds the atomic ones to WgGroup.
// TEST ONLY: lets the CPU suite check every pass against the reference of tests/dictcol_common.py without a GPU, at any chunk
// size.  Two things stand in for the schedules a GPU has and a loop has not:
//   order  the chunks of every per-chunk pass run ascending (0), descending (1) or the odd ones first (2): which row owns a
//          slot then differs, and the output must not
//   stale  every other load of a table word answers "all ones" -- the oldest value the word ever held, which a load on a GPU may
//          legally return: the cas / fetch_min behind it must still decide rightly
// The string buffer is placed so that it ENDS at a page that cannot be read: one dereference of a NULL row's value word, or one
// aligned word behind the last that holds a byte of a string, is a SIGSEGV here and not a fault on a GPU.
// Built by tests/test_host_dictcol.py with g++.
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_dictcol.h"
#include "seq_group.h"

// SeqGroup with load / cas / fetch_min on a 64-bit word, one after the other
struct SeqDcGroup : SeqGroup {
    bool stale = false;
    mutable uint64_t tick = 0;
    sj_u64 load(const sj_u64* p) const { return stale && (++tick & 1) ? DC_EMPTY : *p; }
    sj_u64 cas(sj_u64* p, sj_u64 expected, sj_u64 desired) const {
        const sj_u64 old = *p;
        if (old == expected) *p = desired;
        return old;
    }
    sj_u64 fetch_min(sj_u64* p, sj_u64 v) const {
        const sj_u64 old = *p;
        if (v < old) *p = v;
        return old;
    }
};

// the chunks [0, n) in the order `order`
static std::vector<sj_u64> dc_sim_order(sj_u64 n, uint32_t order) {
    std::vector<sj_u64> ks;
    if (order == 2) {
        for (sj_u64 k = 1; k < n; k += 2) ks.push_back(k);
        for (sj_u64 k = 0; k < n; k += 2) ks.push_back(k);
    } else {
        for (sj_u64 k = 0; k < n; ++k) ks.push_back(order == 1 ? n - 1 - k : k);
    }
    return ks;
}

// every pass of dictcol_launch, in its order, over memory as it is (the callers place it).  ws: dc_scratch_words() words
static void dc_sim_passes(const DcColumn& c, uint32_t order, bool stale, int32_t* indices, sj_u64* validity, sj_u64 dict_capacity, sj_u64* dict_rows,
                          sj_u64* dict_offsets, uint8_t* dict_bytes, sj_u64 byte_capacity, DcResult* res, void* ws) {
    const DcScratch s = dc_scratch(ws, c.n_rows, dict_capacity, c.chunk_rows);
    SeqDcGroup g;
    g.stale = stale;
    const SeqGroup plain;
    const std::vector<sj_u64> ks = dc_sim_order(dc_chunks(c.n_rows, c.chunk_rows), order);
    const sj_u64 dchunks = dc_chunks(dict_capacity, SC_CHUNK_ROWS);
    const ScSums sums = sc_sums(s.sums, dchunks);
    if (c.n_rows) {
        for (sj_u64 i = 2 * s.table.slots; i-- > 0;) dc_clear_word(s.table, i);
        for (sj_u64 k : ks) dc_insert_chunk(g, c, s.table, k, validity, s.slot_of_row, s.counts);
        for (sj_u64 k : ks) dc_count_chunk(g, c, s.table, k, s.slot_of_row, s.firsts);
    }
    dc_scan(g, c, s.counts, s.firsts, dict_capacity, s.dict_n, res);
    if (c.n_rows) {
        for (sj_u64 k : ks) dc_emit_chunk(g, c, s.table, k, s.slot_of_row, s.firsts, dict_capacity, dict_rows, s.ctypes, s.cvalues);
        for (sj_u64 k : ks) dc_index_chunk(g, c, s.table, k, s.slot_of_row, indices);
    }
    if (c.n_rows)
        for (sj_u64 k = dchunks; k-- > 0;) sc_chunk_sums(plain, dc_dict_column(s.ctypes, s.cvalues, s.dict_n), k, nullptr, sums);
    dc_dict_scan(plain, sums, c.n_rows ? dchunks : 0, *s.dict_n, dict_offsets, byte_capacity, res);
    if (c.n_rows && dchunks) {
        const ScColumn d = dc_dict_column(s.ctypes, s.cvalues, s.dict_n);
        for (sj_u64 k = dchunks; k-- > 0;) sc_offsets(plain, d, k, sums, dict_offsets);
        if (byte_capacity) {
            const SeqWave w;
            ScWave* lds = new ScWave;
            for (sj_u64 wave = 0; wave < (d.n_rows + 63) / 64; ++wave) {
                memset(lds, 0xA5, sizeof *lds);  // (LDS is not zero on the device either)
                sc_copy_wave(w, d, wave, dict_offsets, c.sb, dict_bytes, byte_capacity, *lds);
            }
            delete lds;
        }
    }
}

extern "C" {

uint32_t sim_dictcol_chunk_rows() { return DC_CHUNK_ROWS; }

// dc_hash of s[0, len), the string placed so that `tail` bytes lie between its end and the unreadable page
uint64_t sim_dc_hash(const uint8_t* s, uint64_t len, uint64_t tail) {
    Guarded g;
    if (!g.open(len + tail + 1)) return 0;
    std::vector<uint8_t> copy(len + tail, 0x5A);
    if (len) memcpy(copy.data(), s, len);
    return dc_hash(g.place(copy.data(), copy.size()), len);
}

// One column: types (any alignment) / values of n_rows cells, row_count NULL or where the live rows are counted, the string
// buffer sb[0, sb_len) (copied against a guard page), chunk_rows a multiple of 64.  indices: n_rows int32; validity: (n_rows + 63)
// / 64 words or NULL; dict_rows: dict_capacity words or NULL; dict_offsets: dict_capacity + 1 words; dict_bytes: byte_capacity
// bytes (NULL with 0: the sizing call) -- each with whatever canaries the caller put around it.  result: the six words of
// sjmi_dict_result.  -> 0, -2 for a bad argument, -3 without memory
int sim_dictcol(const uint8_t* types, const uint64_t* values, uint64_t n_rows, const uint64_t* row_count, const uint8_t* sb, uint64_t sb_len,
                uint32_t chunk_rows, uint32_t order, uint32_t stale, int32_t* indices, uint64_t* validity, uint64_t dict_capacity, uint64_t* dict_rows,
                uint64_t* dict_offsets, uint8_t* dict_bytes, uint64_t byte_capacity, uint64_t* result) {
    if (!chunk_rows || chunk_rows % 64 || order > 2 || !indices || !dict_offsets || !result || (byte_capacity && !dict_bytes) ||
        dict_capacity > DC_MAX_ENTRIES)
        return -2;
    Guarded gs;
    if (!gs.open(sb_len ? sb_len : 1)) return -3;
    const DcColumn c = {types, (const sj_u64*)values, n_rows, (const sj_u64*)row_count, gs.place(sb, sb_len), chunk_rows};
    std::vector<sj_u64> ws(dc_scratch_words(n_rows, dict_capacity, chunk_rows), 0xA5A5A5A5A5A5A5A5ull);
    DcResult res;
    memset(&res, 0xA5, sizeof res);
    dc_sim_passes(c, order, stale != 0, indices, (sj_u64*)validity, dict_capacity, (sj_u64*)dict_rows, (sj_u64*)dict_offsets, dict_bytes, byte_capacity,
                  &res, ws.data());
    memcpy(result, &res, sizeof res);
    return 0;
}

}  // extern "C"
