// Host simulation of the string-column gather (simdjson-java_amd/csrc/strcol.hip): sj_strcol.h, the header the kernels compile
// verbatim, with the lane primitives in their sequential form (seq_group.h) -- ONE lane for the three scan passes (every scan is empty, every
// total the lane's own value, a validity bit is set on its own), and for the copy a wave whose 64 lanes run one after the other.
// TEST ONLY: lets the CPU suite check the four passes against the reference of tests/strcol_common.py without a GPU, at any
// chunk size.  The string buffer is placed so that it ENDS at a page that cannot be read: one dereference of a NULL row's value
// word, or one byte read behind a string that ends the buffer, is a SIGSEGV here and not a fault on a GPU.
// Built by tests/test_host_strcol.py with g++.
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_strcol.h"
#include "seq_group.h"

extern "C" {

uint32_t sim_strcol_chunk_rows() { return SC_CHUNK_ROWS; }

// One column: types (any alignment) / values of n_rows cells, the string buffer sb[0, sb_len) (copied against a guard page),
// chunk_rows a multiple of 64.  offsets: n_rows + 1 entries, validity: (n_rows + 63) / 64 words or NULL, bytes: byte_capacity
// bytes (NULL with 0: the sizing call) -- each with whatever canaries the caller put behind it.  result = {total_bytes, n_valid,
// n_other, flags}.  -> 0, -2 for a bad argument, -3 without memory
int sim_strcol(const uint8_t* types, const uint64_t* values, uint64_t n_rows, const uint8_t* sb, uint64_t sb_len, uint32_t chunk_rows,
               uint64_t* offsets, uint64_t* validity, uint8_t* bytes, uint64_t byte_capacity, uint64_t* result) {
    if (!chunk_rows || chunk_rows % 64 || !offsets || !result || (byte_capacity && !bytes)) return -2;
    Guarded gs;
    if (!gs.open(sb_len ? sb_len : 1)) return -3;
    const uint8_t* dsb = gs.place(sb, sb_len);
    const ScColumn c = {types, (const sj_u64*)values, n_rows, chunk_rows};
    const sj_u64 nchunks = sc_chunks(c);
    std::vector<sj_u64> ws(3 * nchunks + 1, 0xA5A5A5A5A5A5A5A5ull);
    const ScSums sums = sc_sums(ws.data(), nchunks);
    const SeqGroup g;
    for (sj_u64 k = 0; k < nchunks; ++k) sc_chunk_sums(g, c, k, (sj_u64*)validity, sums);
    ScResult res;
    sc_chunk_scan(g, sums, nchunks, n_rows, (sj_u64*)offsets, byte_capacity, &res);
    for (sj_u64 k = 0; k < nchunks; ++k) sc_offsets(g, c, k, sums, (sj_u64*)offsets);
    if (nchunks && byte_capacity) {
        const SeqWave w;
        ScWave* s = new ScWave;
        for (sj_u64 wave = 0; wave < (n_rows + 63) / 64; ++wave) {
            memset(s, 0xA5, sizeof *s);  // (LDS is not zero on the device either)
            sc_copy_wave(w, c, wave, (const sj_u64*)offsets, dsb, bytes, byte_capacity, *s);
        }
        delete s;
    }
    result[0] = res.total_bytes;
    result[1] = res.n_valid;
    result[2] = res.n_other;
    result[3] = ((uint64_t)res.reserved << 32) | res.flags;
    return 0;
}

}  // extern "C"
