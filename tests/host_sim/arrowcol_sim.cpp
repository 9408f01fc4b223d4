// Host simulation of the Arrow column export (simdjson-java_amd/csrc/arrowcol.hip): sj_arrowcol.h, the header the kernels compile
// verbatim, with the lane primitives in their sequential form (seq_group.h) -- ONE wave per chunk whose 64 lanes run one after the
// other (a ballot collects their answers, every scan is empty and every total the wave's own value).
// TEST ONLY: lets the CPU suite check the two passes against the reference of tests/arrowcol_common.py without a GPU, at any
// chunk size.  The type block, the value block and both output blocks each END at a page that cannot be touched: a read of a row
// at or above the live rows at the end of the last column, or a write past the last field's slice, is a SIGSEGV here and not a
// fault on a GPU.  Built by tests/test_host_arrowcol.py with g++.
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_arrowcol.h"
#include "seq_group.h"

extern "C" {

uint32_t sim_arrowcol_chunk_rows() { return AC_CHUNK_ROWS; }

// n_fields fields (sjmi_arrow_field); n_cols columns types (any alignment) / values strided by col_stride, of which
// cells_readable = (n_cols - 1) * col_stride + live cells are copied in front of a guard page -- the cells behind the last
// column's live rows do not exist here; row_count: NULL, or where the live rows are counted; chunk_rows a multiple of 64.
// data: data_words words or NULL (with data_stride 0: the counting call), validity: validity_words words or NULL -- what the
// caller gives is copied against a guard page and copied back, so whatever canaries it holds are the caller's.  results:
// 4 * n_fields words.  -> 0, -2 for a bad argument, -3 without memory, -4 when a byte in front of an output block was written
int sim_arrowcol(const void* fields, uint64_t n_fields, const uint8_t* types, const uint64_t* values, uint64_t n_cols, uint64_t col_stride,
                 uint64_t n_rows, uint64_t cells_readable, const uint64_t* row_count, uint32_t chunk_rows, uint64_t* data, uint64_t data_stride,
                 uint64_t data_words, uint64_t* validity, uint64_t validity_stride, uint64_t validity_words, uint64_t* results) {
    if (!chunk_rows || chunk_rows % 64 || !results || col_stride < n_rows || (n_rows && (!types || !values))) return -2;
    if (data ? data_stride < n_rows : data_stride != 0) return -2;
    if (validity && validity_stride < (n_rows + 63) / 64) return -2;
    AcPlan plan;
    if (ac_plan_compile((const AcField*)fields, n_fields, n_cols, &plan) != 0) return -2;
    if (cells_readable > n_cols * col_stride) return -2;
    Guarded gt, gv, gd, gb;
    if (!gt.open(cells_readable + 1) || !gv.open(cells_readable * 8 + 8) || !gd.open(data_words * 8 + 8) || !gb.open(validity_words * 8 + 8)) return -3;
    const AcCols c = {gt.place(types, cells_readable), (const sj_u64*)gv.place(values, cells_readable * 8), col_stride, n_rows, (const sj_u64*)row_count,
                      chunk_rows};
    const AcOut o = {data ? (sj_u64*)gd.place(data, data_words * 8) : nullptr, data_stride,
                     validity ? (sj_u64*)gb.place(validity, validity_words * 8) : nullptr, validity_stride};
    const sj_u64 nchunks = ac_chunks(n_rows, chunk_rows);
    std::vector<sj_u64> ws(n_fields * nchunks + 1, 0xA5A5A5A5A5A5A5A5ull);  // (the scratch is not zero on the device either)
    const SeqGroup g;
    for (uint32_t f = 0; f < plan.n_fields; ++f)
        for (sj_u64 k = 0; k < nchunks; ++k) ac_convert_chunk(g, plan, c, k, f, o, ws.data());
    for (uint32_t f = 0; f < plan.n_fields; ++f) ac_finish(g, c, f, ws.data(), (AcResult*)results);
    if (data) memcpy(data, o.data, data_words * 8);
    if (validity) memcpy(validity, o.validity, validity_words * 8);
    for (int i = 1; i <= 64; ++i)  // (place() filled what lies in front of a block with 0xA5)
        if ((data && ((const uint8_t*)o.data)[-i] != 0xA5) || (validity && ((const uint8_t*)o.validity)[-i] != 0xA5)) return -4;
    return 0;
}

}  // extern "C"
