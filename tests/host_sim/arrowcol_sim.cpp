// Host simulation of the Arrow column export (simdjson-java_amd/csrc/arrowcol.hip): sj_arrowcol.h, the header the kernels compile
// verbatim, in the frame of fieldcol_sim.h (the sequential group, the guard pages).
// TEST ONLY: lets the CPU suite check the two passes against the reference of tests/arrowcol_common.py without a GPU, at any
// chunk size.  Built by tests/test_host_arrowcol.py with g++.
#include "../../simdjson-java_amd/csrc/sj_arrowcol.h"
#include "fieldcol_sim.h"

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
    if (!fc_sim_args(types, values, n_cols, col_stride, n_rows, cells_readable, chunk_rows, data, data_stride, validity, validity_stride, results)) return -2;
    AcPlan plan;
    if (ac_plan_compile((const AcField*)fields, n_fields, n_cols, &plan) != 0) return -2;
    FcSimCols in;
    FcSimOut out;
    if (!in.open(cells_readable) || !out.open(data_words, validity_words)) return -3;
    const AcCols c = {in.place(types, values, cells_readable, col_stride, n_rows, row_count), chunk_rows};
    out.place(data, data_stride, validity, validity_stride);
    std::vector<sj_u64> ws(n_fields * ac_chunks(n_rows, chunk_rows) + 1, 0xA5A5A5A5A5A5A5A5ull);  // (the scratch is not zero on the device either)
    fc_sim_run(plan, c, out.o, ws.data(), (AcResult*)results, ac_convert_chunk<SeqGroup>, ac_finish<SeqGroup>);
    return out.copy_back(data, validity) ? 0 : -4;
}

}  // extern "C"
