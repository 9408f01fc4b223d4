// arrowcol.hip -- finished (type, value) columns as Arrow int64, float64 and bool arrays with validity bitmaps and a record of
// counts per field (include/sjmi.h, sjmi_arrow_columns_device).  The passes are sj_arrowcol.h (shared with the
// host simulation, tests/host_sim/arrowcol_sim.cpp), the device form of its lane group is WgGroup of sj_group.h; this file is
// two plain kernels that the stream orders -- no atomics, no workgroup waits for another:
//   k_arrow_convert  one workgroup per 1024 rows and FIELD (gridDim.y = the fields), one lane per row: the data word, the
//                    validity word (a wave is 64 consecutive rows: its ballot is the word; a BOOL field's data word is a
//                    second ballot) and the chunk's three counts, packed, into the scratch
//   k_arrow_finish   one workgroup per field: the sum of its chunk words, the record
// The schema travels BY VALUE as a launch argument, as the filter's plan does: the fields are scalar data of the kernels, nothing
// is uploaded and the context holds no schema.  Where the caller gives a row count in device memory both kernels read it there:
// the grid is sized by n_rows, and a workgroup whose chunk begins at or above the live rows leaves at once.
#include <hip/hip_runtime.h>

#include "sj_arrowcol.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(AC_MAX_FIELDS == SJMI_ARROW_MAX_FIELDS && AC_MAX_FIELDS == SJMI_SELECT_MAX_PATHS, "sj_arrowcol.h restates the limit");
static_assert(AC_INT64 == SJMI_ARROW_INT64 && AC_FLOAT64 == SJMI_ARROW_FLOAT64 && AC_BOOL == SJMI_ARROW_BOOL &&
                  AC_F_INTEGRAL_DOUBLES == SJMI_ARROW_F_INTEGRAL_DOUBLES,
              "sj_arrowcol.h restates the kinds and the flag");
static_assert(sizeof(AcField) == sizeof(sjmi_arrow_field) && sizeof(AcField) == 16, "a field is 16 bytes");
static_assert(sizeof(AcResult) == sizeof(sjmi_arrow_field_result) && sizeof(AcResult) == 32, "the record is 32 bytes");
static_assert(sizeof(AcPlan) == sjmi::ARROWCOL_PLAN_BYTES && sizeof(AcPlan) <= 2048, "the schema is a launch argument");
static_assert(AC_CHUNK_ROWS < (1u << AC_COUNT_BITS), "a chunk's counts fit their bits");

namespace sjmi {

namespace {

constexpr uint32_t AC_FINISH_THREADS = 256;

__global__ __launch_bounds__(AC_CHUNK_ROWS) void k_arrow_convert(const AcPlan p, AcCols c, AcOut o, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[AC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    ac_convert_chunk(g, p, c, blockIdx.x, blockIdx.y, o, counts);
}

__global__ __launch_bounds__(AC_FINISH_THREADS) void k_arrow_finish(AcCols c, const sj_u64* __restrict__ counts, AcResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[AC_FINISH_THREADS / 64];
    const WgGroup g = {s_wave};
    ac_finish(g, c, blockIdx.x, counts, res);
}

}  // namespace

int arrowcol_plan(const sjmi_arrow_field* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out) {
    return ac_plan_compile((const AcField*)fields, n_fields, n_cols, (AcPlan*)plan_out);
}

size_t arrowcol_workspace_bytes(uint64_t n_fields, uint64_t n_rows) {
    return (size_t)(n_fields * ac_chunks(n_rows, AC_CHUNK_ROWS) + 1) * sizeof(sj_u64);
}

hipError_t arrowcol_launch(const void* plan, const void* d_types, const void* d_values, uint64_t col_stride, uint64_t n_rows,
                           const void* d_row_count, void* d_data, uint64_t data_stride, void* d_validity, uint64_t validity_stride,
                           void* d_results, void* d_ws, hipStream_t stream) {
    const AcPlan& p = *(const AcPlan*)plan;
    const AcCols c = {(const uint8_t*)d_types, (const sj_u64*)d_values, col_stride, n_rows, (const sj_u64*)d_row_count, AC_CHUNK_ROWS};
    const AcOut o = {(sj_u64*)d_data, data_stride, (sj_u64*)d_validity, validity_stride};
    const uint64_t nchunks = ac_chunks(n_rows, AC_CHUNK_ROWS);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nchunks) hipLaunchKernelGGL(k_arrow_convert, dim3((unsigned)nchunks, p.n_fields), dim3(AC_CHUNK_ROWS), 0, stream, p, c, o, (sj_u64*)d_ws);
    hipLaunchKernelGGL(k_arrow_finish, dim3(p.n_fields), dim3(AC_FINISH_THREADS), 0, stream, c, (const sj_u64*)d_ws, (AcResult*)d_results);
    return hipGetLastError();
}

}  // namespace sjmi
