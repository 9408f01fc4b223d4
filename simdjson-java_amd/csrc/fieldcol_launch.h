// fieldcol_launch.h -- the device side of sj_fieldcol.h, once for arrowcol.hip and timecol.hip: the finish kernel, the scratch
// size and the launcher of an operator's two kernels.  gfx950 device code only.  An operator's translation unit adds its convert
// kernel -- one workgroup per chunk of rows and FIELD (gridDim.y = the fields) -- and instantiates these with its counts.
//
// The schema travels BY VALUE as a launch argument, as the filter's plan does: the fields are scalar data of the kernels, nothing
// is uploaded and the context holds no schema.  Where the caller gives a row count in device memory both kernels read it there:
// the grid is sized by n_rows, and a workgroup whose chunk begins at or above the live rows leaves at once.  The stream orders
// the two kernels -- no atomics, no workgroup waits for another.
#pragma once
#include <hip/hip_runtime.h>

#include "sj_fieldcol.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(FC_MAX_FIELDS == SJMI_ARROW_MAX_FIELDS && FC_MAX_FIELDS == SJMI_TIME_MAX_FIELDS && FC_MAX_FIELDS == SJMI_SELECT_MAX_PATHS,
              "sj_fieldcol.h restates the limit");
static_assert(sizeof(FcField) == sizeof(sjmi_arrow_field) && sizeof(FcField) == sizeof(sjmi_time_field) && sizeof(FcField) == 16, "a field is 16 bytes");
static_assert(sizeof(FcPlan) == sjmi::FIELDCOL_PLAN_BYTES && sizeof(FcPlan) <= 2048, "the schema is a launch argument");

namespace sjmi {

constexpr uint32_t FC_FINISH_THREADS = 256;

// one workgroup per field: the sum of its chunk words, the record
template <class Counts, class Cols>
__global__ __launch_bounds__(FC_FINISH_THREADS) void k_field_finish(Cols c, const sj_u64* __restrict__ counts, sj_u64* __restrict__ res) {
    __shared__ unsigned long long s_wave[FC_FINISH_THREADS / 64];
    const WgGroup g = {s_wave};
    fc_finish<Counts>(g, c, blockIdx.x, counts, res);
}

// scratch of one call: one packed count word per field and chunk
inline size_t fieldcol_workspace_bytes(uint64_t n_fields, uint64_t n_rows, uint32_t chunk_rows) {
    return (size_t)(n_fields * fc_chunks(n_rows, chunk_rows) + 1) * sizeof(sj_u64);
}

// `convert` with `threads` a workgroup over (the chunks of c.n_rows, the fields) -- only where there are rows --, then the
// finish kernel, always: the records are written by every call
template <class Counts, class Cols>
hipError_t fieldcol_launch(void (*convert)(const FcPlan, Cols, FcOut, sj_u64*), uint32_t threads, const void* plan, const Cols& c, const FieldColArgs& a,
                           void* d_ws, hipStream_t stream) {
    const FcPlan& p = *(const FcPlan*)plan;
    const FcOut o = {(sj_u64*)a.d_data, a.data_stride, (sj_u64*)a.d_validity, a.validity_stride};
    const uint64_t nchunks = fc_chunks(c.n_rows, c.chunk_rows);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nchunks) hipLaunchKernelGGL(convert, dim3((unsigned)nchunks, p.n_fields), dim3(threads), 0, stream, p, c, o, (sj_u64*)d_ws);
    hipLaunchKernelGGL((k_field_finish<Counts, Cols>), dim3(p.n_fields), dim3(FC_FINISH_THREADS), 0, stream, c, (const sj_u64*)d_ws, (sj_u64*)a.d_results);
    return hipGetLastError();
}
// the columns of a call
inline FcCols fieldcol_cols(const FieldColArgs& a) {
    return {(const uint8_t*)a.d_types, (const sj_u64*)a.d_values, a.col_stride, a.n_rows, (const sj_u64*)a.d_row_count};
}

}  // namespace sjmi
