// arrowcol.hip -- finished (type, value) columns as Arrow int64, float64 and bool arrays with validity bitmaps and a record of
// counts per field (include/sjmi.h, sjmi_arrow_columns_device).  The pass is sj_arrowcol.h (shared with the host
// simulation, tests/host_sim/arrowcol_sim.cpp), the device form of its lane group is WgGroup of sj_group.h; the finish kernel
// and the launcher of the two kernels are fieldcol_launch.h's.  This file's own kernel:
//   k_arrow_convert  one workgroup per 1024 rows and FIELD, one lane per row: the data word, the validity word (a wave is 64
//                    consecutive rows: its ballot is the word; a BOOL field's data word is a second ballot) and the chunk's
//                    three counts, packed, into the scratch
#include <hip/hip_runtime.h>

#include "fieldcol_launch.h"
#include "sj_arrowcol.h"

static_assert(AC_INT64 == SJMI_ARROW_INT64 && AC_FLOAT64 == SJMI_ARROW_FLOAT64 && AC_BOOL == SJMI_ARROW_BOOL &&
                  AC_F_INTEGRAL_DOUBLES == SJMI_ARROW_F_INTEGRAL_DOUBLES,
              "sj_arrowcol.h restates the kinds and the flag");
static_assert(sizeof(AcResult) == sizeof(sjmi_arrow_field_result) && sizeof(AcResult) == (AcCounts::COUNTS + 1) * 8, "the record is 32 bytes");

namespace sjmi {

namespace {

__global__ __launch_bounds__(AC_CHUNK_ROWS) void k_arrow_convert(const AcPlan p, AcCols c, AcOut o, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[AC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    ac_convert_chunk(g, p, c, blockIdx.x, blockIdx.y, o, counts);
}

}  // namespace

int arrowcol_plan(const void* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out) {
    return ac_plan_compile((const AcField*)fields, n_fields, n_cols, (AcPlan*)plan_out);
}

size_t arrowcol_workspace_bytes(uint64_t n_fields, uint64_t n_rows) { return fieldcol_workspace_bytes(n_fields, n_rows, AC_CHUNK_ROWS); }

hipError_t arrowcol_launch(const void* plan, const FieldColArgs& a, void* d_ws, hipStream_t stream) {
    const AcCols c = {fieldcol_cols(a), AC_CHUNK_ROWS};
    return fieldcol_launch<AcCounts>(k_arrow_convert, AC_CHUNK_ROWS, plan, c, a, d_ws, stream);
}

}  // namespace sjmi
