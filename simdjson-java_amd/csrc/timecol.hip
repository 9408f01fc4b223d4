// timecol.hip -- the RFC 3339 strings of finished (type, value) columns as Arrow timestamp arrays: int64 words at the unit of the
// field, validity bitmaps and a record of counts per field (include/sjmi.h, sjmi_time_columns_device).  The
// pass is sj_timecol.h (shared with the host simulation, tests/host_sim/timecol_sim.cpp), the device form of its lane group is
// WgGroup of sj_group.h with group_ballots of sj_group_ballots.h; the finish kernel and the launcher of the two kernels are
// fieldcol_launch.h's.  This file's own kernel:
//   k_time_parse    one workgroup of 256 threads per 256 rows and FIELD, one row per lane: type byte -> value word -> string
//                   bytes is a chain of three dependent loads, and what hides it is the eight resident waves per SIMD (39 VGPRs)
//                   -- more rows per lane were measured and were no faster (profiles/r16).  A wave's ballot of VALID is the
//                   validity word; the chunk's five counts go, packed, into the scratch
#include <hip/hip_runtime.h>

#include "fieldcol_launch.h"
#include "sj_group_ballots.h"
#include "sj_timecol.h"

static_assert(TC_SECOND == SJMI_TIME_SECOND && TC_MILLI == SJMI_TIME_MILLI && TC_MICRO == SJMI_TIME_MICRO && TC_NANO == SJMI_TIME_NANO &&
                  TC_F_NAIVE_UTC == SJMI_TIME_F_NAIVE_UTC,
              "sj_timecol.h restates the units and the flag");
static_assert(sizeof(TcResult) == sizeof(sjmi_time_field_result) && sizeof(TcResult) == (TcCounts::COUNTS + 1) * 8, "the record is 48 bytes");

namespace sjmi {

namespace {

constexpr uint32_t TC_THREADS = TC_CHUNK_ROWS / TC_LANE_ROWS;
constexpr bool TC_FETCH_WORDS = true;  // the fetch that was faster on the MI355X (profiles/r16)
static_assert(TC_THREADS % 64 == 0, "whole waves");

__global__ __launch_bounds__(TC_THREADS) void k_time_parse(const TcPlan p, TcCols c, TcOut o, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[TC_THREADS / 64];
    const WgGroup g = {s_wave};
    tc_parse_chunk<TC_FETCH_WORDS, TC_LANE_ROWS>(g, p, c, blockIdx.x, blockIdx.y, o, counts);
}

}  // namespace

int timecol_plan(const void* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out) {
    return tc_plan_compile((const TcField*)fields, n_fields, n_cols, (TcPlan*)plan_out);
}

size_t timecol_workspace_bytes(uint64_t n_fields, uint64_t n_rows) { return fieldcol_workspace_bytes(n_fields, n_rows, TC_CHUNK_ROWS); }

hipError_t timecol_launch(const void* plan, const FieldColArgs& a, void* d_ws, hipStream_t stream) {
    const TcCols c = {fieldcol_cols(a), (const uint8_t*)a.d_string_buffer, TC_CHUNK_ROWS};
    return fieldcol_launch<TcCounts>(k_time_parse, TC_THREADS, plan, c, a, d_ws, stream);
}

}  // namespace sjmi
