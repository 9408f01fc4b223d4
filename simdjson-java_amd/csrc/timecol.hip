// timecol.hip -- the RFC 3339 strings of finished (type, value) columns as Arrow timestamp arrays: int64 words at the unit of the
// field, validity bitmaps and a record of counts per field (include/sjmi.h, sjmi_time_columns_device).  The
// passes are sj_timecol.h (shared with the host simulation, tests/host_sim/timecol_sim.cpp), the device form of its lane group
// is WgGroup of sj_group.h with group_ballots of sj_group_ballots.h; this file is two plain kernels that the stream orders --
// no atomics, no workgroup waits for another:
//   k_time_parse    one workgroup of 256 threads per 256 rows and FIELD (gridDim.y = the fields), one row per lane: type byte ->
//                   value word -> string bytes is a chain of three dependent loads, and what hides it is the eight resident
//                   waves per SIMD (39 VGPRs) -- more rows per lane were measured and were no faster (profiles/r16).  A wave's
//                   ballot of VALID is the validity word; the chunk's five counts go, packed, into the scratch
//   k_time_finish   one workgroup per field: the sum of its chunk words, the record
// The schema travels BY VALUE as a launch argument: the fields are scalar data of the kernels, nothing is uploaded and the
// context holds no schema.  Where the caller gives a row count in device memory both kernels read it there: the grid is sized
// by n_rows, and a workgroup whose chunk begins at or above the live rows leaves at once.
#include <hip/hip_runtime.h>

#include "sj_group_ballots.h"
#include "sj_timecol.h"
#include "stage1.h"

static_assert(TC_MAX_FIELDS == SJMI_TIME_MAX_FIELDS, "sj_timecol.h restates the limit");
static_assert(TC_SECOND == SJMI_TIME_SECOND && TC_MILLI == SJMI_TIME_MILLI && TC_MICRO == SJMI_TIME_MICRO && TC_NANO == SJMI_TIME_NANO &&
                  TC_F_NAIVE_UTC == SJMI_TIME_F_NAIVE_UTC,
              "sj_timecol.h restates the units and the flag");
static_assert(sizeof(TcField) == sizeof(sjmi_time_field) && sizeof(TcField) == 16, "a field is 16 bytes");
static_assert(sizeof(TcResult) == sizeof(sjmi_time_field_result) && sizeof(TcResult) == 48, "the record is 48 bytes");
static_assert(sizeof(TcPlan) == sjmi::TIMECOL_PLAN_BYTES && sizeof(TcPlan) <= 2048, "the schema is a launch argument");
static_assert(TC_CHUNK_ROWS < (1u << TC_COUNT_BITS) && 5 * TC_COUNT_BITS <= 64, "a chunk's five counts fit one word");

namespace sjmi {

namespace {

constexpr uint32_t TC_THREADS = TC_CHUNK_ROWS / TC_LANE_ROWS;
constexpr uint32_t TC_FINISH_THREADS = 256;
constexpr bool TC_FETCH_WORDS = true;  // the fetch that was faster on the MI355X (profiles/r16)
static_assert(TC_THREADS % 64 == 0, "whole waves");

__global__ __launch_bounds__(TC_THREADS) void k_time_parse(const TcPlan p, TcCols c, TcOut o, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[TC_THREADS / 64];
    const WgGroup g = {s_wave};
    tc_parse_chunk<TC_FETCH_WORDS, TC_LANE_ROWS>(g, p, c, blockIdx.x, blockIdx.y, o, counts);
}

__global__ __launch_bounds__(TC_FINISH_THREADS) void k_time_finish(TcCols c, const sj_u64* __restrict__ counts, TcResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[TC_FINISH_THREADS / 64];
    const WgGroup g = {s_wave};
    tc_finish(g, c, blockIdx.x, counts, res);
}

}  // namespace

int timecol_plan(const sjmi_time_field* fields, uint64_t n_fields, uint64_t n_cols, void* plan_out) {
    return tc_plan_compile((const TcField*)fields, n_fields, n_cols, (TcPlan*)plan_out);
}

size_t timecol_workspace_bytes(uint64_t n_fields, uint64_t n_rows) {
    return (size_t)(n_fields * tc_chunks(n_rows, TC_CHUNK_ROWS) + 1) * sizeof(sj_u64);
}

hipError_t timecol_launch(const void* plan, const void* d_types, const void* d_values, uint64_t col_stride, uint64_t n_rows,
                          const void* d_row_count, const void* d_string_buffer, void* d_data, uint64_t data_stride, void* d_validity,
                          uint64_t validity_stride, void* d_results, void* d_ws, hipStream_t stream) {
    const TcPlan& p = *(const TcPlan*)plan;
    const TcCols c = {(const uint8_t*)d_types, (const sj_u64*)d_values, col_stride, n_rows, (const sj_u64*)d_row_count, (const uint8_t*)d_string_buffer,
                      TC_CHUNK_ROWS};
    const TcOut o = {(sj_u64*)d_data, data_stride, (sj_u64*)d_validity, validity_stride};
    const uint64_t nchunks = tc_chunks(n_rows, TC_CHUNK_ROWS);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (nchunks) hipLaunchKernelGGL(k_time_parse, dim3((unsigned)nchunks, p.n_fields), dim3(TC_THREADS), 0, stream, p, c, o, (sj_u64*)d_ws);
    hipLaunchKernelGGL(k_time_finish, dim3(p.n_fields), dim3(TC_FINISH_THREADS), 0, stream, c, (const sj_u64*)d_ws, (TcResult*)d_results);
    return hipGetLastError();
}

}  // namespace sjmi
