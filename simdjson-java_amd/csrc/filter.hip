// filter.hip -- the rows of a set of (type, value) columns filtered by a conjunction of terms and compacted (include/sjmi.h,
// sjmi_filter_columns_device).  The passes are sj_filter.h (shared with the host simulation, tests/host_sim/
// filter_sim.cpp), the device form of its lane group is WgGroup of sj_group.h; this file is three plain kernels that the stream
// orders -- no workgroup waits for another -- and the host side of a plan:
//   k_filter_eval   one workgroup per 1024 rows, one lane per row: the terms in plan order, the keep words (a wave is 64
//                   consecutive rows: its ballot is one word) and the chunk's kept rows
//   k_filter_scan   ONE workgroup: the kept rows in front of every chunk (in place), the result record
//   k_filter_emit   one workgroup per chunk: the selection vector and the compacted columns (not launched by a sizing call)
// The plan travels BY VALUE as a launch argument: the terms are scalar data of the kernel, nothing is uploaded and the context
// holds no plan.  The scans are block_excl_scan / block_scan_in_place of sj_chain.h, as in strcol.hip and explode.hip.
#include <hip/hip_runtime.h>

#include <new>

#include "sj_filter.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(FL_OVERFLOW == SJMI_FILTER_OVERFLOW, "sj_filter.h restates the flag");
static_assert(FL_MAX_TERMS == SJMI_FILTER_MAX_TERMS && FL_MAX_CONST_BYTES == SJMI_FILTER_MAX_CONST_BYTES && FL_MAX_STRING == SJMI_FILTER_MAX_STRING,
              "sj_filter.h restates the limits");
static_assert(sizeof(FlResult) == sizeof(sjmi_filter_result) && sizeof(FlResult) == 16, "the result record is 16 bytes");
static_assert(sizeof(FlTerm) == sizeof(sjmi_filter_term) && sizeof(FlTerm) == 16, "a term is 16 bytes");
static_assert(SJMI_F_TYPE_EQ == (FL_TYPE << 4 | FL_EQ) && SJMI_F_TYPE_NE == (FL_TYPE << 4 | FL_NE) && SJMI_F_LONG_EQ == (FL_LONG << 4 | FL_EQ) &&
                  SJMI_F_LONG_GE == (FL_LONG << 4 | FL_GE) && SJMI_F_DOUBLE_EQ == (FL_DOUBLE << 4 | FL_EQ) &&
                  SJMI_F_DOUBLE_GE == (FL_DOUBLE << 4 | FL_GE) && SJMI_F_STRING_EQ == (FL_STRING << 4 | FL_EQ) &&
                  SJMI_F_STRING_NE == (FL_STRING << 4 | FL_NE) && SJMI_F_STRING_PREFIX == (FL_STRING << 4 | FL_PREFIX),
              "sj_filter.h restates the ops");
static_assert(sizeof(FlPlan) <= 2048, "the plan is a launch argument");

struct sjmi_filter_plan {
    FlPlan image;
    bool has_string;
};

namespace sjmi {

namespace {

static_assert(FL_CHUNK_ROWS == 1024, "block_scan_in_place takes slices of 1024 entries with 1024 threads");

__global__ __launch_bounds__(FL_CHUNK_ROWS) void k_filter_eval(const FlPlan p, FlCols c, sj_u64* __restrict__ keep, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[FL_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    fl_eval_chunk(g, p, c, blockIdx.x, keep, counts);
}

__global__ __launch_bounds__(1024) void k_filter_scan(sj_u64* __restrict__ counts, uint64_t nchunks, uint64_t out_capacity,
                                                      FlResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[16];
    const WgGroup g = {s_wave};
    fl_chunk_scan(g, counts, nchunks, out_capacity, res);
}

__global__ __launch_bounds__(FL_CHUNK_ROWS) void k_filter_emit(FlCols c, const sj_u64* __restrict__ keep, const sj_u64* __restrict__ counts,
                                                               FlOut o) {
    const WgGroup g = {nullptr};  // (no scan in this pass, and no barrier: a chunk behind the capacity leaves at once)
    fl_emit_chunk(g, c, blockIdx.x, keep, counts, o);
}

}  // namespace

int filter_plan_columns(const sjmi_filter_plan* plan, uint64_t n_cols) {
    for (uint32_t k = 0; k < plan->image.n_terms; ++k)
        if (plan->image.terms[k].column >= n_cols) return -1;
    return plan->has_string ? 1 : 0;
}

size_t filter_workspace_bytes(uint64_t n_rows) {
    // the chunk counts | the keep words of a call without d_keep
    return (size_t)((n_rows + FL_CHUNK_ROWS - 1) / FL_CHUNK_ROWS + (n_rows + 63) / 64 + 1) * sizeof(sj_u64);
}

hipError_t filter_launch(const sjmi_filter_plan* plan, const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride,
                         uint64_t n_rows, const void* d_string_buffer, void* d_keep, void* d_rows, uint64_t out_capacity, void* d_out_types,
                         void* d_out_values, void* d_result, void* d_ws, hipStream_t stream) {
    const FlCols c = {(const uint8_t*)d_types, (const sj_u64*)d_values, n_cols, col_stride, n_rows, (const uint8_t*)d_string_buffer, FL_CHUNK_ROWS};
    const uint64_t nchunks = fl_chunks(c);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    sj_u64* counts = (sj_u64*)d_ws;
    sj_u64* keep = d_keep ? (sj_u64*)d_keep : counts + nchunks;
    if (nchunks) hipLaunchKernelGGL(k_filter_eval, dim3((unsigned)nchunks), dim3(FL_CHUNK_ROWS), 0, stream, plan->image, c, keep, counts);
    hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(1024), 0, stream, counts, nchunks, out_capacity, (FlResult*)d_result);
    if (nchunks && out_capacity) {  // (the sizing call does not emit)
        const FlOut o = {(sj_u64*)d_rows, (uint8_t*)d_out_types, (sj_u64*)d_out_values, out_capacity};
        hipLaunchKernelGGL(k_filter_emit, dim3((unsigned)nchunks), dim3(FL_CHUNK_ROWS), 0, stream, c, (const sj_u64*)keep, (const sj_u64*)counts, o);
    }
    return hipGetLastError();
}

}  // namespace sjmi

extern "C" {

int sjmi_filter_plan_compile(const sjmi_filter_term* terms, uint64_t n_terms, const uint8_t* bytes, uint64_t n_bytes, sjmi_filter_plan** out) {
    if (!out) return SJMI_ERR_ARG;
    *out = nullptr;
    sjmi_filter_plan* plan = new (std::nothrow) sjmi_filter_plan;
    if (!plan) return SJMI_ERR_ARG;
    if (fl_plan_compile((const FlTerm*)terms, n_terms, bytes, n_bytes, &plan->image) != 0) {
        delete plan;
        return SJMI_ERR_ARG;
    }
    plan->has_string = fl_plan_has_string(plan->image);
    *out = plan;
    return SJMI_OK;
}

void sjmi_filter_plan_destroy(sjmi_filter_plan* plan) { delete plan; }

}  // extern "C"
