// toprows.hip -- the top k rows of one key column: ORDER BY a value, LIMIT k (include/sjmi.h, sjmi_top_rows_device; DESIGN.md
// 4.18).  The passes are sj_toprows.h (shared with the host simulation, tests/host_sim/toprows_sim.cpp); the device form of their
// lane group is WgGroup of sj_group.h, to which this file adds the atomics -- g.wg on the workgroup's LDS bins, g.agent on the
// scratch and the record (agent scope: the XCDs' L2s are not coherent, DESIGN.md 4.15 "visibility") --, the barrier and the
// minimum / maximum over the workgroup (a wave butterfly, then one LDS entry per wave).  All atomics relaxed, results unused:
// 32- and 64-bit adds, unsigned 64-bit minimum and maximum, each one instruction on gfx950 (no compare-and-swap loop).  Plain
// kernels that the stream orders -- no workgroup waits for another, nothing spins:
//   k_top_clear   the state and the histograms to their identities, the record with n_rows = live
//   k_top_range   a capped grid: every live row classified, the record's counts, the candidates' minimum and maximum key
//   k_top_plan    one lane: n_out, the common high bits, the number of 11-bit digits below them
//   k_top_hist    x 6, a capped grid: the digit's 2048 LDS bins, the non-zero ones to the pass's histogram
//   k_top_pick    x 6, one workgroup: the bin where the count from the top reaches what remains of k
//                 (a pass at or above the plan's number of digits reads the plan and leaves at once)
//   k_top_mark    one workgroup per 1024 rows: its candidates above and equal to the threshold key
//   k_top_scan    one workgroup: these counts in front of every chunk
//   k_top_emit    one workgroup per 1024 rows: the taken rows as (key, row) into n_out slots of the scratch
//   k_top_sort    one workgroup: a bitonic network in LDS under (key descending, row ascending); the rows, the carried cells
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows.
#include <hip/hip_runtime.h>

#include "sj_toprows.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(TR_MAX_K == SJMI_TOP_MAX_K && TR_LONG == SJMI_TOP_LONG && TR_DOUBLE == SJMI_TOP_DOUBLE && TR_SMALLEST == SJMI_TOP_SMALLEST &&
                  TR_RESULT_WORDS == SJMI_TOP_RESULT_WORDS,
              "sj_toprows.h restates the constants");
static_assert(sizeof(TrResult) == sizeof(sjmi_top_result) && sizeof(TrResult) == 72, "the result record is nine words");

namespace sjmi {

namespace {

constexpr uint32_t TR_SMALL_BLOCK = 256;  // threads of k_top_clear
static_assert(TR_CHUNK_ROWS == 1024 && TR_MAX_K == 2 * TR_CHUNK_ROWS, "block_scan_in_place takes 1024 threads; a lane of the sort holds one pair");

template <int SCOPE>
struct TrAtomics {
    __device__ __forceinline__ void add32(uint32_t* p, uint32_t n) const { (void)__hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void umin(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void umax(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE); }
};

struct TrGroup : WgGroup {
    TrAtomics<__HIP_MEMORY_SCOPE_WORKGROUP> wg;
    TrAtomics<__HIP_MEMORY_SCOPE_AGENT> agent;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // a value of every lane of the workgroup -> f over all of them, in every lane: six exchanges in the wave, then the waves'
    // results through s_wave.  Begins with a barrier, as the scans do: s_wave is free by then.
    template <class F>
    __device__ __forceinline__ sj_u64 all(sj_u64 v, F f) const {
        for (int d = 1; d < 64; d <<= 1) v = f(v, __shfl_xor(v, d));
        __syncthreads();
        if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
        __syncthreads();
        sj_u64 r = s_wave[0];
        for (uint32_t i = 1; i < (blockDim.x >> 6); ++i) r = f(r, s_wave[i]);
        return r;
    }
    __device__ __forceinline__ sj_u64 all_umin(sj_u64 v) const { return all(v, [](sj_u64 a, sj_u64 b) { return a < b ? a : b; }); }
    __device__ __forceinline__ sj_u64 all_umax(sj_u64 v) const { return all(v, [](sj_u64 a, sj_u64 b) { return a > b ? a : b; }); }
};

__global__ __launch_bounds__(TR_SMALL_BLOCK) void k_top_clear(TrColumn c, sj_u64* __restrict__ ws, TrResult* __restrict__ res) {
    tr_clear_word(c, (sj_u64)blockIdx.x * TR_SMALL_BLOCK + threadIdx.x, ws, res);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_range(TrColumn c, sj_u64* __restrict__ ws, TrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[TR_CHUNK_ROWS / 64];
    const TrGroup g = {{s_wave}, {}, {}};
    tr_range(g, c, blockIdx.x, gridDim.x, ws, res);
}

__global__ __launch_bounds__(64) void k_top_plan(TrColumn c, sj_u64* __restrict__ ws, TrResult* __restrict__ res) {
    if (threadIdx.x == 0) tr_plan(c, ws, res);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_hist(TrColumn c, uint32_t d, sj_u64* __restrict__ ws) {
    __shared__ uint32_t s_bins[TR_BINS];
    const TrGroup g = {{nullptr}, {}, {}};  // (no scan in this pass)
    tr_hist(g, c, d, blockIdx.x, gridDim.x, ws, s_bins);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_pick(uint32_t d, sj_u64* ws) {  // (one lane writes the state that all have read)
    __shared__ unsigned long long s_wave[TR_CHUNK_ROWS / 64];
    const TrGroup g = {{s_wave}, {}, {}};
    tr_pick(g, d, ws);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_mark(TrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[TR_CHUNK_ROWS / 64];
    const TrGroup g = {{s_wave}, {}, {}};
    tr_mark(g, c, blockIdx.x, ws);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_scan(TrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[TR_CHUNK_ROWS / 64];
    const TrGroup g = {{s_wave}, {}, {}};
    tr_scan(g, c, ws);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_emit(TrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[TR_CHUNK_ROWS / 64];
    const TrGroup g = {{s_wave}, {}, {}};
    tr_emit(g, c, blockIdx.x, ws);
}

__global__ __launch_bounds__(TR_CHUNK_ROWS) void k_top_sort(TrColumn c, TrCarry in, sj_u64* __restrict__ ws, TrOut o, TrResult* __restrict__ res) {
    __shared__ sj_u64 s_key[TR_MAX_K];
    __shared__ uint32_t s_row[TR_MAX_K];
    const TrGroup g = {{nullptr}, {}, {}};  // (no scan in this pass)
    tr_sort(g, c, in, ws, s_key, s_row, o, res);
}

}  // namespace

size_t toprows_workspace_bytes(uint64_t n_rows, uint64_t k) { return (size_t)tr_workspace_words(n_rows, k, TR_CHUNK_ROWS) * sizeof(sj_u64); }

hipError_t toprows_launch(const void* d_key_types, const void* d_key_validity, const void* d_key_values, uint64_t n_rows, const void* d_row_count,
                          uint32_t kind, uint32_t flags, uint64_t k, const void* d_types, const void* d_values, uint64_t n_cols,
                          uint64_t col_stride, void* d_rows, void* d_out_types, void* d_out_values, void* d_result, void* d_ws, hipStream_t stream) {
    const TrColumn c = {(const uint8_t*)d_key_types, (const sj_u64*)d_key_validity, (const sj_u64*)d_key_values, n_rows, (const sj_u64*)d_row_count,
                        kind, flags, k, TR_CHUNK_ROWS};
    const uint64_t nchunks = tr_chunks(n_rows, TR_CHUNK_ROWS);
    if (nchunks > 0x7FFFFFFFull || k > TR_MAX_K) return hipErrorInvalidValue;
    sj_u64* ws = (sj_u64*)d_ws;
    TrResult* res = (TrResult*)d_result;
    const unsigned clear_grid = (unsigned)((TR_STATE_WORDS + TR_HIST_WORDS + TR_SMALL_BLOCK - 1) / TR_SMALL_BLOCK);
    hipLaunchKernelGGL(k_top_clear, dim3(clear_grid), dim3(TR_SMALL_BLOCK), 0, stream, c, ws, res);
    const unsigned grid = tr_grid(n_rows, TR_CHUNK_ROWS);
    if (nchunks) hipLaunchKernelGGL(k_top_range, dim3(grid), dim3(TR_CHUNK_ROWS), 0, stream, c, ws, res);
    hipLaunchKernelGGL(k_top_plan, dim3(1), dim3(64), 0, stream, c, ws, res);
    if (!nchunks || !k) return hipGetLastError();  // (nothing can go out: the record is complete)
    for (uint32_t d = 0; d < TR_MAX_DIGITS; ++d) {
        hipLaunchKernelGGL(k_top_hist, dim3(grid), dim3(TR_CHUNK_ROWS), 0, stream, c, d, ws);
        hipLaunchKernelGGL(k_top_pick, dim3(1), dim3(TR_CHUNK_ROWS), 0, stream, d, ws);
    }
    hipLaunchKernelGGL(k_top_mark, dim3((unsigned)nchunks), dim3(TR_CHUNK_ROWS), 0, stream, c, ws);
    hipLaunchKernelGGL(k_top_scan, dim3(1), dim3(TR_CHUNK_ROWS), 0, stream, c, ws);
    hipLaunchKernelGGL(k_top_emit, dim3((unsigned)nchunks), dim3(TR_CHUNK_ROWS), 0, stream, c, ws);
    const TrCarry in = {(const uint8_t*)d_types, (const sj_u64*)d_values, n_cols, col_stride};
    const TrOut o = {(sj_u64*)d_rows, (uint8_t*)d_out_types, (sj_u64*)d_out_values};
    hipLaunchKernelGGL(k_top_sort, dim3(1), dim3(TR_CHUNK_ROWS), 0, stream, c, in, ws, o, res);
    return hipGetLastError();
}

}  // namespace sjmi
