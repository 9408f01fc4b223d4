// sortrows.hip -- all rows ordered by one key column: a stable radix sort, chainable over several keys (include/sjmi.h,
// sjmi_sort_rows_device).  The passes are sj_sortrows.h (shared with the host simulation,
// tests/host_sim/sortrows_sim.cpp); the device form of their lane group is WgGroup of sj_group.h, to which this file adds the
// agent-scope atomics on the state and the record (relaxed, results unused: 64-bit adds, unsigned 64-bit minimum and maximum,
// each one instruction on gfx950), the barrier, the wave's fence on LDS and the minimum / maximum over the workgroup, as
// toprows.hip does.  No atomic touches LDS: a pair's place is a function of the data (sj_sortrows.h).  Plain kernels that the
// stream orders -- no workgroup waits for another, nothing spins:
//   k_sort_clear     the state to its identities, the record with n_rows = live
//   k_sort_range     a capped grid: every live position classified, the record's counts, the candidates' minimum and maximum key
//   k_sort_plan      one lane: the number of 8-bit digits, where the classes behind the candidates begin, n_passes, the flags
//   k_sort_count     one workgroup per 1024 positions: its four class counts in two words
//   k_sort_scan      one workgroup: these counts in front of every chunk
//   k_sort_emit      one workgroup per 1024 positions: the candidates as (key, position) into buffer A, the others to their final places
//   k_sort_hist      x 8, one workgroup per tile of 4096 pairs: the tile's count of each of the 256 digit values (16 KiB of LDS)
//   k_sort_digit_scan x 8, one workgroup per digit value: the value's counts in front of every tile, and its total
//   k_sort_scatter   x 8, one workgroup per tile: every pair through LDS, in the tile's output order, to its place in the other
//                    buffer (67 KiB of LDS: two workgroups a CU)
//                    (a pass at or above the plan's number of digits reads the plan and leaves at once)
//   k_sort_gather    a lane per output place: the row, the carried cells
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows.
#include <hip/hip_runtime.h>

#include "sj_sortrows.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(SR_LONG == SJMI_SORT_LONG && SR_DOUBLE == SJMI_SORT_DOUBLE && SR_DESCENDING == SJMI_SORT_DESCENDING && SR_BAD_ROW == SJMI_SORT_BAD_ROW &&
                  SR_RESULT_WORDS == SJMI_SORT_RESULT_WORDS,
              "sj_sortrows.h restates the constants");
static_assert(sizeof(SrResult) == sizeof(sjmi_sort_result) && sizeof(SrResult) == 72, "the result record is nine words");

namespace sjmi {

namespace {

constexpr uint32_t SR_BLOCK = 1024;       // threads of every kernel that runs a pass with scans
constexpr uint32_t SR_SMALL_BLOCK = 256;  // threads of k_sort_gather
static_assert(SR_CHUNK_ROWS == SR_BLOCK && SR_TILE_ROWS % SR_BLOCK == 0 && SR_VALUES <= SR_BLOCK,
              "block_scan_in_place takes 1024 threads; a wave's run of a tile is whole steps of 64 pairs");

struct SrAtomics {
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void umin(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void umax(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct SrGroup : WgGroup {
    SrAtomics agent;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ void wave_fence() const { wave_lds_fence(); }
    // (as toprows.hip's: six exchanges in the wave, then the waves' results through s_wave; begins with a barrier)
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

__global__ __launch_bounds__(64) void k_sort_clear(SrColumn c, sj_u64* __restrict__ ws, SrResult* __restrict__ res) {
    sr_clear_word(c, threadIdx.x, ws, res);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_range(SrColumn c, sj_u64* __restrict__ ws, SrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    const SrGroup g = {{s_wave}, {}};
    sr_range(g, c, blockIdx.x, gridDim.x, ws, res);
}

__global__ __launch_bounds__(64) void k_sort_plan(sj_u64* __restrict__ ws, SrResult* __restrict__ res) {
    if (threadIdx.x == 0) sr_plan(ws, res);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_count(SrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    const SrGroup g = {{s_wave}, {}};
    sr_count(g, c, blockIdx.x, ws);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_scan(SrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    const SrGroup g = {{s_wave}, {}};
    sr_scan(g, c, ws);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_emit(SrColumn c, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    const SrGroup g = {{s_wave}, {}};
    sr_emit(g, c, blockIdx.x, ws);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_hist(SrColumn c, uint32_t d, sj_u64* __restrict__ ws) {
    __shared__ uint32_t s_count[SR_BLOCK / 64 * SR_VALUES];
    const SrGroup g = {{nullptr}, {}};  // (no scan in this pass)
    sr_hist(g, c, d, blockIdx.x, ws, s_count);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_digit_scan(SrColumn c, uint32_t d, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    const SrGroup g = {{s_wave}, {}};
    sr_digit_scan(g, c, d, blockIdx.x, ws);
}

__global__ __launch_bounds__(SR_BLOCK) void k_sort_scatter(SrColumn c, uint32_t d, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[SR_BLOCK / 64];
    __shared__ sj_u64 s_base[SR_VALUES];
    __shared__ uint32_t s_start[SR_VALUES];
    __shared__ uint32_t s_count[SR_BLOCK / 64 * SR_VALUES];
    __shared__ sj_u64 s_key[SR_TILE_ROWS];
    __shared__ uint32_t s_pos[SR_TILE_ROWS];
    const SrGroup g = {{s_wave}, {}};
    sr_scatter(g, c, d, blockIdx.x, ws, s_base, s_start, s_count, s_key, s_pos);
}

__global__ __launch_bounds__(SR_SMALL_BLOCK) void k_sort_gather(SrColumn c, SrCarry in, sj_u64* __restrict__ ws, SrOut o) {
    sr_gather(c, in, (sj_u64)blockIdx.x * SR_SMALL_BLOCK + threadIdx.x, ws, o);
}

}  // namespace

size_t sortrows_workspace_bytes(uint64_t n_rows) { return (size_t)sr_workspace_words(n_rows, SR_CHUNK_ROWS, SR_TILE_ROWS) * sizeof(sj_u64); }

hipError_t sortrows_launch(const void* d_key_types, const void* d_key_validity, const void* d_key_values, uint64_t n_source_rows,
                           const void* d_rows_in, uint64_t n_rows, const void* d_row_count, uint32_t kind, uint32_t flags, const void* d_types,
                           const void* d_values, uint64_t n_cols, uint64_t col_stride, void* d_rows, void* d_out_types, void* d_out_values,
                           uint64_t out_stride, void* d_result, void* d_ws, hipStream_t stream) {
    const SrColumn c = {(const uint8_t*)d_key_types, (const sj_u64*)d_key_validity, (const sj_u64*)d_key_values, n_source_rows,
                        (const sj_u64*)d_rows_in, n_rows, (const sj_u64*)d_row_count, kind, flags, SR_CHUNK_ROWS, SR_TILE_ROWS};
    if (n_rows >= (1ull << 32) || n_source_rows >= (1ull << 32)) return hipErrorInvalidValue;
    const unsigned nchunks = (unsigned)sr_chunks(c), ntiles = (unsigned)sr_tiles(c, n_rows);
    sj_u64* ws = (sj_u64*)d_ws;
    SrResult* res = (SrResult*)d_result;
    hipLaunchKernelGGL(k_sort_clear, dim3(1), dim3(64), 0, stream, c, ws, res);
    if (nchunks) hipLaunchKernelGGL(k_sort_range, dim3(sr_grid(n_rows, SR_CHUNK_ROWS)), dim3(SR_BLOCK), 0, stream, c, ws, res);
    hipLaunchKernelGGL(k_sort_plan, dim3(1), dim3(64), 0, stream, ws, res);
    if (!nchunks) return hipGetLastError();  // (no position: the record is complete)
    hipLaunchKernelGGL(k_sort_count, dim3(nchunks), dim3(SR_BLOCK), 0, stream, c, ws);
    hipLaunchKernelGGL(k_sort_scan, dim3(1), dim3(SR_BLOCK), 0, stream, c, ws);
    hipLaunchKernelGGL(k_sort_emit, dim3(nchunks), dim3(SR_BLOCK), 0, stream, c, ws);
    for (uint32_t d = 0; d < SR_MAX_DIGITS; ++d) {
        hipLaunchKernelGGL(k_sort_hist, dim3(ntiles), dim3(SR_BLOCK), 0, stream, c, d, ws);
        hipLaunchKernelGGL(k_sort_digit_scan, dim3(SR_VALUES), dim3(SR_BLOCK), 0, stream, c, d, ws);
        hipLaunchKernelGGL(k_sort_scatter, dim3(ntiles), dim3(SR_BLOCK), 0, stream, c, d, ws);
    }
    const SrCarry in = {(const uint8_t*)d_types, (const sj_u64*)d_values, n_cols, col_stride};
    const SrOut o = {(sj_u64*)d_rows, (uint8_t*)d_out_types, (sj_u64*)d_out_values, out_stride};
    hipLaunchKernelGGL(k_sort_gather, dim3((unsigned)((n_rows + SR_SMALL_BLOCK - 1) / SR_SMALL_BLOCK)), dim3(SR_SMALL_BLOCK), 0, stream, c, in, ws, o);
    return hipGetLastError();
}

}  // namespace sjmi
