// joinrows.hip -- two row sets joined on a long key: inner, left, semi, anti (include/sjmi.h, sjmi_join_rows_device; DESIGN.md
// 4.21).  The passes are sj_joinrows.h (shared with the host simulation, tests/host_sim/joinrows_sim.cpp); the device form of
// their lane group is WgGroup of sj_group.h, to which this file adds the agent-scope atomics on the record (relaxed, results
// unused: a 64-bit add and a 32-bit or), the barrier and parents.hip's inclusive running maximum over the workgroup.  No atomic
// decides a place: a pair's place is a function of the data (sj_joinrows.h).  Plain kernels that the stream orders -- no workgroup
// waits for another, nothing spins:
//   k_join_clear     one lane: the record with n_left = live and n_build; off[0]
//   k_join_keys      one workgroup of 256 lanes per 1024 build places: the keys gathered once into a dense sorted array, the bad
//                    places counted, every key against the one in front of it (9 KiB of LDS)
//   k_join_count     one workgroup of 256 lanes per 1024 left positions: up to 1024 pivots of the dense array into LDS (8 KiB), the class,
//                    a lower bound through the pivots and a galloping upper bound, lo and e as 32-bit words, the chunk's sum of e,
//                    the class counts
//   k_join_scan      one workgroup: the chunk sums scanned in place, n_pairs, the flags
//   k_join_offsets   one workgroup of 1024 lanes per 1024 left positions: off[i + 1], and d_pair_offsets where given
//   k_join_emit      one workgroup of 256 lanes per 1024 OUTPUT pairs: two 64-ary searches, the span's positions into LDS, four trips
//                    of a running maximum, the rows and the carried cells of both sides (8 KiB of LDS); a workgroup at or behind
//                    min(n_pairs, pair_capacity) reads the record and leaves
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_left, n_right and
// pair_capacity.
#include <hip/hip_runtime.h>

#include "sj_joinrows.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(JR_INNER == SJMI_JOIN_INNER && JR_LEFT == SJMI_JOIN_LEFT && JR_SEMI == SJMI_JOIN_SEMI && JR_ANTI == SJMI_JOIN_ANTI &&
                  JR_OVERFLOW == SJMI_JOIN_OVERFLOW && JR_BAD_ROW == SJMI_JOIN_BAD_ROW && JR_BAD_ORDER == SJMI_JOIN_BAD_ORDER &&
                  JR_RESULT_WORDS == SJMI_JOIN_RESULT_WORDS && JR_NO_ROW == SJMI_JOIN_NO_ROW && JR_MAX_PAIR_CAPACITY == SJMI_JOIN_MAX_PAIR_CAPACITY,
              "sj_joinrows.h restates the constants");
static_assert(sizeof(JrResult) == sizeof(sjmi_join_result) && sizeof(JrResult) == 72, "the result record is nine words");

namespace sjmi {

namespace {

// The chunks whose cost is a chain of dependent loads (a gather through the build order, 2 x 33 search steps, the owner search and
// the pairs' cells) run as four waves, as parents.hip's do: several such workgroups share a CU.  The two passes that are one scan
// take the 1024 threads block_scan_in_place is written for.
constexpr uint32_t JR_BLOCK = 256, JR_SCAN_BLOCK = 1024;
static_assert(JR_CHUNK_ROWS % JR_BLOCK == 0 && JR_CHUNK_ROWS == JR_SCAN_BLOCK && JR_BLOCK % 64 == 0, "a chunk is whole trips of whole waves");

struct JrAtomics {
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void or32(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct JrGroup : WgGroup {
    JrAtomics agent;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // (as parents.hip's: the maximum over the lanes up to and including this one; begins with a barrier)
    __device__ __forceinline__ sj_u64 scan_max(sj_u64 v, sj_u64* total) const {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (int d = 1; d < 64; d <<= 1) {
            const sj_u64 o = __shfl_up(v, d);
            if (lane >= (uint32_t)d && o > v) v = o;
        }
        __syncthreads();
        if (lane == 63) s_wave[wave] = v;
        __syncthreads();
        sj_u64 t = 0;
        for (uint32_t i = 0; i < (blockDim.x >> 6); ++i) {
            const sj_u64 w = s_wave[i];
            if (i < wave && w > v) v = w;
            if (w > t) t = w;
        }
        *total = t;
        return v;
    }
};

__global__ __launch_bounds__(64) void k_join_clear(JrArgs a, sj_u64* __restrict__ ws, JrResult* __restrict__ res) {
    if (threadIdx.x == 0) jr_clear(a, ws, res);
}

__global__ __launch_bounds__(JR_BLOCK) void k_join_keys(JrArgs a, sj_u64* __restrict__ ws, JrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[JR_BLOCK / 64];
    __shared__ sj_u64 s_key[JR_CHUNK_ROWS];
    __shared__ uint8_t s_good[JR_CHUNK_ROWS];
    const JrGroup g = {{s_wave}, {}};
    jr_keys(g, a, blockIdx.x, ws, s_key, s_good, res);
}

__global__ __launch_bounds__(JR_BLOCK) void k_join_count(JrArgs a, sj_u64* __restrict__ ws, JrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[JR_BLOCK / 64];
    __shared__ sj_u64 s_pivots[JR_CHUNK_ROWS];
    const JrGroup g = {{s_wave}, {}};
    jr_count(g, a, blockIdx.x, ws, s_pivots, res);
}

__global__ __launch_bounds__(JR_SCAN_BLOCK) void k_join_scan(JrArgs a, sj_u64* __restrict__ ws, JrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[JR_SCAN_BLOCK / 64];
    const JrGroup g = {{s_wave}, {}};
    jr_scan(g, a, ws, res);
}

__global__ __launch_bounds__(JR_SCAN_BLOCK) void k_join_offsets(JrArgs a, sj_u64* __restrict__ ws) {
    __shared__ unsigned long long s_wave[JR_SCAN_BLOCK / 64];
    const JrGroup g = {{s_wave}, {}};
    jr_offsets(g, a, blockIdx.x, ws);
}

__global__ __launch_bounds__(JR_BLOCK) void k_join_emit(JrArgs a, sj_u64* __restrict__ ws, const JrResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[JR_BLOCK / 64];
    __shared__ sj_u64 s_marks[JR_CHUNK_ROWS];
    __shared__ sj_u64 s_seeds[2];
    const JrGroup g = {{s_wave}, {}};
    jr_emit(g, a, blockIdx.x, ws, s_marks, s_seeds, res);
}

SrColumn side_column(const sjmi_join_side& s, const void* rows_in, uint64_t n_rows, const void* row_count) {
    return {(const uint8_t*)s.d_key_types, (const sj_u64*)s.d_key_validity, (const sj_u64*)s.d_key_values, s.n_source_rows,
            (const sj_u64*)rows_in, n_rows, (const sj_u64*)row_count, SR_LONG, 0u, JR_CHUNK_ROWS, SR_TILE_ROWS};
}

}  // namespace

size_t joinrows_workspace_bytes(uint64_t n_left, uint64_t n_right) { return (size_t)jr_workspace_words(n_left, n_right, JR_CHUNK_ROWS) * sizeof(sj_u64); }

hipError_t joinrows_launch(const sjmi_join_side& left, const void* d_left_rows_in, uint64_t n_left, const void* d_left_count,
                           const sjmi_join_side& right, const void* d_right_order, uint64_t n_right, const void* d_right_sort_result,
                           uint32_t how, uint64_t pair_capacity, void* d_left_rows, void* d_right_rows, void* d_left_out_types,
                           void* d_left_out_values, void* d_right_out_types, void* d_right_out_values, uint64_t out_stride,
                           void* d_pair_offsets, void* d_result, void* d_ws, hipStream_t stream) {
    if (n_left >= (1ull << 32) || n_right >= (1ull << 32) || left.n_source_rows >= (1ull << 32) || right.n_source_rows >= (1ull << 32) ||
        pair_capacity >= JR_MAX_PAIR_CAPACITY || how > JR_ANTI || (n_right && (!d_right_order || !d_right_sort_result)))
        return hipErrorInvalidValue;
    // (the live build places are min(n_right, the sort record's n_candidates): its second word)
    const void* n_candidates = n_right ? (const void*)((const sj_u64*)d_right_sort_result + 1) : nullptr;
    const JrArgs a = {side_column(left, d_left_rows_in, n_left, d_left_count),
                      side_column(right, d_right_order, n_right, n_candidates),
                      {(const uint8_t*)left.d_types, (const sj_u64*)left.d_values, left.n_cols, left.col_stride},
                      {(const uint8_t*)right.d_types, (const sj_u64*)right.d_values, right.n_cols, right.col_stride},
                      how,
                      JR_CHUNK_ROWS,
                      pair_capacity,
                      (sj_u64*)d_left_rows,
                      (sj_u64*)d_right_rows,
                      (uint8_t*)d_left_out_types,
                      (sj_u64*)d_left_out_values,
                      (uint8_t*)d_right_out_types,
                      (sj_u64*)d_right_out_values,
                      out_stride,
                      (sj_u64*)d_pair_offsets};
    const unsigned left_chunks = (unsigned)jr_chunks(n_left, JR_CHUNK_ROWS), build_chunks = (unsigned)jr_chunks(n_right, JR_CHUNK_ROWS),
                   pair_chunks = (unsigned)jr_chunks(pair_capacity, JR_CHUNK_ROWS);
    sj_u64* ws = (sj_u64*)d_ws;
    JrResult* res = (JrResult*)d_result;
    hipLaunchKernelGGL(k_join_clear, dim3(1), dim3(64), 0, stream, a, ws, res);
    if (build_chunks) hipLaunchKernelGGL(k_join_keys, dim3(build_chunks), dim3(JR_BLOCK), 0, stream, a, ws, res);
    if (!left_chunks) return hipGetLastError();  // (no left position: no pair, and the record is complete)
    hipLaunchKernelGGL(k_join_count, dim3(left_chunks), dim3(JR_BLOCK), 0, stream, a, ws, res);
    hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(JR_SCAN_BLOCK), 0, stream, a, ws, res);
    hipLaunchKernelGGL(k_join_offsets, dim3(left_chunks), dim3(JR_SCAN_BLOCK), 0, stream, a, ws);
    if (pair_chunks) hipLaunchKernelGGL(k_join_emit, dim3(pair_chunks), dim3(JR_BLOCK), 0, stream, a, ws, res);
    return hipGetLastError();
}

}  // namespace sjmi
