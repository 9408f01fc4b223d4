// census.hip -- the key census: rows per dictionary entry and value type (include/sjmi.h, sjmi_key_census_device).
// The passes are sj_census.h (shared with the host simulation, tests/host_sim/census_sim.cpp); the device form of their lane group
// is WgGroup of sj_group.h, to which this file adds the bin add (an LDS atomic), the 64-bit add (an agent-scope relaxed atomic:
// the XCDs' L2s are not coherent, DESIGN.md 4.15 "visibility"), the barrier and the merge of a wave's equal bins.  Two plain kernels that the stream orders -- no
// workgroup waits for another, nothing spins, the context holds no state:
//   k_census_clear    the counts' words to zero, the record with n_rows = live
//   k_census_lds      n_keys <= SJMI_CENSUS_LDS_KEYS: a capped grid, a workgroup counts its chunks into 32-bit LDS bins and adds
//                     its non-zero bins to the counts once
//   k_census_global   larger n_keys: one workgroup per 1024 rows, equal bins of a wave merged, then atomic adds straight into
//                     the counts
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows.
#include <hip/hip_runtime.h>

#include "sj_census.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(CS_CLASSES == SJMI_CENSUS_CLASSES && CS_LDS_KEYS == SJMI_CENSUS_LDS_KEYS, "sj_census.h restates the constants");
static_assert(sizeof(CsResult) == sizeof(sjmi_census_result) && sizeof(CsResult) == 32, "the result record is 32 bytes");
static_assert(CS_LDS_KEYS * CS_CLASSES * sizeof(uint32_t) + 16 * sizeof(unsigned long long) <= 64 * 1024, "the bins fit a workgroup's LDS");

namespace sjmi {

namespace {

constexpr uint32_t CS_CLEAR_BLOCK = 256;

struct CsGroup : WgGroup {
    __device__ __forceinline__ void bin_add(uint32_t* p) const { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // the wave's active lanes in sets of equal bins, lowest lane first: the lowest lane of a set takes the set's size, the others
    // 0; an active lane that is in none of the first CS_MERGE_ROUNDS sets keeps its own 1.  `todo` is the same in every lane.
    __device__ __forceinline__ uint32_t merge(uint32_t bin, bool active) const {
        const uint32_t lane = threadIdx.x & 63u;
        unsigned long long todo = __ballot(active);
        uint32_t n = 0;
        for (uint32_t round = 0; round < CS_MERGE_ROUNDS && todo; ++round) {
            const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;
            const uint32_t b = (uint32_t)__shfl((int)bin, (int)leader);
            const unsigned long long same = __ballot(active && bin == b);
            if (lane == leader) n = (uint32_t)__popcll(same);
            todo &= ~same;
        }
        if ((todo >> lane) & 1ull) n = 1;
        return n;
    }
};

__global__ __launch_bounds__(CS_CLEAR_BLOCK) void k_census_clear(CsColumn c, sj_u64* __restrict__ counts, CsResult* __restrict__ res) {
    cs_clear_word(c, (sj_u64)blockIdx.x * CS_CLEAR_BLOCK + threadIdx.x, counts, res);
}

__global__ __launch_bounds__(CS_CHUNK_ROWS) void k_census_lds(CsColumn c, sj_u64* __restrict__ counts, CsResult* __restrict__ res) {
    extern __shared__ uint32_t s_bins[];  // n_keys * CS_CLASSES
    __shared__ unsigned long long s_wave[CS_CHUNK_ROWS / 64];
    const CsGroup g = {{s_wave}};
    cs_lds_rows(g, c, blockIdx.x, gridDim.x, s_bins, counts, res);
}

__global__ __launch_bounds__(CS_CHUNK_ROWS) void k_census_global(CsColumn c, sj_u64* __restrict__ counts, CsResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[CS_CHUNK_ROWS / 64];
    const CsGroup g = {{s_wave}};
    cs_global_rows(g, c, blockIdx.x, counts, res);
}

}  // namespace

hipError_t census_launch(const void* d_indices, const void* d_validity, const void* d_types, uint64_t n_rows, const void* d_row_count,
                         uint64_t n_keys, void* d_counts, void* d_result, hipStream_t stream) {
    const CsColumn c = {(const int32_t*)d_indices, (const sj_u64*)d_validity, (const uint8_t*)d_types, n_rows, (const sj_u64*)d_row_count, n_keys,
                        CS_CHUNK_ROWS};
    const uint64_t words = n_keys * CS_CLASSES;
    const uint64_t clear_grid = words ? (words + CS_CLEAR_BLOCK - 1) / CS_CLEAR_BLOCK : 1;  // (the record's lane at least)
    const uint64_t nchunks = cs_chunks(n_rows, CS_CHUNK_ROWS);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_census_clear, dim3((unsigned)clear_grid), dim3(CS_CLEAR_BLOCK), 0, stream, c, (sj_u64*)d_counts, (CsResult*)d_result);
    if (nchunks && n_keys <= CS_LDS_KEYS)
        hipLaunchKernelGGL(k_census_lds, dim3(cs_lds_grid(n_rows, n_keys, CS_CHUNK_ROWS)), dim3(CS_CHUNK_ROWS), words * sizeof(uint32_t), stream, c,
                           (sj_u64*)d_counts, (CsResult*)d_result);
    else if (nchunks)
        hipLaunchKernelGGL(k_census_global, dim3((unsigned)nchunks), dim3(CS_CHUNK_ROWS), 0, stream, c, (sj_u64*)d_counts, (CsResult*)d_result);
    return hipGetLastError();
}

}  // namespace sjmi
