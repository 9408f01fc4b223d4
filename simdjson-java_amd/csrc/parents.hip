// parents.hip -- the document of every exploded row and that document's cells on the row (include/sjmi.h,
// sjmi_parent_columns_device).  The passes are sj_parents.h (shared with the host simulation,
// tests/host_sim/parents_sim.cpp); the device form of their lane group is WgGroup of sj_group.h, to which this file adds the
// agent-scope relaxed add on the record (the XCDs' L2s are not coherent, DESIGN.md 4.15 "visibility"), the barrier and the
// inclusive running maximum over the workgroup (six exchanges in the wave, then one LDS entry per wave).  Plain kernels that the
// stream orders -- no workgroup waits for another, nothing spins:
//   k_parent_clear    one lane: the record with n_rows = live, n_orphans = 0
//   k_parent_dense    one workgroup of 256 lanes per 1024 rows: two 64-ary searches, the span's document starts into LDS, then four
//                     trips of a running maximum, the parents and the carried cells
//   k_parent_sparse   one workgroup per 256 slots: a binary search per lane, the parents and the carried cells
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows.
#include <hip/hip_runtime.h>

#include "sj_parents.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(PA_MAX_COLS == SJMI_PARENT_MAX_COLS && PA_RESULT_WORDS == SJMI_PARENT_RESULT_WORDS, "sj_parents.h restates the constants");
static_assert(sizeof(PaResult) == sizeof(sjmi_parent_result) && sizeof(PaResult) == 24, "the result record is three words");

namespace sjmi {

namespace {

// A workgroup is four waves, whatever its chunk: what a chunk costs is a chain of dependent loads (the search's rounds, the span's
// offsets, the parents' cells), and seven such workgroups share a CU where one of 1024 lanes would hold it alone (106 SGPRs:
// seven waves per SIMD).  A dense chunk is PA_CHUNK_ROWS rows in four trips of the lanes, a sparse one a slot per lane.
constexpr uint32_t PA_BLOCK = 256, PA_SPARSE_ROWS = PA_BLOCK;
static_assert(PA_CHUNK_ROWS % PA_BLOCK == 0 && PA_BLOCK % 64 == 0, "a chunk is whole trips of whole waves");

struct PaAtomics {
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

struct PaGroup : WgGroup {
    PaAtomics agent;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // a value of every lane -> the maximum over the lanes up to and including this one; *total = over all.  Begins with a barrier,
    // as the scans do: s_wave is free by then.
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

__global__ __launch_bounds__(64) void k_parent_clear(PaArgs a, PaResult* __restrict__ res) {
    if (threadIdx.x == 0) pa_clear(a, res);
}

__global__ __launch_bounds__(PA_BLOCK) void k_parent_dense(PaArgs a, PaResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[PA_BLOCK / 64];
    __shared__ sj_u64 s_marks[PA_CHUNK_ROWS];
    __shared__ sj_u64 s_seeds[2];
    const PaGroup g = {{s_wave}, {}};
    pa_dense(g, a, blockIdx.x, s_marks, s_seeds, res);
}

__global__ __launch_bounds__(PA_BLOCK) void k_parent_sparse(PaArgs a, PaResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[PA_BLOCK / 64];
    const PaGroup g = {{s_wave}, {}};
    pa_sparse(g, a, blockIdx.x, res);
}

}  // namespace

hipError_t parents_launch(const void* d_row_offsets, uint64_t n_docs, const void* d_rows, uint64_t n_rows, const void* d_row_count,
                          const void* d_types, const void* d_values, uint64_t n_cols, uint64_t col_stride, void* d_parent_types, void* d_parents,
                          void* d_out_types, void* d_out_values, uint64_t out_stride, void* d_result, hipStream_t stream) {
    const PaArgs a = {(const sj_u64*)d_row_offsets, n_docs, (const sj_u64*)d_rows, n_rows, (const sj_u64*)d_row_count, (const uint8_t*)d_types,
                      (const sj_u64*)d_values, n_cols, col_stride, (uint8_t*)d_parent_types, (sj_u64*)d_parents, (uint8_t*)d_out_types,
                      (sj_u64*)d_out_values, out_stride, d_rows ? PA_SPARSE_ROWS : PA_CHUNK_ROWS};
    const uint64_t nchunks = pa_chunks(a);
    if (nchunks > 0x7FFFFFFFull || n_docs >= (1ull << 32) || n_cols > PA_MAX_COLS) return hipErrorInvalidValue;
    PaResult* res = (PaResult*)d_result;
    hipLaunchKernelGGL(k_parent_clear, dim3(1), dim3(64), 0, stream, a, res);
    if (!nchunks) return hipGetLastError();  // (no row: the record is complete)
    if (d_rows)
        hipLaunchKernelGGL(k_parent_sparse, dim3((unsigned)nchunks), dim3(PA_BLOCK), 0, stream, a, res);
    else
        hipLaunchKernelGGL(k_parent_dense, dim3((unsigned)nchunks), dim3(PA_BLOCK), 0, stream, a, res);
    return hipGetLastError();
}

}  // namespace sjmi
