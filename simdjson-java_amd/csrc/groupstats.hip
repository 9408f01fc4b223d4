// groupstats.hip -- group statistics per dictionary key: count, sum, min, max (include/sjmi.h, sjmi_group_stats_device; DESIGN.md
// 4.17).  The passes are sj_groupstats.h (shared with the host simulation, tests/host_sim/groupstats_sim.cpp); the device form of
// their lane group is WgGroup of sj_group.h, to which this file adds the two sets of atomics -- g.wg on the workgroup's LDS bins,
// g.agent on the stats (agent scope: the XCDs' L2s are not coherent, DESIGN.md 4.15 "visibility") --, the barrier and the combine
// of a wave's equal keys.  All relaxed, results unused: integer adds, a double add, signed and unsigned 64-bit minima and maxima,
// each one instruction on gfx950 (no compare-and-swap loop).  Plain kernels that the stream orders -- no workgroup waits for
// another, nothing spins, the context holds no state:
//   k_group_clear     the stats' words to their identities, the record with n_rows = live
//   k_group_lds       n_keys <= SJMI_GROUP_LDS_KEYS: a capped grid, a workgroup gathers its chunks into 68 bytes of LDS bins per
//                     key and sends the words of the keys it touched to the stats once
//   k_group_global    larger n_keys: one workgroup per 1024 rows, equal keys of a wave combined, then atomics straight into the
//                     stats
//   k_group_finish    per key: the 128-bit sum from its two halves, the doubles' ordered keys back to bits, the empty groups
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows.
#include <hip/hip_runtime.h>

#include "sj_groupstats.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(GS_WORDS == SJMI_GROUP_STATS_WORDS && GS_LDS_KEYS == SJMI_GROUP_LDS_KEYS, "sj_groupstats.h restates the constants");
static_assert(sizeof(GsResult) == sizeof(sjmi_group_result) && sizeof(GsResult) == 40, "the result record is 40 bytes");

namespace sjmi {

namespace {

constexpr uint32_t GS_SMALL_BLOCK = 256;  // threads of k_group_clear and k_group_finish

template <int SCOPE>
struct GsAtomics {
    __device__ __forceinline__ void add32(uint32_t* p, uint32_t n) const { (void)__hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void add64(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void addf(sj_u64* p, double x) const { (void)__hip_atomic_fetch_add((double*)p, x, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void smin(sj_u64* p, sj_i64 v) const { (void)__hip_atomic_fetch_min((sj_i64*)p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void smax(sj_u64* p, sj_i64 v) const { (void)__hip_atomic_fetch_max((sj_i64*)p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void umin(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void umax(sj_u64* p, sj_u64 v) const { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE); }
};

// a value of every lane of the wave -> their sum / minimum / maximum, in every lane (a butterfly: six exchanges)
template <class T, class F>
__device__ __forceinline__ T wave_all(T v, F f) {
    for (int d = 1; d < 64; d <<= 1) v = f(v, __shfl_xor(v, d));
    return v;
}

struct GsGroup : WgGroup {
    GsAtomics<__HIP_MEMORY_SCOPE_WORKGROUP> wg;
    GsAtomics<__HIP_MEMORY_SCOPE_AGENT> agent;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    // The wave's active lanes in sets of equal keys, lowest lane first, as the census's merge takes them: the lowest lane of a set
    // takes the set's combined cell and returns true, the set's other lanes return false; an active lane that is in none of the
    // first GS_MERGE_ROUNDS sets keeps its own cell.  `todo`, `same` and the two class ballots are the same in every lane, so
    // every branch around an exchange is taken by the whole wave.  A set of one lane (the common case where the keys are many)
    // costs no exchange; only the classes the set has are reduced, the lanes outside the set giving the identities.
    __device__ __forceinline__ bool merge(uint32_t key, bool active, GsCell* cell) const {
        const uint32_t lane = threadIdx.x & 63u;
        unsigned long long todo = __ballot(active);
        bool mine = false;
        for (uint32_t round = 0; round < GS_MERGE_ROUNDS && todo; ++round) {
            const uint32_t leader = (uint32_t)__ffsll(todo) - 1u;
            const uint32_t k = (uint32_t)__shfl((int)key, (int)leader);
            const bool in_set = active && key == k;
            const unsigned long long same = __ballot(in_set);
            todo &= ~same;
            if (lane == leader) mine = true;
            if (!(same & (same - 1))) continue;  // (the leader alone: its cell as it is)
            const unsigned long long longs = __ballot(in_set && cell->n_long), doubles = __ballot(in_set && cell->n_double);
            const uint32_t n_other = (uint32_t)__popcll(same & ~longs & ~doubles);
            const GsCell none = gs_empty_cell();
            GsCell set = none;
            set.n_long = (uint32_t)__popcll(longs), set.n_double = (uint32_t)__popcll(doubles), set.n_other = n_other;
            if (longs) {
                set.lo = wave_all(in_set ? cell->lo : none.lo, [](sj_u64 a, sj_u64 b) { return a + b; });
                set.hi = wave_all(in_set ? cell->hi : none.hi, [](sj_i64 a, sj_i64 b) { return a + b; });
                set.min_long = wave_all(in_set ? cell->min_long : none.min_long, [](sj_i64 a, sj_i64 b) { return a < b ? a : b; });
                set.max_long = wave_all(in_set ? cell->max_long : none.max_long, [](sj_i64 a, sj_i64 b) { return a > b ? a : b; });
            }
            if (doubles) {
                set.dsum = wave_all(in_set ? cell->dsum : none.dsum, [](double a, double b) { return a + b; });
                set.min_key = wave_all(in_set ? cell->min_key : none.min_key, [](sj_u64 a, sj_u64 b) { return a < b ? a : b; });
                set.max_key = wave_all(in_set ? cell->max_key : none.max_key, [](sj_u64 a, sj_u64 b) { return a > b ? a : b; });
            }
            if (lane == leader) *cell = set;
        }
        return mine || ((todo >> lane) & 1ull);
    }
};

__global__ __launch_bounds__(GS_SMALL_BLOCK) void k_group_clear(GsColumn c, sj_u64* __restrict__ stats, GsResult* __restrict__ res) {
    gs_clear_word(c, (sj_u64)blockIdx.x * GS_SMALL_BLOCK + threadIdx.x, stats, res);
}

__global__ __launch_bounds__(GS_CHUNK_ROWS) void k_group_lds(GsColumn c, sj_u64* __restrict__ stats, GsResult* __restrict__ res) {
    extern __shared__ sj_u64 s_words[];  // n_keys * GS_BIN_WORDS, and behind them n_keys * 3 32-bit counts
    __shared__ unsigned long long s_wave[GS_CHUNK_ROWS / 64];
    const GsGroup g = {{s_wave}, {}, {}};
    gs_lds_rows(g, c, blockIdx.x, gridDim.x, s_words, (uint32_t*)(s_words + c.n_keys * GS_BIN_WORDS), stats, res);
}

__global__ __launch_bounds__(GS_CHUNK_ROWS) void k_group_global(GsColumn c, sj_u64* __restrict__ stats, GsResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[GS_CHUNK_ROWS / 64];
    const GsGroup g = {{s_wave}, {}, {}};
    gs_global_rows(g, c, blockIdx.x, stats, res);
}

__global__ __launch_bounds__(GS_SMALL_BLOCK) void k_group_finish(GsColumn c, sj_u64* __restrict__ stats) {
    gs_finish_key(c, (sj_u64)blockIdx.x * GS_SMALL_BLOCK + threadIdx.x, stats);
}

}  // namespace

hipError_t groupstats_launch(const void* d_indices, const void* d_validity, const void* d_types, const void* d_values, uint64_t n_rows,
                             const void* d_row_count, uint64_t n_keys, void* d_stats, void* d_result, hipStream_t stream) {
    const GsColumn c = {(const int32_t*)d_indices, (const sj_u64*)d_validity, (const uint8_t*)d_types, (const sj_u64*)d_values, n_rows,
                        (const sj_u64*)d_row_count, n_keys, GS_CHUNK_ROWS};
    const uint64_t words = n_keys * GS_WORDS;
    const uint64_t clear_grid = words ? (words + GS_SMALL_BLOCK - 1) / GS_SMALL_BLOCK : 1;  // (the record's lane at least)
    const uint64_t nchunks = gs_chunks(n_rows, GS_CHUNK_ROWS);
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_clear, dim3((unsigned)clear_grid), dim3(GS_SMALL_BLOCK), 0, stream, c, (sj_u64*)d_stats, (GsResult*)d_result);
    if (nchunks && n_keys <= GS_LDS_KEYS)
        hipLaunchKernelGGL(k_group_lds, dim3(gs_lds_grid(n_rows, n_keys, GS_CHUNK_ROWS)), dim3(GS_CHUNK_ROWS), n_keys * GS_BIN_BYTES, stream, c,
                           (sj_u64*)d_stats, (GsResult*)d_result);
    else if (nchunks)
        hipLaunchKernelGGL(k_group_global, dim3((unsigned)nchunks), dim3(GS_CHUNK_ROWS), 0, stream, c, (sj_u64*)d_stats, (GsResult*)d_result);
    if (n_keys)
        hipLaunchKernelGGL(k_group_finish, dim3((unsigned)((n_keys + GS_SMALL_BLOCK - 1) / GS_SMALL_BLOCK)), dim3(GS_SMALL_BLOCK), 0, stream, c,
                           (sj_u64*)d_stats);
    return hipGetLastError();
}

}  // namespace sjmi
