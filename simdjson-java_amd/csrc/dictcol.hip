// dictcol.hip -- one string column of the selector's encoding dictionary-encoded into Arrow's dictionary shape: int32 indices,
// validity, and the dictionary in the order of first occurrence (include/sjmi.h, sjmi_dictionary_column_device).
// The passes are sj_dictcol.h and, for the dictionary's offsets and bytes, sj_strcol.h (both shared with the host simulation,
// tests/host_sim/dictcol_sim.cpp); the device form of their lane group is WgGroup of sj_group.h, to which this file adds the
// three table operations as agent-scope relaxed atomics (the XCDs' L2s are not coherent: DESIGN.md 4.15, "visibility").  Ten
// plain kernels that the stream orders -- no workgroup waits for another, nothing spins:
//   k_dict_clear        the table's words to all ones
//   k_dict_insert       one workgroup per 1024 rows, one row per lane: hash, probe, claim or find the value's slot, shrink its
//                       FIRST; the validity words, slot_of_row, the chunk's counts.  The ONLY kernel with atomics
//   k_dict_count        one workgroup per chunk: its first rows
//   k_dict_scan         ONE workgroup: the first rows in front of every chunk, the record, the dictionary's row count
//   k_dict_emit         one workgroup per chunk: ranks into the slots, dict_rows, the compacted column
//   k_dict_index        one workgroup per chunk: the indices
//   k_dict_str_sums / k_dict_str_scan / k_dict_str_offsets / k_dict_str_copy
//                       strcol.hip's four kernels over the compacted column, its row count read on the device; their grids are
//                       sized by dict_capacity, the copy is not launched by a sizing call
// Where the caller gives a row count in device memory the kernels read it there: the grids are sized by n_rows, and a workgroup
// whose chunk begins at or above the live rows leaves at once.
#include <hip/hip_runtime.h>

#include "sj_dictcol.h"
#include "sj_group.h"
#include "stage1.h"

static_assert(DC_OVERFLOW == SJMI_DICT_OVERFLOW && DC_BYTES_OVERFLOW == SJMI_DICT_BYTES_OVERFLOW && DC_MAX_ENTRIES == SJMI_DICT_MAX_ENTRIES,
              "sj_dictcol.h restates the flags and the limit");
static_assert(sizeof(DcResult) == sizeof(sjmi_dict_result) && sizeof(DcResult) == 48, "the result record is 48 bytes");
static_assert(DC_CHUNK_ROWS == 1024 && SC_CHUNK_ROWS == 1024, "block_scan_in_place takes slices of 1024 entries with 1024 threads");

namespace sjmi {

namespace {

constexpr uint32_t DC_CLEAR_BLOCK = 256;
constexpr uint32_t DC_COPY_BLOCK = 256;  // four waves = 256 entries per workgroup of the copy

// the workgroup (sj_group.h) with the table operations: every access of the insert kernel to a table word goes through these
struct DcGroup : WgGroup {
    __device__ __forceinline__ sj_u64 load(const sj_u64* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ sj_u64 cas(sj_u64* p, sj_u64 expected, sj_u64 desired) const {
        (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;  // what the word held
    }
    __device__ __forceinline__ sj_u64 fetch_min(sj_u64* p, sj_u64 v) const {
        return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__global__ __launch_bounds__(DC_CLEAR_BLOCK) void k_dict_clear(DcTable t) {
    const sj_u64 i = 2 * ((sj_u64)blockIdx.x * DC_CLEAR_BLOCK + threadIdx.x);
    dc_clear_word(t, i);
    dc_clear_word(t, i + 1);
}

__global__ __launch_bounds__(DC_CHUNK_ROWS) void k_dict_insert(DcColumn c, DcTable t, sj_u64* __restrict__ validity,
                                                               uint32_t* __restrict__ slot_of_row, sj_u64* __restrict__ counts) {
    __shared__ unsigned long long s_wave[DC_CHUNK_ROWS / 64];
    const DcGroup g = {{s_wave}};
    dc_insert_chunk(g, c, t, blockIdx.x, validity, slot_of_row, counts);
}

__global__ __launch_bounds__(DC_CHUNK_ROWS) void k_dict_count(DcColumn c, DcTable t, const uint32_t* __restrict__ slot_of_row,
                                                              sj_u64* __restrict__ firsts) {
    __shared__ unsigned long long s_wave[DC_CHUNK_ROWS / 64];
    const DcGroup g = {{s_wave}};
    dc_count_chunk(g, c, t, blockIdx.x, slot_of_row, firsts);
}

__global__ __launch_bounds__(1024) void k_dict_scan(DcColumn c, const sj_u64* __restrict__ counts, sj_u64* __restrict__ firsts,
                                                    uint64_t dict_capacity, sj_u64* __restrict__ dict_n, DcResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[16];
    const DcGroup g = {{s_wave}};
    dc_scan(g, c, counts, firsts, dict_capacity, dict_n, res);
}

__global__ __launch_bounds__(DC_CHUNK_ROWS) void k_dict_emit(DcColumn c, DcTable t, const uint32_t* __restrict__ slot_of_row,
                                                             const sj_u64* __restrict__ firsts, uint64_t dict_capacity,
                                                             sj_u64* __restrict__ dict_rows, uint8_t* __restrict__ ctypes,
                                                             sj_u64* __restrict__ cvalues) {
    __shared__ unsigned long long s_wave[DC_CHUNK_ROWS / 64];
    const DcGroup g = {{s_wave}};
    dc_emit_chunk(g, c, t, blockIdx.x, slot_of_row, firsts, dict_capacity, dict_rows, ctypes, cvalues);
}

__global__ __launch_bounds__(DC_CHUNK_ROWS) void k_dict_index(DcColumn c, DcTable t, const uint32_t* __restrict__ slot_of_row,
                                                              int32_t* __restrict__ indices) {
    const DcGroup g = {{nullptr}};
    dc_index_chunk(g, c, t, blockIdx.x, slot_of_row, indices);
}

__global__ __launch_bounds__(SC_CHUNK_ROWS) void k_dict_str_sums(const uint8_t* __restrict__ ctypes, const sj_u64* __restrict__ cvalues,
                                                                 const sj_u64* __restrict__ dict_n, ScSums sums) {
    __shared__ unsigned long long s_wave[SC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    sc_chunk_sums(g, dc_dict_column(ctypes, cvalues, dict_n), blockIdx.x, nullptr, sums);
}

__global__ __launch_bounds__(1024) void k_dict_str_scan(ScSums sums, uint64_t nchunks, const sj_u64* __restrict__ dict_n,
                                                        sj_u64* __restrict__ dict_offsets, uint64_t byte_capacity, DcResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[16];
    const WgGroup g = {s_wave};
    dc_dict_scan(g, sums, nchunks, *dict_n, dict_offsets, byte_capacity, res);
}

__global__ __launch_bounds__(SC_CHUNK_ROWS) void k_dict_str_offsets(const uint8_t* __restrict__ ctypes, const sj_u64* __restrict__ cvalues,
                                                                    const sj_u64* __restrict__ dict_n, ScSums sums, sj_u64* __restrict__ dict_offsets) {
    __shared__ unsigned long long s_wave[SC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    sc_offsets(g, dc_dict_column(ctypes, cvalues, dict_n), blockIdx.x, sums, dict_offsets);
}

__global__ __launch_bounds__(DC_COPY_BLOCK) void k_dict_str_copy(const uint8_t* __restrict__ ctypes, const sj_u64* __restrict__ cvalues,
                                                                 const sj_u64* __restrict__ dict_n, const sj_u64* __restrict__ dict_offsets,
                                                                 const uint8_t* __restrict__ sb, uint8_t* __restrict__ bytes, uint64_t byte_capacity) {
    __shared__ ScWave s_waves[DC_COPY_BLOCK / 64];
    const ScColumn c = dc_dict_column(ctypes, cvalues, dict_n);
    const uint64_t wave = (uint64_t)blockIdx.x * (DC_COPY_BLOCK / 64) + (threadIdx.x >> 6);
    if (wave >= (c.n_rows + 63) / 64) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const WaveGroup w;
    sc_copy_wave(w, c, wave, dict_offsets, sb, bytes, byte_capacity, s_waves[threadIdx.x >> 6]);
}

}  // namespace

size_t dictcol_workspace_bytes(uint64_t n_rows, uint64_t dict_capacity) {
    return (size_t)dc_scratch_words(n_rows, dict_capacity, DC_CHUNK_ROWS) * sizeof(sj_u64);
}

hipError_t dictcol_launch(const void* d_types, const void* d_values, uint64_t n_rows, const void* d_row_count, const void* d_string_buffer,
                          void* d_indices, void* d_validity, uint64_t dict_capacity, void* d_dict_rows, void* d_dict_offsets, void* d_dict_bytes,
                          uint64_t dict_byte_capacity, void* d_result, void* d_ws, hipStream_t stream) {
    const DcColumn c = {(const uint8_t*)d_types, (const sj_u64*)d_values, n_rows, (const sj_u64*)d_row_count, (const uint8_t*)d_string_buffer,
                        DC_CHUNK_ROWS};
    const DcScratch s = dc_scratch(d_ws, n_rows, dict_capacity, DC_CHUNK_ROWS);
    const uint64_t nchunks = dc_chunks(n_rows, DC_CHUNK_ROWS);
    const uint64_t dchunks = dc_chunks(dict_capacity, SC_CHUNK_ROWS), dwaves = (dict_capacity + 63) / 64;
    const uint64_t copy_grid = (dwaves + DC_COPY_BLOCK / 64 - 1) / (DC_COPY_BLOCK / 64);
    const uint64_t clear_grid = (s.table.slots + DC_CLEAR_BLOCK - 1) / DC_CLEAR_BLOCK;  // two words per thread
    if (nchunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 rows((unsigned)nchunks), wg(DC_CHUNK_ROWS);
    const ScSums sums = sc_sums(s.sums, dchunks);
    if (nchunks) {
        hipLaunchKernelGGL(k_dict_clear, dim3((unsigned)clear_grid), dim3(DC_CLEAR_BLOCK), 0, stream, s.table);
        hipLaunchKernelGGL(k_dict_insert, rows, wg, 0, stream, c, s.table, (sj_u64*)d_validity, s.slot_of_row, s.counts);
        hipLaunchKernelGGL(k_dict_count, rows, wg, 0, stream, c, s.table, (const uint32_t*)s.slot_of_row, s.firsts);
    }
    hipLaunchKernelGGL(k_dict_scan, dim3(1), dim3(1024), 0, stream, c, (const sj_u64*)s.counts, s.firsts, dict_capacity, s.dict_n, (DcResult*)d_result);
    if (nchunks) {
        hipLaunchKernelGGL(k_dict_emit, rows, wg, 0, stream, c, s.table, (const uint32_t*)s.slot_of_row, (const sj_u64*)s.firsts, dict_capacity,
                           (sj_u64*)d_dict_rows, s.ctypes, s.cvalues);
        hipLaunchKernelGGL(k_dict_index, rows, wg, 0, stream, c, s.table, (const uint32_t*)s.slot_of_row, (int32_t*)d_indices);
    }
    if (nchunks && dchunks)
        hipLaunchKernelGGL(k_dict_str_sums, dim3((unsigned)dchunks), dim3(SC_CHUNK_ROWS), 0, stream, (const uint8_t*)s.ctypes, (const sj_u64*)s.cvalues,
                           (const sj_u64*)s.dict_n, sums);
    // (without rows nothing wrote the sums: the scan then takes no chunk, and dict_offsets[0] = 0)
    hipLaunchKernelGGL(k_dict_str_scan, dim3(1), dim3(1024), 0, stream, sums, nchunks ? dchunks : 0, (const sj_u64*)s.dict_n, (sj_u64*)d_dict_offsets,
                       dict_byte_capacity, (DcResult*)d_result);
    if (nchunks && dchunks) {
        hipLaunchKernelGGL(k_dict_str_offsets, dim3((unsigned)dchunks), dim3(SC_CHUNK_ROWS), 0, stream, (const uint8_t*)s.ctypes, (const sj_u64*)s.cvalues,
                           (const sj_u64*)s.dict_n, sums, (sj_u64*)d_dict_offsets);
        if (dict_byte_capacity)  // (the sizing call does not copy)
            hipLaunchKernelGGL(k_dict_str_copy, dim3((unsigned)copy_grid), dim3(DC_COPY_BLOCK), 0, stream, (const uint8_t*)s.ctypes,
                               (const sj_u64*)s.cvalues, (const sj_u64*)s.dict_n, (const sj_u64*)d_dict_offsets, (const uint8_t*)d_string_buffer,
                               (uint8_t*)d_dict_bytes, dict_byte_capacity);
    }
    return hipGetLastError();
}

}  // namespace sjmi
