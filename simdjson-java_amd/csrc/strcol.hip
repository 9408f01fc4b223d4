// strcol.hip -- one string column of the selector's encoding gathered into Arrow offsets, validity and bytes (include/sjmi.h,
// sjmi_string_column_device).  The passes are sj_strcol.h (shared with the host simulation, tests/host_sim/
// strcol_sim.cpp), the device forms of its lane groups are WgGroup and WaveGroup of sj_group.h; this file is four plain kernels
// that the stream orders -- no workgroup waits for another:
//   k_strcol_chunk_sums   one workgroup per 1024 rows: the bytes, the VALID rows and the other-typed rows of the chunk; the
//                         validity words (a wave is 64 consecutive rows: its ballot is one word)
//   k_strcol_chunk_scan   ONE workgroup: the bytes in front of every chunk (in place), offsets[n_rows], the result record
//   k_strcol_offsets      one workgroup per chunk: offsets[r]
//   k_strcol_copy         one wave per 64 rows: the bytes (not launched by a sizing call)
// The scans are block_excl_scan / block_scan_in_place of sj_chain.h, as in walk.hip and explode.hip.
#include <hip/hip_runtime.h>

#include "sj_group.h"
#include "sj_strcol.h"
#include "stage1.h"

static_assert(SC_OVERFLOW == SJMI_STRCOL_OVERFLOW, "sj_strcol.h restates the flag");
static_assert(sizeof(ScResult) == sizeof(sjmi_strcol_result) && sizeof(ScResult) == 32, "the result record is 32 bytes");

namespace sjmi {

namespace {

constexpr uint32_t SC_COPY_BLOCK = 256;  // four waves = 256 rows per workgroup of the copy
static_assert(SC_CHUNK_ROWS == 1024, "block_scan_in_place takes slices of 1024 entries with 1024 threads");

__global__ __launch_bounds__(SC_CHUNK_ROWS) void k_strcol_chunk_sums(ScColumn c, sj_u64* __restrict__ validity, ScSums sums) {
    __shared__ unsigned long long s_wave[SC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    sc_chunk_sums(g, c, blockIdx.x, validity, sums);
}

__global__ __launch_bounds__(1024) void k_strcol_chunk_scan(ScSums sums, uint64_t nchunks, uint64_t n_rows, sj_u64* __restrict__ offsets,
                                                            uint64_t byte_capacity, ScResult* __restrict__ res) {
    __shared__ unsigned long long s_wave[16];
    const WgGroup g = {s_wave};
    sc_chunk_scan(g, sums, nchunks, n_rows, offsets, byte_capacity, res);
}

__global__ __launch_bounds__(SC_CHUNK_ROWS) void k_strcol_offsets(ScColumn c, ScSums sums, sj_u64* __restrict__ offsets) {
    __shared__ unsigned long long s_wave[SC_CHUNK_ROWS / 64];
    const WgGroup g = {s_wave};
    sc_offsets(g, c, blockIdx.x, sums, offsets);
}

__global__ __launch_bounds__(SC_COPY_BLOCK) void k_strcol_copy(ScColumn c, uint64_t nwaves, const sj_u64* __restrict__ offsets,
                                                               const uint8_t* __restrict__ sb, uint8_t* __restrict__ bytes,
                                                               uint64_t byte_capacity) {
    __shared__ ScWave s_waves[SC_COPY_BLOCK / 64];
    const uint64_t wave = (uint64_t)blockIdx.x * (SC_COPY_BLOCK / 64) + (threadIdx.x >> 6);
    if (wave >= nwaves) return;  // (wave-uniform; the kernel has no workgroup barrier)
    const WaveGroup w;
    sc_copy_wave(w, c, wave, offsets, sb, bytes, byte_capacity, s_waves[threadIdx.x >> 6]);
}

}  // namespace

size_t strcol_workspace_bytes(uint64_t n_rows) {
    return (size_t)(3 * ((n_rows + SC_CHUNK_ROWS - 1) / SC_CHUNK_ROWS) + 1) * sizeof(sj_u64);  // bytes | valid | other per chunk
}

hipError_t strcol_launch(const void* d_types, const void* d_values, uint64_t n_rows, const void* d_string_buffer, void* d_offsets,
                         void* d_validity, void* d_bytes, uint64_t byte_capacity, void* d_result, void* d_ws, hipStream_t stream) {
    const ScColumn c = {(const uint8_t*)d_types, (const sj_u64*)d_values, n_rows, SC_CHUNK_ROWS};
    const uint64_t nchunks = sc_chunks(c), nwaves = (n_rows + 63) / 64;
    const uint64_t copy_grid = (nwaves + SC_COPY_BLOCK / 64 - 1) / (SC_COPY_BLOCK / 64);
    if (nchunks > 0x7FFFFFFFull || copy_grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const ScSums sums = sc_sums(d_ws, nchunks);
    if (nchunks)
        hipLaunchKernelGGL(k_strcol_chunk_sums, dim3((unsigned)nchunks), dim3(SC_CHUNK_ROWS), 0, stream, c, (sj_u64*)d_validity, sums);
    hipLaunchKernelGGL(k_strcol_chunk_scan, dim3(1), dim3(1024), 0, stream, sums, nchunks, n_rows, (sj_u64*)d_offsets, byte_capacity,
                       (ScResult*)d_result);
    if (nchunks) hipLaunchKernelGGL(k_strcol_offsets, dim3((unsigned)nchunks), dim3(SC_CHUNK_ROWS), 0, stream, c, sums, (sj_u64*)d_offsets);
    if (nchunks && byte_capacity)  // (the sizing call does not copy)
        hipLaunchKernelGGL(k_strcol_copy, dim3((unsigned)copy_grid), dim3(SC_COPY_BLOCK), 0, stream, c, nwaves, (const sj_u64*)d_offsets,
                           (const uint8_t*)d_string_buffer, (uint8_t*)d_bytes, byte_capacity);
    return hipGetLastError();
}

}  // namespace sjmi
