// ndjson.hip -- document offsets of a buffer of newline-delimited JSON, made on the device (include/sjmi.h, sjmi_ndjson_offsets*;
// DESIGN.md 4.10).  The passes are sj_ndjson.h (shared with the host simulation, tests/host_sim/ndjson_sim.cpp), the workgroup
// form of its lane group is WgGroup of sj_group.h; this file adds what is NdState's own to that group (the block load and the scan
// of the states) and is three plain kernels that the stream orders -- no workgroup waits for another:
//   k_ndjson_summary   one workgroup per 64 KiB tile: the tile's state and its starts
//   k_ndjson_scan      ONE workgroup: the states and the starts in front of every tile (in place), the result record
//   k_ndjson_emit      one workgroup per tile, reading the bytes a second time: doc_offsets[1 ..]
// The input is read twice at most; a call that only sizes (offset_capacity <= 1) reads it once.
#include <hip/hip_runtime.h>

#include "sj_group.h"
#include "sj_ndjson.h"
#include "stage1.h"

static_assert(ND_TAIL_BLANK == SJMI_NDJSON_TAIL_BLANK && ND_OVERFLOW == SJMI_NDJSON_OVERFLOW, "sj_ndjson.h restates the flags");
static_assert(sizeof(NdResult) == sizeof(sjmi_ndjson_result) && sizeof(NdResult) == 24, "the result record is 24 bytes");

namespace sjmi {

namespace {

constexpr uint32_t ND_BLOCK = 256;    // threads of a tile's workgroup: four steps of 256 blocks
constexpr uint32_t ND_SCAN = 1024;    // threads of the scan's workgroup

// the workgroup (sj_group.h) with what sj_ndjson.h asks besides: s_wave is the adder's LDS, s_state the states'
struct NdGroup : WgGroup {
    NdState* s_state;  // one entry per wave
    __device__ __forceinline__ void load(const uint8_t* p, uint32_t w[16]) const {
        const uint4* src = reinterpret_cast<const uint4*>(p);
        const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
        w[0] = q0.x, w[1] = q0.y, w[2] = q0.z, w[3] = q0.w;
        w[4] = q1.x, w[5] = q1.y, w[6] = q1.z, w[7] = q1.w;
        w[8] = q2.x, w[9] = q2.y, w[10] = q2.z, w[11] = q2.w;
        w[12] = q3.x, w[13] = q3.y, w[14] = q3.z, w[15] = q3.w;
    }
    // (begins with a barrier, like block_excl_scan: it may be called again without one in between)
    __device__ __forceinline__ NdState scan_state(NdState v, NdState* total) const {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
        NdState incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const NdState o = __shfl_up(incl, d);
            if (lane >= d) incl = nd_combine(o, incl);
        }
        NdState excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0;
        __syncthreads();
        if (lane == 63) s_state[wave] = incl;
        __syncthreads();
        NdState base = 0, t = 0;
        for (int i = 0; i < nw; ++i) {
            if (i < wave) base = nd_combine(base, s_state[i]);
            t = nd_combine(t, s_state[i]);
        }
        *total = t;
        return nd_combine(base, excl);
    }
};

__global__ __launch_bounds__(ND_BLOCK) void k_ndjson_summary(NdGeom ge, NdTile* __restrict__ tiles) {
    __shared__ NdState s_state[ND_BLOCK / 64];
    __shared__ unsigned long long s_add[ND_BLOCK / 64];
    const NdGroup g = {{s_add}, s_state};
    const NdTile t = nd_tile_summary(g, ge, blockIdx.x);
    if (threadIdx.x == 0) tiles[blockIdx.x] = t;
}

__global__ __launch_bounds__(ND_SCAN) void k_ndjson_scan(NdGeom ge, NdTile* __restrict__ tiles, uint64_t ntiles,
                                                          unsigned long long* __restrict__ offsets, uint64_t capacity,
                                                          NdResult* __restrict__ res) {
    __shared__ NdState s_state[ND_SCAN / 64];
    __shared__ unsigned long long s_add[ND_SCAN / 64];
    const NdGroup g = {{s_add}, s_state};
    const NdTile all = nd_scan_tiles(g, tiles, ntiles);
    if (threadIdx.x == 0) nd_finish(ge, all, offsets, capacity, res);
}

__global__ __launch_bounds__(ND_BLOCK) void k_ndjson_emit(NdGeom ge, const NdTile* __restrict__ tiles,
                                                          unsigned long long* __restrict__ offsets, uint64_t capacity) {
    __shared__ NdState s_state[ND_BLOCK / 64];
    __shared__ unsigned long long s_add[ND_BLOCK / 64];
    const NdGroup g = {{s_add}, s_state};
    nd_tile_emit(g, ge, blockIdx.x, tiles[blockIdx.x], offsets, capacity);
}

}  // namespace

uint64_t ndjson_tile_bytes() { return (uint64_t)ND_TILE_BLOCKS * 64; }

size_t ndjson_workspace_bytes(uint64_t len) {
    // (a pointer's low four bits move the blocks by up to 15 bytes: one tile more than len alone needs)
    return (size_t)((len + 15 + ndjson_tile_bytes() - 1) / ndjson_tile_bytes() + 1) * sizeof(NdTile);
}

hipError_t ndjson_launch(const void* d_buf, uint64_t len, void* d_doc_offsets, uint64_t offset_capacity, void* d_result, void* d_ws,
                         hipStream_t stream) {
    const NdGeom ge = nd_geom(d_buf, len, ND_TILE_BLOCKS);
    const uint64_t ntiles = nd_tiles(ge);
    if (ntiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    NdTile* tiles = static_cast<NdTile*>(d_ws);
    if (ntiles) hipLaunchKernelGGL(k_ndjson_summary, dim3((unsigned)ntiles), dim3(ND_BLOCK), 0, stream, ge, tiles);
    hipLaunchKernelGGL(k_ndjson_scan, dim3(1), dim3(ND_SCAN), 0, stream, ge, tiles, ntiles, (unsigned long long*)d_doc_offsets,
                       offset_capacity, (NdResult*)d_result);
    if (ntiles && offset_capacity > 1)  // (entry 0 is the scan's)
        hipLaunchKernelGGL(k_ndjson_emit, dim3((unsigned)ntiles), dim3(ND_BLOCK), 0, stream, ge, (const NdTile*)tiles,
                           (unsigned long long*)d_doc_offsets, offset_capacity);
    return hipGetLastError();
}

}  // namespace sjmi
