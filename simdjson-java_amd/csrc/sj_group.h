// sj_group.h -- the device forms of the lane groups that the column operators' pass headers are written against (sj_select.h,
// sj_ndjson.h, sj_strcol.h, sj_filter.h), once.  gfx950 device code only: the host simulations take the sequential forms of the
// same members from tests/host_sim/seq_group.h, and both compile the pass headers verbatim.
//
// A pass takes its lanes from the caller as a type G and asks nothing of it but the members below, so the same text runs as a
// workgroup of a kernel and as one lane of a loop on the host.  Three groups:
//
// WgGroup -- a WORKGROUP of waves of 64 lanes; s_wave is one LDS entry per wave (it may be null where no scan is called).
//   g.lanes() / g.lane()                 how many lanes work side by side, and which one this is (lane 0 writes a result record)
//   g.waves() / g.wave()                 the same in waves
//   g.first()                            true in ONE lane of every wave (the one that stores a wave-uniform value)
//   g.ballot(f)                          the 64-bit word whose bit t is f(t), f called for every lane t of the wave
//   g.each(f)                            f(t) for every lane t of the wave
//   g.scan_add(v, &total)                exclusive + scan of v over all lanes of the group, total = their sum
//   g.scan_in_place(sums, n)             sums[0, n) -> their exclusive + scan, in place; returns the total (1024 threads)
//   g.validity_bit(words, r, live, flag) called by every lane with its row r: bit r & 63 of words[r >> 6] = flag; a row that is
//                                        not live gives a 0 bit, and a word without a live row is not written.  (A wave is 64
//                                        consecutive rows: ONE ballot is the word, and lane 0 of a wave with a live row stores
//                                        it -- r is a multiple of 64 there, and that row is live iff any of the wave's is.)
//   g.any(flag)                          is the flag set in any lane of the group
//   BARRIERS: scan_add, scan_in_place and any are workgroup barriers and must be reached by EVERY lane of the workgroup.  The
//   scans BEGIN with one, so they may be called again without a barrier in between.  The other members have none and may be
//   called by a partial workgroup (k_filter_emit's chunks leave early), ballot / each / validity_bit by whole waves.
//   An operator with a scan of its own derives from WgGroup and adds it (ndjson.hip: load, scan_state).
//
// WaveGroup -- ONE wave and its LDS (no workgroup barrier anywhere):
//   w.each(f)                            f(t) for every lane t of the wave
//   w.fence()                            what the lanes wrote to the wave's LDS is visible to all of them
//
// Lanes16 -- the SEL_GROUP = 16 lanes of a wave that hold one document (a DPP row, like k_doc_pass); four groups to a wave:
//   g.stride_first() / g.stride()        the lane's first element and the step of a cooperative copy
//   g.fence()                            orders the group's slice / scratch accesses (the whole wave's: no barrier)
//   g.ballot(f)                          f(lane) in every lane of the group -> bit j = what lane j returned
//   group_lanes() makes the calling thread's; doc_words() is a document's tape words; stage_plan() brings a plan image to LDS.
#pragma once
#include "sj_chain.h"
#include "sj_select.h"

namespace sjmi {

struct WgGroup {
    unsigned long long* s_wave;  // one entry per wave
    __device__ __forceinline__ uint32_t lanes() const { return blockDim.x; }
    __device__ __forceinline__ uint32_t lane() const { return threadIdx.x; }
    __device__ __forceinline__ uint32_t waves() const { return blockDim.x >> 6; }
    __device__ __forceinline__ uint32_t wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ bool first() const { return (threadIdx.x & 63u) == 0; }
    template <class F>
    __device__ __forceinline__ sj_u64 ballot(F f) const {
        return __ballot(f(threadIdx.x & 63u));
    }
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        f(threadIdx.x & 63u);
    }
    __device__ __forceinline__ sj_u64 scan_add(sj_u64 v, sj_u64* total) const { return block_excl_scan(v, s_wave, total); }
    __device__ __forceinline__ sj_u64 scan_in_place(sj_u64* sums, sj_u64 n) const { return block_scan_in_place(sums, n, s_wave); }
    __device__ __forceinline__ void validity_bit(sj_u64* words, sj_u64 r, bool live, bool flag) const {
        const sj_u64 word = __ballot(live && flag);
        if ((threadIdx.x & 63u) == 0 && live) words[r >> 6] = word;
    }
    __device__ __forceinline__ bool any(bool flag) const { return __syncthreads_or(flag ? 1 : 0) != 0; }
};

struct WaveGroup {
    template <class F>
    __device__ __forceinline__ void each(F f) const {
        f(threadIdx.x & 63u);
    }
    __device__ __forceinline__ void fence() const { wave_lds_fence(); }
};

struct Lanes16 {
    uint32_t lane, shift;
    __device__ __forceinline__ uint32_t stride_first() const { return lane; }
    __device__ __forceinline__ uint32_t stride() const { return SEL_GROUP; }
    __device__ __forceinline__ void fence() const { wave_lds_fence(); }
    template <class F>
    __device__ __forceinline__ uint32_t ballot(F f) const {
        const bool mine = f(lane);
        return (uint32_t)(__ballot(mine) >> shift) & 0xFFFFu;
    }
};
__device__ __forceinline__ Lanes16 group_lanes() {
    Lanes16 g;
    g.lane = threadIdx.x % SEL_GROUP;
    g.shift = (threadIdx.x & 63u) / SEL_GROUP * SEL_GROUP;
    return g;
}
// the tape words of document `doc`
__device__ __forceinline__ uint32_t doc_words(const unsigned long long* tape_offsets, uint64_t doc) {
    const unsigned long long lo = tape_offsets[doc], hi = tape_offsets[doc + 1];
    const unsigned long long n = hi > lo ? hi - lo : 0;
    return n > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)n;
}
// a plan image into the workgroup's LDS (BLOCK threads, all of them: it ends with a barrier) -> the plan
template <uint32_t BLOCK>
__device__ __forceinline__ const SelHeader* stage_plan(sj_u64* lds_plan, const sj_u64* __restrict__ plan_image, uint32_t image_words) {
    for (uint32_t i = threadIdx.x; i < image_words; i += BLOCK) lds_plan[i] = plan_image[i];
    __syncthreads();
    return (const SelHeader*)lds_plan;
}

}  // namespace sjmi
