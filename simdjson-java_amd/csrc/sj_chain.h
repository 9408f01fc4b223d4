// sj_chain.h -- device-only primitives shared by the kernels: the single-pass chain of the two persistent kernels (stage1.hip,
// strings.hip) with its scanner, and the wave / workgroup scans (also batch.hip, walk.hip).  gfx950 device code only (DPP,
// s_getreg, LDS fences): the host simulations never include it.
//
// The CHAIN.  A persistent kernel cuts its input into granules.  A worker wave classifies a granule, publishes its AGGREGATE as
// one u64 granule state, and picks the granule's inclusive PREFIX up one classification later, so nobody waits for the chain.
// Prefixes come from a scanner workgroup (chain_scanner_wave).  A granule state is one naturally aligned 8-byte relaxed
// agent-scope store / load: the data is the flag (cdna_hip_programming.md Guideline 16, form R2), so no fences are needed.
//   bits 63..62 : 0 = nothing yet, 1 = AGGREGATE, 2 = INCLUSIVE PREFIX; the other bits are each kernel's own
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sj_block.h"

namespace sjmi {

constexpr sj_u64 CHAIN_AGG = 1ull << 62, CHAIN_PFX = 2ull << 62;
// bounded spins: ~2^19 polls of >= 100 cycles (s_sleep 1 + an uncached load) = tens of milliseconds; a healthy chain needs
// a handful of polls.  A launch whose grid is not resident trips it, and the kernel reports that (each in its own way).
constexpr uint32_t CHAIN_SPIN_LIMIT = 1u << 19;

__device__ __forceinline__ void granule_store(sj_u64* p, sj_u64 v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ sj_u64 granule_load(const sj_u64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------------
// wave helpers (wave = 64 lanes)
// ---------------------------------------------------------------------------------------------------------------------
// Inclusive scans with DPP (no LDS traffic): Kogge-Stone inside each row of 16 lanes (row_shr 1/2/4/8, out-of-row reads give
// 0), then the row totals are carried across with row_bcast:15 / :31.  Each rung is one v_add_u32_dpp / v_max_u32_dpp.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
    return v > o ? v : o;
}
// inside each row of 16 lanes
__device__ __forceinline__ uint32_t row_incl_add(uint32_t v) {
    v = dpp_add<0x111, 0xF>(v);  // row_shr:1
    v = dpp_add<0x112, 0xF>(v);  // row_shr:2
    v = dpp_add<0x114, 0xF>(v);  // row_shr:4
    v = dpp_add<0x118, 0xF>(v);  // row_shr:8
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
    v = row_incl_add(v);
    v = dpp_add<0x142, 0xA>(v);  // row_bcast:15 -> rows 1 and 3
    v = dpp_add<0x143, 0xC>(v);  // row_bcast:31 -> rows 2 and 3
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v) {
    v = dpp_max<0x111, 0xF>(v);
    v = dpp_max<0x112, 0xF>(v);
    v = dpp_max<0x114, 0xF>(v);
    v = dpp_max<0x118, 0xF>(v);
    v = dpp_max<0x142, 0xA>(v);
    v = dpp_max<0x143, 0xC>(v);
    return v;
}

__device__ __forceinline__ void wave_lds_fence() {
    // LDS accesses of one wave execute in order; this only stops the compiler from reordering them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// (xcc, se, sh, cu) of the CU this wave runs on, never 0
__device__ __forceinline__ uint32_t cu_id() {
    return (((uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 8) & 0xFFu) |
           (((uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xFu) << 8) | 0x80000000u;
}

// Executed by all 64 lanes: the next ticket of `counter`, wave-uniform.
__device__ __forceinline__ uint32_t take_ticket(uint32_t* counter) {
    uint32_t t = 0;
    if ((threadIdx.x & 63) == 0) t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)t);
}

// A worker's wait for the PREFIX at *p: `pf` is the granule state as requested ahead of its use, polled until it is a prefix.
// If the bound trips (never expected: the scanner is not running), on_timeout() reports it and the wait ends.
// (No sleep in front of the first poll: the string pass took 0.407 ms instead of 0.389 -- the polls compete with the stores;
// 2 .. 8: no change.)
template <class OnTimeout>
__device__ __forceinline__ void wait_prefix(const sj_u64* p, sj_u64& pf, OnTimeout on_timeout) {
    for (uint32_t spins = 0; (pf >> 62) != 2; ++spins) {
        if (spins > CHAIN_SPIN_LIMIT) {
            on_timeout();
            break;
        }
        if (spins) __builtin_amdgcn_s_sleep(1);
        pf = granule_load(p);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// workgroup scans
// ---------------------------------------------------------------------------------------------------------------------
// Exclusive + scan of one value per thread over a workgroup of NW waves (0: blockDim.x / 64); *total = the workgroup's sum.
// s_wave holds one entry per wave.  It begins with a barrier, so it may be called again without one in between.
template <int NW = 0>
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, unsigned long long* s_wave,
                                                              unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = NW ? NW : (int)(blockDim.x >> 6);
    unsigned long long incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long base = 0, t = 0;
    for (int i = 0; i < nw; ++i) {
        if (i < wave) base += s_wave[i];
        t += s_wave[i];
    }
    *total = t;
    return base + incl - v;
}

// One workgroup of 1024 threads turns sums[0, n) into their exclusive + scan in place, 1024 entries at a time, carrying the
// total from slice to slice; returns the total.  (The barrier behind each slice is one more than block_excl_scan needs.)
template <int NW = 0>
__device__ __forceinline__ unsigned long long block_scan_in_place(unsigned long long* sums, uint64_t n, unsigned long long* s_wave) {
    unsigned long long carry = 0;
    for (uint64_t b = 0; b < n; b += 1024) {
        const uint64_t i = b + threadIdx.x;
        const unsigned long long v = i < n ? sums[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_excl_scan<NW>(v, s_wave, &total);
        if (i < n) sums[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    return carry;
}

// ---------------------------------------------------------------------------------------------------------------------
// the SCANNER: one workgroup of four waves turns the workers' per-granule AGGREGATEs, in order, into per-granule inclusive
// PREFIXes in a second array.  Every granule crosses the chip exactly twice (aggregate: worker -> scanner, prefix: scanner ->
// worker).  Measured alternative: every worker polling a 64..256-granule window of uncached granules itself, whose traffic and
// round trips (one per window of distance to the nearest prefix) were the bottleneck.  The workers need a granule's prefix one
// whole classification after they published its aggregate, so the scanner's latency (load + store visibility, ~3 us) is off
// the critical path; its THROUGHPUT is not (200+ granules per us): a single wave managed ~250/us, so the four waves take the
// windows of 64 * K granules round-robin, do everything that does not depend on the running state (polling, folding K granules
// per lane, cross-lane scans) in parallel, and pass the running state from window to window through LDS, which is the only
// serial step.  At the workers' frontier a wave publishes whatever is ready lane by lane, so that a launch with few resident
// workgroups cannot deadlock on a half-handed-out window.
//
// A kernel supplies a Policy: its window width K, the fold and scans of its aggregates, its prefix words and what it reports:
//   Window window(v, lane)                     everything of a complete window that does not depend on the running state
//   ChainState advance(in, v, w)               the state behind the window; reports the window's errors before it is passed on
//   void publish_window(v, pfx, first, n, in, w)    the prefixes of the lane's granules
//   ChainState publish_ready(v, pfx, first, n, lane, act, in)   the same for the lanes `act` of a window at the frontier, in order
//   void give_up()                             (lane 0) a spin bound tripped
//   void finish(out)                           (lane 0) behind the last window
// ---------------------------------------------------------------------------------------------------------------------
// the running state: a 32-bit word and a 64-bit count (stage 1: parity, structurals; string pass: strings, bytes)
struct ChainState {
    uint32_t w;
    sj_u64 c;
};
// (one 16-byte struct for both kernels: a {seq, State} template would pad the 12 bytes of state behind `seq` to 24)
struct ChainHandoff {
    uint32_t seq;  // window whose entry state is in w / c; CHAIN_GAVE_UP = a scanner wave gave up
    uint32_t w;
    sj_u64 c;
};
constexpr uint32_t CHAIN_GAVE_UP = 0xFFFFFFFFu;

template <int K>
__device__ __forceinline__ void chain_load(sj_u64 (&v)[K], const sj_u64* agg, sj_u64 first, uint32_t n) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = first + j < n ? granule_load(&agg[first + j]) : CHAIN_AGG;  // past the end: empty aggregates
}
template <int K>
__device__ __forceinline__ bool chain_ready(const sj_u64 (&v)[K]) {
    bool ready = true;
#pragma unroll
    for (int j = 0; j < K; ++j) ready &= v[j] != 0;
    return ready;
}
// false = a scanner wave gave up
__device__ __forceinline__ bool chain_wait_turn(ChainHandoff* hand, uint32_t win) {
    uint32_t seq;
    do {
        seq = __hip_atomic_load(&hand->seq, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } while (seq != win && seq != CHAIN_GAVE_UP);
    return seq != CHAIN_GAVE_UP;
}
__device__ __forceinline__ void chain_hand_on(ChainHandoff* hand, uint32_t win, ChainState s, int lane) {
    if (lane == 0) {
        hand->w = s.w;
        hand->c = s.c;
        __hip_atomic_store(&hand->seq, win + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Executed by all 64 lanes of scanner wave `wave` (of four); hand->seq = 0 and the entry state in hand before the first call.
template <class Policy>
__device__ __forceinline__ void chain_scanner_wave(ChainHandoff* hand, int wave, int lane, const sj_u64* agg, sj_u64* pfx,
                                                   uint32_t n, const Policy& pol) {
    constexpr int K = Policy::K;
    constexpr uint32_t WIN = 64 * K;
    __builtin_amdgcn_s_setprio(3);  // everybody waits for these four waves
    for (sj_u64 win = (sj_u64)wave; win * WIN < n; win += 4) {
        const sj_u64 first = win * WIN + (sj_u64)lane * K;  // this lane's granules
        sj_u64 v[K];
        ChainState out;
        // poll the window until it is complete (then most of the work can be done before the running state arrives) or
        // until the running state has arrived (then the ready part cannot wait for the rest)
        bool full;
        for (;;) {
            chain_load(v, agg, first, n);
            full = __ballot(chain_ready(v)) == ~0ull;
            if (full) break;
            const uint32_t seq = __hip_atomic_load(&hand->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (seq == (uint32_t)win || seq == CHAIN_GAVE_UP) break;
            __builtin_amdgcn_s_sleep(1);
        }
        if (full) {
            // ---- the scanner is behind the workers: the window is complete at the first look.  Everything that does
            //      not depend on the running state is done before waiting for it ----
            const typename Policy::Window w = pol.window(v, lane);
            // the serial step: take the running state from the previous window's wave, pass it on
            if (!chain_wait_turn(hand, (uint32_t)win)) return;
            const ChainState in = {hand->w, hand->c};
            out = pol.advance(in, v, w);
            chain_hand_on(hand, (uint32_t)win, out, lane);
            pol.publish_window(v, pfx, first, n, in, w);
        } else {
            // ---- the scanner is at the workers' frontier: take the running state first, then publish whatever
            //      becomes ready, lane by lane in order (a worker may be waiting for a prefix in the front part of this
            //      window while the back part has not even been handed out) ----
            if (!chain_wait_turn(hand, (uint32_t)win)) return;
            out = {hand->w, hand->c};
            int done = 0;  // lanes already turned into prefixes
            for (uint32_t spins = 0;; ++spins) {
                const sj_u64 rb = __ballot(chain_ready(v));
                const int nr = ~rb ? __builtin_ctzll(~rb) : 64;  // lanes ready in a row from lane 0
                if (nr > done) {
                    out = pol.publish_ready(v, pfx, first, n, lane, lane >= done && lane < nr, out);
                    done = nr;
                    spins = 0;
                }
                if (done == 64) break;
                if (spins > CHAIN_SPIN_LIMIT) {  // never expected: a worker did not publish
                    if (lane == 0) {
                        __hip_atomic_store(&hand->seq, CHAIN_GAVE_UP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        pol.give_up();
                    }
                    return;
                }
                __builtin_amdgcn_s_sleep(1);
                sj_u64 nv[K];
                chain_load(nv, agg, first, n);
#pragma unroll
                for (int j = 0; j < K; ++j)
                    if (lane >= done) v[j] = nv[j];  // (finished lanes keep what their prefixes were computed from)
            }
            chain_hand_on(hand, (uint32_t)win, out, lane);
        }
        if ((win + 1) * WIN >= n && lane == 0) pol.finish(out);  // that was the last window
    }
}

}  // namespace sjmi
