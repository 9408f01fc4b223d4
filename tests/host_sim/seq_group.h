// seq_group.h -- the SEQUENTIAL forms of the lane groups of simdjson-java_amd/csrc/sj_group.h (the contract is written there),
// and the guard-page placement, once for the host simulations of the column operators (sel_sim, explode_sim, ndjson_sim,
// strcol_sim, filter_sim).  TEST ONLY, host only.  Where the lanes of a group are independent they run in DESCENDING order:
// any order must do.
#pragma once
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include "../../simdjson-java_amd/csrc/sj_block.h"

// WgGroup as ONE lane that is also ONE wave of 64: every scan is empty and every total the caller's own value, a ballot
// collects the answers of a loop over the wave's lanes, a validity bit is set on its own
struct SeqGroup {
    uint32_t lanes() const { return 1; }
    uint32_t lane() const { return 0; }
    uint32_t waves() const { return 1; }
    uint32_t wave() const { return 0; }
    bool first() const { return true; }
    template <class F>
    sj_u64 ballot(F f) const {
        sj_u64 w = 0;
        for (uint32_t t = 64; t-- > 0;)
            if (f(t)) w |= 1ull << t;
        return w;
    }
    template <class F>
    void each(F f) const {
        for (uint32_t t = 64; t-- > 0;) f(t);
    }
    sj_u64 scan_add(sj_u64 v, sj_u64* total) const {
        *total = v;
        return 0;
    }
    sj_u64 scan_in_place(sj_u64* sums, sj_u64 n) const {
        sj_u64 run = 0;
        for (sj_u64 i = 0; i < n; ++i) {
            const sj_u64 v = sums[i];
            sums[i] = run;
            run += v;
        }
        return run;
    }
    void validity_bit(sj_u64* words, sj_u64 r, bool live, bool flag) const {
        if (!live) return;
        if (!(r & 63)) words[r >> 6] = 0;  // (rows come in order: the first live row of a word clears it)
        if (flag) words[r >> 6] |= 1ull << (r & 63);
    }
    bool any(bool flag) const { return flag; }
};

// WaveGroup: the 64 lanes one after the other (between two fences they are independent)
struct SeqWave {
    template <class F>
    void each(F f) const {
        for (uint32_t t = 64; t-- > 0;) f(t);
    }
    void fence() const {}
};

// Lanes16 (GROUP = SEL_GROUP): the cooperative copy done by one "lane", the ballot a loop over the group's lanes
template <uint32_t GROUP>
struct SeqLanes {
    uint32_t stride_first() const { return 0; }
    uint32_t stride() const { return 1; }
    void fence() const {}
    template <class F>
    uint32_t ballot(F f) const {
        uint32_t m = 0;
        for (uint32_t j = GROUP; j-- > 0;) m |= (f(j) ? 1u : 0u) << j;
        return m;
    }
};

// Memory that ENDS where a PROT_NONE page begins: a load that leaves what place() copied there by a single byte is a SIGSEGV
// here and not a fault on a GPU.  (What lies in front of the copy is readable: the passes only ever move forward.)
struct Guarded {
    uint8_t* map = nullptr;
    size_t bytes = 0;  // readable bytes in front of the guard page
    size_t page = 0;
    bool open(size_t need) {
        page = (size_t)sysconf(_SC_PAGESIZE);
        bytes = (need + page - 1) / page * page + page;
        void* m = mmap(nullptr, bytes + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return false;
        map = (uint8_t*)m;
        return mprotect(map + bytes, page, PROT_NONE) == 0;
    }
    uint8_t* place(const void* src, size_t n) {  // -> the copy, ending at the guard page
        memset(map, 0xA5, bytes);
        uint8_t* at = map + bytes - n;
        if (n) memcpy(at, src, n);
        return at;
    }
    ~Guarded() {
        if (map) munmap(map, bytes + page);
    }
};
