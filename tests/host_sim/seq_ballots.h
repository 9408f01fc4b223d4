// seq_ballots.h -- the SEQUENTIAL form of group_ballots (simdjson-java_amd/csrc/sj_group_ballots.h, where the contract is
// written) for SeqGroup of seq_group.h: the wave's lanes one after the other, in descending order.  TEST ONLY, host only.
#pragma once
#include "seq_group.h"

template <class F, uint32_t N>
void group_ballots(const SeqGroup&, F f, sj_u64 (&out)[N]) {
    for (uint32_t k = 0; k < N; ++k) out[k] = 0;
    for (uint32_t t = 64; t-- > 0;) {
        bool vote[N];
        f(t, vote);
        for (uint32_t k = 0; k < N; ++k)
            if (vote[k]) out[k] |= 1ull << t;
    }
}
