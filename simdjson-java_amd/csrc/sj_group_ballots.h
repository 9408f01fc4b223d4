// sj_group_ballots.h -- one more member of the lane-group contract of sj_group.h, as a free function so that an operator which
// needs it brings it along: the device form for WgGroup here, the sequential form in tests/host_sim/seq_ballots.h.
//   group_ballots(g, f, out)   f(t, vote) is called ONCE for every lane t of the wave and fills vote[0, N); out[k] is the 64-bit
//                              word whose bit t is what lane t put into vote[k].  A lane that works on N rows at once -- all
//                              their loads requested before the first is used -- votes on all of them in one call; N ballots of
//                              one row each would put every row's loads behind the row before it.  No barrier: whole waves.
#pragma once
#include "sj_group.h"

namespace sjmi {

template <class F, uint32_t N>
__device__ __forceinline__ void group_ballots(const WgGroup&, F f, sj_u64 (&out)[N]) {
    bool vote[N];
    f(threadIdx.x & 63u, vote);
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) out[k] = __ballot(vote[k]);
}

}  // namespace sjmi
