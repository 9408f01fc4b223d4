// Host simulation of the per-block tape-word counts (SjBlockMasks::words, what k_stage1_batch stores as blkw and k_doc_prepare
// sums into a document's predicted tape length): a buffer walked block by block with the real carries, as sim_masks does, and
// for every block the count from sj_block (sj_block.h) and from sj_block32 (sj_block32.h), the tail block through the same
// tail masking as in the kernels.  TEST ONLY.  Built by tests/test_host_block_words.py with g++.
#include <string.h>
#include <stdint.h>
#include "../../simdjson-java_amd/csrc/sj_block32.h"

// out[2 * b] = words of block b by sj_block, out[2 * b + 1] = by sj_block32 (low byte: entered outside a string, next byte: inside)
extern "C" int sim_words(const uint8_t* buf, uint64_t len, uint32_t* out) {
    const uint64_t nblocks = len / 64 + 1;
    for (uint64_t b = 0; b < nblocks; ++b) {
        const uint64_t start = b * 64;
        const uint32_t valid = (uint32_t)(len - start < 64 ? len - start : 64);
        uint32_t w[16];
        memset(w, 0xA5, sizeof w);  // bytes past the end are garbage on the device too: they must be invisible
        memcpy(w, buf + start, valid);
        sj_u64 p[8];
        uint32_t lo[8], hi[8];
        sj_transpose_butterfly(w, p);
        sj_transpose32(w, lo, hi);
        sj_mask_tail(p, valid);
        sj_mask_tail32(lo, hi, valid);
        uint32_t e_in = 0, p_in = 0;
        SjUtf8Carry uc = {0, 0, 0, 0};
        if (b > 0) {
            sj_u64 halo;
            memcpy(&halo, buf + start - 8, 8);
            uc = sj_utf8_carry(halo);
            if (!sj_carry_from_halo(halo, &e_in, &p_in)) sj_carry_slow(buf, 0, start, &e_in, &p_in);
        }
        out[2 * b] = sj_block(p, e_in, p_in, uc, true, nullptr, true).words;
        out[2 * b + 1] = sj_block32(lo, hi, e_in, p_in, uc, true, true).words;
    }
    return 0;
}
