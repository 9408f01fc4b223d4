// Host simulation of the device-resident selector (simdjson-java_amd/csrc/select.hip): sj_select.h, the header the kernel
// compiles verbatim, with the group primitives in their sequential form -- the cooperative copy done by one "lane", the
// ballot a loop over the sixteen lanes.  TEST ONLY: lets the CPU suite check the walk the kernel runs (the trie, the chain,
// first-match, the slice and the global path) against the oracle's JsonValue walk without a GPU.
// Built by tests/test_host_select.py with g++.
#include <vector>
#include "../../simdjson-java_amd/csrc/sj_select.h"

struct SeqLanes {
    uint32_t stride_first() const { return 0; }
    uint32_t stride() const { return 1; }
    void fence() const {}
    template <class F>
    uint32_t ballot(F f) const {
        uint32_t m = 0;
        for (uint32_t j = SEL_GROUP; j-- > 0;)  // (any order must do: the lanes are independent)
            m |= (f(j) ? 1u : 0u) << j;
        return m;
    }
};

extern "C" uint32_t sim_select_slice_words(void) { return SEL_SLICE_WORDS; }

// n_docs documents: tapes back to back (document k: tape[tape_offsets[k], tape_offsets[k + 1])), one string buffer, the
// columns as sjmi_select_batch_device writes them.  -> 0, or -2 when the plan does not compile.
extern "C" int sim_select(const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths, const uint64_t* tape,
                          const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, uint64_t n_docs,
                          uint8_t* types, uint64_t* values) {
    std::vector<sj_u64> image;
    if (!sel_compile(pointers, pointer_offsets, n_paths, &image)) return -2;
    const SelHeader* plan = (const SelHeader*)image.data();
    SeqLanes g;
    SelScratch* s = new SelScratch;
    for (uint64_t k = 0; k < n_docs; ++k) {
        memset(s, 0xA5, sizeof *s);  // (LDS is not zero on the device either)
        for (uint32_t p = 0; p < plan->n_paths; ++p) {
            s->types[p] = 0;
            s->values[p] = 0;
        }
        if (doc_errors[k] == 0) {
            // a copy of exactly the document's words: a read outside them is a read outside an allocation
            std::vector<sj_u64> words((const sj_u64*)tape + tape_offsets[k], (const sj_u64*)tape + tape_offsets[k + 1]);
            sel_document(g, plan, words.data(), (uint32_t)words.size(), sb, *s);
        }
        for (uint32_t p = 0; p < plan->n_paths; ++p) {
            types[p * n_docs + k] = s->types[p];
            values[p * n_docs + k] = sel_finish(s->types[p], s->values[p], sb);
        }
    }
    delete s;
    return 0;
}
