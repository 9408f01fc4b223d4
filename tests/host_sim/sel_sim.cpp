// Host simulation of the device-resident selector (simdjson-java_amd/csrc/select.hip): sj_select.h, the header the kernel
// compiles verbatim, with the group primitives in their sequential form (seq_group.h) -- the cooperative copy done by one
// "lane", the ballot a loop over the sixteen lanes.  TEST ONLY: lets the CPU suite check the walk the kernel runs (the trie,
// the chain, first-match, the slice and the global path) against the oracle's JsonValue walk without a GPU.
// sim_select_guarded (below) runs the same walk with every tape and string record placed against a PROT_NONE page.
// Built by tests/test_host_select.py with g++.
#include <vector>
#include "../../simdjson-java_amd/csrc/sj_select.h"
#include "seq_group.h"

extern "C" uint32_t sim_select_slice_words(void) { return SEL_SLICE_WORDS; }

// n_docs documents: tapes back to back (document k: tape[tape_offsets[k], tape_offsets[k + 1])), one string buffer, the
// columns as sjmi_select_batch_device writes them.  -> 0, or -2 when the plan does not compile.
extern "C" int sim_select(const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths, const uint64_t* tape,
                          const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, uint64_t n_docs,
                          uint8_t* types, uint64_t* values) {
    std::vector<sj_u64> image;
    if (!sel_compile(pointers, pointer_offsets, n_paths, &image)) return -2;
    const SelHeader* plan = (const SelHeader*)image.data();
    SeqLanes<SEL_GROUP> g;
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

// ---- the guarded entry: the same walk with every document's memory placed against a page that cannot be read --------------
// Each document's tape is copied so that its LAST WORD ends where a PROT_NONE page begins, and the document's part of the
// string buffer, [sb_offsets[k], sb_ends[k]), so that its LAST RECORD ends at one: a load that leaves the tape or the key it
// belongs to by a single byte is a SIGSEGV.  (What lies in front of the copies is readable: the walk only ever moves forward.)
// Host only; tests/test_host_select_fuzz.py runs it in a child process and asserts on how that ends.
// as sim_select; document k's string records are sb[sb_offsets[k], sb_ends[k]).  -> 0, -2 (the plan), -3 (no memory)
extern "C" int sim_select_guarded(const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths, const uint64_t* tape,
                                  const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, const uint64_t* sb_offsets,
                                  const uint64_t* sb_ends, uint64_t n_docs, uint8_t* types, uint64_t* values) {
    std::vector<sj_u64> image;
    if (!sel_compile(pointers, pointer_offsets, n_paths, &image)) return -2;
    const SelHeader* plan = (const SelHeader*)image.data();
    size_t max_words = 1, max_sb = 1;
    for (uint64_t k = 0; k < n_docs; ++k) {
        if (tape_offsets[k + 1] - tape_offsets[k] > max_words) max_words = tape_offsets[k + 1] - tape_offsets[k];
        if (sb_ends[k] - sb_offsets[k] > max_sb) max_sb = sb_ends[k] - sb_offsets[k];
    }
    Guarded gt, gs;
    if (!gt.open(max_words * 8) || !gs.open(max_sb)) return -3;
    SeqLanes<SEL_GROUP> g;
    SelScratch* s = new SelScratch;
    for (uint64_t k = 0; k < n_docs; ++k) {
        memset(s, 0xA5, sizeof *s);
        for (uint32_t p = 0; p < plan->n_paths; ++p) {
            s->types[p] = 0;
            s->values[p] = 0;
        }
        // (the tape's string words hold offsets into the batch's buffer: the base is moved, not the words)
        const uint8_t* dsb = gs.place(sb + sb_offsets[k], sb_ends[k] - sb_offsets[k]) - sb_offsets[k];
        if (doc_errors[k] == 0) {
            const size_t n = tape_offsets[k + 1] - tape_offsets[k];
            const sj_u64* words = (const sj_u64*)gt.place(tape + tape_offsets[k], n * 8);
            sel_document(g, plan, words, (uint32_t)n, dsb, *s);
        }
        for (uint32_t p = 0; p < plan->n_paths; ++p) {
            types[p * n_docs + k] = s->types[p];
            values[p * n_docs + k] = sel_finish(s->types[p], s->values[p], dsb);
        }
    }
    delete s;
    return 0;
}
