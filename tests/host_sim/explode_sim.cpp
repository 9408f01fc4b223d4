// Host simulation of explode (simdjson-java_amd/csrc/explode.hip): sj_select.h, the header the kernels compile verbatim, with
// the group primitives in their sequential form (seq_group.h).  TEST ONLY: lets the CPU suite check what k_explode_count and
// k_explode_rows run per document (the base pointer's walk, the iterator chain's count, the element plan from every element)
// against the oracle without a GPU.  The prefix sum and the capacity rule are restated here in plain loops.
// sim_explode_guarded runs the same with every tape and every document's last string record placed against a PROT_NONE page.
// Built by tests/test_host_explode.py with g++.
#include <vector>
#include "../../simdjson-java_amd/csrc/sj_select.h"
#include "seq_group.h"

namespace {
// sb_offsets != nullptr: the guarded form
int explode(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths,
            const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, const uint64_t* sb_offsets,
            const uint64_t* sb_ends, uint64_t n_docs, uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    std::vector<sj_u64> base_image, image;
    const uint64_t base_offsets[2] = {0, base_len};
    if (!sel_compile(base, base_offsets, 1, &base_image) || !sel_compile(pointers, pointer_offsets, n_paths, &image)) return -2;
    const SelHeader* base_plan = (const SelHeader*)base_image.data();
    const SelHeader* plan = (const SelHeader*)image.data();
    Guarded gt, gs;
    if (sb_offsets) {
        size_t max_words = 1, max_sb = 1;
        for (uint64_t k = 0; k < n_docs; ++k) {
            if (tape_offsets[k + 1] - tape_offsets[k] > max_words) max_words = tape_offsets[k + 1] - tape_offsets[k];
            if (sb_ends[k] - sb_offsets[k] > max_sb) max_sb = sb_ends[k] - sb_offsets[k];
        }
        if (!gt.open(max_words * 8) || !gs.open(max_sb)) return -3;
    }
    SeqLanes<SEL_GROUP> g;
    SelScratch* s = new SelScratch;
    std::vector<uint32_t> counts(n_docs), bases(n_docs);
    // the document's memory for one pass: a copy of exactly its words (a read outside them is a read outside an allocation),
    // or the guarded placement
    std::vector<sj_u64> words;
    auto place = [&](uint64_t k, const uint8_t** dsb) -> const sj_u64* {
        const size_t n = tape_offsets[k + 1] - tape_offsets[k];
        if (!sb_offsets) {
            *dsb = sb;
            words.assign(tape + tape_offsets[k], tape + tape_offsets[k + 1]);
            return words.data();
        }
        // (the tape's string words hold offsets into the batch's buffer: the base is moved, not the words)
        *dsb = gs.place(sb + sb_offsets[k], sb_ends[k] - sb_offsets[k]) - sb_offsets[k];
        return (const sj_u64*)gt.place(tape + tape_offsets[k], n * 8);
    };
    // ---- k_explode_count
    for (uint64_t k = 0; k < n_docs; ++k) {
        memset(s, 0xA5, sizeof *s);  // (LDS is not zero on the device either)
        s->types[0] = 0;
        s->values[0] = 0;
        counts[k] = bases[k] = 0;
        if (doc_errors[k] != 0) continue;
        const uint8_t* dsb;
        const sj_u64* w = place(k, &dsb);
        const SelDoc d = sel_stage(g, w, (uint32_t)(tape_offsets[k + 1] - tape_offsets[k]), dsb, *s);
        counts[k] = sel_explode_count(g, base_plan, d, *s, &bases[k]);
    }
    // ---- the scan
    row_offsets[0] = 0;
    for (uint64_t k = 0; k < n_docs; ++k) row_offsets[k + 1] = row_offsets[k] + counts[k];
    if (!row_capacity || !n_paths) {
        delete s;
        return 0;
    }
    // ---- k_explode_rows
    for (uint64_t k = 0; k < n_docs; ++k) {
        if (!bases[k] || !counts[k] || row_offsets[k] >= row_capacity) continue;
        memset(s, 0xA5, sizeof *s);
        const uint8_t* dsb;
        const sj_u64* w = place(k, &dsb);
        const SelDoc d = sel_stage(g, w, (uint32_t)(tape_offsets[k + 1] - tape_offsets[k]), dsb, *s);
        const uint64_t room = row_capacity - row_offsets[k];
        sel_explode_rows(g, plan, d, *s, bases[k], room < counts[k] ? (uint32_t)room : counts[k], [&](uint32_t j) {
            const uint64_t r = row_offsets[k] + j;
            if (r >= row_capacity) return;
            for (uint32_t p = 0; p < plan->n_paths; ++p) {
                types[p * row_capacity + r] = s->types[p];
                values[p * row_capacity + r] = sel_finish(s->types[p], s->values[p], dsb);
            }
        });
    }
    delete s;
    return 0;
}
}  // namespace

extern "C" uint32_t sim_explode_slice_words(void) { return SEL_SLICE_WORDS; }

// n_docs documents: tapes back to back (document k: tape[tape_offsets[k], tape_offsets[k + 1])), one string buffer; the outputs
// as sjmi_explode_batch_device writes them (row_offsets always complete; the columns strided by row_capacity, rows at or past
// it not written; row_capacity 0: types / values may be null).  -> 0, or -2 when a plan does not compile.
extern "C" int sim_explode(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths,
                           const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, uint64_t n_docs,
                           uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    return explode(base, base_len, pointers, pointer_offsets, n_paths, tape, tape_offsets, doc_errors, sb, nullptr, nullptr, n_docs, row_offsets,
                   row_capacity, types, values);
}

// as sim_explode; document k's string records are sb[sb_offsets[k], sb_ends[k]): each document's tape is placed so that its
// LAST WORD ends where a PROT_NONE page begins, and its part of the string buffer so that its LAST RECORD ends at one.
// -> 0, -2 (a plan), -3 (no memory).  Host only; tests/test_host_explode.py runs it in a child process.
extern "C" int sim_explode_guarded(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                                   uint64_t n_paths, const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors,
                                   const uint8_t* sb, const uint64_t* sb_offsets, const uint64_t* sb_ends, uint64_t n_docs,
                                   uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    return explode(base, base_len, pointers, pointer_offsets, n_paths, tape, tape_offsets, doc_errors, sb, sb_offsets, sb_ends, n_docs,
                   row_offsets, row_capacity, types, values);
}
