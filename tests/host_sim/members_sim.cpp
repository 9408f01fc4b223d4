// Host simulation of a MEMBERS explode (simdjson-java_amd/csrc/explode.hip, k_explode_count<true> / k_explode_rows<true>):
// sj_select.h, the header the kernels compile verbatim, with the group primitives in their sequential form (seq_group.h).  TEST
// ONLY: lets the CPU suite check what the two kernels run per document (the base pointer's walk, the member chain's count, the
// element plan from every member's value, the key's cell) against the oracle without a GPU.  The prefix sum, the capacity rule
// and the row buffer (rows = min(EXP_ROWS, EXP_CELLS / n_cols), flushed when it is full and at the last row) are restated here.
// sim_members_guarded runs the same with every tape and every document's last string record placed against a PROT_NONE page.
// sim_array runs the ARRAY instantiation of the same header over the same inputs (a members plan must not change it).
// Built by tests/test_host_members.py with g++.
#include <vector>
#include "../../simdjson-java_amd/csrc/sj_select.h"
#include "seq_group.h"

namespace {
constexpr uint32_t ROWS = 8, CELLS = 96;  // EXP_ROWS, EXP_CELLS of csrc/explode.hip

// sb_offsets != nullptr: the guarded form
template <bool MEMBERS>
int explode(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths,
            const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, const uint64_t* sb_offsets,
            const uint64_t* sb_ends, uint64_t n_docs, uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    std::vector<sj_u64> base_image, image;
    const uint64_t base_offsets[2] = {0, base_len};
    if (MEMBERS && n_paths > SEL_MAX_PATHS - 1) return -2;
    if (!sel_compile(base, base_offsets, 1, &base_image) || !sel_compile(pointers, pointer_offsets, n_paths, &image)) return -2;
    const SelHeader* base_plan = (const SelHeader*)base_image.data();
    const SelHeader* plan = (const SelHeader*)image.data();
    const uint32_t n_cols = plan->n_paths + (MEMBERS ? 1u : 0u);
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
    std::vector<sj_u64> words;
    auto place = [&](uint64_t k, const uint8_t** dsb) -> const sj_u64* {
        const size_t n = tape_offsets[k + 1] - tape_offsets[k];
        if (!sb_offsets) {
            *dsb = sb;
            words.assign(tape + tape_offsets[k], tape + tape_offsets[k + 1]);
            return words.data();
        }
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
        counts[k] = sel_explode_count<MEMBERS>(g, base_plan, d, *s, &bases[k]);
    }
    // ---- the scan
    row_offsets[0] = 0;
    for (uint64_t k = 0; k < n_docs; ++k) row_offsets[k + 1] = row_offsets[k] + counts[k];
    if (!row_capacity || !n_cols) {
        delete s;
        return 0;
    }
    // ---- k_explode_rows
    uint32_t rows = CELLS / n_cols;
    rows = rows < 1 ? 1 : rows > ROWS ? ROWS : rows;
    std::vector<sj_u64> bvalues(CELLS);
    std::vector<uint8_t> btypes(CELLS);
    for (uint64_t k = 0; k < n_docs; ++k) {
        if (!bases[k] || !counts[k] || row_offsets[k] >= row_capacity) continue;
        memset(s, 0xA5, sizeof *s);
        const uint8_t* dsb;
        const sj_u64* w = place(k, &dsb);
        const SelDoc d = sel_stage(g, w, (uint32_t)(tape_offsets[k + 1] - tape_offsets[k]), dsb, *s);
        const uint64_t room = row_capacity - row_offsets[k], first = row_offsets[k];
        const uint32_t limit = room < counts[k] ? (uint32_t)room : counts[k];
        sel_explode_rows<MEMBERS>(g, plan, d, *s, bases[k], limit, [&](uint32_t j) {
            const uint32_t q = j % rows;
            for (uint32_t p = 0; p < n_cols; ++p) {
                btypes[p * rows + q] = s->types[p];
                bvalues[p * rows + q] = s->values[p];
            }
            if (q + 1 != rows && j + 1 != limit) return;
            const uint64_t r0 = first + (j - q);
            for (uint32_t i = n_cols * (q + 1); i-- > 0;) {  // (any order must do)
                const uint32_t p = i / (q + 1), e = i % (q + 1);
                if (r0 + e < row_capacity) {
                    types[p * row_capacity + r0 + e] = btypes[p * rows + e];
                    values[p * row_capacity + r0 + e] = sel_finish(btypes[p * rows + e], bvalues[p * rows + e], dsb);
                }
            }
        });
    }
    delete s;
    return 0;
}
}  // namespace

extern "C" uint32_t sim_members_slice_words(void) { return SEL_SLICE_WORDS; }
extern "C" uint32_t sim_members_group(void) { return SEL_GROUP; }

// n_docs documents: tapes back to back (document k: tape[tape_offsets[k], tape_offsets[k + 1])), one string buffer; the outputs
// as sjmi_explode_batch_device writes them under a members plan (row_offsets always complete; n_paths + 1 columns strided by
// row_capacity, rows at or past it not written; row_capacity 0: types / values may be null).  -> 0, or -2 when a plan does not compile.
extern "C" int sim_members(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths,
                           const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, uint64_t n_docs,
                           uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    return explode<true>(base, base_len, pointers, pointer_offsets, n_paths, tape, tape_offsets, doc_errors, sb, nullptr, nullptr, n_docs,
                         row_offsets, row_capacity, types, values);
}

// as sim_members; document k's string records are sb[sb_offsets[k], sb_ends[k]): each document's tape is placed so that its LAST
// WORD ends where a PROT_NONE page begins, and its part of the string buffer so that its LAST RECORD ends at one.
// -> 0, -2 (a plan), -3 (no memory).  Host only; tests/test_host_members.py runs it in a child process.
extern "C" int sim_members_guarded(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                                   uint64_t n_paths, const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors,
                                   const uint8_t* sb, const uint64_t* sb_offsets, const uint64_t* sb_ends, uint64_t n_docs,
                                   uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    return explode<true>(base, base_len, pointers, pointer_offsets, n_paths, tape, tape_offsets, doc_errors, sb, sb_offsets, sb_ends, n_docs,
                         row_offsets, row_capacity, types, values);
}

// the ARRAY instantiation over the same inputs (n_paths columns)
extern "C" int sim_array(const uint8_t* base, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths,
                         const uint64_t* tape, const uint64_t* tape_offsets, const int32_t* doc_errors, const uint8_t* sb, uint64_t n_docs,
                         uint64_t* row_offsets, uint64_t row_capacity, uint8_t* types, uint64_t* values) {
    return explode<false>(base, base_len, pointers, pointer_offsets, n_paths, tape, tape_offsets, doc_errors, sb, nullptr, nullptr, n_docs,
                          row_offsets, row_capacity, types, values);
}
