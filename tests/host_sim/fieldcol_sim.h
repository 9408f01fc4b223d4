// fieldcol_sim.h -- what the host simulations of the fixed-width Arrow column operators share (arrowcol_sim.cpp, timecol_sim.cpp):
// the frame of simdjson-java_amd/csrc/sj_fieldcol.h run with the sequential group (seq_group.h) -- ONE wave per chunk whose 64
// lanes run one after the other (a ballot collects their answers, every scan is empty and every total the wave's own value).
// TEST ONLY, host only.  The type block, the value block and both output blocks each END at a page that cannot be touched, the
// type and value blocks right behind the last column's last LIVE row: a read of a row at or above the live rows, or a write past
// the last field's slice, is a SIGSEGV here and not a fault on a GPU.
#pragma once
#include <vector>

#include "../../simdjson-java_amd/csrc/sj_fieldcol.h"
#include "seq_group.h"

// the arguments every simulation refuses with -2, as the entry points of include/sjmi.h do
inline bool fc_sim_args(const uint8_t* types, const uint64_t* values, uint64_t n_cols, uint64_t col_stride, uint64_t n_rows, uint64_t cells_readable,
                        uint32_t chunk_rows, const uint64_t* data, uint64_t data_stride, const uint64_t* validity, uint64_t validity_stride,
                        const uint64_t* results) {
    if (!chunk_rows || chunk_rows % 64 || !results || col_stride < n_rows || (n_rows && (!types || !values))) return false;
    if (data ? data_stride < n_rows : data_stride != 0) return false;
    if (validity && validity_stride < (n_rows + 63) / 64) return false;
    return cells_readable <= n_cols * col_stride;
}

// the cells_readable = (n_cols - 1) * col_stride + live cells of a column set, copied in front of guard pages -- the cells behind
// the last column's live rows do not exist here
struct FcSimCols {
    Guarded gt, gv;
    bool open(uint64_t cells) { return gt.open(cells + 1) && gv.open(cells * 8 + 8); }
    FcCols place(const uint8_t* types, const uint64_t* values, uint64_t cells, uint64_t col_stride, uint64_t n_rows, const uint64_t* row_count) {
        return {gt.place(types, cells), (const sj_u64*)gv.place(values, cells * 8), col_stride, n_rows, (const sj_u64*)row_count};
    }
};

// data: data_words words or NULL (with data_stride 0: the counting call), validity: validity_words words or NULL -- what the
// caller gives is copied against a guard page and copied back, so whatever canaries it holds are the caller's
struct FcSimOut {
    Guarded gd, gb;
    FcOut o;
    uint64_t data_words, validity_words;
    bool open(uint64_t dw, uint64_t vw) { return data_words = dw, validity_words = vw, gd.open(dw * 8 + 8) && gb.open(vw * 8 + 8); }
    void place(const uint64_t* data, uint64_t data_stride, const uint64_t* validity, uint64_t validity_stride) {
        o = {data ? (sj_u64*)gd.place(data, data_words * 8) : nullptr, data_stride, validity ? (sj_u64*)gb.place(validity, validity_words * 8) : nullptr,
             validity_stride};
    }
    // the blocks back to the caller; false when a byte in front of one was written (place() filled what lies there with 0xA5)
    bool copy_back(uint64_t* data, uint64_t* validity) const {
        if (data) memcpy(data, o.data, data_words * 8);
        if (validity) memcpy(validity, o.validity, validity_words * 8);
        for (int i = 1; i <= 64; ++i)
            if ((data && ((const uint8_t*)o.data)[-i] != 0xA5) || (validity && ((const uint8_t*)o.validity)[-i] != 0xA5)) return false;
        return true;
    }
};

// both passes, as the operator names them: its chunk pass for every (field, chunk), then its finish pass for every field
template <class Cols, class Result, class Pass, class Finish>
static void fc_sim_run(const FcPlan& plan, const Cols& c, const FcOut& o, sj_u64* ws, Result* results, Pass chunk_pass, Finish finish_pass) {
    const SeqGroup g;
    const sj_u64 nchunks = fc_chunks(c.n_rows, c.chunk_rows);
    for (uint32_t f = 0; f < plan.n_fields; ++f)
        for (sj_u64 k = 0; k < nchunks; ++k) chunk_pass(g, plan, c, k, f, o, ws);
    for (uint32_t f = 0; f < plan.n_fields; ++f) finish_pass(g, c, f, ws, results);
}
