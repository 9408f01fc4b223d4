// explode.hip -- one array per document of a parsed batch becomes a run of rows (include/sjmi.h, sjmi_explode_*):
// the array is the value of a BASE pointer, and every path of an element plan is evaluated on every element, into one typed
// column per path.  A MEMBERS plan takes an OBJECT there: a row is a member, the element plan is evaluated on its
// value, and its key is one more column behind the paths'.  The two kernels that walk are instantiated per mode.  The walk is sj_select.h (sel_explode_count / sel_explode_rows, shared with the host simulation,
// tests/host_sim/explode_sim.cpp), the 16-lane form of its group primitives is Lanes16 of sj_group.h; this file is the plan object
// and the kernels:
//   k_explode_count       rows and the base array's tape index of every document
//   k_explode_chunk_sums / k_explode_chunk_scan / k_explode_offsets   the counts' exclusive scan (block_excl_scan, the chunk-sum
//                         scheme of walk.hip's tape offsets) -> row_offsets[n_docs + 1]
//   k_explode_rows        the cells, a few rows of a group buffered in LDS so that a column store is a run of neighbouring rows
#include <hip/hip_runtime.h>

#include <atomic>
#include <new>

#include "sj_group.h"
#include "stage1.h"

struct sjmi_explode_plan {
    std::vector<sj_u64> image;  // [the base pointer as a plan of one path][the element plan]
    size_t base_words;
    bool members;  // rows are the members of an object: the key is a column behind the element plan's
    uint64_t serial;  // never reused: how a context knows that the plan it holds on the device is this one
};

static_assert(SJMI_EXPLODE_MEMBERS_MAX_PATHS + 1 == SEL_MAX_PATHS, "a members plan's key takes the last cell of a row");

namespace sjmi {

namespace {

constexpr uint32_t EXP_BLOCK = 128;  // two waves: eight documents per workgroup and trip, as k_select
constexpr uint32_t EXP_BLOCK_DOCS = EXP_BLOCK / SEL_GROUP;
constexpr uint32_t EXP_MAX_GRID = 16384;  // a workgroup loads the plan once and takes documents in a grid stride
constexpr uint32_t EXP_SCAN_DOCS = 1024;  // documents per workgroup of the scan's passes
// the rows a group buffers before it stores them: EXP_ROWS at most, and as many as EXP_CELLS cells hold for the plan's paths
// and, under a members plan, the key (12 columns: 8 rows = 64-byte runs in a value column; 64 columns: one row)
constexpr uint32_t EXP_ROWS = 8;
constexpr uint32_t EXP_CELLS = 96;

template <bool MEMBERS>
__global__ __launch_bounds__(EXP_BLOCK) void k_explode_count(const sj_u64* __restrict__ plan_image, uint32_t image_words,
                                                              const sj_u64* __restrict__ tape,
                                                              const unsigned long long* __restrict__ tape_offsets,
                                                              const int32_t* __restrict__ doc_errors, const uint8_t* __restrict__ sb,
                                                              uint64_t n_docs, uint32_t* __restrict__ counts, uint32_t* __restrict__ bases) {
    extern __shared__ sj_u64 lds_plan[];
    __shared__ SelScratch scratch[EXP_BLOCK_DOCS];
    const SelHeader* plan = stage_plan<EXP_BLOCK>(lds_plan, plan_image, image_words);
    Lanes16 g = group_lanes();
    SelScratch& s = scratch[threadIdx.x / SEL_GROUP];
    for (uint64_t doc = (uint64_t)blockIdx.x * EXP_BLOCK_DOCS + threadIdx.x / SEL_GROUP; doc < n_docs;
         doc += (uint64_t)gridDim.x * EXP_BLOCK_DOCS) {
        if (g.lane == 0) {  // MISSING until the walk says otherwise
            s.types[0] = 0;
            s.values[0] = 0;
        }
        g.fence();
        uint32_t n = 0, base = 0;
        if (doc_errors[doc] == 0) {  // (a failed document's tape slot is never read: its contents are unspecified)
            const SelDoc d = sel_stage(g, tape + tape_offsets[doc], doc_words(tape_offsets, doc), sb, s);
            n = sel_explode_count<MEMBERS>(g, plan, d, s, &base);
        }
        if (g.lane == 0) {
            counts[doc] = n;
            bases[doc] = base;
        }
        g.fence();
    }
}

// ---- the counts' exclusive scan: sums per EXP_SCAN_DOCS documents, their scan by one workgroup, the offsets ----------------
__global__ void __launch_bounds__(1024) k_explode_chunk_sums(const uint32_t* __restrict__ counts, uint64_t n_docs,
                                                              unsigned long long* __restrict__ chunk_sums) {
    __shared__ unsigned long long s_wave[16];
    const uint64_t k = (uint64_t)blockIdx.x * EXP_SCAN_DOCS + threadIdx.x;
    unsigned long long total;
    (void)block_excl_scan(k < n_docs ? counts[k] : 0u, s_wave, &total);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = total;
}
__global__ void __launch_bounds__(1024) k_explode_chunk_scan(unsigned long long* __restrict__ chunk_sums, uint64_t nchunks, uint64_t n_docs,
                                                              unsigned long long* __restrict__ row_offsets) {
    __shared__ unsigned long long s_wave[16];
    const unsigned long long carry = block_scan_in_place(chunk_sums, nchunks, s_wave);
    if (threadIdx.x == 0) {
        row_offsets[0] = 0;
        row_offsets[n_docs] = carry;  // the total number of rows
    }
}
__global__ void __launch_bounds__(1024) k_explode_offsets(const uint32_t* __restrict__ counts, uint64_t n_docs,
                                                           const unsigned long long* __restrict__ chunk_base,
                                                           unsigned long long* __restrict__ row_offsets) {
    __shared__ unsigned long long s_wave[16];
    const uint64_t k = (uint64_t)blockIdx.x * EXP_SCAN_DOCS + threadIdx.x;
    unsigned long long total;
    const unsigned long long off = chunk_base[blockIdx.x] + block_excl_scan(k < n_docs ? counts[k] : 0u, s_wave, &total);
    if (k < n_docs) row_offsets[k] = off;
}

// what a group buffers of its rows: cell (p, q) of the buffered rows at p * rows + q, in sel_emit's form
struct RowBuf {
    sj_u64 values[EXP_CELLS];
    uint8_t types[EXP_CELLS];
};

template <bool MEMBERS>
__global__ __launch_bounds__(EXP_BLOCK) void k_explode_rows(const sj_u64* __restrict__ plan_image, uint32_t image_words,
                                                             const sj_u64* __restrict__ tape,
                                                             const unsigned long long* __restrict__ tape_offsets,
                                                             const uint8_t* __restrict__ sb, uint64_t n_docs,
                                                             const uint32_t* __restrict__ counts, const uint32_t* __restrict__ bases,
                                                             const unsigned long long* __restrict__ row_offsets, uint64_t row_capacity,
                                                             uint32_t rows, uint8_t* __restrict__ types, sj_u64* __restrict__ values) {
    extern __shared__ sj_u64 lds_plan[];
    __shared__ SelScratch scratch[EXP_BLOCK_DOCS];
    __shared__ RowBuf bufs[EXP_BLOCK_DOCS];
    const SelHeader* plan = stage_plan<EXP_BLOCK>(lds_plan, plan_image, image_words);
    const uint32_t n_paths = plan->n_paths + (MEMBERS ? 1u : 0u);  // the columns: the key's cell lies behind the paths'
    Lanes16 g = group_lanes();
    SelScratch& s = scratch[threadIdx.x / SEL_GROUP];
    RowBuf& b = bufs[threadIdx.x / SEL_GROUP];
    for (uint64_t doc = (uint64_t)blockIdx.x * EXP_BLOCK_DOCS + threadIdx.x / SEL_GROUP; doc < n_docs;
         doc += (uint64_t)gridDim.x * EXP_BLOCK_DOCS) {
        const uint32_t base = bases[doc], n = counts[doc];
        const unsigned long long first = row_offsets[doc];
        if (!base || !n || first >= row_capacity) continue;  // (base != 0: the document did not fail, k_explode_count read its tape)
        // the elements whose rows lie below the capacity: the others are neither walked nor stored
        const uint32_t limit = row_capacity - first < n ? (uint32_t)(row_capacity - first) : n;
        const SelDoc d = sel_stage(g, tape + tape_offsets[doc], doc_words(tape_offsets, doc), sb, s);
        sel_explode_rows<MEMBERS>(g, plan, d, s, base, limit, [&](uint32_t j) {
            const uint32_t q = j % rows;
            for (uint32_t p = g.lane; p < n_paths; p += SEL_GROUP) {
                b.types[p * rows + q] = s.types[p];
                b.values[p * rows + q] = s.values[p];
            }
            g.fence();
            if (q + 1 != rows && j + 1 != limit) return;
            // the buffered rows [j - q, j]: in every column a run of q + 1 neighbouring rows; the string headers of all of
            // them are read here, side by side
            const unsigned long long r0 = first + (j - q);
            for (uint32_t i = g.lane; i < n_paths * (q + 1); i += SEL_GROUP) {
                const uint32_t p = i / (q + 1), e = i % (q + 1);
                if (r0 + e < row_capacity) {
                    const uint8_t t = b.types[p * rows + e];
                    types[(uint64_t)p * row_capacity + r0 + e] = t;
                    values[(uint64_t)p * row_capacity + r0 + e] = sel_finish(t, b.values[p * rows + e], sb);
                }
            }
            g.fence();
        });
    }
}

}  // namespace

const void* explode_plan_image(const sjmi_explode_plan* plan, size_t* bytes, size_t* base_bytes, uint64_t* serial, uint32_t* n_cols,
                               bool* members) {
    *bytes = plan->image.size() * sizeof(sj_u64);
    *base_bytes = plan->base_words * sizeof(sj_u64);
    *serial = plan->serial;
    *members = plan->members;
    *n_cols = ((const SelHeader*)(plan->image.data() + plan->base_words))->n_paths + (plan->members ? 1u : 0u);
    return plan->image.data();
}

size_t explode_workspace_bytes(uint64_t n_docs) {
    // counts [n] | base tape indexes [n] | chunk sums
    return 2 * ((n_docs * sizeof(uint32_t) + 63) / 64 * 64) + ((n_docs + EXP_SCAN_DOCS - 1) / EXP_SCAN_DOCS + 2) * sizeof(unsigned long long);
}

hipError_t explode_launch(const void* d_plan, size_t plan_bytes, size_t base_bytes, uint32_t n_cols, bool members, const void* d_tape,
                          const void* d_tape_offsets, const void* d_doc_errors, const void* d_string_buffer, uint64_t n_docs, void* d_ws,
                          void* d_row_offsets, uint64_t row_capacity, void* d_types, void* d_values, hipStream_t stream) {
    uint8_t* ws = static_cast<uint8_t*>(d_ws);
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws);
    uint32_t* bases = reinterpret_cast<uint32_t*>(ws + (n_docs * sizeof(uint32_t) + 63) / 64 * 64);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(ws + 2 * ((n_docs * sizeof(uint32_t) + 63) / 64 * 64));
    const uint64_t need = (n_docs + EXP_BLOCK_DOCS - 1) / EXP_BLOCK_DOCS;
    const uint32_t grid = need < EXP_MAX_GRID ? (uint32_t)need : EXP_MAX_GRID;
    const uint64_t nchunks = (n_docs + EXP_SCAN_DOCS - 1) / EXP_SCAN_DOCS;
    const sj_u64* base_plan = (const sj_u64*)d_plan;
    const sj_u64* elem_plan = base_plan + base_bytes / 8;
    if (n_docs) {
        hipLaunchKernelGGL(members ? k_explode_count<true> : k_explode_count<false>, dim3(grid), dim3(EXP_BLOCK), base_bytes, stream, base_plan,
                           (uint32_t)(base_bytes / 8),
                           (const sj_u64*)d_tape, (const unsigned long long*)d_tape_offsets, (const int32_t*)d_doc_errors,
                           (const uint8_t*)d_string_buffer, n_docs, counts, bases);
        hipLaunchKernelGGL(k_explode_chunk_sums, dim3((unsigned)nchunks), dim3(1024), 0, stream, (const uint32_t*)counts, n_docs, sums);
    }
    hipLaunchKernelGGL(k_explode_chunk_scan, dim3(1), dim3(1024), 0, stream, sums, nchunks, n_docs, (unsigned long long*)d_row_offsets);
    if (n_docs)
        hipLaunchKernelGGL(k_explode_offsets, dim3((unsigned)nchunks), dim3(1024), 0, stream, (const uint32_t*)counts, n_docs,
                           (const unsigned long long*)sums, (unsigned long long*)d_row_offsets);
    if (n_docs && n_cols && row_capacity) {
        uint32_t rows = EXP_CELLS / n_cols;
        rows = rows < 1 ? 1 : rows > EXP_ROWS ? EXP_ROWS : rows;
        const size_t elem_bytes = plan_bytes - base_bytes;
        hipLaunchKernelGGL(members ? k_explode_rows<true> : k_explode_rows<false>, dim3(grid), dim3(EXP_BLOCK), elem_bytes, stream, elem_plan,
                           (uint32_t)(elem_bytes / 8),
                           (const sj_u64*)d_tape, (const unsigned long long*)d_tape_offsets, (const uint8_t*)d_string_buffer, n_docs,
                           (const uint32_t*)counts, (const uint32_t*)bases, (const unsigned long long*)d_row_offsets, row_capacity, rows,
                           (uint8_t*)d_types, (sj_u64*)d_values);
    }
    return hipGetLastError();
}

}  // namespace sjmi

// both kinds of plan: the rules are one, a members plan leaves the last cell to the key
static int explode_compile(bool members, const uint8_t* base_pointer, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                           uint64_t n_paths, sjmi_explode_plan** out) {
    static std::atomic<uint64_t> next_serial{1};
    if (!out) return SJMI_ERR_ARG;
    *out = nullptr;
    if (members && n_paths > SJMI_EXPLODE_MEMBERS_MAX_PATHS) return SJMI_ERR_ARG;
    if (base_len && !base_pointer) return SJMI_ERR_ARG;
    if (n_paths && (!pointer_offsets || (!pointers && pointer_offsets[n_paths] != pointer_offsets[0]))) return SJMI_ERR_ARG;
    sjmi_explode_plan* plan = new (std::nothrow) sjmi_explode_plan();
    if (!plan) return SJMI_ERR_ARG;
    const uint64_t base_offsets[2] = {0, base_len};
    std::vector<sj_u64> elems;
    if (!sel_compile(base_pointer, base_offsets, 1, &plan->image) || !sel_compile(pointers, pointer_offsets, n_paths, &elems)) {
        delete plan;
        return SJMI_ERR_ARG;
    }
    plan->base_words = plan->image.size();
    plan->image.insert(plan->image.end(), elems.begin(), elems.end());
    plan->members = members;
    plan->serial = next_serial.fetch_add(1);
    *out = plan;
    return SJMI_OK;
}

extern "C" {

int sjmi_explode_plan_compile(const uint8_t* base_pointer, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                              uint64_t n_paths, sjmi_explode_plan** out) {
    return explode_compile(false, base_pointer, base_len, pointers, pointer_offsets, n_paths, out);
}

int sjmi_explode_members_plan_compile(const uint8_t* base_pointer, uint64_t base_len, const uint8_t* pointers, const uint64_t* pointer_offsets,
                                      uint64_t n_paths, sjmi_explode_plan** out) {
    return explode_compile(true, base_pointer, base_len, pointers, pointer_offsets, n_paths, out);
}

void sjmi_explode_plan_destroy(sjmi_explode_plan* plan) { delete plan; }

}  // extern "C"
