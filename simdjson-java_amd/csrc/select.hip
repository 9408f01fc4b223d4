// select.hip -- the device-resident selector (include/sjmi.h, sjmi_select_*): every path of a compiled plan on every
// document of a parsed batch, into one typed column per path.  The walk itself is sj_select.h (shared with the host
// simulation, tests/host_sim/sel_sim.cpp), the 16-lane form of its group primitives is Lanes16 of sj_group.h; this file is the
// plan object and k_select.
#include <hip/hip_runtime.h>

#include <atomic>
#include <new>

#include "sj_group.h"
#include "stage1.h"

struct sjmi_select_plan {
    std::vector<sj_u64> image;
    uint64_t serial;  // never reused: how a context knows that the plan it holds on the device is this one
};

namespace sjmi {

namespace {

constexpr uint32_t SEL_BLOCK = 128;                          // two waves: eight documents per workgroup and trip
constexpr uint32_t SEL_BLOCK_DOCS = SEL_BLOCK / SEL_GROUP;
constexpr uint32_t SEL_MAX_GRID = 16384;                     // a workgroup loads the plan once and takes documents in a grid stride

__global__ __launch_bounds__(SEL_BLOCK) void k_select(const sj_u64* __restrict__ plan_image, uint32_t image_words,
                                                       const sj_u64* __restrict__ tape,
                                                       const unsigned long long* __restrict__ tape_offsets,
                                                       const int32_t* __restrict__ doc_errors, const uint8_t* __restrict__ sb,
                                                       uint64_t n_docs, uint8_t* __restrict__ types, sj_u64* __restrict__ values) {
    extern __shared__ sj_u64 lds_plan[];
    __shared__ SelScratch scratch[SEL_BLOCK_DOCS];
    const SelHeader* plan = stage_plan<SEL_BLOCK>(lds_plan, plan_image, image_words);
    const uint32_t n_paths = plan->n_paths;
    const uint32_t grp = threadIdx.x / SEL_GROUP;
    Lanes16 g = group_lanes();
    SelScratch& s = scratch[grp];
    for (uint64_t base = (uint64_t)blockIdx.x * SEL_BLOCK_DOCS; base < n_docs; base += (uint64_t)gridDim.x * SEL_BLOCK_DOCS) {
        for (uint32_t p = g.lane; p < n_paths; p += SEL_GROUP) {  // MISSING until the walk says otherwise
            s.types[p] = 0;
            s.values[p] = 0;
        }
        g.fence();
        const uint64_t doc = base + grp;
        if (doc < n_docs && doc_errors[doc] == 0) {  // (a failed document's tape slot is never read: its contents are unspecified)
            sel_document(g, plan, tape + tape_offsets[doc], doc_words(tape_offsets, doc), sb, s);
        }
        __syncthreads();
        // path-major columns: the workgroup's eight documents are neighbours in every column
        for (uint32_t i = threadIdx.x; i < n_paths * SEL_BLOCK_DOCS; i += SEL_BLOCK) {
            const uint32_t p = i / SEL_BLOCK_DOCS, k = i % SEL_BLOCK_DOCS;
            if (base + k < n_docs) {
                const uint8_t t = scratch[k].types[p];
                types[(uint64_t)p * n_docs + base + k] = t;
                values[(uint64_t)p * n_docs + base + k] = sel_finish(t, scratch[k].values[p], sb);
            }
        }
        __syncthreads();
    }
}

}  // namespace

const void* select_plan_image(const sjmi_select_plan* plan, size_t* bytes, uint64_t* serial, uint32_t* n_paths) {
    *bytes = plan->image.size() * sizeof(sj_u64);
    *serial = plan->serial;
    *n_paths = ((const SelHeader*)plan->image.data())->n_paths;
    return plan->image.data();
}

hipError_t select_launch(const void* d_plan, size_t plan_bytes, const void* d_tape, const void* d_tape_offsets, const void* d_doc_errors,
                         const void* d_string_buffer, uint64_t n_docs, void* d_types, void* d_values, hipStream_t stream) {
    if (!n_docs) return hipSuccess;
    const uint64_t need = (n_docs + SEL_BLOCK_DOCS - 1) / SEL_BLOCK_DOCS;
    const uint32_t grid = need < SEL_MAX_GRID ? (uint32_t)need : SEL_MAX_GRID;
    hipLaunchKernelGGL(k_select, dim3(grid), dim3(SEL_BLOCK), plan_bytes, stream, (const sj_u64*)d_plan, (uint32_t)(plan_bytes / 8),
                       (const sj_u64*)d_tape, (const unsigned long long*)d_tape_offsets, (const int32_t*)d_doc_errors,
                       (const uint8_t*)d_string_buffer, n_docs, (uint8_t*)d_types, (sj_u64*)d_values);
    return hipGetLastError();
}

}  // namespace sjmi

extern "C" {

int sjmi_select_plan_compile(const uint8_t* pointers, const uint64_t* pointer_offsets, uint64_t n_paths, sjmi_select_plan** out) {
    static std::atomic<uint64_t> next_serial{1};
    if (!out) return SJMI_ERR_ARG;
    *out = nullptr;
    if (n_paths && (!pointer_offsets || (!pointers && pointer_offsets[n_paths] != pointer_offsets[0]))) return SJMI_ERR_ARG;
    sjmi_select_plan* plan = new (std::nothrow) sjmi_select_plan();
    if (!plan) return SJMI_ERR_ARG;
    if (!sel_compile(pointers, pointer_offsets, n_paths, &plan->image)) {
        delete plan;
        return SJMI_ERR_ARG;
    }
    plan->serial = next_serial.fetch_add(1);
    *out = plan;
    return SJMI_OK;
}

void sjmi_select_plan_destroy(sjmi_select_plan* plan) { delete plan; }

}  // extern "C"
