// batch_stages.h -- the parts SimdJsonParser::parseBatch (simdjson_parser.cpp) is put together from: the plan of a batch
// (sub-batches, walk ranges: pure functions of the offsets), the record of one call that its stage routines share, and the
// hand-off between the caller's thread and the feeder threads.  Nothing here calls the engine.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace org_simdjson {

// The most sub-batches of one batch.  Sub-batch j's indexes lie 2 j behind its bytes' offset (below), so the parser's index
// array has 2 * MAX_SUB_BATCHES entries more than a single document needs, and SJMI_PARSE_PIPELINE is bounded by it.
constexpr size_t MAX_SUB_BATCHES = 64;

// Cut the n elements behind an ascending prefix array (prefix[k] = weight in front of element k; `total` = all of it) into
// `parts` contiguous ranges of about equal weight: cut[t] = the first element at which t / parts of the total is reached,
// never below cut[t - 1]; cut[0] = 0, cut[parts] = n.
inline std::vector<size_t> balancedCut(const uint64_t* prefix, size_t n, uint64_t total, size_t parts) {
    std::vector<size_t> cut(parts + 1, n);
    cut[0] = 0;
    for (size_t t = 1; t < parts; ++t) {
        const uint64_t want = total * t / parts;
        cut[t] = std::max(cut[t - 1], (size_t)(std::lower_bound(prefix, prefix + n, want) - prefix));
    }
    return cut;
}

// One sub-batch: whole documents [docLo, docHi) = bytes [byteStart, byteStart + byteLen) of the batch.  Its indexes, string
// records and index / string offsets are placed at fixed bases of the parser's shared arrays (sized for the worst case: one
// structural per byte, three string-buffer bytes per document byte), so with more than one sub-batch the string buffer has
// unused gaps between them; tape STRING payloads are offsets into that one buffer.
struct SubBatch {
    size_t docLo = 0, docHi = 0, byteStart = 0, byteLen = 0;
    size_t idxBase = 0;  // byteStart + 2 j: count + sentinel <= byteLen + 1
    size_t sbBase = 0;   // 3 byteStart + 8 j: 4 + L <= 2 (L + 2) for every string, so its records take <= 2 byteLen
    size_t offBase = 0;  // docLo + j: n + 1 offsets per sub-batch
    // the GPU part's results (written by its feeder, read by the caller once the sub-batch is ready)
    uint64_t count = 0, total = 0;  // structurals; bytes of string records
    std::vector<uint64_t> rel;      // document offsets relative to byteStart
    std::exception_ptr error;
    std::vector<size_t> cut;        // the walk: range t = documents [cut[t], cut[t + 1]) of the sub-batch
    double tGpu = 0, tWalk = 0;     // SJMI_PARSE_TIMING: ms since the call began
    size_t docs() const { return docHi - docLo; }
    size_t walkers() const { return cut.size() - 1; }
};

// How many sub-batches: about 8 MiB or more each, eight at the most; SJMI_PARSE_PIPELINE (`forced` > 0) overrides; never more
// than there are documents.
inline size_t subBatchCount(size_t totalLen, size_t nDocs, int forced) {
    size_t n = std::min<size_t>(8, totalLen / (8u << 20) + 1);
    if (forced > 0) n = (size_t)forced;
    if (n > nDocs) n = nDocs ? nDocs : 1;
    return n;
}

// The batch cut into `parts` sub-batches of whole documents and about equal bytes (some may be empty: one huge document).
inline std::vector<SubBatch> planSubBatches(const uint64_t* docOffsets, size_t nDocs, size_t totalLen, size_t parts) {
    const std::vector<size_t> cut = balancedCut(docOffsets, nDocs, totalLen, parts);
    std::vector<SubBatch> subs(parts);
    for (size_t j = 0; j < parts; ++j) {
        SubBatch& sb = subs[j];
        sb.docLo = cut[j];
        sb.docHi = cut[j + 1];
        sb.byteStart = nDocs ? (size_t)docOffsets[sb.docLo] : 0;
        sb.byteLen = nDocs ? (size_t)docOffsets[sb.docHi] - sb.byteStart : 0;
        sb.idxBase = sb.byteStart + 2 * j;
        sb.sbBase = 3 * sb.byteStart + 8 * j;
        sb.offBase = sb.docLo + j;
    }
    return subs;
}

// The walk of a sub-batch of n documents with `count` structurals (indexOffsets: its n + 1 index offsets) on up to `threads`
// threads: contiguous document ranges of about equal structural count, one per thread.
inline std::vector<size_t> planWalk(const uint64_t* indexOffsets, size_t n, uint64_t count, size_t threads) {
    const size_t minPerThread = 4096;  // structurals: below this a thread costs more than it walks
    size_t walkers = std::min(threads, (size_t)count / minPerThread + 1);
    if (walkers > n) walkers = n ? n : 1;
    return balancedCut(indexOffsets, n, count, walkers);
}

// One parseBatch call: its arguments, its plan and its clock -- what the stage routines share.
struct BatchCall {
    using Clock = std::chrono::steady_clock;
    const uint8_t* buffer;
    size_t totalLen;
    const uint64_t* docOffsets;
    size_t nDocs;
    size_t threads;
    std::vector<SubBatch> subs;
    Clock::time_point t0 = Clock::now();
    double tCopy = 0;
    double since() const { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
    // SJMI_PARSE_TIMING: the phase times of the call, one line on stderr
    void printTiming() const {
        fprintf(stderr, "parseBatch %zu docs %zu B, %zu threads, %zu sub-batches: copy+pad done at %.2f ms;", nDocs, totalLen, threads, subs.size(), tCopy);
        for (size_t j = 0; j < subs.size(); ++j) fprintf(stderr, " [%zu] gpu %.2f walked+placed %.2f;", j, subs[j].tGpu, subs[j].tWalk);
        fprintf(stderr, " done at %.2f ms\n", since());
    }
};

// The hand-off between the caller's thread and the feeders.  The caller copies the batch in sub-batch by sub-batch and marks
// each `copied`; feeder f (of one or two, each with an engine context of its own) waits for that, takes sub-batches f, f + 2,
// ... through the GPU and marks each `ready`; the caller waits for that before it walks one.
// Whatever is thrown on the caller's thread while the feeders run -- the pool, an allocation -- must not leave them waiting
// with joinable std::thread objects going out of scope (that is std::terminate): the destructor marks every sub-batch copied,
// so the feeders run dry, and joins them.
class FeederHandOff {
public:
    explicit FeederHandOff(size_t subBatches) : copied_(subBatches, false), ready_(subBatches, false) {}
    FeederHandOff(const FeederHandOff&) = delete;
    FeederHandOff& operator=(const FeederHandOff&) = delete;
    ~FeederHandOff() {
        {
            std::lock_guard<std::mutex> g(m_);
            copied_.assign(copied_.size(), true);
        }
        copiedCv_.notify_all();
        for (std::thread& th : feeders_)
            if (th.joinable()) th.join();
    }
    // start `feeders` (1 or 2) threads; feeder f runs gpuPart(j) for j = f, f + 2, ... (gpuPart does not throw)
    void start(size_t feeders, const std::function<void(size_t feeder, size_t j)>& gpuPart) {
        for (size_t f = 0; f < feeders && f < 2; ++f)
            feeders_[f] = std::thread([this, f, gpuPart] {
                for (size_t j = f; j < ready_.size(); j += 2) {
                    await(copiedCv_, copied_, j);
                    gpuPart(f, j);
                    mark(readyCv_, ready_, j);
                }
            });
    }
    void markCopied(size_t j) { mark(copiedCv_, copied_, j); }
    void awaitReady(size_t j) { await(readyCv_, ready_, j); }

private:
    void mark(std::condition_variable& cv, std::vector<bool>& marks, size_t j) {
        {
            std::lock_guard<std::mutex> g(m_);
            marks[j] = true;
        }
        cv.notify_all();
    }
    void await(std::condition_variable& cv, const std::vector<bool>& marks, size_t j) {
        std::unique_lock<std::mutex> g(m_);
        cv.wait(g, [&] { return (bool)marks[j]; });
    }
    std::mutex m_;
    std::condition_variable copiedCv_, readyCv_;
    std::vector<bool> copied_, ready_;  // per sub-batch, under m_
    std::thread feeders_[2];
};

}  // namespace org_simdjson
