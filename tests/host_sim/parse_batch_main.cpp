// SimdJsonParser::parseBatch (csrc/host/simdjson_parser.cpp) without a GPU, as a stand-alone program for the sanitizers.
// TEST ONLY: the engine ABI is stubbed by a CPU engine made of the oracle's C (oracle/sj_oracle.c: sjo_stage1,
// sjo_unescape_all), which keeps what include/sjmi.h promises of the two batch calls: per-document status, no indexes from a
// failing document, indexes as offsets into the buffer handed in, string records in structural order with the offset of every
// document's first record.  The stub reads only [0, total_len) of that buffer, as the real engine's upload does, and can be
// told to fail one call with SJMI_ERR_HIP.  Everything else is the product's own code: the sub-batch plan, the feeder threads
// and their hand-off, the worker pool, the walk into slabs and their placement.
// Inputs are restricted to documents whose strings all unescape (a failing string's marker record is the kernels' business).
// Built and run by tests/test_host_parse_batch.py under ThreadSanitizer and under AddressSanitizer + UBSan.
#include "../../simdjson-java_amd/csrc/host/simdjson_parser.cpp"
#include "../../oracle/sj_oracle.h"

#include <atomic>
#include <map>

// ---- the CPU engine -----------------------------------------------------------------------------------------------------------
struct sjmi_ctx {
    int ordinal = 0;              // 0: the parser's first context, 1: its second
    std::atomic<long> calls{0};   // batch calls answered so far (stage 1 and string calls alike)
    std::atomic<long> failAt{-1}; // the call that is to fail, once
    std::string error;
    // the last stage-1 batch: a private copy of its bytes, and what stage 1 made of them
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> docOffsets, indexOffsets;
    std::vector<uint32_t> indexes;
};

static std::atomic<int> g_created{0};
static sjmi_ctx* g_ctx[2] = {nullptr, nullptr};

// fail the n-th batch call from now on context `ordinal` (n = 0: its next call)
static void failCall(int ordinal, long n) { g_ctx[ordinal]->failAt = g_ctx[ordinal]->calls + n; }

static bool failsNow(sjmi_ctx* ctx, const char* what) {
    const long call = ctx->calls++;
    if (call != ctx->failAt) return false;
    ctx->failAt = -1;
    ctx->error = std::string("injected failure in ") + what;
    return true;
}

extern "C" {
int sjmi_create(sjmi_ctx** out, int, uint64_t) {
    sjmi_ctx* ctx = new sjmi_ctx();
    ctx->ordinal = g_created++;
    if (ctx->ordinal < 2) g_ctx[ctx->ordinal] = ctx;
    *out = ctx;
    return SJMI_OK;
}
void sjmi_destroy(sjmi_ctx* ctx) {
    if (ctx && ctx->ordinal < 2) g_ctx[ctx->ordinal] = nullptr;
    delete ctx;
}
const char* sjmi_last_error(const sjmi_ctx* ctx) { return ctx->error.c_str(); }
int sjmi_host_register(sjmi_ctx*, void*, uint64_t) { return SJMI_ERR_NO_DEVICE; }  // (the parser: "not pinned")
int sjmi_set_input_staging(sjmi_ctx*, void*, uint64_t) { return SJMI_ERR_NO_DEVICE; }
int sjmi_host_unregister(sjmi_ctx*, void*) { return SJMI_ERR_NO_DEVICE; }
// the single-document entry points are not what this program is about
int sjmi_stage1_unescape(sjmi_ctx*, const uint8_t*, uint64_t, uint32_t*, uint64_t, uint64_t*, uint32_t*, uint8_t*, uint64_t,
                         uint64_t*, uint64_t*, uint32_t*) { return SJMI_ERR_NO_DEVICE; }
int sjmi_stage1(sjmi_ctx*, const uint8_t*, uint64_t, uint32_t*, uint64_t, uint64_t*, uint32_t*) { return SJMI_ERR_NO_DEVICE; }
int sjmi_parse_document(sjmi_ctx*, const uint8_t*, uint64_t, int, uint64_t*, uint64_t, uint64_t*, uint8_t*, uint64_t, uint64_t*, int32_t*,
                        uint32_t*) { return SJMI_ERR_NO_DEVICE; }

int sjmi_stage1_batch_isolated(sjmi_ctx* ctx, const uint8_t* buf, uint64_t total_len, const uint64_t* doc_offsets, uint64_t n_docs,
                               uint32_t* indexes, uint64_t index_capacity, uint64_t* index_offsets, uint32_t* doc_status,
                               uint64_t* count, uint32_t* status) {
    if (failsNow(ctx, "sjmi_stage1_batch_isolated")) return SJMI_ERR_HIP;
    ctx->bytes.assign(buf, buf + total_len);
    ctx->docOffsets.assign(doc_offsets, doc_offsets + n_docs + 1);
    ctx->indexes.clear();
    ctx->indexOffsets.assign(n_docs + 1, 0);
    uint32_t all = 0;
    std::vector<uint8_t> padded;
    std::vector<uint32_t> own;
    for (uint64_t k = 0; k < n_docs; ++k) {
        const uint64_t lo = doc_offsets[k], len = doc_offsets[k + 1] - lo;
        padded.assign(len + 64, 0);
        if (len) memcpy(padded.data(), ctx->bytes.data() + lo, len);
        own.assign(len + 2, 0);
        uint64_t n = 0;
        uint32_t st = 0;
        if (sjo_stage1(padded.data(), len, own.data(), own.size(), &n, &st) != 0) return SJMI_ERR_INTERNAL;
        doc_status[k] = st;
        all |= st;
        if (st == 0)
            for (uint64_t i = 0; i < n; ++i) ctx->indexes.push_back(own[i] + (uint32_t)lo);
        ctx->indexOffsets[k + 1] = ctx->indexes.size();
    }
    if (ctx->indexes.size() + 1 > index_capacity) {
        ctx->error = "index capacity";
        return SJMI_ERR_CAPACITY;
    }
    if (!ctx->indexes.empty()) memcpy(indexes, ctx->indexes.data(), ctx->indexes.size() * sizeof(uint32_t));
    indexes[ctx->indexes.size()] = 0;  // BitIndexes.finish's sentinel
    memcpy(index_offsets, ctx->indexOffsets.data(), (n_docs + 1) * sizeof(uint64_t));
    *count = ctx->indexes.size();
    *status = all;
    return SJMI_OK;
}

int sjmi_unescape_batch(sjmi_ctx* ctx, uint8_t* string_buffer, uint64_t string_capacity, uint64_t* doc_string_offsets,
                        uint64_t* total_bytes, uint64_t* first_error_index, uint32_t* first_error_code) {
    if (failsNow(ctx, "sjmi_unescape_batch")) return SJMI_ERR_HIP;
    const uint64_t nDocs = ctx->docOffsets.size() - 1;
    uint64_t pos = 0;
    std::vector<uint8_t> padded;
    std::vector<uint32_t> own;
    for (uint64_t k = 0; k < nDocs; ++k) {
        doc_string_offsets[k] = pos;
        const uint64_t lo = ctx->docOffsets[k], len = ctx->docOffsets[k + 1] - lo;
        const uint64_t from = ctx->indexOffsets[k], n = ctx->indexOffsets[k + 1] - from;
        if (!n) continue;
        padded.assign(len + 64, 0);
        if (len) memcpy(padded.data(), ctx->bytes.data() + lo, len);
        own.resize(n);
        for (uint64_t i = 0; i < n; ++i) own[i] = ctx->indexes[from + i] - (uint32_t)lo;
        uint64_t strings = 0;
        int64_t failed = -1;
        int code = 0;
        pos += sjo_unescape_all(padded.data(), own.data(), n, string_buffer + pos, string_capacity - pos, nullptr, &strings, &failed, &code);
        if (failed >= 0) {  // (this program's inputs have none; capacity shows here too)
            ctx->error = "a string did not unescape: code " + std::to_string(code);
            return SJMI_ERR_ARG;
        }
    }
    doc_string_offsets[nDocs] = pos;
    *total_bytes = pos;
    *first_error_index = 0;
    *first_error_code = 0;
    return SJMI_OK;
}
}  // extern "C"

// ---- inputs -------------------------------------------------------------------------------------------------------------------
namespace {

struct Rng {  // xorshift64*: the same documents everywhere
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    size_t below(size_t n) { return (size_t)(next() % n); }
};

struct Batch {
    std::string name;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets{0};
    size_t docs() const { return offsets.size() - 1; }
    void add(const std::string& doc) {  // NDJSON-style: the document's range includes its '\n'
        bytes.insert(bytes.end(), doc.begin(), doc.end());
        bytes.push_back('\n');
        offsets.push_back(bytes.size());
    }
};

std::string value(Rng& rng, int depth) {
    static const char* const atoms[] = {"\"s\"", "\"a\\nb\"", "\"\xc3\xa9\xe2\x82\xac\"", "\"\\u00e9\"", "\"\\uD83D\\uDE00 \\\\ \\\"\"", "1", "-2.5e3",
                                        "true", "false", "null", "\"\"", "12345678", "0.1", "\"a longer string value, no escapes\""};
    const size_t r = rng.below(100);
    if (depth > 3 || r < 35) return atoms[rng.below(sizeof atoms / sizeof *atoms)];
    std::string s;
    const size_t n = rng.below(7);
    if (r < 65) {
        s = "[";
        for (size_t i = 0; i < n; ++i) s += (i ? "," : "") + value(rng, depth + 1);
        return s + "]";
    }
    s = "{";
    for (size_t i = 0; i < n; ++i) s += std::string(i ? "," : "") + "\"k" + std::to_string(i) + "\":" + value(rng, depth + 1);
    return s + "}";
}

// failing documents: stage 1 (unclosed string -- an even number of them cancels in a whole-batch parity --, broken UTF-8,
// unescaped characters), the grammar, and the empty document
const std::string kBad[] = {"[\"abc", "{\"k\": \"v", "\"", "[\"\xc3\"]", "\"\x80\"", "[\"\xe2\x82\"]", "[\"a\x01" "b\"]", "[\"tab\there\"]",
                            "[1 1]", "[1,,1]", "{\"a\" 1}", "[1,2", "{\"a\":1,}", "tru", "[01]", "1 2", "[-]", "nul", "[", "{\"a\":{}", "", ""};

Batch manyDocuments(size_t n, uint64_t seed) {
    Batch b;
    b.name = "many";
    Rng rng{seed};
    size_t bad = 0;
    for (size_t k = 0; k < n; ++k) {
        if (k % 23 == 7 || k + 1 == n) b.add(kBad[bad++ % (sizeof kBad / sizeof *kBad)]);  // (the last document fails too)
        else b.add("{\"id\":" + std::to_string(k) + ",\"v\":" + value(rng, 0) + ",\"w\":" + value(rng, 1) + "}");
    }
    return b;
}

std::string largeDocument(size_t bytes) {
    Rng rng{99};
    std::string s = "{\"statuses\":[";
    for (size_t k = 0; s.size() < bytes; ++k) s += std::string(k ? "," : "") + "{\"id\":" + std::to_string(k) + ",\"user\":" + value(rng, 1) + "}";
    return s + "],\"n\":1}";
}

Batch of(const char* name, const std::vector<std::string>& docs) {
    Batch b;
    b.name = name;
    for (const std::string& d : docs) b.add(d);
    return b;
}

// ---- the oracle's answer for a batch: every document parsed alone ----------------------------------------------------------------
struct Expected {
    std::vector<sjo_doc> docs;
    uint64_t structurals = 0;  // of the documents that pass stage 1
    explicit Expected(const Batch& b) : docs(b.docs()) {
        for (size_t k = 0; k < b.docs(); ++k) {
            sjo_parse(b.bytes.data() + b.offsets[k], b.offsets[k + 1] - b.offsets[k], 1024, &docs[k]);
            if (!docs[k].stage1_status) structurals += docs[k].n_structurals;
        }
    }
    ~Expected() {
        for (sjo_doc& d : docs) sjo_doc_free(&d);
    }
    Expected(const Expected&) = delete;
};

int g_failures = 0;
void complain(const std::string& what) {
    fprintf(stderr, "FAIL: %s\n", what.c_str());
    ++g_failures;
}

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

struct Result {
    std::vector<uint64_t> tape, offsets;
    std::vector<int32_t> errors;
    std::vector<uint8_t> strings;
};

Result resultOf(const org_simdjson::SimdJsonParser& p) {
    Result r;
    r.tape.assign(p.batchTape(), p.batchTape() + p.batchTapeLen());
    r.offsets = p.batchTapeOffsets();
    r.errors = p.batchErrors();
    r.strings.assign(p.stringBuffer().data(), p.stringBuffer().data() + p.stringBufferLen());
    return r;
}

// error code and tape of every document against the oracle's, word for word; a STRING word by the record it points at
void check(const std::string& what, const Batch& b, const Expected& want, const Result& got) {
    if (got.errors.size() != b.docs() || got.offsets.size() != b.docs() + 1 || got.offsets[0] != 0 || got.offsets.back() != got.tape.size())
        return complain(what + ": shape of the result");
    for (size_t k = 0; k < b.docs(); ++k) {
        const sjo_doc& w = want.docs[k];
        const std::string doc = what + " document " + std::to_string(k);
        if (got.errors[k] != w.error) {
            complain(doc + ": error " + std::to_string(got.errors[k]) + ", the oracle's " + std::to_string(w.error));
            continue;
        }
        const uint64_t lo = got.offsets[k], n = got.offsets[k + 1] - lo;
        if (n != (w.error ? 0 : w.tape_len)) {
            complain(doc + ": tape length");
            continue;
        }
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t g = got.tape[lo + i], e = w.tape[i];
            if ((e >> 56) != '"') {
                if (g != e) {
                    complain(doc + ": tape word " + std::to_string(i));
                    break;
                }
                continue;
            }
            const uint64_t go = g & 0x00FFFFFFFFFFFFFFull, eo = e & 0x00FFFFFFFFFFFFFFull;
            if ((g >> 56) != '"' || go + 4 > got.strings.size() || be32(&got.strings[go]) != be32(w.string_buffer + eo) ||
                go + 4 + be32(&got.strings[go]) > got.strings.size() ||
                memcmp(&got.strings[go], w.string_buffer + eo, 4 + (size_t)be32(w.string_buffer + eo)) != 0) {
                complain(doc + ": string word " + std::to_string(i));
                break;
            }
        }
    }
}

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void add(const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 0x100000001b3ull;
    }
    void add(const Result& r) {
        add(r.tape.data(), r.tape.size() * 8);
        add(r.offsets.data(), r.offsets.size() * 8);
        add(r.errors.data(), r.errors.size() * 4);
        const uint64_t n = r.strings.size();
        add(&n, 8);
    }
};

struct Config {
    int threads, pipeline;
};

// sub-batches of a batch under SJMI_PARSE_PIPELINE = pipeline: with one, string buffer and tapes are the same bytes everywhere
size_t subBatches(const Config& c, const Batch& b) { return std::max<size_t>(1, std::min<size_t>((size_t)c.pipeline, b.docs())); }

}  // namespace

int main() {
    Batch tiny = of("tiny", {"[1]", "{\"a\":\"b\"}", "tru"});
    Batch many = manyDocuments(2000, 81);
    Batch other = manyDocuments(700, 82);
    other.name = "other";
    const std::string big = largeDocument(256u << 10);
    const std::vector<Batch> batches = {
        // one parser, batches of changing shape: small -> large -> empty -> small, then another large one
        tiny, many, of("empty", {}), tiny, other,
        // sub-batch cuts with nothing in them (tests/test_gpu_batch.py test_parse_batch_odd_shapes)
        of("one", {"[1]"}), of("big among small", {"1", big, "\"s\"", "[2]"}), of("big first", {big, "{}"}),
        of("only failing", {"[", "\"", "nul"}), of("only empty", {"", "", "", "", ""})};
    std::vector<std::unique_ptr<Expected>> expected;
    size_t capacity = 0;
    for (const Batch& b : batches) {
        expected.emplace_back(new Expected(b));
        capacity = std::max(capacity, b.bytes.size() + 64);
    }
    const size_t iMany = 1;
    size_t failing = 0, stage1Failing = 0;
    for (const sjo_doc& d : expected[iMany]->docs) {
        failing += d.error != 0;
        stage1Failing += d.stage1_status != 0;
    }
    // enough structurals for a third of the batch to be walked as several ranges (4096 structurals per thread at least)
    if (expected[iMany]->structurals < 3 * 3 * 4096 || stage1Failing < 20 || failing - stage1Failing < 20)
        complain("the large batch is not what this program needs: " + std::to_string(expected[iMany]->structurals) + " structurals, " +
                 std::to_string(failing) + " failing documents");

    const Config configs[] = {{1, 1}, {3, 2}, {8, 3}, {2, 64}};
    std::map<size_t, Result> single;  // batch -> its result in the first configuration that took it as one sub-batch
    std::vector<std::vector<int32_t>> errors(batches.size());
    for (const Config& c : configs) {
        setenv("SJMI_PARSE_THREADS", std::to_string(c.threads).c_str(), 1);
        setenv("SJMI_PARSE_PIPELINE", std::to_string(c.pipeline).c_str(), 1);
        const std::string cfg = "(" + std::to_string(c.threads) + "," + std::to_string(c.pipeline) + ")";
        g_created = 0;
        org_simdjson::SimdJsonParser parser((int)capacity, 1024);
        Fnv digest;
        for (size_t b = 0; b < batches.size(); ++b) {
            const Batch& in = batches[b];
            const std::string what = cfg + " " + in.name;
            parser.parseBatch(in.bytes.data(), in.bytes.size(), in.offsets.data(), in.docs());
            const Result got = resultOf(parser);
            check(what, in, *expected[b], got);
            digest.add(got);
            // independent of the configuration: errors everywhere, tapes and strings wherever there is one sub-batch
            if (errors[b].empty()) errors[b] = got.errors;
            else if (errors[b] != got.errors) complain(what + ": errors differ between configurations");
            if (subBatches(c, in) == 1) {
                auto seen = single.find(b);
                if (seen == single.end()) single.emplace(b, got);
                else if (seen->second.tape != got.tape || seen->second.offsets != got.offsets || seen->second.strings != got.strings)
                    complain(what + ": tapes or strings differ between configurations with one sub-batch");
            }
        }
        // the failure path: one engine call fails -- stage 1 or the string call, of the first or of a later sub-batch --; the call
        // throws (no deadlock, no std::terminate) and the parser's next batch is right
        const size_t J = subBatches(c, many);
        std::vector<std::pair<int, long>> plans = {{0, 0}, {0, 1}};
        if (J >= 2) plans.insert(plans.end(), {{1, 0}, {1, 1}});
        if (J >= 3) plans.insert(plans.end(), {{0, 2}, {0, 3}});
        for (const std::pair<int, long>& plan : plans) {
            const std::string what = cfg + " failing call " + std::to_string(plan.second) + " of context " + std::to_string(plan.first);
            failCall(plan.first, plan.second);
            bool thrown = false;
            try {
                parser.parseBatch(many.bytes.data(), many.bytes.size(), many.offsets.data(), many.docs());
            } catch (const org_simdjson::JsonParsingException&) {
            } catch (const std::runtime_error& e) {
                thrown = strstr(e.what(), "injected failure") != nullptr;
            }
            if (!thrown) complain(what + ": parseBatch did not throw the engine's error");
            const Batch& next = plan.second % 2 ? other : many;
            parser.parseBatch(next.bytes.data(), next.bytes.size(), next.offsets.data(), next.docs());
            const Result got = resultOf(parser);
            check(what + ", the next batch", next, *expected[plan.second % 2 ? 4 : iMany], got);
            digest.add(got);
        }
        printf("parse_batch threads=%d sub-batches=%d digest=%016llx\n", c.threads, c.pipeline, (unsigned long long)digest.h);
    }
    if (g_failures) {
        fprintf(stderr, "%d failures\n", g_failures);
        return 1;
    }
    printf("all configurations agree with the oracle\n");
    return 0;
}
