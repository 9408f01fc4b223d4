// A stand-alone program around the host simulation's passes for a sanitizer run (nothing sanitized is loaded into Python):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -o joinrows_asan tests/host_sim/joinrows_asan_main.cpp && ./joinrows_asan [cases]
// Random adversarial sides through sj_joinrows.h with the sequential group: position counts around the wave and chunk edges, every
// type byte, keys from a handful of values (m x n runs), one value (a few positions with thousands of matches each), the ends of
// the range, or wide (few matches), poison behind every type byte that makes no candidate, with and without types, a validity
// bitmap, a device left count, carried columns on both sides, a left rows_in with BAD entries (n_source_rows, 2^32 - 1, 2^63), all
// four hows, a pair capacity above, at and below the pairs; the right side ordered by std::stable_sort as the sort would order
// it, or WILD: reversed, with entries above the source rows, on non-candidate cells, or noise; the chunks in three orders, small
// chunks.
// Every block is a heap allocation of EXACTLY its size -- the source columns end behind row n_source_rows - 1, rows_in behind the
// last LIVE position, the build order behind entry n_build, the outputs behind pair `capacity` and offset `n_left`; the scratch and
// a chunk's marks are such blocks inside joinrows_sim.cpp -- so one byte too far is a report.  Every run on a sorted right side is
// compared with a std::multimap join, every wild one with its flag and n_right_bad.  TEST ONLY.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

#include "joinrows_sim.cpp"

static uint64_t state = 0x2545F4914F6CDD1Dull;
static uint32_t rnd(uint32_t n) {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (uint32_t)((state >> 11) % n);
}
static uint64_t rnd64() { return ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 11) ^ rnd(1u << 31); }
template <class T>
static T* exact(const std::vector<T>& v, uint64_t n) {  // a heap block of exactly n entries
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n) memcpy(p, v.data(), n * sizeof(T));
    return p;
}

struct Side {
    uint64_t n;
    bool with_types, with_validity;
    std::vector<uint8_t> types, ctypes;
    std::vector<sj_u64> values, validity, cvalues;
    uint64_t n_cols, stride;
    bool candidate(uint64_t r) const {
        if (with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) return false;
        return !with_types || types[r] == 'l';
    }
    uint32_t cls(uint64_t r) const {  // 0 candidate, 1 null, 2 other
        if (with_validity && !((validity[r >> 6] >> (r & 63)) & 1)) return 1;
        if (!with_types || types[r] == 'l') return 0;
        return types[r] == 0 || types[r] == 'n' ? 1 : 2;
    }
};

static Side make_side(uint64_t n, uint32_t shape, bool with_types, bool with_validity, uint64_t n_cols) {
    static const int64_t ends[] = {INT64_MIN, -1, 0, 1, INT64_MAX};
    Side s;
    s.n = n, s.with_types = with_types, s.with_validity = with_validity, s.n_cols = n_cols, s.stride = n + rnd(3);
    s.types.resize(n), s.values.resize(n), s.validity.assign((n + 63) / 64, 0), s.ctypes.resize(n_cols * s.stride), s.cvalues.resize(n_cols * s.stride);
    for (uint64_t r = 0; r < n; ++r) {
        s.types[r] = rnd(5) ? (uint8_t)'l' : rnd(3) ? (uint8_t)"d\0n\"t["[rnd(6)] : (uint8_t)rnd(256);
        if (rnd(6)) s.validity[r >> 6] |= 1ull << (r & 63);
        if (with_types && s.types[r] != 'l')
            s.values[r] = rnd(2) ? ~0ull : 0x7FF8DEADBEEF0001ull;  // (poison: never read)
        else
            s.values[r] = shape == 0 ? (sj_u64)rnd(7) : shape == 1 ? (sj_u64)ends[rnd(5)] : shape == 2 ? (sj_u64)rnd(400) : shape == 3 ? rnd64() % 3000 : 42;
    }
    for (uint64_t j = 0; j < n_cols * s.stride; ++j) s.ctypes[j] = (uint8_t)rnd(256), s.cvalues[j] = rnd64();
    return s;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    static const uint64_t counts[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 4097};
    static const uint64_t bad_entries[] = {0, 0xFFFFFFFFull, 1ull << 63};  // (entry 0 stands for n_source_rows)
    unsigned long long runs = 0, pairs_seen = 0, wild_seen = 0, bad_seen = 0, overflow_seen = 0, hot = 0, unmatched = 0;
    for (int i = 0; i < cases; ++i) {
        const bool one_key = i % 11 == 10;  // a handful of left positions with thousands of matches each: output chunks that begin no position
        const uint64_t n_l = one_key ? 1 + rnd(9) : i < 10 ? counts[i] : rnd(4) ? rnd(2600) : counts[rnd(10)];
        const uint64_t n_r = one_key ? 2049 + rnd(2100) : i < 10 ? counts[9 - i] : rnd(4) ? rnd(1500) : counts[rnd(9)];
        const uint32_t shape = one_key ? 4 : rnd(4), how = i % 4, wild = i % 5 == 4 ? 1 + rnd(4) : 0;
        const Side L = make_side(n_l, shape, i % 5 != 0, i % 3 != 0, i % 4 == 3 ? 0 : 1 + i % 3);
        const Side R = make_side(n_r, shape, i % 7 != 0, i % 2 != 0, how < 2 ? i % 3 : 0);
        std::vector<sj_u64> rows_in;
        const bool with_rows = i % 3 == 1;
        if (with_rows)
            for (uint64_t r = 0; r < n_l + 3; ++r)
                if (rnd(3)) {
                    const uint64_t bad = bad_entries[rnd(3)];
                    rows_in.push_back(rnd(9) && r < n_l ? (rnd(4) ? r : rnd((uint32_t)n_l)) : bad ? bad : n_l);
                }
        const uint64_t n_left = with_rows ? rows_in.size() : n_l;
        sj_u64 lc = rnd((uint32_t)n_left + 5);
        const sj_u64* left_count = i % 2 ? &lc : nullptr;
        const uint64_t live = left_count && lc < n_left ? lc : n_left;
        // the build order as the sort writes it: the candidates by (key, position), then the rest
        std::vector<sj_u64> order;
        for (uint64_t r = 0; r < n_r; ++r)
            if (R.candidate(r)) order.push_back(r);
        std::stable_sort(order.begin(), order.end(), [&](sj_u64 a, sj_u64 b) { return (int64_t)R.values[a] < (int64_t)R.values[b]; });
        uint64_t n_cand = order.size(), want_right_bad = 0;
        for (uint64_t r = 0; r < n_r; ++r)
            if (!R.candidate(r)) order.push_back(r);
        if (wild == 1) {
            std::reverse(order.begin(), order.begin() + n_cand);
        } else if (wild == 2) {
            for (uint64_t p = 0; p < n_cand; p += 5) order[p] = p % 2 ? n_r + rnd(3) : bad_entries[1 + rnd(2)], ++want_right_bad;
        } else if (wild == 3) {
            for (uint64_t r = 0; r < n_r; ++r) order[r] = r;
            want_right_bad = n_r - n_cand;
            n_cand = n_r;  // (the record claims every position)
        } else if (wild == 4) {
            for (uint64_t r = 0; r < n_r; ++r) order[r] = rnd(2) ? rnd64() : rnd((uint32_t)n_r + 2);
            n_cand = n_r;
        }
        SrResult sort_record;
        memset(&sort_record, 0xEE, sizeof sort_record);
        sort_record.n_rows = n_r, sort_record.n_candidates = i % 6 == 5 ? n_cand + rnd(3) * (n_cand == n_r) : n_cand;
        const uint64_t n_build = n_cand;
        // the reference: a multimap from key to the build places, in place order
        std::multimap<int64_t, uint64_t> places;
        if (!wild)
            for (uint64_t p = 0; p < n_build; ++p) places.emplace_hint(places.end(), (int64_t)R.values[order[p]], p);
        std::vector<sj_u64> want_l, want_r, want_off(1, 0);
        uint64_t n_matched = 0, n_null = 0, n_other = 0, n_bad = 0;
        for (uint64_t p = 0; p < live; ++p) {
            const uint64_t l = with_rows ? rows_in[p] : p;
            uint64_t m = 0;
            const uint32_t cls = l >= n_l ? 3 : L.cls(l);
            n_null += cls == 1, n_other += cls == 2, n_bad += cls == 3;
            if (cls == 0) {
                const auto run = places.equal_range((int64_t)L.values[l]);
                for (auto it = run.first; it != run.second; ++it, ++m)
                    if (how == JR_INNER || how == JR_LEFT || (how == JR_SEMI && m == 0)) want_l.push_back(l), want_r.push_back(order[it->second]);
            }
            n_matched += m > 0;
            hot += m > 1024;
            if (!m && (how == JR_LEFT || how == JR_ANTI)) want_l.push_back(l), want_r.push_back(JR_NO_ROW), ++unmatched;
            want_off.push_back(want_l.size());
        }
        const uint64_t n_pairs = want_l.size();
        for (uint32_t chunk : {64u, JR_CHUNK_ROWS})
            for (uint32_t order_of = 0; order_of < 3; ++order_of)
                for (uint32_t cap_form = 0; cap_form < 3; ++cap_form) {
                    const uint64_t capacity = wild ? rnd(9000) : cap_form == 0 ? n_pairs + rnd(3) : cap_form == 1 ? n_pairs - (n_pairs > 0) : rnd((uint32_t)n_pairs + 1);
                    uint8_t* lt = L.with_types ? exact(L.types, n_l) : nullptr;
                    sj_u64* lval = exact(L.values, n_l);
                    sj_u64* lv = L.with_validity ? exact(L.validity, (n_l + 63) / 64) : nullptr;
                    uint8_t* rt = R.with_types ? exact(R.types, n_r) : nullptr;
                    sj_u64* rval = exact(R.values, n_r);
                    sj_u64* rv = R.with_validity ? exact(R.validity, (n_r + 63) / 64) : nullptr;
                    sj_u64* ri = with_rows ? exact(rows_in, live) : nullptr;
                    sj_u64* ord = exact(order, n_build < n_r ? n_build : n_r);
                    uint8_t* lct = exact(L.ctypes, L.n_cols * L.stride);
                    sj_u64* lcv = exact(L.cvalues, L.n_cols * L.stride);
                    uint8_t* rct = exact(R.ctypes, R.n_cols * R.stride);
                    sj_u64* rcv = exact(R.cvalues, R.n_cols * R.stride);
                    sj_u64* out_l = (sj_u64*)malloc(capacity ? capacity * 8 : 1);
                    sj_u64* out_r = (sj_u64*)malloc(capacity ? capacity * 8 : 1);
                    uint8_t* lot = (uint8_t*)malloc(L.n_cols * capacity ? L.n_cols * capacity : 1);
                    sj_u64* lov = (sj_u64*)malloc(L.n_cols * capacity ? L.n_cols * capacity * 8 : 1);
                    uint8_t* rot = (uint8_t*)malloc(R.n_cols * capacity ? R.n_cols * capacity : 1);
                    sj_u64* rov = (sj_u64*)malloc(R.n_cols * capacity ? R.n_cols * capacity * 8 : 1);
                    sj_u64* off = (sj_u64*)malloc((n_left + 1) * 8);
                    SrResult* rec = (SrResult*)malloc(sizeof(SrResult));
                    JrResult* res = (JrResult*)malloc(sizeof(JrResult));
                    memset(out_l, 0xEE, capacity * 8), memset(out_r, 0xEE, capacity * 8), memset(lot, 0xEE, L.n_cols * capacity);
                    memset(lov, 0xEE, L.n_cols * capacity * 8), memset(rot, 0xEE, R.n_cols * capacity), memset(rov, 0xEE, R.n_cols * capacity * 8);
                    memset(off, 0xEE, (n_left + 1) * 8), memset(res, 0xEE, sizeof *res);
                    *rec = sort_record;
                    const JrArgs a = {{lt, lv, lval, n_l, ri, n_left, left_count, SR_LONG, 0u, chunk, SR_TILE_ROWS},
                                      {rt, rv, rval, n_r, ord, n_r, n_r ? &rec->n_candidates : nullptr, SR_LONG, 0u, chunk, SR_TILE_ROWS},
                                      {lct, lcv, L.n_cols, L.stride},
                                      {rct, rcv, R.n_cols, R.stride},
                                      how,
                                      chunk,
                                      capacity,
                                      out_l,
                                      how < 2 || rnd(2) ? out_r : nullptr,
                                      lot,
                                      lov,
                                      rot,
                                      rov,
                                      capacity,
                                      rnd(4) ? off : nullptr};
                    jr_sim_passes(a, order_of, res);
                    ++runs;
                    bool ok = res->n_left == live && res->n_build == (n_build < n_r ? n_build : n_r) && res->n_null == n_null && res->n_other == n_other &&
                              res->n_bad == n_bad && res->reserved == 0 && !(res->flags & ~7u) && !(res->flags & JR_BAD_ROW) == !n_bad &&
                              !(res->flags & JR_OVERFLOW) == (res->n_pairs <= capacity);
                    if (wild) {
                        // (a reversed run of equal keys and noise that happens to ascend set nothing; a bad place always does)
                        ok = ok && (wild == 4 || res->n_right_bad == want_right_bad) && (!res->n_right_bad || (res->flags & JR_BAD_ORDER));
                        wild_seen += (res->flags & JR_BAD_ORDER) != 0;
                    } else {
                        ok = ok && res->n_pairs == n_pairs && res->n_matched == n_matched && res->n_right_bad == 0 && !(res->flags & JR_BAD_ORDER);
                        for (uint64_t j = 0; ok && j < capacity; ++j) {
                            const bool in = j < n_pairs;
                            ok = out_l[j] == (in ? want_l[j] : 0xEEEEEEEEEEEEEEEEull);
                            if (a.right_rows) ok = ok && out_r[j] == (in ? want_r[j] : 0xEEEEEEEEEEEEEEEEull);
                            for (uint64_t col = 0; ok && col < L.n_cols; ++col) {
                                const bool bad = in && want_l[j] >= n_l;
                                ok = !in   ? lot[col * capacity + j] == 0xEE && lov[col * capacity + j] == 0xEEEEEEEEEEEEEEEEull
                                     : bad ? lot[col * capacity + j] == 0 && lov[col * capacity + j] == 0
                                           : lot[col * capacity + j] == L.ctypes[col * L.stride + want_l[j]] && lov[col * capacity + j] == L.cvalues[col * L.stride + want_l[j]];
                            }
                            for (uint64_t col = 0; ok && col < R.n_cols; ++col) {
                                const bool none = in && want_r[j] == JR_NO_ROW;
                                ok = !in    ? rot[col * capacity + j] == 0xEE && rov[col * capacity + j] == 0xEEEEEEEEEEEEEEEEull
                                     : none ? rot[col * capacity + j] == 0 && rov[col * capacity + j] == 0
                                            : rot[col * capacity + j] == R.ctypes[col * R.stride + want_r[j]] && rov[col * capacity + j] == R.cvalues[col * R.stride + want_r[j]];
                            }
                        }
                        if (a.pair_offsets)
                            for (uint64_t p = 0; ok && p <= n_left; ++p) ok = off[p] == (p <= live ? want_off[p] : 0xEEEEEEEEEEEEEEEEull);
                    }
                    overflow_seen += (res->flags & JR_OVERFLOW) != 0;
                    free(lt), free(lval), free(lv), free(rt), free(rval), free(rv), free(ri), free(ord), free(lct), free(lcv), free(rct), free(rcv);
                    free(out_l), free(out_r), free(lot), free(lov), free(rot), free(rov), free(off), free(rec), free(res);
                    if (!ok) return fprintf(stderr, "case %d: how %u, wild %u, chunk %u, order %u, capacity form %u differs from the reference\n", i, how, wild, chunk, order_of, cap_form), 1;
                }
        pairs_seen += n_pairs, bad_seen += n_bad;
    }
    printf("%d cases, %llu runs: %llu pairs, %llu unmatched pairs, %llu bad left entries, %llu positions above 1024 matches, %llu wild runs flagged, %llu overflows; all runs agree with the reference\n",
           cases, runs, pairs_seen, unmatched, bad_seen, hot, wild_seen, overflow_seen);
    return pairs_seen && unmatched && bad_seen && hot && wild_seen && overflow_seen ? 0 : 1;
}
