// sj_select.h -- the device-resident selector: JSON Pointers (RFC 6901) compiled to a trie (the PLAN), and the walk that
// evaluates every path of the plan on ONE document's tape the way the reference's JsonValue.get (JsonValue.java:91-107) and
// ArrayIterator (:143-168) would, step by step.
//
// A group of SEL_GROUP lanes works on one document.  Everything that decides where the walk goes is the same in all lanes
// of the group (the computeNextIndex chain, Tape.java:86-98, the frames of the trie descent, the results); only two things
// are spread over the lanes: the copy of the tape into the group's slice, and the comparison of up to 16 member keys of the
// object at hand with the names of the trie node (sel_match_round).  The group primitives come from the caller: takes a group G
// of SEL_GROUP lanes (sj_group.h, Lanes16); uses: stride_first, stride, fence, ballot.  csrc/select.hip and csrc/explode.hip run
// this file with the 16-lane form (four groups to a wave), tests/host_sim/sel_sim.cpp and explode_sim.cpp with the sequential one
// (tests/host_sim/seq_group.h): it is compiled verbatim by all of them, so the CPU suite checks the walk the kernels run.
//
// The chain is walked serially, so whether a tape word is a header or the raw second word of an 'l' / 'd' entry is never a
// question: only words AT chain positions are read as headers (an int64 of 0x5B00000000000005 is a payload, not '[').
#pragma once
#include <stdint.h>
#include <string.h>

#include "sj_block.h"

// ---- limits of a plan (include/sjmi.h states them) ----------------------------------------------------------------------
constexpr uint32_t SEL_MAX_PATHS = 64;        // paths of a plan
constexpr uint32_t SEL_MAX_STEPS = 16;        // reference tokens of one path
constexpr uint32_t SEL_MAX_NAME_BYTES = 4096; // the plan's name table: every trie edge's unescaped token, padded to 8 bytes
// ---- shape of the walk ---------------------------------------------------------------------------------------------------
constexpr uint32_t SEL_GROUP = 16;        // lanes per document = members compared per round
constexpr uint32_t SEL_SLICE_WORDS = 256; // tape words of a document that are staged in the group's slice (configs[3]: ~135)
constexpr uint32_t SEL_NO_INDEX = 0xFFFFFFFFu;  // SelNode.index of a token that is no array index ("", "-", "01", "a")
constexpr uint32_t SEL_INDEX_HUGE = 0xFFFFFFFEu;  // ... and of a decimal too large to be one of any tape
constexpr uint32_t SEL_NO_PATH = 0xFFu;
constexpr uint32_t SEL_NO_CHILD = 0xFFu;

// The plan as the kernel sees it, one flat image of 8-byte words: [SelHeader][SelNode x n_nodes][names].  Node 0 is the root
// (the pointer ""); the children of a node lie next to each other.
struct SelNode {
    uint16_t first_child;  // node number of the first child
    uint16_t n_children;   // <= SEL_MAX_PATHS
    uint16_t name_word;    // the token that leads here: first 8-byte word of its bytes in the name table (zero padded)
    uint16_t name_len;     // ... and its length in bytes
    uint32_t index;        // the token as an array index, SEL_INDEX_HUGE, or SEL_NO_INDEX
    uint8_t path_first;    // first path that ends here (the others by SelHeader.path_next), or SEL_NO_PATH
    uint8_t pad[3];
};
struct SelHeader {
    uint32_t n_paths, n_nodes, name_words, image_words;
    uint8_t path_next[SEL_MAX_PATHS];  // paths with the same pointer are chained
};
static_assert(sizeof(SelNode) == 16 && sizeof(SelHeader) == 80, "the plan image is laid out in 8-byte words");

SJ_HD const SelNode* sel_nodes(const SelHeader* h) { return (const SelNode*)(h + 1); }
SJ_HD const sj_u64* sel_names(const SelHeader* h) { return (const sj_u64*)(sel_nodes(h) + h->n_nodes); }

// one container of the document that paths pass through, while its members are being enumerated
struct SelFrame {
    sj_u64 found;   // children of `node` that are decided (an object: matched; an array: matched, or no index at all)
    uint32_t pos;   // tape index of the next member to look at
    uint32_t end;   // tape index of the container's closing word (getMatchingBraceIndex - 1: the end of the iterator chain)
    uint32_t k;     // an array: element number of `pos`; an object: SEL_NO_INDEX
    uint32_t node;
};
// what one group needs besides the plan
struct SelScratch {
    sj_u64 slice[SEL_SLICE_WORDS];
    sj_u64 values[SEL_MAX_PATHS];
    SelFrame frames[SEL_MAX_STEPS];
    uint32_t memb[SEL_GROUP];   // tape index of the VALUE of member j of the round
    uint8_t mchild[SEL_GROUP];  // child of the frame's node that member j's key names, or SEL_NO_CHILD
    uint8_t types[SEL_MAX_PATHS];
};

struct SelDoc {
    const sj_u64* tape;  // the document's tape in global memory (tape[0] = the root word)
    uint32_t n;          // its words
    bool staged;         // the words are in the slice
    const uint8_t* sb;   // the batch's string buffer
};

SJ_HD sj_u64 sel_word(const SelDoc& d, const SelScratch& s, uint32_t i) {
    if (i >= d.n) return 0;  // (never for a tape the walkers wrote; a word of type 0 ends every walk)
    return d.staged ? s.slice[i] : d.tape[i];
}
SJ_HD uint32_t sel_type(sj_u64 w) { return (uint32_t)(w >> 56); }
SJ_HD bool sel_is_container(uint32_t t) { return t == '[' || t == '{'; }
// Tape.computeNextIndex (Tape.java:86-98), made to move forward whatever the words hold
SJ_HD uint32_t sel_next(const SelDoc& d, const SelScratch& s, uint32_t i, uint32_t end) {
    const sj_u64 w = sel_word(d, s, i);
    const uint32_t t = sel_type(w);
    uint32_t nx = i + 1;
    if (sel_is_container(t)) nx = (uint32_t)w;
    else if (t == 'l' || t == 'd') nx = i + 2;
    if (nx <= i || nx > end) nx = end;
    return nx;
}

// the result of the value at tape index v, for every path that ends at `node`
SJ_HD void sel_emit(const SelHeader* plan, const SelNode& node, const SelDoc& d, SelScratch& s, uint32_t v) {
    if (node.path_first == SEL_NO_PATH) return;
    const sj_u64 w = sel_word(d, s, v);
    uint32_t t = sel_type(w);
    sj_u64 val = 0;
    switch (t) {
        case 'l':
        case 'd': val = sel_word(d, s, v + 1); break;  // Tape.getInt64Value :69-71
        case 't': val = 1; break;
        case 'f':
        case 'n': break;
        case '"': val = w & 0x00FFFFFFFFFFFFFFull; break;  // the record's offset: sel_finish reads its length
        case '[':
        case '{': val = (((w >> 32) & 0xFFFFFFull) << 32) | v; break;  // Tape.getScopeCount :82-84
        default: t = 0; break;
    }
    for (uint32_t p = node.path_first; p != SEL_NO_PATH; p = plan->path_next[p]) {
        s.types[p] = (uint8_t)t;
        s.values[p] = val;
    }
}

// What the column holds for a result of sel_emit: a string's record is read here, by whoever stores the column, so that the
// records of a document's strings are fetched side by side and not one after the other inside the walk.
SJ_HD sj_u64 sel_finish(uint32_t type, sj_u64 val, const uint8_t* sb) {
    if (type != '"') return val;
    uint32_t be;  // JsonValue.getString :85-89
    memcpy(&be, sb + val, 4);
    const uint32_t len = (be >> 24) | ((be >> 8) & 0xFF00u) | ((be << 8) & 0xFF0000u) | (be << 24);
    return ((sj_u64)len << 32) | (uint32_t)(val + 4);
}

// Bytes [i, i + 8) of a key of `len` bytes at r (i a multiple of 8, i < len), zero padded behind the key: loads that never
// leave the key and never depend on one another -- a whole word, a word that ends with the key, or two / three pieces
SJ_HD sj_u64 sel_key_word(const uint8_t* r, uint32_t len, uint32_t i) {
    sj_u64 w;
    if (len - i >= 8) {
        memcpy(&w, r + i, 8);
        return w;
    }
    const uint32_t rest = len - i;  // 1..7
    if (len >= 8) {
        memcpy(&w, r + len - 8, 8);
        return w >> (8 * (8 - rest));
    }
    if (len >= 4) {
        uint32_t a, b;
        memcpy(&a, r, 4);
        memcpy(&b, r + len - 4, 4);
        return (sj_u64)a | ((sj_u64)b << (8 * (len - 4)));  // (bytes both pieces hold are the same bytes)
    }
    return (sj_u64)r[0] | ((sj_u64)r[len >> 1] << (8 * (len >> 1))) | ((sj_u64)r[len - 1] << (8 * (len - 1)));
}

// One round over an object: the keys of up to SEL_GROUP members from f.pos on against the undecided children of the frame's
// node.  -> bit j set = member j names one of them (s.mchild[j]); *n_members, *next_pos = what the round covered.
template <class G>
SJ_HD uint32_t sel_match_round(G& g, const SelHeader* plan, const SelDoc& d, SelScratch& s, const SelFrame& f, uint32_t* next_pos) {
    // the chain, the same in every lane: key at p (a string: one word), value at p + 1
    uint32_t m = 0, p = f.pos;
    while (m < SEL_GROUP && p + 1 < f.end) {
        s.memb[m++] = p + 1;
        p = sel_next(d, s, p + 1, f.end);
    }
    *next_pos = p + 1 < f.end ? p : f.end;
    g.fence();
    const SelNode& node = sel_nodes(plan)[f.node];
    const SelNode* kids = sel_nodes(plan) + node.first_child;
    const sj_u64* names = sel_names(plan);
    const sj_u64 found = f.found;
    const uint32_t hits = g.ballot([&](uint32_t j) -> bool {
        if (j >= m) return false;
        const sj_u64 off = sel_word(d, s, s.memb[j] - 1) & 0x00FFFFFFFFFFFFFFull;
        const uint8_t* r = d.sb + off;  // the record: [be32 length][unescaped bytes] (StringParser.java:18-68)
        uint32_t be;
        memcpy(&be, r, 4);
        const uint32_t len = (be >> 24) | ((be >> 8) & 0xFF00u) | ((be << 8) & 0xFF0000u) | (be << 24);
        r += 4;
        // the key's first word is fetched once, whatever the number of names it is compared with; the words behind it only
        // when a name of the same length begins with the same eight bytes
        const sj_u64 kw0 = len ? sel_key_word(r, len, 0) : 0;  // (the empty key: nothing is read)
        uint32_t hit = SEL_NO_CHILD;
        for (uint32_t c = 0; c < node.n_children; ++c) {
            if (((found >> c) & 1) || kids[c].name_len != len) continue;
            const sj_u64* nm = names + kids[c].name_word;
            bool same = len == 0 || nm[0] == kw0;
            for (uint32_t i = 8; same && i < len; i += 8) same = sel_key_word(r, len, i) == nm[i >> 3];
            if (same) {  // (sibling names differ, so no other child can match)
                hit = c;
                break;
            }
        }
        s.mchild[j] = (uint8_t)hit;
        return hit != SEL_NO_CHILD;
    });
    g.fence();
    return hits;
}

// The document's tape, staged in the group's slice when it fits (a larger one is walked in global memory by the same code).
template <class G>
SJ_HD SelDoc sel_stage(G& g, const sj_u64* tape, uint32_t n_words, const uint8_t* sb, SelScratch& s) {
    SelDoc d;
    d.tape = tape;
    d.n = n_words;
    d.staged = n_words <= SEL_SLICE_WORDS;
    d.sb = sb;
    if (d.staged) {
        // every load of the copy is issued before the first store waits for one: one memory latency, not one per piece
        constexpr uint32_t PIECES = SEL_SLICE_WORDS / SEL_GROUP;
        sj_u64 r[PIECES];
        const uint32_t first = g.stride_first(), step = g.stride();
        for (uint32_t base = 0; base < n_words; base += PIECES * step) {
#pragma unroll
            for (uint32_t q = 0; q < PIECES; ++q) {
                const uint32_t i = base + first + q * step;
                r[q] = i < n_words ? tape[i] : 0;
            }
#pragma unroll
            for (uint32_t q = 0; q < PIECES; ++q) {
                const uint32_t i = base + first + q * step;
                if (i < n_words) s.slice[i] = r[q];
            }
        }
        g.fence();
    }
    return d;
}

// what enumerating the container at tape index v covers: [v + 1, the closing word) -- Tape.getMatchingBraceIndex :78-80, kept
// inside the document whatever the word holds
SJ_HD uint32_t sel_container_end(const SelDoc& d, sj_u64 w, uint32_t v) {
    const uint32_t match = (uint32_t)w;
    return match > v + 1 && match - 1 <= d.n ? match - 1 : v + 1;
}

// Every path of the plan with the value at tape index v as the root (v = 1: the document's root value).  s.types / s.values of
// the group must be zero (MISSING) on entry.
template <class G>
SJ_HD void sel_walk(G& g, const SelHeader* plan, const SelDoc& d, SelScratch& s, uint32_t v0) {
    const SelNode* nodes = sel_nodes(plan);
    int level = -1;
    // the value at tape index v belongs to `node`: its result, and a frame if paths go on through it
    auto enter = [&](uint32_t ni, uint32_t v) {
        const SelNode& node = nodes[ni];
        sel_emit(plan, node, d, s, v);
        if (!node.n_children || level + 1 >= (int)SEL_MAX_STEPS) return false;
        const sj_u64 w = sel_word(d, s, v);
        if (!sel_is_container(sel_type(w))) return false;  // a scalar at hand: everything below is MISSING
        SelFrame& f = s.frames[++level];
        f.node = ni;
        f.pos = v + 1;
        f.end = sel_container_end(d, w, v);
        f.k = sel_type(w) == '[' ? 0 : SEL_NO_INDEX;
        f.found = 0;
        if (sel_type(w) == '[')
            for (uint32_t c = 0; c < node.n_children; ++c)
                if (nodes[node.first_child + c].index == SEL_NO_INDEX) f.found |= 1ull << c;
        return true;
    };
    enter(0, v0);
    while (level >= 0) {
        SelFrame& f = s.frames[level];
        const SelNode& node = nodes[f.node];
        const sj_u64 all = node.n_children >= 64 ? ~0ull : (1ull << node.n_children) - 1ull;
        if (f.pos >= f.end || f.found == all) {
            --level;
            continue;
        }
        if (f.k == SEL_NO_INDEX) {  // an object (k is not used there)
            uint32_t next_pos;
            uint32_t hits = sel_match_round(g, plan, d, s, f, &next_pos);
            bool descended = false;
            for (; hits && !descended; hits &= hits - 1) {  // lowest member first: the FIRST matching key wins
                const uint32_t j = (uint32_t)__builtin_ctz(hits);
                const uint32_t c = s.mchild[j];
                if ((f.found >> c) & 1) continue;  // (a duplicate key later in the same round)
                f.found |= 1ull << c;
                // a child that opens a frame: the enumeration goes on behind this member afterwards (s.memb / s.mchild are the
                // group's, not the frame's; the members in front of it are done, lowest first)
                const uint32_t v = s.memb[j];
                const uint32_t behind = sel_next(d, s, v, f.end);
                descended = enter(node.first_child + c, v);
                if (descended) f.pos = behind;
            }
            if (!descended) f.pos = next_pos;
        } else {  // an array: the k-th element of the iterator chain
            const uint32_t v = f.pos, k = f.k;
            f.pos = sel_next(d, s, v, f.end);
            f.k = k + 1;
            for (uint32_t c = 0; c < node.n_children; ++c)
                if (nodes[node.first_child + c].index == k && !((f.found >> c) & 1)) {
                    f.found |= 1ull << c;
                    enter(node.first_child + c, v);
                    break;  // (sibling tokens differ: one child per index)
                }
        }
    }
}

// Every path of the plan on one document.  s.types / s.values of the group must be zero (MISSING) on entry.
template <class G>
SJ_HD void sel_document(G& g, const SelHeader* plan, const sj_u64* tape, uint32_t n_words, const uint8_t* sb, SelScratch& s) {
    const SelDoc d = sel_stage(g, tape, n_words, sb, s);
    if (n_words < 2) return;
    sel_walk(g, plan, d, s, 1);
}

// ---- explode (csrc/explode.hip): one container per document becomes rows, an element plan is walked on
// every row's value.  The container is the value of a BASE pointer, compiled as a plan of one path.  MEMBERS = false: the base is
// an ARRAY and a row is an element; MEMBERS = true: the base is an OBJECT and a row is a member -- its value is the root of the
// element plan, its key one more cell behind the plan's paths.  The mode is a template parameter: the array form pays for no
// run-time branch.
// The staged document's base container: its rows by the iterator chain (JsonValue.arrayIterator :143-168 -- from idx + 1, by
// Tape.computeNextIndex, to getMatchingBraceIndex - 1; JsonValue.objectIterator :170-194 -- the same chain, the key one word at
// pos, the value at pos + 1, the next member behind the value), never by the 24-bit scope count, which saturates.
// -> the number of rows; *base = the container's tape index, 0 when the base is MISSING or not of the mode's kind (then no rows).
// s.types[0] / s.values[0] must be zero on entry.
template <bool MEMBERS = false, class G>
SJ_HD uint32_t sel_explode_count(G& g, const SelHeader* base_plan, const SelDoc& d, SelScratch& s, uint32_t* base) {
    *base = 0;
    if (d.n < 2) return 0;
    sel_walk(g, base_plan, d, s, 1);
    if (s.types[0] != (MEMBERS ? '{' : '[')) return 0;
    const uint32_t v = (uint32_t)s.values[0];
    *base = v;
    const uint32_t end = sel_container_end(d, sel_word(d, s, v), v);
    uint32_t n = 0;
    if (MEMBERS) {  // (a key without a value in front of the closing word is no member: sel_match_round's rule)
        for (uint32_t pos = v + 1; pos + 1 < end; pos = sel_next(d, s, pos + 1, end)) ++n;
    } else {
        for (uint32_t pos = v + 1; pos < end; pos = sel_next(d, s, pos, end)) ++n;
    }
    return n;
}

// Every path of the element plan on the first `limit` rows of the container at tape index `base` of the staged document (the
// rows that fit the caller's columns: the others are not walked): for row j, row(j) is called with the results in s.types /
// s.values (sel_emit's form: sel_finish is the caller's, when it stores the row).  MEMBERS: the member's key is cell
// plan->n_paths (< SEL_MAX_PATHS there), a string cell in sel_emit's form like the others.  row() runs in every lane of the group
// and may use the group's primitives.
template <bool MEMBERS = false, class G, class Row>
SJ_HD void sel_explode_rows(G& g, const SelHeader* plan, const SelDoc& d, SelScratch& s, uint32_t base, uint32_t limit, Row row) {
    const uint32_t end = sel_container_end(d, sel_word(d, s, base), base);
    uint32_t j = 0;
    for (uint32_t pos = base + 1; pos + (MEMBERS ? 1u : 0u) < end && j < limit; pos = sel_next(d, s, pos + (MEMBERS ? 1u : 0u), end), ++j) {
        const uint32_t v = pos + (MEMBERS ? 1u : 0u);  // the row's value
        for (uint32_t p = g.stride_first(); p < plan->n_paths; p += g.stride()) {  // MISSING until the walk says otherwise
            s.types[p] = 0;
            s.values[p] = 0;
        }
        g.fence();
        sel_walk(g, plan, d, s, v);
        if (MEMBERS && g.stride_first() == 0) {  // the key: one word at pos, its record's offset
            s.types[plan->n_paths] = '"';
            s.values[plan->n_paths] = sel_word(d, s, pos) & 0x00FFFFFFFFFFFFFFull;
        }
        g.fence();
        row(j);
    }
}

// ---- the plan compiler (host code) -----------------------------------------------------------------------------------------
#include <string>
#include <vector>

// the token as an array index: "0" or a decimal without a leading zero (RFC 6901 section 4)
inline uint32_t sel_token_index(const std::string& t) {
    if (t.empty() || (t.size() > 1 && t[0] == '0')) return SEL_NO_INDEX;
    sj_u64 v = 0;
    for (char ch : t) {
        if (ch < '0' || ch > '9') return SEL_NO_INDEX;
        v = v * 10 + (sj_u64)(ch - '0');
        if (v >= SEL_INDEX_HUGE) v = SEL_INDEX_HUGE;
    }
    return (uint32_t)v;
}

// n_paths JSON Pointers, pointer p = pointers[offsets[p], offsets[p + 1]) -> the plan image (SelHeader, nodes, names) in
// 8-byte words.  false: a pointer is malformed (does not begin with '/', '~' not followed by '0' or '1') or a limit is exceeded.
inline bool sel_compile(const uint8_t* pointers, const uint64_t* offsets, uint64_t n_paths, std::vector<sj_u64>* image) {
    if (n_paths > SEL_MAX_PATHS || (n_paths && !offsets)) return false;
    struct Tmp {
        std::string name;
        std::vector<uint32_t> kids;
        std::vector<uint32_t> paths;
    };
    std::vector<Tmp> trie(1);
    for (uint64_t p = 0; p < n_paths; ++p) {
        if (offsets[p + 1] < offsets[p]) return false;
        const uint8_t* s = pointers + offsets[p];
        const uint64_t len = offsets[p + 1] - offsets[p];
        if (len && s[0] != '/') return false;
        uint32_t at = 0, steps = 0;
        for (uint64_t i = 0; i < len;) {  // s[i] == '/': one reference token
            std::string tok;
            for (++i; i < len && s[i] != '/'; ++i) {
                if (s[i] != '~') {
                    tok.push_back((char)s[i]);
                    continue;
                }
                if (i + 1 >= len || (s[i + 1] != '0' && s[i + 1] != '1')) return false;
                tok.push_back(s[++i] == '0' ? '~' : '/');
            }
            if (++steps > SEL_MAX_STEPS || tok.size() > SEL_MAX_NAME_BYTES) return false;
            uint32_t next = 0;
            for (uint32_t k : trie[at].kids)
                if (trie[k].name == tok) next = k;
            if (!next) {
                next = (uint32_t)trie.size();
                trie.emplace_back();
                trie[next].name = tok;
                trie[at].kids.push_back(next);
            }
            at = next;
        }
        trie[at].paths.push_back((uint32_t)p);
    }
    // breadth first, so that the children of a node lie next to each other
    std::vector<uint32_t> order(1, 0);
    for (size_t i = 0; i < order.size(); ++i)
        for (uint32_t k : trie[order[i]].kids) order.push_back(k);
    std::vector<uint32_t> number(trie.size());
    for (size_t i = 0; i < order.size(); ++i) number[order[i]] = (uint32_t)i;
    SelHeader h;
    memset(&h, 0, sizeof h);
    memset(h.path_next, (int)SEL_NO_PATH, sizeof h.path_next);
    std::vector<SelNode> nodes(trie.size());
    std::vector<sj_u64> names;
    for (size_t i = 0; i < order.size(); ++i) {
        const Tmp& t = trie[order[i]];
        SelNode& n = nodes[i];
        memset(&n, 0, sizeof n);
        n.n_children = (uint16_t)t.kids.size();
        n.first_child = t.kids.empty() ? 0 : (uint16_t)number[t.kids[0]];
        n.name_word = (uint16_t)names.size();
        n.name_len = (uint16_t)t.name.size();
        n.index = sel_token_index(t.name);
        names.resize(names.size() + (t.name.size() + 7) / 8, 0);
        if (names.size() * 8 > SEL_MAX_NAME_BYTES) return false;
        if (!t.name.empty()) memcpy(&names[n.name_word], t.name.data(), t.name.size());
        n.path_first = (uint8_t)SEL_NO_PATH;
        for (size_t q = t.paths.size(); q-- > 0;) {  // chained in ascending order
            h.path_next[t.paths[q]] = n.path_first;
            n.path_first = (uint8_t)t.paths[q];
        }
    }
    h.n_paths = (uint32_t)n_paths;
    h.n_nodes = (uint32_t)nodes.size();
    h.name_words = (uint32_t)names.size();
    h.image_words = (uint32_t)((sizeof h + nodes.size() * sizeof(SelNode)) / 8 + names.size());
    image->assign(h.image_words, 0);
    memcpy(image->data(), &h, sizeof h);
    memcpy(image->data() + sizeof h / 8, nodes.data(), nodes.size() * sizeof(SelNode));
    if (!names.empty()) memcpy(image->data() + sizeof h / 8 + nodes.size() * 2, names.data(), names.size() * 8);
    return true;
}
