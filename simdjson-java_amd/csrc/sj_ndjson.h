// sj_ndjson.h -- splitting a buffer of newline-delimited JSON into documents (include/sjmi.h, sjmi_ndjson_offsets*; DESIGN.md
// 4.10): the block algebra, the state that crosses a block or tile edge with its operator, and the three passes over the tiles.
//
// NL is 0x0A; BLANK is 0x20, 0x09, 0x0D and nothing else.  Per 64-byte block two masks: N = the NL bytes, B = the bytes that
// are neither NL nor BLANK.  A LINE runs up to and including its NL; a line with a B bit is a document, and it begins at its
// line start -- the byte behind the NL in front of it, however many blocks back that is.  One START is emitted for the FIRST B
// bit of every line, found with one addition: in ~N + B a carry is born at a B bit and runs through the line's bytes until the
// line's N bit absorbs it, so a B bit that RECEIVES a carry is not the first of its line.  The bytes behind the last NL (the
// tail) are not a line: a non-blank tail still gives a start, which is the entry doc_offsets[n_docs] = consumed, and the
// number of documents is the number of starts less that one.
//
// What crosses an edge is NdState = (has_nl, last_nl_pos, seen): is there an NL so far, where is the last one, and is there a B
// bit behind it (without an NL: a B bit at all).  States combine with nd_combine, which is associative with 0 as its identity,
// so the states in front of every block of a tile, and in front of every tile, are exclusive scans.  Only a segment's HEAD --
// what lies in front of its first NL -- depends on the state it is entered with: its first B bit is a start unless the entry
// state has `seen`.  A tile's summary therefore counts the starts behind its first NL and says whether its head has a B bit.
//
// Positions are VIRTUAL: they count from the 16-byte boundary at or below the caller's pointer, so that every block is loaded
// with aligned 16-byte loads whatever the pointer's alignment; the bytes in front of the buffer and behind its end (the
// padding) are masked out of N and B (nd_valid) and read as BLANK.
//
// The lanes that share a tile come from the caller: takes a workgroup G (sj_group.h; one block per lane); uses: lanes, lane,
// scan_add, any, and two members that csrc/ndjson.hip and tests/host_sim/ndjson_sim.cpp add to the group:
//   g.load(p, w)                  -- the 64 bytes at p (16-byte aligned) as 16 little-endian dwords
//   g.scan_state(v, &total)       -- exclusive nd_combine scan of v over the lanes, total = all of them combined (a workgroup
//                                    barrier that begins with one, like scan_add)
// This file is compiled verbatim by both, so the CPU suite checks the passes the kernels run, at any tile size.
#pragma once
#include <stdint.h>

#include "sj_block32.h"

constexpr uint32_t ND_TILE_BLOCKS = 1024;  // 64-byte blocks of a tile: 64 KiB (a 256-thread workgroup takes it in four steps)
constexpr uint32_t ND_TAIL_BLANK = 1u, ND_OVERFLOW = 2u;  // SJMI_NDJSON_TAIL_BLANK / _OVERFLOW

typedef sj_u64 NdState;
constexpr sj_u64 ND_HAS_NL = 1ull << 63;  // an NL so far; then bits 0..61 = the virtual position of the last one (else 0)
constexpr sj_u64 ND_SEEN = 1ull << 62;    // a B bit behind that NL (without one: a B bit at all)
constexpr sj_u64 ND_POS = ND_SEEN - 1;

// a (+) b, a in front of b
SJ_HD NdState nd_combine(NdState a, NdState b) { return (b & ND_HAS_NL) ? b : (a | (b & ND_SEEN)); }

struct NdGeom {
    const uint8_t* base;   // the 16-byte boundary at or below the buffer
    sj_u64 vbeg, vend;     // the buffer in virtual positions: [vbeg, vend), vbeg < 16
    sj_u64 nblocks;        // blocks that hold a byte of it (0 for an empty buffer)
    uint32_t tile_blocks;  // blocks per tile
};
SJ_HD NdGeom nd_geom(const void* buf, sj_u64 len, uint32_t tile_blocks) {
    NdGeom ge;
    const uintptr_t a = (uintptr_t)buf;
    ge.base = (const uint8_t*)(a & ~(uintptr_t)15);
    ge.vbeg = a & 15;
    ge.vend = ge.vbeg + len;
    ge.nblocks = len ? (ge.vend + 63) / 64 : 0;
    ge.tile_blocks = tile_blocks;
    return ge;
}
SJ_HD sj_u64 nd_tiles(const NdGeom& ge) { return (ge.nblocks + ge.tile_blocks - 1) / ge.tile_blocks; }

// bits of the block at virtual position pos that belong to the buffer
SJ_HD sj_u64 nd_valid(const NdGeom& ge, sj_u64 pos) {
    const sj_u64 lo = ge.vbeg > pos ? ge.vbeg - pos : 0;                                 // (vbeg < 16: lo < 64)
    const sj_u64 hi = ge.vend >= pos + 64 ? 64 : ge.vend > pos ? ge.vend - pos : 0;
    const sj_u64 below_hi = hi >= 64 ? ~0ull : (1ull << hi) - 1;
    return below_hi & ~((1ull << lo) - 1);
}

struct NdBlock {
    sj_u64 nl, nb;  // N and B
    NdState state;  // the block on its own
};

// N and B of one half from its planes (sj_transpose32: x[k] = bit k of its 32 bytes)
SJ_HD void nd_classify32(const uint32_t p[8], uint32_t* nl, uint32_t* nb) {
    const uint32_t c = sj_bop<SJ_TT_NOR3>(p[7], p[6], p[5]) & ~p[4];                      // 0x00..0x0F
    const uint32_t n = sj_bop<SJ_TT_A_B_NC>(c, sj_bop<SJ_TT_A_NB_C>(p[3], p[2], p[1]), p[0]);  // 0x0A
    const uint32_t tr = c & sj_bop<SJ_TT_A_NB_C>(p[3], p[1], p[0]);                       // 0x09, 0x0D
    const uint32_t s = sj_bop<SJ_TT_A_NB_NC>(p[5], p[7], p[6]) & ~p[4];                   // 0x20..0x2F
    const uint32_t sp = sj_bop<SJ_TT_A_B_NC>(s, sj_bop<SJ_TT_NOR3>(p[3], p[2], p[1]), p[0]);   // 0x20
    *nl = n;
    *nb = sj_bop<SJ_TT_NOR3>(n, tr, sp);
}

// the state of a block on its own: the carry out of ~N + B is `seen`
SJ_HD NdState nd_block_state(sj_u64 nl, sj_u64 nb, sj_u64 pos) {
    const sj_u64 x = ~nl;
    NdState st = (x + nb < x) ? ND_SEEN : 0;
    if (nl) st |= ND_HAS_NL | (pos + 63 - (sj_u64)__builtin_clzll(nl));
    return st;
}
// the first B bit of every line of the block; seen_in = the state in front of the block has `seen`
SJ_HD sj_u64 nd_first_bits(sj_u64 nl, sj_u64 nb, sj_u64 seen_in) {
    const sj_u64 x = ~nl;
    const sj_u64 carries = (x + nb + seen_in) ^ x ^ nb;  // bit i = the carry INTO bit i
    return nb & ~carries;
}
// the B bits of the block's head (in front of its first NL)
SJ_HD sj_u64 nd_head_bits(sj_u64 nl, sj_u64 nb) { return nl ? nb & ((nl & (0 - nl)) - 1) : nb; }
// virtual line start of the line that bit `bit` of the block lies in; ex = the state in front of the block
SJ_HD sj_u64 nd_line_start(const NdGeom& ge, sj_u64 nl, uint32_t bit, sj_u64 pos, NdState ex) {
    const sj_u64 below = nl & ((1ull << bit) - 1);
    if (below) return pos + 64 - (sj_u64)__builtin_clzll(below);
    return (ex & ND_HAS_NL) ? (ex & ND_POS) + 1 : ge.vbeg;
}

// block `blk` (active: it is one of the tile's; the others read as blank)
template <class G>
SJ_HD NdBlock nd_block(const G& g, const NdGeom& ge, sj_u64 blk, bool active) {
    uint32_t w[16], lo[8], hi[8];
    g.load(ge.base + (blk < ge.nblocks ? blk : ge.nblocks - 1) * 64, w);  // (never a load past the last block)
    sj_transpose32(w, lo, hi);
    uint32_t nl0, nb0, nl1, nb1;
    nd_classify32(lo, &nl0, &nb0);
    nd_classify32(hi, &nl1, &nb1);
    const sj_u64 valid = active ? nd_valid(ge, blk * 64) : 0;
    NdBlock b;
    b.nl = (((sj_u64)nl1 << 32) | nl0) & valid;
    b.nb = (((sj_u64)nb1 << 32) | nb0) & valid;
    b.state = nd_block_state(b.nl, b.nb, blk * 64);
    return b;
}

// What the passes keep per tile.  Behind nd_tile_summary: state = the tile on its own, cnt = (starts behind its first NL) << 1
// | (its head has a B bit).  Behind nd_scan_tiles: state = the state in front of the tile, cnt = the starts in front of it.
struct NdTile {
    NdState state;
    sj_u64 cnt;
};

// pass 1, per tile (ge.nblocks != 0)
template <class G>
SJ_HD NdTile nd_tile_summary(const G& g, const NdGeom& ge, sj_u64 tile) {
    const sj_u64 first = tile * ge.tile_blocks;
    const sj_u64 end = first + ge.tile_blocks < ge.nblocks ? first + ge.tile_blocks : ge.nblocks;
    NdState run = 0;
    sj_u64 starts = 0;
    bool head = false;
    for (sj_u64 at = first; at < end; at += g.lanes()) {
        const sj_u64 blk = at + g.lane();
        const NdBlock b = nd_block(g, ge, blk, blk < end);
        NdState total;
        const NdState ex = nd_combine(run, g.scan_state(b.state, &total));
        starts += (sj_u64)__builtin_popcountll(nd_first_bits(b.nl, b.nb, (ex >> 62) & 1));
        if (!(ex & ND_HAS_NL)) head |= nd_head_bits(b.nl, b.nb) != 0;
        run = nd_combine(run, total);
    }
    sj_u64 all;
    (void)g.scan_add(starts, &all);
    const sj_u64 h = g.any(head) ? 1 : 0;  // entered without `seen`, the head's first B bit is among the starts counted
    NdTile t = {run, ((all - h) << 1) | h};
    return t;
}

// pass 2, one group over all tiles: summaries -> (state in front, starts in front); -> the state and the starts of the buffer
template <class G>
SJ_HD NdTile nd_scan_tiles(const G& g, NdTile* tiles, sj_u64 ntiles) {
    NdTile all = {0, 0};
    for (sj_u64 at = 0; at < ntiles; at += g.lanes()) {
        const sj_u64 i = at + g.lane();
        NdTile t = {0, 0};
        if (i < ntiles) t = tiles[i];
        NdState total;
        const NdState entry = nd_combine(all.state, g.scan_state(t.state, &total));
        const sj_u64 starts = (t.cnt >> 1) + ((t.cnt & 1) & ((entry & ND_SEEN) ? 0 : 1));
        sj_u64 sum;
        const sj_u64 rank = all.cnt + g.scan_add(starts, &sum);
        if (i < ntiles) {
            tiles[i].state = entry;
            tiles[i].cnt = rank;
        }
        all.state = nd_combine(all.state, total);
        all.cnt += sum;
    }
    return all;
}

struct NdResult {  // sjmi_ndjson_result
    sj_u64 n_docs, consumed;
    uint32_t flags, reserved;
};
// ... and what ONE lane writes behind it: the result record, doc_offsets[0] and doc_offsets[n_docs]
SJ_HD void nd_finish(const NdGeom& ge, NdTile all, sj_u64* offsets, sj_u64 capacity, NdResult* res) {
    const sj_u64 seen = (all.state >> 62) & 1;  // the tail is not blank: its start is not a document
    const sj_u64 n_docs = all.cnt - seen;
    const sj_u64 consumed = (all.state & ND_HAS_NL) ? (all.state & ND_POS) + 1 - ge.vbeg : 0;
    if (capacity >= 1) offsets[0] = 0;
    if (n_docs >= 1 && n_docs < capacity) offsets[n_docs] = consumed;
    res->n_docs = n_docs;
    res->consumed = consumed;
    res->flags = (seen ? 0u : ND_TAIL_BLANK) | (capacity < n_docs + 1 ? ND_OVERFLOW : 0u);
    res->reserved = 0;
}

// pass 3, per tile: start number k (k >= 1) goes to offsets[k] if k < capacity; entry = what pass 2 left for the tile
template <class G>
SJ_HD void nd_tile_emit(const G& g, const NdGeom& ge, sj_u64 tile, NdTile entry, sj_u64* offsets, sj_u64 capacity) {
    if (entry.cnt >= capacity) return;  // (every start of the tile lies behind the capacity)
    const sj_u64 first = tile * ge.tile_blocks;
    const sj_u64 end = first + ge.tile_blocks < ge.nblocks ? first + ge.tile_blocks : ge.nblocks;
    NdState run = entry.state;
    sj_u64 rank = entry.cnt;
    for (sj_u64 at = first; at < end; at += g.lanes()) {
        const sj_u64 blk = at + g.lane();
        const NdBlock b = nd_block(g, ge, blk, blk < end);
        NdState total;
        const NdState ex = nd_combine(run, g.scan_state(b.state, &total));
        sj_u64 f = nd_first_bits(b.nl, b.nb, (ex >> 62) & 1);
        sj_u64 sum;
        // the lanes' starts are numbered in block order: where a block has at most one (documents of 64 bytes and more), the
        // lanes that have one store to neighbouring entries
        sj_u64 k = rank + g.scan_add((sj_u64)__builtin_popcountll(f), &sum);
        for (; f; f &= f - 1, ++k)
            if (k >= 1 && k < capacity) offsets[k] = nd_line_start(ge, b.nl, (uint32_t)__builtin_ctzll(f), blk * 64, ex) - ge.vbeg;
        run = nd_combine(run, total);
        rank += sum;
    }
}
