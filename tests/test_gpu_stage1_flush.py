"""The store side of the stage-1 kernel: a granule's indexes are staged in the wave's LDS slice at the position their final
address has inside its 128-byte line and leave as line-aligned 16-byte stores; the expansion's last flush is issued behind the
wait for, and the transposition of, the next granule's first step.  Every case is bit-exact against oracle.stage1: indexes, count, status, and the
sentinel 0 at [count].

  * burst alignment: inputs of 2 to 5 granules behind a run of k commas, k = 0 .. 31, so that the structurals in front of every
    granule take every residue modulo 32;
  * every flush path on both sides of its fit test: one input per granule size made of granules with a chosen number of
    indexes WT -- 0 (blanks; the inside of one long string, full of commas), 1 .. 8, CAP - 34 .. CAP + 1 (CAP = the wave's
    staging slots; the round fits if WT + 31 <= CAP, before line alignment if WT + 3 <= CAP), a structural every 5, 3 and 2
    bytes (the split path where a granule has two halves), '[' repeated (the windowed fallback), and one granule on either
    side of SJMI_S1_SORT_MIN per step; every other granule is entered inside a string;
  * nothing outside [base, base + count] is written: the device path on a pre-filled tensor, the index array at each of the
    eight 16-byte offsets inside a line, capacity count + 1, and count once (SJMI_ST_CAPACITY);
  * the first and the last iteration: inputs of exactly one granule, and the small grid (debug flag 32) on which every wave's
    last granule is reached by ticket.
The largest input is 59 granules of 16 KiB (0.92 MiB)."""
import random

import numpy as np
import pytest

from oracle import oracle as O

STEPS = (1, 2, 4)
CAP = {1: 6144 // 4, 2: 9216 // 4, 4: 9216 // 4}  # staging slots of a wave (stage1.hip: LDSW / 4)
PAD = 31                                          # slots in front of a round's first index: its position in its line
SORT_MIN = 192                                    # SJMI_S1_SORT_MIN
ST_CAPACITY = 0x100
PATTERN = 0x5A5A5A5A
KS = (0, 1, 13, 31)  # commas in front of the path inputs

_PARTS = ['"name"', '"va\\"lue"', '"é€😀"', "12345", "-1.5e10", "true", "null", '"' + "abc def " * 9 + '"', '""', "{", "}", "[", "]",
          ":", ",", " ", "\n", '{"k":[1,2,{"z":null}]}', '"\\\\\\\\"']


def _filler(rng, n):
    """n bytes of string-complete JSON-like text, blanks behind it."""
    out = bytearray()
    while True:
        part = rng.choice(_PARTS).encode()
        if len(out) + len(part) > n:
            break
        out += part
    return bytes(out) + b" " * (n - len(out))


def _with_commas(body, k):
    """body's first 32 bytes are blanks: k of them become commas (the granule layout behind them does not move)."""
    assert body[:32] == b" " * 32 and 0 <= k < 32
    return np.frombuffer(b"," * k + body[k:] + b" " * 128, dtype=np.uint8)


def _alignment_inputs(steps):
    """[(name, text, n)]: 2 .. 5 granules behind k commas."""
    G = 4096 * steps
    rng = random.Random(100 + steps)
    cases = []
    whole = b" " * 32 + _filler(rng, G - 96) + b" " * 64 + b"".join(_filler(rng, G - 64) + b" " * 64 for _ in range(4))
    for k in range(32):
        ng = 2 + k % 4
        body = whole[:ng * G - 64]  # (- 64: the tail block is the last granule's last block)
        cases.append(("align-k%d" % k, _with_commas(body, k), len(body)))
    return cases


def _granule(G, W, entered_inside, leave_inside):
    """G bytes with exactly W structurals, spread evenly: commas, and the opening quote of the string it is left in."""
    g = bytearray(b" " * G)
    lo, hi = 32, G - 8  # (the first 32 bytes stay free for _with_commas)
    if entered_inside:
        g[0:34] = b"z" * 33 + b'"'  # the string ends here
        lo = 40
    commas = W
    if leave_inside:
        assert W >= 1
        g[G - 4:G] = b'"zzz'
        commas = W - 1
    assert commas <= hi - lo
    for i in range(commas):
        g[lo + (i * (hi - lo)) // commas] = ord(",")
    return bytes(g)


def _every(G, stride):
    g = bytearray(b" " * G)
    for p in range(32, G, stride):
        g[p] = ord(",")
    return bytes(g)


def _wt_classes(steps):
    cap = CAP[steps]
    return [0] + list(range(1, 9)) + list(range(cap - 34, cap + 2)) + [SORT_MIN * steps - 7, SORT_MIN * steps + 9]


def _path_body(steps):
    """One input whose granules take every flush path; every other granule with indexes is entered inside a string."""
    G = 4096 * steps
    gr = [b" " * G]  # (granule 0: blanks -- WT = 0 -- and the place of the commas in front)
    inside = False
    for n, W in enumerate(_wt_classes(steps)):
        leave = W >= 1 and n % 2 == 0
        gr.append(_granule(G, W, inside, leave))
        inside = leave
    if inside:
        gr.append(_granule(G, 2, True, False))
    # the inside of one long string, full of commas: no index, potential structurals in every byte
    gr.append(b" " * (G - 1) + b'"')
    gr.append(b"," * G)
    gr.append(b'"' + b" " * (G - 1))
    for stride in (5, 3, 2):
        gr.append(_every(G, stride))
    gr.append(b" " * 32 + b"[" * (G - 32))
    gr.append(b"[" * G)
    gr.append(_granule(G, 3, False, False))
    gr.append(b" " * (G - 64))  # (the tail block closes the last granule)
    return b"".join(gr)


def _single_inputs(steps):
    """exactly one granule: no parked granule when the first step is consumed, no next one when the flush is issued"""
    G = 4096 * steps
    rng = random.Random(200 + steps)
    cases = []
    for n in (0, 1, 100, 4095, G - 128, G - 65):
        cases.append(("single-%d" % n, np.frombuffer(_filler(rng, n) + b" " * 128, dtype=np.uint8), n))
    dense = _every(G, 5)[:G - 64]
    cases.append(("single-dense", np.frombuffer(dense + b" " * 128, dtype=np.uint8), len(dense)))
    return cases


_cache = {}


def _inputs(steps):
    """[(name, text, length, reference indexes, reference status)], made once per granule size and shared by every test."""
    if steps not in _cache:
        cases = _alignment_inputs(steps) + _single_inputs(steps)
        body = _path_body(steps)
        for k in KS:
            cases.append(("paths-k%d" % k, _with_commas(body, k), len(body)))
        _cache[steps] = [(name, text, n) + O.stage1(text, n) for name, text, n in cases]
    return _cache[steps]


def _per_granule(idx, n, steps):
    """(indexes in front of each granule, indexes in it, indexes in its first half)"""
    G = 4096 * steps
    ng = (n // 64 + 1 + 64 * steps - 1) // (64 * steps)
    edges = np.searchsorted(idx, np.arange(ng + 1, dtype=np.int64) * G)
    half = np.searchsorted(idx, np.arange(ng, dtype=np.int64) * G + G // 2)
    return edges[:-1], np.diff(edges), half - edges[:-1]


def test_inputs_cover_residues_and_paths():
    """The generator itself (no GPU work), from the oracle's indexes alone: every residue modulo 32 in front of a granule, every
    WT class, and every flush path on both sides of the old and the new fit test."""
    for steps in STEPS:
        cap, G = CAP[steps], 4096 * steps
        cases = _inputs(steps)
        sizes = set()
        residues = set()
        for name, text, n, idx, st in cases:
            if not name.startswith("align"):
                continue
            front, cnt, _ = _per_granule(idx.astype(np.int64), n, steps)
            sizes.add(front.size)
            residues.update(int(f) % 32 for f in front[1:])
            assert front.size >= 2 and cnt[1:].max() > 0
        assert sizes == {2, 3, 4, 5}, sizes
        assert residues == set(range(32)), sorted(set(range(32)) - residues)
        seen, paths, edge_residues = set(), set(), set()
        zero_with_potential = False
        for name, text, n, idx, st in cases:
            if not name.startswith("paths"):
                continue
            assert st == 0, (name, st)
            front, cnt, first = _per_granule(idx.astype(np.int64), n, steps)
            for g in range(front.size):
                W, h = int(cnt[g]), int(first[g])
                seen.add(W)
                if W + PAD <= cap:
                    paths.add("sorted" if W > SORT_MIN * steps else "fast")
                elif steps >= 2 and h + PAD <= cap and W - h + PAD <= cap:
                    paths.add("split")
                else:
                    paths.add("window")
                if cap - 34 <= W <= cap + 1:
                    edge_residues.add(int(front[g]) % 32)
                if W == 0 and bytes(text[g * G:g * G + G]) == b"," * G:
                    zero_with_potential = True
        assert set(_wt_classes(steps)) <= seen, sorted(set(_wt_classes(steps)) - seen)
        assert {G - 32, G} <= seen and max(seen) == G           # '[' repeated: fits neither half
        assert len(range(32, G, 5)) in seen                      # a structural every 5 bytes
        assert zero_with_potential
        assert paths == ({"fast", "sorted", "split", "window"} if steps >= 2 else {"fast", "sorted", "window"}), paths
        assert edge_residues == set(range(32)), sorted(set(range(32)) - edge_residues)
        singles = [c for c in cases if c[0].startswith("single")]
        assert all(_per_granule(c[3].astype(np.int64), c[2], steps)[0].size == 1 for c in singles)
        assert max(c[1].size for c in cases) <= 2 * 1024 * 1024 + 4096


@pytest.fixture(scope="module", params=[(m, f) for m in ("fast", "ticket") for f in (0, 32)], ids=lambda p: "%s-flags%d" % p)
def ctx(request):
    import simdjson_java_amd as S
    mode, flags = request.param
    c = S.Context(device=0, capacity=80 * 4096 * 4 + 4096)
    c.set_tile_mode(mode == "ticket")
    c.debug_set_flags(flags)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
def test_flush_alignment_and_paths(ctx, steps):
    ctx.set_tile_steps(steps)
    try:
        for name, text, n, want_idx, want_st in _inputs(steps):
            got_idx, got_st = ctx.stage1(text, n)  # (asserts the sentinel at [count])
            assert got_st == want_st, (name, got_st, want_st)
            assert got_idx.size == want_idx.size, (name, got_idx.size, want_idx.size)
            if not np.array_equal(got_idx, want_idx):
                bad = int(np.nonzero(got_idx != want_idx)[0][0])
                raise AssertionError("%s: first index mismatch at %d: got %d want %d" % (name, bad, got_idx[bad], want_idx[bad]))
    finally:
        ctx.set_tile_steps(0)


@pytest.mark.gpu
@pytest.mark.parametrize("steps", STEPS)
def test_nothing_outside_the_burst_is_written(steps):
    import torch
    import simdjson_java_amd as S
    c = S.Context(device=0, capacity=1 << 20)
    c.set_tile_steps(steps)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        for name, text, n, want_idx, want_st in _inputs(steps):
            if name not in ("paths-k13", "align-k7", "single-100"):
                continue
            count = int(want_idx.size)
            buf = torch.from_numpy(text.copy()).cuda()
            res = torch.zeros(2, dtype=torch.int64, device="cuda")
            want = torch.from_numpy(want_idx.astype(np.int64)).cuda()
            for quad in range(8):  # the index array begins 16 * quad bytes into a 128-byte line
                whole = torch.full((count + 1 + 32 + 64,), PATTERN, dtype=torch.int32, device="cuda")
                assert whole.data_ptr() % 128 == 0
                base = 4 * quad
                for cap in (count + 1, count):
                    whole.fill_(PATTERN)
                    out = whole[base:]
                    c.stage1_device(buf.data_ptr(), n, out.data_ptr(), cap, res.data_ptr(), stream)
                    torch.cuda.synchronize()
                    r = res.cpu().numpy()
                    status = int(r[1]) & 0xFFFFFFFF
                    assert int(r[0]) == count, (name, quad, cap, r)
                    assert bool((whole[:base] == PATTERN).all()), (name, quad, cap, "written in front of the base")
                    if cap == count + 1:
                        assert status == want_st, (name, quad, status)
                        assert torch.equal(out[:count].to(torch.int64) & 0xFFFFFFFF, want), (name, quad)
                        assert int(out[count].item()) == 0, (name, quad, "sentinel")
                        assert bool((whole[base + count + 1:] == PATTERN).all()), (name, quad, "written behind [count]")
                    else:
                        assert status & ST_CAPACITY, (name, quad, status)
                        assert bool((whole[base + count:] == PATTERN).all()), (name, quad, "written behind the capacity")
    finally:
        c.set_tile_steps(0)
        c.close()
