"""What schema discovery on the device costs -> profiles/r23/members.json, everything from ONE process on one box (boxes differ by
several per cent: only numbers of the same run are compared).  Three sections, every leg verified before it is timed, the legs of
a section interleaved by tools/opbench.py:

  explode   --docs documents (a pool of distinct ones, repeated) with an 8-member root object: the members explode with the
            element pointers "" and "/a" against the ARRAY explode of the same values written as a root array -- the same rows,
            the same element pointers; both at the exact capacity.  Verified against tests/members_common.py /
            tests/explode_common.py on the pool.
  census    --rows rows at 8, 1024, SJMI_CENSUS_LDS_KEYS + 1 and 2^18 keys, uniform and with all rows in one bin, 80 % of the
            rows valid; beside each the yardstick "read_only": torch reductions over the same indices, type bytes and bitmap words
            (three kernels that only read the 5 bytes a row plus the bitmap).  Verified against members_common.expected_census_large.
  discover  BatchShard.discover_keys("") on the documents of `explode` (its readbacks included, wall clock) against the host
            route: D2H of the tapes, their offsets and the string buffer, then a numpy walk of the member chains and a numpy count.
            Both verified against the pool's own keys and counts.
No figure is a pass mark.
  python tools/bench_members.py [--docs N] [--rows N] [--steps K] [--warmup W] [--sections a,b] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SECTIONS = ("explode", "census", "discover")
POOL, STRIDE = 509, 211
POINTERS = ["", "/a"]


def pool_values(i):
    """the eight values of pool document i: every kind, strings and containers among them"""
    return [b"%d" % (i * 31 + 7), b'"s%d"' % i, b'{"a":%d,"b":"x"}' % i, b"[%d,2]" % i, b"true", b"null", b"%d.5" % i, b'{"a":"deep%d"}' % (i % 9)]


def pool_keys(i):
    """its eight keys: six that every document has, one of 16, one of the document's own"""
    return [b"id", b"name", b"owner", b"tags", b"public", b"parent", b"score_%d" % (i % 16), b"extra_%d" % i]


def host_discover(tape, tape_offsets, sb):
    """the host route's count over downloaded buffers, in numpy: the root objects' member chains walked for all documents at once
    (member j of every document in one step), the keys as fixed-width rows, np.unique for the dictionary in first-occurrence
    order, np.bincount for the counts -> [(key bytes, [8 counts])]"""
    tape = tape.view(np.uint64)
    first = tape_offsets[:-1].astype(np.int64)
    root = tape[first + 1]
    is_obj = (root >> np.uint64(56)) == ord("{")
    end = first + (root & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1  # the closing word
    pos = first + 2
    live = is_obj & (pos + 1 < end)
    key_off, val_type, doc_of = [], [], []
    table = np.full(256, 7, dtype=np.int64)
    for t, cl in ((b"l", 0), (b"d", 1), (b'"', 2), (b"t", 3), (b"f", 3), (b"n", 4), (b"[", 5), (b"{", 6)):
        table[t[0]] = cl
    while live.any():
        at = pos[live]
        kw, vw = tape[at], tape[at + 1]
        vt = (vw >> np.uint64(56)).astype(np.int64)
        key_off.append((kw & np.uint64(0x00FFFFFFFFFFFFFF)).astype(np.int64))
        val_type.append(table[vt])
        doc_of.append(np.nonzero(live)[0])
        nxt = np.where((vt == ord("[")) | (vt == ord("{")), first[live] + (vw & np.uint64(0xFFFFFFFF)).astype(np.int64),
                       np.where((vt == ord("l")) | (vt == ord("d")), at + 3, at + 2))
        pos[live] = nxt
        live = live & (pos + 1 < end)
    if not key_off:
        return []
    n_members = len(key_off)
    # member-major -> document-major (tape order): sort by (document, member number)
    doc = np.concatenate(doc_of)
    member = np.concatenate([np.full(d.size, j, dtype=np.int64) for j, d in enumerate(doc_of)])
    order = np.lexsort((member, doc))
    off, cls = np.concatenate(key_off)[order], np.concatenate(val_type)[order]
    be = sb[off[:, None] + np.arange(4)].astype(np.int64)
    length = (be[:, 0] << 24) | (be[:, 1] << 16) | (be[:, 2] << 8) | be[:, 3]
    width = int(length.max()) if length.size else 0
    rows = np.zeros((off.size, width + 4), dtype=np.uint8)
    rows[:, :4] = be
    cols = np.arange(width)
    text = sb[np.minimum(off[:, None] + 4 + cols, sb.size - 1)]
    rows[:, 4:] = np.where(cols[None, :] < length[:, None], text, 0)
    _, first_row, inverse = np.unique(rows.view(np.dtype((np.void, width + 4))).ravel(), return_index=True, return_inverse=True)
    rank = np.empty(first_row.size, dtype=np.int64)
    rank[np.argsort(first_row)] = np.arange(first_row.size)
    counts = np.bincount(rank[inverse] * 8 + cls, minlength=first_row.size * 8).reshape(-1, 8)
    keys = [bytes(rows[r, 4:4 + int(length[r])]) for r in np.sort(first_row)]
    assert n_members
    return [(k, counts[j].tolist()) for j, k in enumerate(keys)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "members.json"))
    a = ap.parse_args(argv)
    sections = [s for s in a.sections.split(",") if s]
    if a.docs < 1 or a.rows < 1 or a.steps < 1 or a.warmup < 0:
        ap.error("--docs, --rows and --steps must be >= 1, --warmup >= 0")
    if not sections or any(s not in SECTIONS for s in sections):
        ap.error("--sections: a list of " + ", ".join(SECTIONS))
    import torch
    import simdjson_java_amd as S
    from oracle import oracle as O
    from tests import explode_common as EC
    from tests import members_common as MC
    from tests.test_gpu_batch import _pack
    from tests.test_gpu_explode import _check_trip_batch
    from tools import opbench
    O.build()
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "docs": a.docs, "rows": a.rows, "lds_keys": MC.header_constant("SJMI_CENSUS_LDS_KEYS")}
    idx = (np.arange(a.docs, dtype=np.int64) * STRIDE) % POOL
    objects = [b"{" + b",".join(b'"' + k + b'":' + v for k, v in zip(pool_keys(i), pool_values(i))) + b"}" for i in range(POOL)]
    arrays = [b"[" + b",".join(pool_values(i)) + b"]" for i in range(POOL)]

    def as_pool(docs, offs, want):
        counts, first = np.diff(np.array(offs, dtype=np.int64)), np.array(offs[:-1], dtype=np.int64)
        cols = []
        for col in want:
            t = np.array([c[0] for c in col], dtype=np.uint8)
            v = np.array([0 if c[0] == ord('"') else c[1] for c in col], dtype=np.uint64)
            ln = np.array([len(c[1]) if c[0] == ord('"') else 0 for c in col], dtype=np.int64)
            text = np.zeros((len(col), max(1, int(ln.max()))), dtype=np.uint8)
            for i, c in enumerate(col):
                if c[0] == ord('"'):
                    text[i, :len(c[1])] = np.frombuffer(c[1], dtype=np.uint8)
            cols.append((t, v, ln, text))
        return docs, counts, first, cols

    def batch(docs):
        buf, offs = _pack([docs[i] for i in idx])
        return opbench.parsed_shard(ctx, dev, stream, buf, offs)

    shard = None
    if "explode" in sections or "discover" in sections:
        shard, counts = batch(objects)
    if "explode" in sections:
        ashard, _ = batch(arrays)
        mplan, aplan = S.ExplodePlan("", POINTERS, members=True), S.ExplodePlan("", POINTERS)
        total = 8 * a.docs
        for sh, plan, pool in ((shard, mplan, as_pool(objects, *MC.expected_members([O.parse(d) for d in objects], "", POINTERS))),
                               (ashard, aplan, as_pool(arrays, *EC.expected_explode([O.parse(d) for d in arrays], "", POINTERS)))):
            offs, types, values = sh.explode(plan, total, stream)
            torch.cuda.synchronize()
            sb = bytes(sh.sb[:int(sh.result.cpu()[2])].cpu().numpy())
            assert _check_trip_batch(pool, offs.cpu().numpy().view(np.uint64), types.cpu().numpy(), values.cpu().numpy().view(np.uint64), sb, idx, {}) == total
        legs = {"members_explode": lambda: shard.explode(mplan, total, stream), "array_explode": lambda: ashard.explode(aplan, total, stream)}
        out = opbench.measure(legs, a.steps, a.warmup)
        out["members_over_array"] = out["members_explode"]["median_ms"] / out["array_explode"]["median_ms"]
        out["rows"] = total
        res["explode"] = out
        mplan.close()
        aplan.close()
        del ashard
    if "census" in sections:
        rng = np.random.default_rng(23)
        res["census"] = []
        bits = rng.random(a.rows) < 0.8
        words = torch.from_numpy(MC.pack_bits(bits).view(np.int64)).to(dev)
        uniform_types = rng.choice(np.frombuffer(b'ld"tfn[{\0', dtype=np.uint8), a.rows)
        for n_keys in (8, 1024, res["lds_keys"] + 1, 1 << 18):
            for kind in ("uniform", "one_bin"):
                ix = rng.integers(0, n_keys, a.rows).astype(np.int32) if kind == "uniform" else np.full(a.rows, n_keys // 2, dtype=np.int32)
                ty = uniform_types if kind == "uniform" else np.full(a.rows, ord("l"), dtype=np.uint8)
                d_ix, d_ty = torch.from_numpy(ix).to(dev), torch.from_numpy(ty).to(dev)
                counts = torch.empty((n_keys, 8), dtype=torch.int64, device=dev)
                record = torch.empty(4, dtype=torch.int64, device=dev)
                call = lambda: ctx.key_census_device(d_ix.data_ptr(), words.data_ptr(), d_ty.data_ptr(), a.rows, 0, n_keys, counts.data_ptr(),
                                                     record.data_ptr(), stream)
                call()
                torch.cuda.synchronize()
                want, counted, outside = MC.expected_census_large(ix, bits, ty, n_keys, a.rows)
                assert counts.cpu().numpy().tolist() == want and record.cpu().tolist() == [a.rows, counted, outside, 0], (n_keys, kind)
                legs = {"census": call, "read_only": lambda: (d_ix.sum(), d_ty.sum(), words.sum())}
                out = {"n_keys": n_keys, "rows_in": kind, "path": "lds" if n_keys <= res["lds_keys"] else "global"}
                out.update(opbench.measure(legs, a.steps, a.warmup))
                out["census_over_read_only"] = out["census"]["median_ms"] / out["read_only"]["median_ms"]
                res["census"].append(out)
    if "discover" in sections:
        want = MC.python_key_census([[(k.decode(), MC.loads_pairs(v)) for k, v in zip(pool_keys(i), pool_values(i))] for i in idx[:POOL]])
        got = shard.discover_keys("", dict_capacity=4096, stream=stream)[0]
        assert [k for k, _ in got] == [k for k, _ in want] and sum(sum(c) for _, c in got) == 8 * a.docs

        def host_route():
            torch.cuda.synchronize()
            n_words = int(shard.tape_offsets[shard.n_docs].cpu())
            return host_discover(shard.tape[:n_words].cpu().numpy(), shard.tape_offsets.cpu().numpy(), shard.sb[:int(shard.result.cpu()[2])].cpu().numpy())

        assert host_route() == got
        legs = {"discover_keys": lambda: shard.discover_keys("", dict_capacity=4096, stream=stream), "host_route": host_route}
        out = opbench.measure(legs, a.steps, a.warmup, host=("discover_keys", "host_route"))
        out["host_over_device"] = out["host_route"]["median_ms"] / out["discover_keys"]["median_ms"]
        out["distinct_keys"] = len(got)
        res["discover"] = out
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
