"""What dictionary-encoding a string column on the device costs -> profiles/r17/dictcol.json, everything from ONE process on one
box (boxes differ by several per cent: only numbers of the same run are compared).

Columns: 1,000,000 rows over 4, 1024 and 2^18 distinct values of 2 to 40 bytes (every occurrence with bytes of its own in the
string buffer, 5 % NULL rows), and the two end-to-end columns: /type of github_events.json through parse and select, /user/lang
of the twitter statuses through parse and explode.  Every column is first verified (numpy: first-occurrence order from the
vocabulary picks; the fixtures against tests/dictcol_common.py).  Then, interleaved, by HIP events, per column:
  (a) the sizing call;  (b) the full call into buffers of the exact size;
  (c) sjmi_string_column_device over the same column -- what a consumer pays today before it can even start encoding;
  (d) the yardstick: a torch device-to-device copy of 13 * n_rows + dict_bytes bytes, the least the call must move (a type byte
      and a value word read, an index written per row; the dictionary);
  (e) with --host and pyarrow: the host route, wall clock: string gather, D2H, pyarrow dictionary_encode().
The insert kernel's share comes from a run of its own under rocprofv3 --kernel-trace --stats (--columns NAME --steps K).
SJMI_LIB names a variant library for an A/B (tools/build_variant.sh).
  python tools/bench_dictcol.py [--rows N] [--steps K] [--warmup W] [--columns a,b] [--host] [--out PATH]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRING = ord('"')


def synthetic(rng, n, distinct, p_null=0.05):
    """-> (types, values, sb, expected indices, expected n_distinct): n rows over `distinct` different strings of 2 to 40 bytes"""
    lens = rng.integers(2, 41, size=distinct)
    lens[4096:] = np.maximum(lens[4096:], 4)
    vocab = rng.integers(97, 123, size=(distinct, 40), dtype=np.uint8)
    ids = np.arange(distinct, dtype=np.uint32)
    for b in range(3):  # (the value's number in its first bytes: no two are equal)
        vocab[:, b] = np.where(b < lens, (ids >> (8 * b)) & 0xFF, vocab[:, b])
    pick = rng.integers(0, distinct, size=n)
    null = rng.random(n) < p_null
    row_len = np.where(null, 0, lens[pick]).astype(np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(row_len, out=offs[1:])
    sb = vocab[pick][np.arange(40)[None, :] < row_len[:, None]]
    types = np.where(null, rng.choice(np.array([0, ord("n"), ord("l")], dtype=np.uint8), size=n), np.uint8(STRING)).astype(np.uint8)
    values = ((row_len.astype(np.uint64) << np.uint64(32)) | offs[:-1].astype(np.uint64))
    values[null] = np.uint64(0xFFFFFFFFFFFFFFFF)
    valid = ~null
    _, first_index, inverse = np.unique(pick[valid], return_index=True, return_inverse=True)
    order = np.argsort(first_index)
    rank = np.empty(order.size, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32)
    want = np.zeros(n, dtype=np.int32)
    want[valid] = rank[inverse]
    return types, values, np.ascontiguousarray(sb), want, int(order.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--columns", default="distinct4,distinct1024,distinct262144,github_type,twitter_user_lang")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "dictcol.json"))
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    from oracle import oracle as O
    from tests import dictcol_common as DC
    from tests import explode_common as EC
    from tests import select_common as SEL
    from tests.conftest import load_fixture
    from tests.test_gpu_batch import _pack
    from tools import opbench
    dev, ctx, stream = opbench.device()
    rng = np.random.default_rng(17)
    wanted = a.columns.split(",")
    cols = []
    keep = []  # (shards and plans stay alive)
    for name in wanted:
        if name.startswith("distinct"):
            d = int(name[len("distinct"):])
            t, v, sb, want, nd = synthetic(rng, a.rows, d)
            cols.append(dict(name=name, types=torch.from_numpy(t).to(dev), values=torch.from_numpy(v.view(np.int64)).to(dev), sb=torch.from_numpy(sb).to(dev),
                             want=want, n_distinct=nd, capacity=1 << (max(nd, 2) - 1).bit_length()))
        else:
            if name == "github_type":
                docs = SEL.reserialised("github_events.json", lambda x: x)
                cells = SEL.expected_columns([O.parse(x) for x in docs], ["/type"])[0]
            else:
                docs = [load_fixture("twitter.json")]
                cells = EC.expected_explode([O.parse(x) for x in docs], "/statuses", ["/user/lang"])[1][0]
            buf, offs = _pack(docs)
            shard = sharding.BatchShard(ctx, buf, offs, dev)
            shard.step(stream)
            if name == "github_type":
                plan = S.SelectPlan(["/type"])
                ty, va = shard.select(plan, stream)
            else:
                plan = S.ExplodePlan("/statuses", ["/user/lang"])
                _, ty, va = shard.explode(plan, len(cells), stream)
            torch.cuda.synchronize()
            assert shard.check()["failed_documents"] == 0
            ref = DC.reference_from_cells(cells)
            keep.append((shard, plan))
            cols.append(dict(name=name, types=ty[0].clone(), values=va[0].clone(), sb=shard.sb, want=ref.indices, n_distinct=ref.n_distinct, capacity=64))

    def buffers(col):
        n, cap = col["types"].numel(), col["capacity"]
        col.update(n=n, indices=torch.empty(n, dtype=torch.int32, device=dev), validity=torch.empty((n + 63) // 64, dtype=torch.int64, device=dev),
                   dict_rows=torch.empty(cap, dtype=torch.int64, device=dev), dict_offsets=torch.empty(cap + 1, dtype=torch.int64, device=dev),
                   result=torch.empty(6, dtype=torch.int64, device=dev), offsets=torch.empty(n + 1, dtype=torch.int64, device=dev),
                   sresult=torch.empty(4, dtype=torch.int64, device=dev))

    def encode(col, full):
        ctx.dictionary_column_device(col["types"].data_ptr(), col["values"].data_ptr(), col["n"], 0, col["sb"].data_ptr(), col["indices"].data_ptr(),
                                     col["validity"].data_ptr(), col["capacity"], col["dict_rows"].data_ptr(), col["dict_offsets"].data_ptr(),
                                     col["dict_bytes"].data_ptr() if full and col["dict_bytes"].numel() else 0, col["dict_bytes"].numel() if full else 0,
                                     col["result"].data_ptr(), stream)

    def gather(col):
        ctx.string_column_device(col["types"].data_ptr(), col["values"].data_ptr(), col["n"], col["sb"].data_ptr(), col["offsets"].data_ptr(),
                                 col["validity"].data_ptr(), col["str_bytes"].data_ptr(), col["str_bytes"].numel(), col["sresult"].data_ptr(), stream)

    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SJMI_LIB") or "libsjmi.so", "columns": []}
    for col in cols:
        buffers(col)
        col["dict_bytes"] = torch.empty(0, dtype=torch.uint8, device=dev)
        encode(col, False)
        torch.cuda.synchronize()
        r = col["result"].cpu().tolist()
        assert r[0] == col["n"] and r[3] == col["n_distinct"] and not r[5] & 1, (col["name"], r)
        col["dict_bytes"] = torch.empty(max(r[4], 1), dtype=torch.uint8, device=dev)[:r[4]]
        encode(col, True)
        torch.cuda.synchronize()
        assert col["result"].cpu().tolist()[5] == 0 and np.array_equal(col["indices"].cpu().numpy(), col["want"]), col["name"]
        col["str_bytes"] = torch.empty(1, dtype=torch.uint8, device=dev)
        ctx.string_column_device(col["types"].data_ptr(), col["values"].data_ptr(), col["n"], col["sb"].data_ptr(), col["offsets"].data_ptr(), 0, 0, 0,
                                 col["sresult"].data_ptr(), stream)
        torch.cuda.synchronize()
        col["str_bytes"] = torch.empty(max(int(col["sresult"][0]), 1), dtype=torch.uint8, device=dev)
        moved = 13 * col["n"] + r[4]
        src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
        legs = {"sizing": lambda: encode(col, False), "full": lambda: encode(col, True), "string_gather": lambda: gather(col), "d2d_copy": lambda: dst.copy_(src)}
        out = {"name": col["name"], "rows": col["n"], "n_valid": r[1], "n_distinct": r[3], "dict_capacity": col["capacity"], "dict_bytes": r[4],
               "string_bytes": int(col["sresult"][0]), "least_bytes_moved": moved}
        out.update(opbench.measure(legs, a.steps, a.warmup))
        full = out["full"]["median_ms"]
        out["full_over_string_gather"] = full / out["string_gather"]["median_ms"]
        out["full_over_d2d_copy"] = full / out["d2d_copy"]["median_ms"]
        out["host_route"] = "not measured"
        if a.host:
            try:
                import pyarrow as pa
            except ImportError:
                pa = None
            if pa is not None:
                ms = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    gather(col)
                    torch.cuda.synchronize()
                    offsets, data, validity = col["offsets"].cpu().numpy(), col["str_bytes"].cpu().numpy(), col["validity"].cpu().numpy()
                    arr = pa.LargeStringArray.from_buffers(col["n"], pa.py_buffer(offsets), pa.py_buffer(data), pa.py_buffer(validity))
                    enc = arr.dictionary_encode()
                    ms.append((time.perf_counter() - t0) * 1e3)
                assert len(enc.dictionary) == col["n_distinct"]
                out["host_route"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "steps": 3, "over_full": statistics.median(ms) / full}
        res["columns"].append(out)
        del src, dst
    opbench.write(a.out, res)
    for _, plan in keep:
        plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
