"""What selecting fields of a parsed batch on the device costs -> profiles/r7/select.json, everything from ONE process on one
box (boxes differ by several per cent: only numbers of the same run are compared).

The configs[3] batch (1,000,000 unique documents, tools/docgen.c) and a 12-path plan; the columns are first verified against
tests/select_common.py (the oracle's tapes read by the oracle's walk) on the first 20,000 documents.  Then:
  (a) k_select alone, by HIP events around single launches;
  (b) a parse step alone, and a parse step with the select queued behind it (events around the whole step);
  (c) two yardsticks: a read-only pass over exactly the tape words and string-record bytes the batch made, and the D2H copy
      of those bytes into pinned memory -- the only way to select before this.
  python tools/bench_select.py [--docs N] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINTERS = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]
VERIFY_DOCS = 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "select.json"))
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from simdjson_java_amd import sharding
    from oracle import oracle as O
    from tests import select_common as SC
    from tools import workloads as W
    dev = torch.device("cuda", 0)
    data, offs = W.unique_docs(0, a.docs)
    ctx = S.Context(0, 1 << 20)
    shard = sharding.BatchShard(ctx, torch.from_numpy(data), offs, dev, index_ratio=4, string_ratio=1.0, tape_ratio=0.25)
    plan = S.SelectPlan(POINTERS)
    # (handle 0 names the context's own stream in the C ABI, so torch's default stream cannot carry the events: a stream of its own)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    assert stream != 0
    shard.step(stream)
    shard.select(plan, stream)
    torch.cuda.synchronize()
    c = shard.check()
    assert c["failed_documents"] == 0 and not getattr(shard, "rejected_steps", 0), c

    # ---- verify before timing: every pair of the first VERIFY_DOCS documents
    nv = min(VERIFY_DOCS, a.docs)
    parsed = [O.parse(bytes(data[int(offs[k]):int(offs[k + 1]) - 1])) for k in range(nv)]
    types = shard.sel_types[:, :nv].cpu().numpy()
    values = shard.sel_values[:, :nv].cpu().numpy().view(np.uint64)
    sb_bytes = int(c["string_bytes"])
    present = SC.check_columns(types, values, bytes(shard.sb[:sb_bytes].cpu().numpy()), SC.expected_columns(parsed, POINTERS), "bench")
    tape_bytes = 8 * int(c["tape_words"])

    def timed(fn, steps, warmup):
        """median / min of `steps` single executions of fn(), each between two HIP events"""
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "steps": steps}

    res = {"documents": a.docs, "input_bytes": int(offs[-1]), "paths": POINTERS, "verified_pairs": nv * len(POINTERS), "verified_present": int(present),
           "tape_bytes": tape_bytes, "string_record_bytes": sb_bytes, "column_bytes": 9 * len(POINTERS) * a.docs,
           "device": torch.cuda.get_device_name(0)}
    # interleaved, so that drift of the box hits every leg alike
    legs = {"select": lambda: shard.select(plan, stream), "parse": lambda: shard.step(stream),
            "parse_select": lambda: (shard.step(stream), shard.select(plan, stream))}
    tape_view, sb_view = shard.tape[:tape_bytes // 8], shard.sb[:sb_bytes // 8 * 8].view(torch.int64)
    legs["read_tape_and_strings"] = lambda: (tape_view.sum(), sb_view.sum())
    host_tape = torch.empty(tape_bytes // 8, dtype=torch.int64).pin_memory()
    host_sb = torch.empty(sb_bytes, dtype=torch.uint8).pin_memory()
    legs["d2h_tape_and_strings"] = lambda: (host_tape.copy_(tape_view, non_blocking=True), host_sb.copy_(shard.sb[:sb_bytes], non_blocking=True))
    rounds = 3
    runs = {k: [] for k in legs}
    for r in range(rounds):
        for name, fn in legs.items():
            few = name == "d2h_tape_and_strings"
            runs[name].append(timed(fn, max(3, a.steps // (3 if few else 1) // rounds), a.warmup if r == 0 else 1))
    for name, rs in runs.items():
        res[name] = {"median_ms": statistics.median(x["median_ms"] for x in rs), "min_ms": min(x["min_ms"] for x in rs),
                     "steps": sum(x["steps"] for x in rs)}
    assert shard.check()["failed_documents"] == 0
    sel, par = res["select"]["median_ms"], res["parse"]["median_ms"]
    res["select_over_parse_step"] = sel / par
    res["parse_select_over_parse"] = res["parse_select"]["median_ms"] / par
    res["select_over_read_yardstick"] = sel / res["read_tape_and_strings"]["median_ms"]
    res["d2h_over_select"] = res["d2h_tape_and_strings"]["median_ms"] / sel
    res["select_docs_per_s"] = a.docs / (sel * 1e-3)
    res["select_read_TBps"] = (tape_bytes + sb_bytes) / (sel * 1e-3) / 1e12
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
