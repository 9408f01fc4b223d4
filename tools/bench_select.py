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
import os
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
    from oracle import oracle as O
    from tests import select_common as SC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    data, offs, shard, c = opbench.configs_shard(ctx, dev, stream, a.docs)
    plan = S.SelectPlan(POINTERS)
    shard.select(plan, stream)
    torch.cuda.synchronize()

    # ---- verify before timing: every pair of the first VERIFY_DOCS documents
    nv = min(VERIFY_DOCS, a.docs)
    parsed = [O.parse(bytes(data[int(offs[k]):int(offs[k + 1]) - 1])) for k in range(nv)]
    types = shard.sel_types[:, :nv].cpu().numpy()
    values = shard.sel_values[:, :nv].cpu().numpy().view(np.uint64)
    sb_bytes = int(c["string_bytes"])
    present = SC.check_columns(types, values, bytes(shard.sb[:sb_bytes].cpu().numpy()), SC.expected_columns(parsed, POINTERS), "bench")
    tape_bytes = 8 * int(c["tape_words"])

    res = {"documents": a.docs, "input_bytes": int(offs[-1]), "paths": POINTERS, "verified_pairs": nv * len(POINTERS), "verified_present": int(present),
           "tape_bytes": tape_bytes, "string_record_bytes": sb_bytes, "column_bytes": 9 * len(POINTERS) * a.docs,
           "device": torch.cuda.get_device_name(0)}
    legs = {"select": lambda: shard.select(plan, stream), "parse": lambda: shard.step(stream),
            "parse_select": lambda: (shard.step(stream), shard.select(plan, stream))}
    tape_view, sb_view = shard.tape[:tape_bytes // 8], shard.sb[:sb_bytes // 8 * 8].view(torch.int64)
    legs["read_tape_and_strings"] = lambda: (tape_view.sum(), sb_view.sum())
    host_tape = torch.empty(tape_bytes // 8, dtype=torch.int64).pin_memory()
    host_sb = torch.empty(sb_bytes, dtype=torch.uint8).pin_memory()
    legs["d2h_tape_and_strings"] = lambda: (host_tape.copy_(tape_view, non_blocking=True), host_sb.copy_(shard.sb[:sb_bytes], non_blocking=True))
    res.update(opbench.measure(legs, a.steps, a.warmup, third={"d2h_tape_and_strings"}))
    assert shard.check()["failed_documents"] == 0
    sel, par = res["select"]["median_ms"], res["parse"]["median_ms"]
    res["select_over_parse_step"] = sel / par
    res["parse_select_over_parse"] = res["parse_select"]["median_ms"] / par
    res["select_over_read_yardstick"] = sel / res["read_tape_and_strings"]["median_ms"]
    res["d2h_over_select"] = res["d2h_tape_and_strings"]["median_ms"] / sel
    res["select_docs_per_s"] = a.docs / (sel * 1e-3)
    res["select_read_TBps"] = (tape_bytes + sb_bytes) / (sel * 1e-3) / 1e12
    opbench.write(a.out, res)
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
