"""What gathering string columns on the device costs -> profiles/r12/strcol.json, everything from ONE process on one box (boxes
differ by several per cent: only numbers of the same run are compared).

The configs[3] batch (1,000,000 unique documents, tools/docgen.c), the 12-path plan of tools/bench_select.py, and of its
columns those that hold strings.  Every such column is first verified against tests/strcol_common.py (numpy) on its first
20,000 rows.  Then, interleaved, each leg over ALL string-valued columns, by HIP events:
  (a) the sizing calls (chunk sums, their scan, the offsets; validity written);
  (b) the full calls into buffers of the exact size; the copy kernel's share is (b) - (a): the two calls differ by that launch;
  (c) the yardstick: a torch device-to-device copy of total_bytes + 17 * n_rows bytes per column, which is what the pass must
      at least move (a type byte, a value word and an offset per row; the bytes once -- read and written by the copy);
  (d) the select step the gather follows.
  python tools/bench_strcol.py [--docs N] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINTERS = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]
VERIFY_ROWS = 20000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "strcol.json"))
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from tests import strcol_common as SC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    data, offs, shard, c = opbench.configs_shard(ctx, dev, stream, a.docs)
    plan = S.SelectPlan(POINTERS)
    types, values = shard.select(plan, stream)
    torch.cuda.synchronize()
    sb_host = shard.sb[:int(c["string_bytes"])].cpu().numpy()

    # ---- the string-valued columns, sized, and verified before timing
    n = a.docs
    cols = []
    for p, ptr in enumerate(POINTERS):
        if not bool((types[p] == ord('"')).any()):
            continue
        offsets, validity, out, result = shard.string_column(types[p], values[p], stream=stream)
        torch.cuda.synchronize()
        r = result.cpu().numpy()
        nv = min(VERIFY_ROWS, n)
        ref = SC.reference(types[p][:nv].cpu().numpy(), values[p][:nv].cpu().numpy(), sb_host)
        assert np.array_equal(offsets[:nv + 1].cpu().numpy(), ref[0]), ptr
        assert np.array_equal(validity[:nv // 64].cpu().numpy().view(np.uint64), ref[1][:nv // 64]), ptr
        assert bytes(out[:len(ref[2])].cpu().numpy()) == ref[2], ptr
        assert int(r[0]) == out.numel() == int(offsets[-1]) and not (int(r[3]) & 1), ptr
        cols.append({"pointer": ptr, "p": p, "total_bytes": int(r[0]), "n_valid": int(r[1]), "n_other": int(r[2]),
                     "offsets": offsets, "validity": validity, "out": out, "result": result})
    assert cols, "no string-valued column"

    def gather(col, full):
        p = col["p"]
        ctx.string_column_device(types[p].data_ptr(), values[p].data_ptr(), n, shard.sb.data_ptr(), col["offsets"].data_ptr(),
                                 col["validity"].data_ptr(), col["out"].data_ptr() if full and col["total_bytes"] else 0,
                                 col["total_bytes"] if full else 0, col["result"].data_ptr(), stream)

    moved = sum(col["total_bytes"] + 17 * n for col in cols)
    src = torch.empty(moved, dtype=torch.uint8, device=dev)
    dst = torch.empty(moved, dtype=torch.uint8, device=dev)
    res = {"documents": n, "input_bytes": int(offs[-1]), "paths": POINTERS, "verified_rows_per_column": min(VERIFY_ROWS, n),
           "string_columns": [{k: col[k] for k in ("pointer", "total_bytes", "n_valid", "n_other")} for col in cols],
           "least_bytes_moved": moved, "device": torch.cuda.get_device_name(0)}
    legs = {"sizing": lambda: [gather(col, False) for col in cols], "full": lambda: [gather(col, True) for col in cols],
            "d2d_copy": lambda: dst.copy_(src), "select": lambda: shard.select(plan, stream)}
    res.update(opbench.measure(legs, a.steps, a.warmup))
    full, sizing = res["full"]["median_ms"], res["sizing"]["median_ms"]
    res["copy_kernels_ms"] = full - sizing  # (a difference of two medians, not a measurement of its own)
    res["full_over_d2d_copy"] = full / res["d2d_copy"]["median_ms"]
    res["full_over_select"] = full / res["select"]["median_ms"]
    res["sizing_over_full"] = sizing / full
    res["full_GBps_of_least_bytes"] = moved / (full * 1e-3) / 1e9
    res["one_long_string"] = "not measured"
    opbench.write(a.out, res)
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
