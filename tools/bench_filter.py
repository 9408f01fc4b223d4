"""What filtering the rows of selected columns on the device costs -> profiles/r14/filter.json, everything from ONE process on one
box (boxes differ by several per cent: only numbers of the same run are compared).

The configs[3] batch (1,000,000 unique documents, tools/docgen.c) and the 12-path plan of tools/bench_select.py.  Every leg's
result -- the kept rows and every compacted cell -- is first verified against the framework formulation a caller uses today (type
and value compares, nonzero, one index_select per column).  Then, interleaved, by HIP events around warmed calls:
  numeric / string_eq / mixed4   sjmi_filter_columns_device with all outputs at capacity n_rows (no read-back anywhere), each
                                 against (t) the framework formulation and (r) a read-only pass (a torch sum) over the bytes the
                                 call must at least move: the term columns' type bytes and the value words they need, 9 bytes read
                                 and written per kept cell, 8 bytes per kept row (least_bytes() below);
  sizing                         the numeric plan with out_capacity 0;
  strcol_*                       sjmi_string_column_device on the heaviest string column ("/z") into buffers of the exact size:
                                 all rows, against filter + the gather of the compacted column at roughly 1 %, 10 % and 50 % kept.
--trace-legs K: no timing; after the verification each of the three filter plans K times in a row (numeric, string_eq, mixed4), for
a rocprofv3 --kernel-trace run of its own, whose dispatches then come in that order.
  python tools/bench_filter.py [--docs N] [--steps K] [--warmup W] [--out PATH] [--trace-legs K]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINTERS = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]
K0, K1, Z, K12 = 0, 1, 6, 7
STRING, LONG, DOUBLE = ord('"'), ord("l"), ord("d")


def torch_keep(terms, types, values, sb):
    """the framework formulation of a plan: a bool mask per term from type and value compares (a string term gathers the
    candidates' bytes one position at a time), and-ed; LONG constants a double holds exactly, so that like compares with like"""
    import torch
    ops = {"eq": torch.eq, "ne": torch.ne, "lt": torch.lt, "le": torch.le, "gt": torch.gt, "ge": torch.ge}
    keep = None
    for column, op, const in terms:
        kind, cmp = op.split("_")
        t, v = types[column], values[column]
        if kind == "type":
            m = (t == const) if cmp == "eq" else (t != const)
        elif kind == "long":
            assert abs(const) <= 1 << 53
            m = ((t == LONG) & ops[cmp](v, const)) | ((t == DOUBLE) & ops[cmp](v.view(torch.float64), float(const)))
        else:
            const = bytes(const)
            lens = v >> 32
            cand = (t == STRING) & ((lens >= len(const)) if cmp == "prefix" else (lens == len(const)))
            idx = cand.nonzero().squeeze(1)
            src = v[idx] & 0xFFFFFFFF
            same = torch.ones(idx.numel(), dtype=torch.bool, device=t.device)
            for i, byte in enumerate(const):
                same &= sb[src + i] == byte
            m = torch.zeros_like(cand)
            m[idx] = same
            if cmp == "ne":
                m = (t == STRING) & ~m
        keep = m if keep is None else keep & m
    return keep


def torch_filter(terms, types, values, sb):
    """... nonzero, and one index_select per column -> (rows, out_types, out_values)"""
    import torch
    rows = torch_keep(terms, types, values, sb).nonzero().squeeze(1)
    out_types = torch.stack([types[c].index_select(0, rows) for c in range(types.shape[0])])
    out_values = torch.stack([values[c].index_select(0, rows) for c in range(values.shape[0])])
    return rows, out_types, out_values


def least_bytes(terms, types, n_kept):
    """the bytes a call must at least move: per column a term looks at its n type bytes once, and per term kind on that column
    the value words of the cells it can compare with; 9 bytes read and 9 written per kept cell, 8 bytes written per kept row"""
    n_cols, n = int(types.shape[0]), int(types.shape[1])
    total = n * len({c for c, _, _ in terms})
    for column, kind in {(c, op.split("_")[0]) for c, op, _ in terms}:
        t = types[column]
        if kind == "string":
            total += 8 * int((t == STRING).sum())
        elif kind in ("long", "double"):
            total += 8 * int(((t == LONG) | (t == DOUBLE)).sum())
    return total + (18 * n_cols + 8) * n_kept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "filter.json"))
    ap.add_argument("--trace-legs", type=int, default=0)
    a = ap.parse_args()
    import torch
    import simdjson_java_amd as S
    from tools import opbench
    dev, ctx, stream = opbench.device()
    _, offs, shard, _ = opbench.configs_shard(ctx, dev, stream, a.docs)
    select = S.SelectPlan(POINTERS)
    types, values = shard.select(select, stream)
    torch.cuda.synchronize()
    n, n_cols, sb = a.docs, len(POINTERS), shard.sb

    # ---- the plans: constants from the data, so that the kept share is what the leg's name says
    first_string = int((types[K0] == STRING).nonzero()[0])
    w = int(values[K0][first_string])
    some_k0 = bytes(sb[(w & 0xFFFFFFFF):(w & 0xFFFFFFFF) + (w >> 32)].cpu().numpy())
    longs = values[K1][types[K1] == LONG]
    at_share = lambda share: int(torch.quantile(longs[:1 << 20].double(), 1.0 - share * n / max(1, longs.numel())))  # k1 >= this keeps `share` of ALL rows
    plans = {"numeric": [(K1, "long_ge", at_share(0.10))],
             "string_eq": [(K0, "string_eq", some_k0)],
             "mixed4": [(K0, "type_ne", 0), (K1, "long_lt", at_share(0.15)), (Z, "string_ne", b"x"), (K12, "type_ne", ord("n"))],
             "kept_1pc": [(Z, "string_prefix", b"a")],
             "kept_10pc": [(K1, "long_ge", at_share(0.10))],
             "kept_50pc": [(K0, "type_ne", STRING), (K1, "type_ne", ord("{"))]}
    compiled = {name: S.FilterPlan(terms) for name, terms in plans.items()}
    out = {"rows": torch.empty(n, dtype=torch.int64, device=dev), "types": torch.empty((n_cols, n), dtype=torch.uint8, device=dev),
           "values": torch.empty((n_cols, n), dtype=torch.int64, device=dev), "keep": torch.empty((n + 63) // 64, dtype=torch.int64, device=dev),
           "result": torch.empty(2, dtype=torch.int64, device=dev)}

    def run_filter(name, capacity=None):
        capacity = n if capacity is None else capacity
        ctx.filter_columns_device(compiled[name], types.data_ptr(), values.data_ptr(), n_cols, n, n, sb.data_ptr(), out["keep"].data_ptr(),
                                  out["rows"].data_ptr() if capacity else 0, capacity, out["types"].data_ptr() if capacity else 0,
                                  out["values"].data_ptr() if capacity else 0, out["result"].data_ptr(), stream)

    # ---- every plan verified against the framework formulation before timing
    kept = {}
    for name, terms in plans.items():
        out["rows"].fill_(-1)
        run_filter(name)
        torch.cuda.synchronize()
        want_rows, want_types, want_values = torch_filter(terms, types, values, sb)
        k = int(out["result"][0])
        assert k == want_rows.numel() and int(out["result"][1]) == 0, (name, k, want_rows.numel())
        assert torch.equal(out["rows"][:k], want_rows) and bool((out["rows"][k:] == -1).all()), name
        assert torch.equal(out["types"][:, :k], want_types) and torch.equal(out["values"][:, :k], want_values), name
        bits = torch_keep(terms, types, values, sb)
        assert int(bits.sum()) == k
        word = out["keep"][:n // 64].cpu().numpy().view("uint64")
        assert np.array_equal(word, np.packbits(bits[:n // 64 * 64].cpu().numpy(), bitorder="little").view("<u8")), name
        kept[name] = k
    assert kept["string_eq"] >= 1

    if a.trace_legs:
        for name in ("numeric", "string_eq", "mixed4"):
            for _ in range(a.trace_legs):
                run_filter(name)
            torch.cuda.synchronize()
        print(json.dumps({"traced": ["numeric", "string_eq", "mixed4"], "calls_each": a.trace_legs, "kept_rows": kept}))
        return

    # ---- the string gather of "/z": all rows, and the compacted column of each kept share (buffers of the exact size, sized here)
    def gather_buffers(t, v, rows):
        offsets, validity, data, result = shard.string_column(t, v, stream=stream)
        torch.cuda.synchronize()
        return {"t": t, "v": v, "rows": rows, "offsets": offsets, "validity": validity, "data": data, "result": result, "bytes": int(result[0])}

    def gather(g):
        ctx.string_column_device(g["t"].data_ptr(), g["v"].data_ptr(), g["rows"], sb.data_ptr(), g["offsets"].data_ptr(), g["validity"].data_ptr(),
                                 g["data"].data_ptr() if g["bytes"] else 0, g["bytes"], g["result"].data_ptr(), stream)

    g_all = gather_buffers(types[Z], values[Z], n)
    g_kept = {}
    for name in ("kept_1pc", "kept_10pc", "kept_50pc"):
        run_filter(name)
        torch.cuda.synchronize()
        g_kept[name] = gather_buffers(out["types"][Z][:kept[name]], out["values"][Z][:kept[name]], kept[name])  # (views of `out`: filled again by every run_filter)

    def filter_then_gather(name):
        run_filter(name)
        gather(g_kept[name])

    legs = {"sizing": lambda: run_filter("numeric", 0), "strcol_all_rows": lambda: gather(g_all)}
    least = {}
    scratch = torch.zeros(max(least_bytes(plans[k], types, kept[k]) for k in ("numeric", "string_eq", "mixed4")) // 8 + 1, dtype=torch.int64, device=dev)
    for name in ("numeric", "string_eq", "mixed4"):
        least[name] = least_bytes(plans[name], types, kept[name])
        legs[name] = lambda name=name: run_filter(name)
        legs[name + "_torch"] = lambda name=name: torch_filter(plans[name], types, values, sb)
        legs[name + "_read_pass"] = lambda name=name: scratch[:least[name] // 8].sum()
    for name in g_kept:
        legs["strcol_" + name] = lambda name=name: filter_then_gather(name)
    res = {"documents": n, "input_bytes": int(offs[-1]), "paths": POINTERS, "columns": n_cols, "device": torch.cuda.get_device_name(0),
           "plans": {k: [[c, op, const.decode("latin-1") if isinstance(const, bytes) else const] for c, op, const in v] for k, v in plans.items()},
           "kept_rows": kept, "least_bytes_moved": least, "strcol_bytes": dict({"all_rows": g_all["bytes"]}, **{k: g["bytes"] for k, g in g_kept.items()}),
           "verified": "every plan: n_kept, rows, keep words and all compacted cells equal the framework formulation's"}
    res.update(opbench.measure(legs, a.steps, a.warmup))
    for name in ("numeric", "string_eq", "mixed4"):
        res[name + "_over_torch"] = res[name]["median_ms"] / res[name + "_torch"]["median_ms"]
        res[name + "_over_read_pass"] = res[name]["median_ms"] / res[name + "_read_pass"]["median_ms"]
    for name in g_kept:
        res["strcol_" + name + "_over_all_rows"] = res["strcol_" + name]["median_ms"] / res["strcol_all_rows"]["median_ms"]
    opbench.write(a.out, res)
    for p in compiled.values():
        p.close()
    select.close()
    ctx.close()


if __name__ == "__main__":
    main()
