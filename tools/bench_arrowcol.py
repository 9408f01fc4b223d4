"""What turning selected columns into Arrow int64 / float64 / bool arrays on the device costs -> profiles/r15/arrowcol.json,
everything from ONE process on one box (boxes differ by several per cent: only numbers of the same run are compared).

The configs[3] batch (1,000,000 unique documents, tools/docgen.c) and the 12-path plan of tools/bench_select.py.  Every leg's
outputs -- data words, validity words and records -- are first verified against the framework formulation a caller writes today
(type compares, where, casts, bit-packing).  Then, interleaved, medians of single calls between HIP events:
  float64        the numeric columns (those whose commonest type is 'l' or 'd') as FLOAT64
  int64          the same as INT64 with SJMI_ARROW_F_INTEGRAL_DOUBLES
  mixed12        all 12 columns, the kinds in rotation: INT64 with the flag, FLOAT64, BOOL (whatever the column holds: a cell
                 of another type is NULL and counted)
  counting       the mixed schema as the counting call (no data block)
  mixed12_after_filter   the mixed schema on the columns a filter compacted, its rows taken from the filter's n_kept on the device
each beside (t) the framework formulation and (c) ONE device-to-device copy that moves the bytes the call must at least move: 9
bytes read and 8.125 written per live cell (the counting call: 0.125 written) -- a copy of half that sum reads and writes it.
--trace-legs K: no timing; after the verification each leg K times in a row, for a rocprofv3 --kernel-trace run of its own.
  python tools/bench_arrowcol.py [--docs N] [--steps K] [--warmup W] [--out PATH] [--trace-legs K]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
POINTERS = ["/k0", "/k1", "/k3/x", "/k3/y", "/k5/0", "/k2/7", "/z", "/k12", "/k20/y", "/k4/3", "/nope", "/k7"]
LONG, DOUBLE, TRUE, FALSE, NULL = ord("l"), ord("d"), ord("t"), ord("f"), ord("n")


def pack_bits(bits):
    """bool [n] -> int64 words, LSB first"""
    import torch
    n = bits.numel()
    padded = torch.zeros((n + 63) // 64 * 64, dtype=torch.int64, device=bits.device)
    padded[:n] = bits
    return (padded.view(-1, 64) << torch.arange(64, device=bits.device)).sum(1)


def torch_field(kind, flags, t, v):
    """the framework formulation of one field -> (data int64 words, validity words, (n_valid, n_other, n_inexact))"""
    import torch
    is_l, is_d = t == LONG, t == DOUBLE
    inexact = 0
    if kind == "bool":
        valid = (t == TRUE) | (t == FALSE)
        data = pack_bits(t == TRUE)
    elif kind == "float64":
        valid = is_l | is_d
        as_double = v.double()
        data = torch.where(is_l, as_double, torch.where(is_d, v.view(torch.float64), 0.0)).view(torch.int64)
        inexact = int((is_l & (as_double.long() != v)).sum())
    else:
        x = v.view(torch.float64)
        ok = is_d & torch.isfinite(x) & (x == x.floor()) & (x >= -2.0 ** 63) & (x < 2.0 ** 63) if flags else torch.zeros_like(is_d)
        valid = is_l | ok
        data = torch.where(is_l, v, torch.where(ok, torch.where(ok, x, 0.0).long(), 0))
    other = ~valid & (t != 0) & (t != NULL)
    return data, pack_bits(valid), (int(valid.sum()), int(other.sum()), inexact)


def torch_fields(fields, types, values, live):
    return [torch_field(f[1], f[2:], types[f[0]][:live], values[f[0]][:live]) for f in fields]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1000000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "arrowcol.json"))
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
    n, n_cols = a.docs, len(POINTERS)

    # ---- the schemas: the numeric columns from the data (those whose commonest type is a number), the mixed one by rotation
    commonest = [int(torch.bincount(types[col].long(), minlength=256)[1:].argmax()) + 1 for col in range(n_cols)]
    numeric = [col for col in range(n_cols) if commonest[col] in (LONG, DOUBLE)]
    assert numeric, commonest
    kind_of = lambda col: (("int64", "integral_doubles"), ("float64",), ("bool",))[col % 3]
    schemas = {"float64": [(col, "float64") for col in numeric], "int64": [(col, "int64", "integral_doubles") for col in numeric],
               "mixed12": [(col,) + kind_of(col) for col in range(n_cols)]}
    # the filtered input: the first numeric column at or above its median, compacted (n_kept stays on the device)
    longs = values[numeric[0]][types[numeric[0]] == LONG]
    terms = [(numeric[0], "long_ge", int(longs[:1 << 20].double().median()))]
    plan = S.FilterPlan(terms)
    _, f_types, f_values, _, f_result = shard.filter(plan, types, values, stream=stream)
    torch.cuda.synchronize()
    n_kept = int(f_result[0])
    assert 0 < n_kept < n
    legs = {"float64": ("float64", types, values, None, True), "int64": ("int64", types, values, None, True), "mixed12": ("mixed12", types, values, None, True),
            "counting": ("mixed12", types, values, None, False), "mixed12_after_filter": ("mixed12", f_types, f_values, f_result[0:1], True)}
    live_of = {name: n_kept if leg[3] is not None else n for name, leg in legs.items()}
    words = (n + 63) // 64
    out = {"data": torch.empty((n_cols, n), dtype=torch.int64, device=dev), "validity": torch.empty((n_cols, words), dtype=torch.int64, device=dev),
           "results": torch.empty((n_cols, 4), dtype=torch.int64, device=dev)}

    def run_leg(name):
        schema, t, v, rc, with_data = legs[name]
        ctx.arrow_columns_device(schemas[schema], t.data_ptr(), v.data_ptr(), n_cols, n, n, rc.data_ptr() if rc is not None else 0,
                                 out["data"].data_ptr() if with_data else 0, n if with_data else 0, out["validity"].data_ptr(), words,
                                 out["results"].data_ptr(), stream)

    # ---- every leg verified against the framework formulation before timing
    counts = {}
    for name, (schema, t, v, rc, with_data) in legs.items():
        fields, live = schemas[schema], live_of[name]
        out["data"].fill_(-1)
        out["validity"].fill_(-1)
        run_leg(name)
        torch.cuda.synchronize()
        want = torch_fields(fields, t, v, live)
        got = out["results"][:len(fields)].cpu().tolist()
        assert got == [[live] + list(w[2]) for w in want], (name, got, [w[2] for w in want])
        for f, (w_data, w_valid, _) in enumerate(want):
            assert torch.equal(out["validity"][f, :w_valid.numel()], w_valid) and bool((out["validity"][f, w_valid.numel():] == -1).all()), (name, f)
            if with_data:
                assert torch.equal(out["data"][f, :w_data.numel()], w_data) and bool((out["data"][f, w_data.numel():] == -1).all()), (name, f)
            else:
                assert bool((out["data"][f] == -1).all()), (name, f)
        counts[name] = {"fields": len(fields), "live_rows": live, "n_valid": [w[2][0] for w in want], "n_other": [w[2][1] for w in want],
                        "n_inexact": [w[2][2] for w in want]}

    if a.trace_legs:
        for name in legs:
            for _ in range(a.trace_legs):
                run_leg(name)
            torch.cuda.synchronize()
        print(json.dumps({"traced": list(legs), "calls_each": a.trace_legs, "counts": counts}))
        return

    least = {name: int(live_of[name] * counts[name]["fields"] * (9 + (8.125 if legs[name][4] else 0.125))) for name in legs}
    src = torch.zeros(max(least.values()) // 16 + 1, dtype=torch.int64, device=dev)
    dst = torch.empty_like(src)
    timed_legs = {}
    for name, (schema, t, v, rc, with_data) in legs.items():
        timed_legs[name] = lambda name=name: run_leg(name)
        timed_legs[name + "_torch"] = lambda schema=schema, t=t, v=v, name=name: torch_fields(schemas[schema], t, v, live_of[name])
        timed_legs[name + "_copy"] = lambda name=name: dst[:least[name] // 16].copy_(src[:least[name] // 16])
    res = {"documents": n, "input_bytes": int(offs[-1]), "paths": POINTERS, "columns": n_cols, "device": torch.cuda.get_device_name(0),
           "commonest_type": [chr(x) for x in commonest], "schemas": {k: [list(f) for f in v] for k, v in schemas.items()}, "filter": [list(x) for x in terms],
           "counts": counts, "least_bytes_moved": least,
           "verified": "every leg: records, validity words and data words equal the framework formulation's; nothing written behind the live rows"}
    res.update(opbench.measure(timed_legs, a.steps, a.warmup))
    for name in legs:
        res[name + "_over_torch"] = res[name]["median_ms"] / res[name + "_torch"]["median_ms"]
        res[name + "_over_copy"] = res[name]["median_ms"] / res[name + "_copy"]["median_ms"]
    opbench.write(a.out, res)
    plan.close()
    select.close()
    ctx.close()


if __name__ == "__main__":
    main()
