"""What a sort of all rows by a column costs on the device -> profiles/r31/sortrows.json, everything from ONE process on one box
(boxes differ by several per cent: only numbers of the same run are compared).  For every --rows count (default 1 Mi and 8 Mi),
80 % of the rows candidates, every --cases case:

  counters   longs 0 .. 10^4 (2 digit passes)                   longs     uniform 64-bit longs (8 passes)
  doubles    doubles of both signs, zeros, infinities            chain     two keys: (20 small values, counters descending), two calls
  carried    the counters with 4 carried columns

Every leg is verified before it is timed, the legs of a configuration are interleaved by tools/opbench.py, and every leg's spread
is in its record:

  sort_rows    sjmi_sort_rows_device (chain: both calls); verified against tests/sortrows_common.expected / chain (rows, carried
               cells and records equal)
  read_only    the floor of one pass: torch reductions that only read the 9 bytes a row of the key column (type byte, value word)
  digit_copy   a device copy of the bytes ONE digit pass must move: 12 bytes (key, position) per candidate, read and written
  torch_route  the route a user has today: masks for the classes, the key made order-preserving (a double's totalOrder as an
               int64), torch.sort(stable=True), the other classes appended in row order, index_select of the carried columns.
               Verified against the same reference, rows included
No figure is a pass mark.
  python tools/bench_sortrows.py [--rows a,b] [--cases a,b] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CASES = ("counters", "longs", "doubles", "chain", "carried")


def bench_keys(n, case, seed=31):
    """-> [(types uint8, values uint64, kind, descending)], most significant first: the key columns of the case"""
    from tests import toprows_common as TC
    from tools.bench_toprows import bench_column
    if case == "chain":
        ty, va, kind = bench_column(n, "counters", seed)
        few = (np.random.default_rng(seed + 1).integers(0, 20, n, dtype=np.int64)).view(np.uint64)
        return [(np.full(n, ord("l"), dtype=np.uint8), few, TC.LONG, False), (ty, va, kind, True)]
    ty, va, kind = bench_column(n, {"longs": "uniform", "carried": "counters"}.get(case, case), seed)
    return [(ty, va, kind, False)]


def torch_route(torch, ty, val, double, descending, rows_in=None, carry_val=None):
    """one key -> (rows [n] int64: the candidates by (value, position), then the NaN, OTHER and NULL positions in position order,
    as source rows; the carried cells [n_cols, n] or None)"""
    src = rows_in if rows_in is not None else torch.arange(ty.numel(), device=ty.device)
    t, b = (ty, val) if rows_in is None else (ty[rows_in], val[rows_in])
    cand = (t == ord("l")) | (t == ord("d")) if double else t == ord("l")
    null = (t == 0) | (t == ord("n"))
    if double:
        as_long = t == ord("l")
        b = torch.where(as_long, b.to(torch.float64).view(torch.int64), b)
        nan = cand & ((b & 0x7FFFFFFFFFFFFFFF) > 0x7FF0000000000000)
        cand = cand & ~nan
        b = b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)  # (totalOrder as the order of int64)
    else:
        nan = torch.zeros_like(cand)
    other = ~cand & ~null & ~nan
    at = cand.nonzero().squeeze(1)
    order = torch.sort(b[at], stable=True, descending=descending).indices
    rows = torch.cat([src[at[order]], src[nan], src[other], src[null]])
    return rows, None if carry_val is None else carry_val.index_select(1, rows)


def torch_chain(torch, keys, carry_val=None):
    """keys as bench_keys gives them, on the device as (types, values int64, kind, descending): the last key first"""
    from tests import toprows_common as TC
    rows = None
    for i, (ty, val, kind, descending) in enumerate(reversed(keys)):
        rows, cells = torch_route(torch, ty, val, kind == TC.DOUBLE, descending, rows, carry_val if i == len(keys) - 1 else None)
    return rows, cells


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="%d,%d" % (1 << 20, 8 << 20))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31", "sortrows.json"))
    a = ap.parse_args(argv)
    cases = [s for s in a.cases.split(",") if s]
    try:
        row_counts = [int(s) for s in a.rows.split(",") if s]
    except ValueError:
        row_counts = []
    if not row_counts or any(not 1 <= n < 1 << 32 for n in row_counts) or a.steps < 1 or a.warmup < 0:
        ap.error("--rows: a list of counts in [1, 2^32), --steps >= 1, --warmup >= 0")
    if not cases or any(s not in CASES for s in cases):
        ap.error("--cases: a list of " + ", ".join(CASES))
    import torch
    from tests import sortrows_common as SO
    from tests import toprows_common as TC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "library": os.environ.get("SJMI_LIB") or "libsjmi.so", "configurations": []}
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    for n in row_counts:
        for case in cases:
            keys = bench_keys(n, case)
            d_keys = [(up(ty), up(va), kind, desc) for ty, va, kind, desc in keys]
            n_cols = 4 if case == "carried" else 0
            c_ty, c_va = TC.carried(n_cols, n, n, 31) if n_cols else (None, None)
            d_cty, d_cva = (up(c_ty), up(c_va)) if n_cols else (None, None)
            bufs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2)]
            out_ty, out_va = torch.empty((n_cols, n), dtype=torch.uint8, device=dev), torch.empty((n_cols, n), dtype=torch.int64, device=dev)
            records = torch.empty((len(keys), 9), dtype=torch.int64, device=dev)

            def call():
                src = 0
                for i, at in enumerate(range(len(keys) - 1, -1, -1)):
                    ty, va, kind, desc = d_keys[at]
                    carry = n_cols if at == 0 else 0
                    ctx.sort_rows_device(ty.data_ptr(), 0, va.data_ptr(), n, src, n, 0, kind, 1 if desc else 0, d_cty.data_ptr() if carry else 0,
                                         d_cva.data_ptr() if carry else 0, carry, n if carry else 0, bufs[i % 2].data_ptr(),
                                         out_ty.data_ptr() if carry else 0, out_va.data_ptr() if carry else 0, n if carry else 0,
                                         records[at].data_ptr(), stream)
                    src = bufs[i % 2].data_ptr()
                return bufs[(len(keys) - 1) % 2]

            route = lambda: torch_chain(torch, d_keys, d_cva)
            rows = call()
            torch.cuda.synchronize()
            want_rows, want = SO.chain([(ty, None, va, kind, desc) for ty, va, kind, desc in keys], n)
            assert records.cpu().numpy().view(np.uint64).tolist() == want and (rows.cpu().numpy().view(np.uint64) == want_rows).all()
            at = want_rows.astype(np.int64)
            if n_cols:
                assert (out_va.cpu().numpy().view(np.uint64) == c_va[:, at]).all() and (out_ty.cpu().numpy() == c_ty[:, at]).all()
            their_rows, their_cells = route()
            assert (their_rows.cpu().numpy() == at).all() and (not n_cols or (their_cells.cpu().numpy().view(np.uint64) == c_va[:, at]).all())
            n_cand = want[-1][1]
            moved, landed = torch.empty(12 * n_cand, dtype=torch.uint8, device=dev), torch.empty(12 * n_cand, dtype=torch.uint8, device=dev)
            k_ty, k_va = d_keys[-1][0], d_keys[-1][1]
            out = {"rows": n, "case": case, "n_candidates": [w[1] for w in want], "n_passes": [w[7] for w in want], "carried_columns": n_cols}
            out.update(opbench.measure({"sort_rows": call, "read_only": lambda: (k_ty.sum(), k_va.sum()), "digit_copy": lambda: landed.copy_(moved),
                                        "torch_route": route}, a.steps, a.warmup, third=("torch_route",)))
            for name in ("read_only", "digit_copy", "torch_route"):
                out["sort_rows_over_" + name] = out["sort_rows"]["median_ms"] / out[name]["median_ms"]
            res["configurations"].append(out)
            print("%d rows, %s (%s passes): sort_rows %.3f ms, read_only %.3f ms, digit_copy %.3f ms, torch_route %.3f ms" % (
                n, case, out["n_passes"], out["sort_rows"]["median_ms"], out["read_only"]["median_ms"], out["digit_copy"]["median_ms"],
                out["torch_route"]["median_ms"]), file=sys.stderr, flush=True)
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
