"""What the top k rows of a column cost on the device -> profiles/r26/toprows.json, everything from ONE process on one box (boxes
differ by several per cent: only numbers of the same run are compared).  --rows rows, 80 % of them candidates, for every --ks k
(default 1, 100, 2048) over every --columns key column (uniform 64-bit longs, counters 0 .. 10^4, all equal, doubles), one
carried column.  Every leg is verified before it is timed, the legs of a configuration are interleaved by tools/opbench.py, and
every leg's spread is in its record:

  top_rows     sjmi_top_rows_device; verified against tests/toprows_common.expected (rows, carried cells and record equal)
  read_only    the floor: torch reductions that only read the 9 bytes a row the operator must read once (type byte, value word)
  torch_route  the route a user has today: the column masked to a dense int64 / float64 tensor, torch.topk, the row indices
               through the mask's nonzero(), index_select of the carried column.  Verified by VALUES only: torch.topk leaves the
               order of ties unspecified, so its rows may differ from run to run
SJMI_LIB=<a variant built by tools/build_variant.sh> measures that library instead (the range narrowing switched off:
profiles/r26/README.md).  No figure is a pass mark.
  python tools/bench_toprows.py [--rows N] [--ks a,b,..] [--columns a,b] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COLUMNS = ("uniform", "counters", "equal", "doubles")
MAX_K = 2048


def bench_column(n, what, seed=26):
    """-> (types uint8, values uint64, kind): 80 % of the cells numbers of the kind, the others strings, nulls and booleans"""
    from tests import toprows_common as TC
    rng = np.random.default_rng(seed)
    number = rng.random(n) < 0.8
    types = rng.choice(np.frombuffer(b'"ntf', dtype=np.uint8), n)
    types[number] = ord("d") if what == "doubles" else ord("l")
    values = {"uniform": TC.longs_full, "counters": TC.counters, "equal": lambda n, s: np.full(n, 7, dtype=np.uint64),
              "doubles": TC.doubles_wide}[what](n, seed)
    values[~number] = TC.POISON[0]
    return types, values, TC.DOUBLE if what == "doubles" else TC.LONG


def torch_route(torch, ty, val, carry_val, k, double, largest=True):
    """-> (values [n_out] int64 or float64 in rank order, rows [n_out] int64 -- the ties in an unspecified order --, the carried
    cells [n_cols, n_out])"""
    mask = ty == (ord("d") if double else ord("l"))
    dense = (val.view(torch.float64) if double else val)[mask]
    top, at = torch.topk(dense, min(k, int(dense.numel())), largest=largest)
    rows = mask.nonzero().squeeze(1)[at]
    return top, rows, carry_val.index_select(1, rows)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--ks", default="1,100,2048")
    ap.add_argument("--columns", default=",".join(COLUMNS))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "toprows.json"))
    a = ap.parse_args(argv)
    columns = [s for s in a.columns.split(",") if s]
    if a.rows < 1 or a.rows >= 1 << 32 or a.steps < 1 or a.warmup < 0:
        ap.error("--rows must be in [1, 2^32), --steps >= 1, --warmup >= 0")
    if not columns or any(s not in COLUMNS for s in columns):
        ap.error("--columns: a list of " + ", ".join(COLUMNS))
    try:
        ks = [int(s) for s in a.ks.split(",") if s]
    except ValueError:
        ks = []
    if not ks or any(not 1 <= k <= MAX_K for k in ks):
        ap.error("--ks: a list of k in [1, %d]" % MAX_K)
    import torch
    from tests import toprows_common as TC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "library": os.environ.get("SJMI_LIB") or "libsjmi.so", "configurations": []}
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    c_ty, c_va = TC.carried(1, a.rows, a.rows, 26)
    d_cty, d_cva = up(c_ty), up(c_va)
    for what in columns:
        ty, va, kind = bench_column(a.rows, what)
        d_ty, d_va = up(ty), up(va)
        for k in ks:
            rows = torch.empty(k, dtype=torch.int64, device=dev)
            out_ty, out_va = torch.empty((1, k), dtype=torch.uint8, device=dev), torch.empty((1, k), dtype=torch.int64, device=dev)
            record = torch.empty(9, dtype=torch.int64, device=dev)
            call = lambda: ctx.top_rows_device(d_ty.data_ptr(), 0, d_va.data_ptr(), a.rows, 0, kind, 0, k, d_cty.data_ptr(), d_cva.data_ptr(), 1, a.rows,
                                               rows.data_ptr(), out_ty.data_ptr(), out_va.data_ptr(), record.data_ptr(), stream)
            route = lambda: torch_route(torch, d_ty, d_va, d_cva, k, kind == TC.DOUBLE)
            call()
            torch.cuda.synchronize()
            want_rows, want = TC.expected(ty, None, va, a.rows, kind, True, k)
            n_out = want[6]
            assert record.cpu().numpy().view(np.uint64).tolist() == want and rows.cpu().numpy()[:n_out].tolist() == want_rows.tolist()
            assert (out_va.cpu().numpy().view(np.uint64)[0, :n_out] == c_va[0, want_rows]).all() and (out_ty.cpu().numpy()[0, :n_out] == c_ty[0, want_rows]).all()
            top, their_rows, _ = route()
            column = va.view(np.float64) if kind == TC.DOUBLE else va.view(np.int64)
            assert top.cpu().numpy().tolist() == column[want_rows].tolist() and column[their_rows.cpu().numpy()].tolist() == column[want_rows].tolist()
            out = {"column": what, "k": k, "n_candidates": want[1]}
            out.update(opbench.measure({"top_rows": call, "read_only": lambda: (d_ty.sum(), d_va.sum()), "torch_route": route}, a.steps, a.warmup))
            for name in ("read_only", "torch_route"):
                out["top_rows_over_" + name] = out["top_rows"]["median_ms"] / out[name]["median_ms"]
            res["configurations"].append(out)
            print("%s, k = %d: top_rows %.3f ms, read_only %.3f ms, torch_route %.3f ms" % (
                what, k, out["top_rows"]["median_ms"], out["read_only"]["median_ms"], out["torch_route"]["median_ms"]), file=sys.stderr, flush=True)
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
