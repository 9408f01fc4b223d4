"""What carrying document columns onto exploded rows costs on the device -> profiles/r28/parents.json, everything from ONE process
on one box (boxes differ by several per cent: only numbers of the same run are compared).  --rows rows over --docs documents with
every --cols number of carried columns, in these --shapes:

  dense          the rows of an explode, every document with 0 .. 2 * rows / docs rows
  dense_empty    the same rows over the same documents, 90 % of which have none
  dense_skewed   one document owns half of all rows
  sparse_ranked  2048 row indices in no order (the rows of a top k)
  sparse_tenth   an ascending selection of a tenth of the rows (a filter's rows)

Every leg's complete output is compared with the torch formulation before it is timed, the legs of a configuration are
interleaved by tools/opbench.py, and every leg's spread is in its record:

  parent_columns  sjmi_parent_columns_device: the parents, their type bytes and the carried cells
  torch_route     the route a user has today: torch.searchsorted(offsets[1:], x, right=True), then an index_select per carried
                  type and value column (x, for the dense shapes an arange, is made outside the timed region)
  copy_floor      a device copy that moves the least bytes the result needs: 8 per offset read, 9 per parent written, 18 per carried
                  cell (9 read, 9 written) -- a copy of half of them, since a copy reads and writes every byte it moves
No figure is a pass mark.
  python tools/bench_parents.py [--rows N] [--docs N] [--cols a,b,..] [--shapes a,b] [--steps K] [--warmup W] [--out PATH]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ("dense", "dense_empty", "dense_skewed", "sparse_ranked", "sparse_tenth")
MAX_COLS = 64
RANKED = 2048


def bench_counts(n_rows, n_docs, shape, seed=28):
    """-> the rows of every document, int64 [n_docs], that sum to exactly n_rows"""
    rng = np.random.default_rng(seed)
    if shape == "dense_skewed":
        counts = bench_counts(n_rows - n_rows // 2, n_docs, "dense", seed)
        counts[n_docs // 2] += n_rows // 2
        return counts
    with_rows = np.ones(n_docs, dtype=bool) if shape != "dense_empty" else rng.random(n_docs) < 0.1
    with_rows[0] = True
    m = int(with_rows.sum())
    counts = np.zeros(n_docs, dtype=np.int64)
    counts[with_rows] = rng.multinomial(n_rows, np.full(m, 1.0 / m))  # (sums to n_rows)
    return counts


def bench_rows(n_rows, shape, seed=28):
    """-> None for a dense shape, else the row indices, int64"""
    rng = np.random.default_rng(seed)
    if shape == "sparse_ranked":
        return rng.integers(0, n_rows, size=min(RANKED, n_rows)).astype(np.int64)
    if shape == "sparse_tenth":
        return np.flatnonzero(rng.random(n_rows) < 0.1).astype(np.int64)
    return None


def torch_route(torch, offsets, x, types, values):
    """-> (parents int64 [n], the carried types [n_cols, n] uint8, the carried values [n_cols, n] int64); every x below
    offsets[-1]"""
    k = torch.searchsorted(offsets[1:], x, right=True)
    n_cols = int(types.shape[0])
    out_types = [types[c].index_select(0, k) for c in range(n_cols)]
    out_values = [values[c].index_select(0, k) for c in range(n_cols)]
    return k, out_types, out_values


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8 << 20)
    ap.add_argument("--docs", type=int, default=1 << 20)
    ap.add_argument("--cols", default="0,1,4,12")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28", "parents.json"))
    a = ap.parse_args(argv)
    shapes = [s for s in a.shapes.split(",") if s]
    if a.rows < 1 or a.rows >= 1 << 32 or a.docs < 1 or a.docs >= 1 << 32 or a.steps < 1 or a.warmup < 0:
        ap.error("--rows and --docs must be in [1, 2^32), --steps >= 1, --warmup >= 0")
    if not shapes or any(s not in SHAPES for s in shapes):
        ap.error("--shapes: a list of " + ", ".join(SHAPES))
    try:
        cols = [int(s) for s in a.cols.split(",") if s]
    except ValueError:
        cols = []
    if not cols or any(not 0 <= c <= MAX_COLS for c in cols):
        ap.error("--cols: a list of column counts in [0, %d]" % MAX_COLS)
    import torch
    from tests import parents_common as PC
    from tools import opbench
    dev, ctx, stream = opbench.device()
    res = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "docs": a.docs, "library": "libsjmi.so", "configurations": []}
    up = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    ty, va = PC.doc_columns(max(cols) or 1, a.docs, a.docs, 28)
    d_ty_all, d_va_all = up(ty), up(va)
    for shape in shapes:
        d_off = up(PC.offsets_of(bench_counts(a.rows, a.docs, shape)))
        rows = bench_rows(a.rows, shape)
        d_rows = None if rows is None else up(rows)
        n = a.rows if rows is None else int(rows.size)
        x = torch.arange(n, dtype=torch.int64, device=dev) if rows is None else d_rows
        for n_cols in cols:
            d_ty, d_va = d_ty_all[:n_cols].contiguous(), d_va_all[:n_cols].contiguous()
            pt, p = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
            ot, ov = torch.empty((n_cols, n), dtype=torch.uint8, device=dev), torch.empty((n_cols, n), dtype=torch.int64, device=dev)
            record = torch.empty(3, dtype=torch.int64, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else 0
            call = lambda: ctx.parent_columns_device(d_off.data_ptr(), a.docs, ptr(d_rows), n, 0, ptr(d_ty), ptr(d_va), n_cols, a.docs, pt.data_ptr(),
                                                     p.data_ptr(), ptr(ot), ptr(ov), n, record.data_ptr(), stream)
            route = lambda: torch_route(torch, d_off, x, d_ty, d_va)
            call()
            torch.cuda.synchronize()
            k, their_types, their_values = route()
            assert record.cpu().tolist() == [n, 0, 0] and torch.equal(p, k) and bool((pt == ord("l")).all())
            assert all(torch.equal(ot[c], their_types[c]) and torch.equal(ov[c], their_values[c]) for c in range(n_cols))
            least = 8 * (a.docs + 1) + 9 * n + 18 * n_cols * n
            src, dst = torch.empty(least // 2, dtype=torch.uint8, device=dev), torch.empty(least // 2, dtype=torch.uint8, device=dev)
            out = {"shape": shape, "n_cols": n_cols, "slots": n, "least_bytes": least}
            out.update(opbench.measure({"parent_columns": call, "torch_route": route, "copy_floor": lambda: dst.copy_(src)}, a.steps, a.warmup))
            for name in ("torch_route", "copy_floor"):
                out["parent_columns_over_" + name] = out["parent_columns"]["median_ms"] / out[name]["median_ms"]
            res["configurations"].append(out)
            print("%s, %d columns: parent_columns %.3f ms, torch_route %.3f ms, copy_floor %.3f ms" % (
                shape, n_cols, out["parent_columns"]["median_ms"], out["torch_route"]["median_ms"], out["copy_floor"]["median_ms"]),
                file=sys.stderr, flush=True)
            del src, dst, their_types, their_values
    opbench.write(a.out, res)
    ctx.close()


if __name__ == "__main__":
    main()
